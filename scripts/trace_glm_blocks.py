#!/usr/bin/env python3
"""Per-block timeline of the fused LR round at the bench shape (10M × 1000 bf16, 100k batch,
the shape's default grid): start, prologue-done, rows-done and atomics-drained stamps
(s_memrealtime, 100 MHz) of every block, summarised per round as spreads relative to the earliest
block start, plus per-XCD means; then the three spans of a block (start → prologue done → rows
done → end) as per-block medians and spreads. On the loader/consumer row path the loader wave also
stamps when it got past the prologue and when it saw each prefetched ring step landed (it drains
its prefetch for that, so a traced round starts its ring a little later than an untraced one):
"steps landed" counts the prefetched steps that were in LDS when the prologue ended. The same path
stamps the links of its launch head (the "head" spans): consumer wave 0 knows the round number, has
issued the previous round's accumulator loads, has them; the loader wave knows the round number and
has issued its first fill. --head 1 | 0 picks the lean or the generic head.

Shows how much of a round is launch skew, prologue, load imbalance (the slowest block's rows) and
tail.
Usage: python scripts/trace_glm_blocks.py [--rounds 20] [--defer 1] [--head 1]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flink_ml_amd.common.optimizer import SGD, DeviceGlmTrainer  # noqa: E402
from flink_ml_amd.ops import glm as gk  # noqa: E402

TICK_US = 0.01  # s_memrealtime runs at 100 MHz
REC = 16  # int64 words per block (csrc/glm.hip TRACE_REC)
PROLOGUE, LOADER = 4, 5  # (TRACE_PROLOGUE, TRACE_LOADER: loader past the prologue, then one per prefetched step)
HEAD = 11  # TRACE_HEAD: round known, accumulator loads issued, landed (consumer wave 0); round known, first fill (loader)
H_ROUND, H_ISSUED, H_LANDED, H_LD_ROUND, H_LD_FILL = range(HEAD, HEAD + 5)
# a prefetched step counts as landed at the end of the prologue when the loader's wait for it
# returned within this many ticks of the previous stamp (one s_memrealtime read takes 3–6)
LANDED_TICKS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--defer", type=int, default=1)
    ap.add_argument("--head", type=int, default=gk.HEAD, help="launch head of the loader path: 1 lean, 0 generic")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gk.DEFER = bool(a.defer)
    gk.set_head(a.head)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.empty((a.rows, a.dim), dtype=torch.bfloat16, device=dev)
    for s in range(0, a.rows, 1 << 20):
        e = min(s + (1 << 20), a.rows)
        X[s:e] = torch.rand((e - s, a.dim), generator=g, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 2, (a.rows,), generator=g, device=dev).float()
    sgd = SGD(max_iter=10 ** 8, learning_rate=0.1, global_batch_size=a.batch, tol=0.0)
    tr = DeviceGlmTrainer(sgd, np.zeros(a.dim), X, y, None, "logistic", use_graph=False)
    tr.run_rounds(30)
    torch.cuda.synchronize()
    nb = tr.nparts
    buf = torch.zeros((nb, REC), dtype=torch.int64, device=dev)
    gk.set_trace(buf)
    rows = []
    try:
        for _ in range(a.rounds):
            buf.zero_()
            tr._launch_round(1)
            torch.cuda.synchronize()
            rows.append(buf.cpu().numpy().copy())
    finally:
        gk.set_trace(None)
    summary = []
    for t in rows:
        t0 = t[:, 0].min()
        start = (t[:, 0] - t0) * TICK_US
        done = (t[:, 1] - t0) * TICK_US
        drained = (t[:, 2] - t0) * TICK_US
        xcc = (t[:, 3] >> 32) & 0xF
        per_x = {int(x): round(float(done[xcc == x].mean()), 2) for x in sorted(set(xcc.tolist()))}
        summary.append({
            "start_max_us": round(float(start.max()), 2),
            "rows_done_min_us": round(float(done.min()), 2),
            "rows_done_med_us": round(float(np.median(done)), 2),
            "rows_done_max_us": round(float(done.max()), 2),
            "drained_max_us": round(float(drained.max()), 2),
            "block_rows_us_med": round(float(np.median(done - start)), 2),
            "rows_done_mean_by_xcd": per_x,
        })
    for s in summary:
        print(json.dumps(s))
    # is the imbalance systematic? correlation of each block's rows-done time between rounds,
    # and how often the same XCD is the slowest
    done = np.stack([(t[:, 1] - t[:, 0].min()).astype(np.float64) for t in rows])
    cc = [float(np.corrcoef(done[i], done[i + 1])[0, 1]) for i in range(len(done) - 1)]
    xcc = (rows[0][:, 3] >> 32) & 0xF
    slow = [int(max(set(xcc.tolist()), key=lambda x: done[i][xcc == x].mean())) for i in range(len(done))]
    print(json.dumps({"block_done_corr_between_rounds_median": round(statistics.median(cc), 3),
                      "slowest_xcd_per_round": slow,
                      "block_done_spread_us_if_per_block_mean_removed": round(float(
                          np.median(np.ptp(done - done.mean(0, keepdims=True), axis=1)) * TICK_US), 2)}))
    spans(rows)
    print(json.dumps({"head": gk.last_head() if gk.row_path() == -1 else None}))
    keys = ["start_max_us", "rows_done_min_us", "rows_done_med_us", "rows_done_max_us", "block_rows_us_med"]
    xm = {x: round(statistics.median(s["rows_done_mean_by_xcd"][x] for s in summary), 2)
          for x in summary[0]["rows_done_mean_by_xcd"]}
    print(json.dumps({"median_over_rounds": {k: round(statistics.median(s[k] for s in summary), 2) for k in keys},
                      "rows_done_mean_by_xcd_median": xm, "blocks": nb}))


def spans(rows):
    """Per-block spans over all rounds: median, 10th–90th percentile and maximum in µs, and the
    loader wave's landed-step census (blocks whose record carries no prologue stamp, i.e. any row
    path but the loader's, print only the whole-round spans)."""
    t = np.stack(rows).astype(np.float64)  # [rounds, blocks, REC]

    def stat(x):
        x = x.reshape(-1) * TICK_US
        return {"med": round(float(np.median(x)), 2), "p10": round(float(np.percentile(x, 10)), 2),
                "p90": round(float(np.percentile(x, 90)), 2), "max": round(float(x.max()), 2)}

    out = {"rows_done_to_end_us": stat(t[:, :, 2] - t[:, :, 1])}
    if (t[:, :, PROLOGUE] > 0).all():
        out["start_to_prologue_done_us"] = stat(t[:, :, PROLOGUE] - t[:, :, 0])
        out["prologue_done_to_rows_done_us"] = stat(t[:, :, 1] - t[:, :, PROLOGUE])
        if (t[:, :, H_ROUND] > 0).all() and (t[:, :, H_ISSUED] > 0).all():  # (launch 0 has no accumulator to read)
            out["head_consumer_us"] = {
                "start_to_round_known": stat(t[:, :, H_ROUND] - t[:, :, 0]),
                "round_known_to_acc_issued": stat(t[:, :, H_ISSUED] - t[:, :, H_ROUND]),
                "acc_issued_to_landed": stat(t[:, :, H_LANDED] - t[:, :, H_ISSUED]),
                "acc_landed_to_prologue_done": stat(t[:, :, PROLOGUE] - t[:, :, H_LANDED])}
            out["head_loader_us"] = {
                "start_to_round_known": stat(t[:, :, H_LD_ROUND] - t[:, :, 0]),
                "round_known_to_first_fill": stat(t[:, :, H_LD_FILL] - t[:, :, H_LD_ROUND]),
                "start_to_first_fill": stat(t[:, :, H_LD_FILL] - t[:, :, 0])}
        ld = t[:, :, LOADER:HEAD]
        ns = int((ld[0, 0] > 0).sum()) - 1  # prefetched steps
        if ns > 0:
            d = np.diff(ld[:, :, :ns + 1], axis=2)  # wait for step i, from the previous stamp
            landed = (np.cumprod(d <= LANDED_TICKS, axis=2)).sum(axis=2)
            out["prefetched_steps"] = ns
            out["steps_landed_at_prologue_end"] = {"med": float(np.median(landed)), "min": int(landed.min()),
                                                   "max": int(landed.max()), "mean": round(float(landed.mean()), 2)}
            out["loader_wait_per_step_us_med"] = [round(float(np.median(d[:, :, i])) * TICK_US, 2) for i in range(ns)]
            out["start_to_last_prefetched_step_landed_us"] = stat(ld[:, :, ns] - t[:, :, 0])
    else:
        out["start_to_rows_done_us"] = stat(t[:, :, 1] - t[:, :, 0])
    print(json.dumps({"block_spans": out}))


if __name__ == "__main__":
    main()
