"""KMeans on dense bf16 rows wider than 256 (ops/csrc/kmeans_wide.hip) on one MI355X.

One ``ops.kmeans.assign`` and one whole ``KMeansRound.run`` + ``finalize`` at n = 1M rows,
D in {512, 768, 1024, 2048}, k in {64, 1024}: the wide kernels (``FMLX_KMEANS_WIDE=1``) against the
route before them (``=0``: an fp32 copy of the matrix and the wave-per-row assign) in one process,
timed new, old, old, new after a warm-up of both, device events around enough repeats to fill
0.3 s. At D = 2048 the old route has no round (its chunk sum refuses rows wider than 1024): the
assign alone is compared there and the record says so. Each record carries the share of rows on
which the two routes' labels agree on the timed input, and the assign's achieved FLOP/s
(2·n·k·D over its time: the one kernel of the new route's assign) with its share of the bf16 MFMA
peak.

One JSON line per shape. Usage: python scripts/bench_kmeans_wide.py [--out FILE] [--n N] [--Ds ...] [--ks ...]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_FLOPS = 2.5e15  # MI355X dense bf16 matrix peak


def timed(fn, min_s=0.3, max_reps=50):
    """ms per call between device events: one call, then as many as fill ``min_s``."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    first = ev[0].elapsed_time(ev[1])
    reps = min(max_reps, int(min_s * 1e3 / max(first, 1e-3)))
    if reps < 2:
        return first
    ev[2].record()
    for _ in range(reps):
        fn()
    ev[3].record()
    ev[3].synchronize()
    return ev[2].elapsed_time(ev[3]) / reps


def make_input(n, D, k, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((n, D), dtype=torch.bfloat16, device="cuda")
    for r0 in range(0, n, 1 << 16):
        X[r0:r0 + (1 << 16)] = torch.randn((min(1 << 16, n - r0), D), generator=g, device="cuda").to(torch.bfloat16)
    return X, X[:k].double().cpu()


def ab(sides):
    """{side: [ms, ms]} timed new, old, old, new (both warmed by the caller)."""
    tm = {s: [] for s in sides}
    for s in ("new", "old", "old", "new"):
        if s in sides:
            tm[s].append(round(timed(sides[s]), 4))
    return tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--Ds", default="512,768,1024,2048")
    ap.add_argument("--ks", default="64,1024")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kmeans_wide.py measures on a GPU"
    from flink_ml_amd.ops import kmeans as kk

    path = a.out or os.path.join(ROOT, "profiles", "r20", "kmeans_wide_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    n = a.n
    with open(path, "w") as out:
        for D in [int(s) for s in a.Ds.split(",")]:
            for k in [int(s) for s in a.ks.split(",")]:
                X, C = make_input(n, D, k)
                cb = kk.CentroidBuffers(k, D, X.device, torch.float32)
                lab = {s: torch.empty(n, dtype=torch.int32, device=X.device) for s in ("new", "old")}

                def assign(side):
                    kk.WIDE = side == "new"
                    assert kk.mfma_wide_ok(X, "euclidean") == kk.WIDE
                    kk.assign(X, cb, "euclidean", lab[side])

                def round_(side, rnd):
                    kk.WIDE = side == "new"
                    rnd.finalize(cb, rnd.run(cb))

                cb.set(C)
                sides = {s: (lambda s=s: assign(s)) for s in ("new", "old")}
                for s in sides:  # warm
                    sides[s]()
                agree = float((lab["new"] == lab["old"]).double().mean())
                t_assign = ab(sides)
                rec = {"n": n, "D": D, "k": k, "assign_ms": t_assign, "labels_agree": agree,
                       "assign_new_wins_both_orders": max(t_assign["new"]) < min(t_assign["old"])}
                flops = 2.0 * n * k * D / (min(t_assign["new"]) * 1e-3)
                rec["assign_new_flops"] = flops
                rec["assign_new_share_of_bf16_mfma_peak"] = round(flops / PEAK_BF16_FLOPS, 4)
                rounds = {}
                for s in ("new", "old"):
                    if s == "old" and D > 1024:
                        rec["round_note"] = "the old route has no round at this width (chunk sum: -3); assign only"
                        continue
                    kk.WIDE = s == "new"
                    rnd = kk.KMeansRound(X, k, "euclidean")
                    rounds[s] = (lambda s=s, rnd=rnd: round_(s, rnd))
                # the rounds move the centroids: every timed round starts from wherever the last one
                # ended (same work per round: the grouping and the sums do not depend on the values)
                for s in rounds:
                    rounds[s]()
                t_round = ab(rounds)
                rec["round_ms"] = t_round
                if "old" in rounds:
                    rec["round_new_wins_both_orders"] = max(t_round["new"]) < min(t_round["old"])
                kk.WIDE = True
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                del X, cb, lab, rounds, sides
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
