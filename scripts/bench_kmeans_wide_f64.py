"""KMeans on dense fp64 rows (ops/csrc/kmeans_wide_f64.hip) on one MI355X.

One ``ops.kmeans.assign`` and one whole ``KMeansRound.run`` + ``finalize`` per shape: the wide fp64
kernels at every shape (``FMLX_KMEANS_WIDE=force``; ``=1`` routes by ``ops.kmeans.wide64_route``,
which these measurements set) against the routes before them (``=0``: the wave-per-row kernel up
to D = 1024 and the thread-per-row kernel above; the scalar-load chunk sum on an int64 copy of the
row order) in one process, timed new, old, old, new after a warm-up of both, device events around
enough repeats to fill 0.3 s. Past D = 1024 the old route has no round (its chunk sum refuses the
rows): the new round is reported alone and the record says so. Each record carries the share of
rows on which the two routes' labels agree on the timed input, and the assign's achieved FLOP/s
(2·n·k·D over the whole call) with its share of the fp64 MFMA peak.

Default shapes: 1M rows, D in {128, 512, 1024, 2048} x k in {16, 64, 1024}, then 10,000 and 100,000
rows at D = 512 and 2048. One JSON line per shape.
Usage: python scripts/bench_kmeans_wide_f64.py [--out FILE] [--shapes n:D:k,n:D:k,...] [--routed]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_wide import ab  # noqa: E402  (the same timing loop as the bf16 A/B)

PEAK_FP64_MFMA_FLOPS = 78.6e12  # MI355X dense fp64 matrix peak


def default_shapes():
    big = [(1_000_000, D, k) for D in (128, 512, 1024, 2048) for k in (16, 64, 1024)]
    return big + [(n, D, k) for n in (10_000, 100_000) for D in (512, 2048) for k in (16, 64, 1024)]


def make_input(n, D, k, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((n, D), dtype=torch.float64, device="cuda")
    for r0 in range(0, n, 1 << 16):
        X[r0:r0 + (1 << 16)].normal_(generator=g)
    return X, X[:k].cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="n:D:k,... instead of the default sweep")
    ap.add_argument("--routed", action="store_true",
                    help="the new side as shipped (FMLX_KMEANS_WIDE=1: assign routed by wide64_route) instead of forced")
    a = ap.parse_args()
    new_mode = True if a.routed else "force"
    assert torch.cuda.is_available(), "bench_kmeans_wide_f64.py measures on a GPU"
    from flink_ml_amd.ops import kmeans as kk

    shapes = default_shapes() if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    path = a.out or os.path.join(ROOT, "profiles", "r23", "kmeans_wide_f64_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        for n, D, k in shapes:
            X, C = make_input(n, D, k)
            cb = kk.CentroidBuffers(k, D, X.device, torch.float64)
            lab = {s: torch.empty(n, dtype=torch.int32, device=X.device) for s in ("new", "old")}

            def assign(side):
                kk.WIDE = new_mode if side == "new" else False  # the kernel itself, not assign's routing
                assert kk.mfma_wide_f64_ok(X, "euclidean") == bool(kk.WIDE)
                kk.assign(X, cb, "euclidean", lab[side])

            def round_(side, rnd):
                kk.WIDE = new_mode if side == "new" else False
                rnd.finalize(cb, rnd.run(cb))

            cb.set(C)
            sides = {s: (lambda s=s: assign(s)) for s in ("new", "old")}
            for s in sides:  # warm
                sides[s]()
            agree = float((lab["new"] == lab["old"]).double().mean())
            t_assign = ab(sides)
            rec = {"n": n, "D": D, "k": k, "new_side": "routed" if a.routed else "force", "assign_ms": t_assign,
                   "labels_agree": agree, "assign_new_wins_both_orders": max(t_assign["new"]) < min(t_assign["old"]),
                   "assign_old_over_new": round(min(t_assign["old"]) / max(t_assign["new"]), 2)}
            flops = 2.0 * n * k * D / (min(t_assign["new"]) * 1e-3)
            rec["assign_new_flops"] = flops
            rec["assign_new_share_of_fp64_mfma_peak"] = round(flops / PEAK_FP64_MFMA_FLOPS, 4)
            rounds = {}
            for s in ("new", "old"):
                if s == "old" and D > 1024:
                    rec["round_note"] = "the old route has no round at this width (chunk sum: -3); new alone"
                    continue
                kk.WIDE = new_mode if s == "new" else False
                rnd = kk.KMeansRound(X, k, "euclidean")
                assert a.routed or rnd.wide64 == bool(kk.WIDE)  # routed: wide64_sum_route decides
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
