"""KMeans under cosine distance on wide dense rows (the cosine instantiations of
ops/csrc/kmeans_wide.hip, kmeans_wide_f32.hip and kmeans_wide_f64.hip) on one MI355X.

One ``ops.kmeans.assign`` and one whole ``KMeansRound.run`` + ``finalize`` per (dtype, shape): the
wide kernels at every shape (``FMLX_KMEANS_WIDE=force``; ``--routed``: ``=1``, as shipped) against
the routes before them (``=0``: for bf16 an fp32 copy of the matrix per call, then the generic
wave-per-row kernel up to D = 1024 and the thread-per-row kernel above) in one process, timed new,
old, old, new after a warm-up of both, device events around enough repeats to fill 0.3 s. An old
side whose warm-up call took longer than ``--slow-ms`` is not timed again: that one call is the
record's figure and the record says so. Past D = 1024 the old route has no round (its chunk sum
refuses the rows): the new round is reported alone. Each record carries the share of rows on which
the two routes' labels agree on the timed input.

Default shapes: 1M rows, D in {256, 512, 1024, 2048} x k in {64, 1024} for bf16, fp32 and fp64, bf16
also at D = 64 and 128. One JSON line per (dtype, shape).
Usage: python scripts/bench_kmeans_cosine.py [--out FILE] [--shapes dtype:n:D:k,...] [--routed] [--metric M]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_wide import ab, timed  # noqa: E402  (the same timing loop as the bf16 A/B)

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp64": torch.float64}


def default_shapes():
    out = [("bf16", 1_000_000, D, k) for D in (64, 128) for k in (64, 1024)]
    return out + [(dt, 1_000_000, D, k) for dt in DTYPES for D in (256, 512, 1024, 2048) for k in (64, 1024)]


def make_input(dt, n, D, k, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((n, D), dtype=DTYPES[dt], device="cuda")
    for r0 in range(0, n, 1 << 16):
        X[r0:r0 + (1 << 16)] = torch.randn((min(1 << 16, n - r0), D), generator=g, device="cuda").to(DTYPES[dt])
    return X, X[:k].double().cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="dtype:n:D:k,... instead of the default sweep")
    ap.add_argument("--routed", action="store_true", help="the new side as shipped (FMLX_KMEANS_WIDE=1) instead of forced")
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--slow-ms", type=float, default=1000.0)
    a = ap.parse_args()
    new_mode = True if a.routed else "force"
    assert torch.cuda.is_available(), "bench_kmeans_cosine.py measures on a GPU"
    from flink_ml_amd.ops import kmeans as kk

    shapes = default_shapes() if a.shapes is None else [
        (s.split(":")[0],) + tuple(int(v) for v in s.split(":")[1:]) for s in a.shapes.split(",")]
    path = a.out or os.path.join(ROOT, "profiles", "r25", "kmeans_cosine_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        for dt, n, D, k in shapes:
            X, C = make_input(dt, n, D, k)
            cb = kk.CentroidBuffers(k, D, X.device, torch.float64 if dt == "fp64" else torch.float32)
            lab = {s: torch.empty(n, dtype=torch.int32, device=X.device) for s in ("new", "old")}

            def assign(side):
                kk.WIDE = new_mode if side == "new" else False
                kk.assign(X, cb, a.metric, lab[side])

            def round_(side, rnd):
                kk.WIDE = new_mode if side == "new" else False
                rnd.finalize(cb, rnd.run(cb))

            def measure(sides, rec, what):
                """Warm both sides (timed: a slow old side keeps that single call), then the A/B."""
                warm = {s: round(timed(sides[s], min_s=0.0), 4) for s in sides}
                slow = [s for s in sides if warm[s] > a.slow_ms]
                tm = ab({s: f for s, f in sides.items() if s not in slow})
                for s in slow:
                    tm[s] = [warm[s]]
                    rec[what + "_note"] = "%s side: one call (the warm-up), not repeated" % s
                rec[what + "_ms"] = tm
                if "old" in tm:
                    rec[what + "_new_wins_both_orders"] = max(tm["new"]) < min(tm["old"])

            cb.set(C)
            rec = {"dtype": dt, "n": n, "D": D, "k": k, "metric": a.metric, "new_side": "routed" if a.routed else "force"}
            measure({s: (lambda s=s: assign(s)) for s in ("new", "old")}, rec, "assign")
            rec["labels_agree"] = float((lab["new"] == lab["old"]).double().mean())
            rounds = {}
            for s in ("new", "old"):
                if s == "old" and D > 1024:
                    rec["round_note"] = "the old route has no round at this width (chunk sum: -3); new alone"
                    continue
                kk.WIDE = new_mode if s == "new" else False
                rnd = kk.KMeansRound(X, k, a.metric)
                rounds[s] = (lambda s=s, rnd=rnd: round_(s, rnd))
            # the rounds move the centroids: every timed round starts from wherever the last one
            # ended (same work per round: the grouping and the sums do not depend on the values)
            measure(rounds, rec, "round")
            kk.WIDE = True
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            del X, cb, lab, rounds
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
