"""KMeans under manhattan distance: the tiled assign of ops/csrc/kmeans_l1.hip on one MI355X.

One ``ops.kmeans.assign`` and one whole ``KMeansRound.run`` + ``finalize`` per (dtype, shape): the
new kernel at every shape (``L1 = "force"``; ``--routed``: ``True``, as shipped) against the generic
route (``L1 = False``: for bf16 an fp32 copy of the matrix per call, then the wave-per-row kernel up
to D = 1024 and the thread-per-row kernel above) in one process, timed new, old, old, new after a
warm-up of both, device events around enough repeats to fill ``--min-s``. An old side whose warm-up
call took longer than ``--slow-ms`` is not timed again: that one call is the record's figure and the
record says so. Each record carries the share of rows on which the two routes' labels agree and
the new assign's pair-elements per second (n·k·D over its slower timing).

``--sweep main``: 1M rows, D in {128, 512, 1024, 2048} x k in {64, 1024} for fp32, bf16 and fp64, and
the reference benchmark's corner 1M x 100, k = 10 in fp32. ``--sweep crossover``: k in {2, 8, 16, 32,
64} x rows in {1,000, 10,000, 100,000} x D in {128, 512, 1024}, the assign alone.
Usage: python scripts/bench_kmeans_l1.py [--sweep main|crossover] [--out FILE] [--shapes dtype:n:D:k,...]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_cosine import DTYPES, make_input  # noqa: E402  (the same inputs as the cosine A/B)
from scripts.bench_kmeans_wide import timed  # noqa: E402  (the same timing loop as the bf16 A/B)


def sweep(which):
    if which == "main":
        return [(dt, 1_000_000, D, k) for dt in ("fp32", "bf16", "fp64") for D in (128, 512, 1024, 2048)
                for k in (64, 1024)] + [("fp32", 1_000_000, 100, 10)]
    return [(dt, n, D, k) for dt in ("fp32", "bf16", "fp64") for n in (1_000, 10_000, 100_000)
            for D in (128, 512, 1024) for k in (2, 8, 16, 32, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", default="main", choices=("main", "crossover"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="dtype:n:D:k,... instead of the sweep")
    ap.add_argument("--routed", action="store_true", help="the new side as shipped (FMLX_KMEANS_L1=1) instead of forced")
    ap.add_argument("--assign-only", action="store_true")
    ap.add_argument("--min-s", type=float, default=None)
    ap.add_argument("--slow-ms", type=float, default=1000.0)
    a = ap.parse_args()
    new_mode = True if a.routed else "force"
    assign_only = a.assign_only or (a.sweep == "crossover" and a.shapes is None)
    min_s = a.min_s if a.min_s is not None else (0.1 if a.sweep == "crossover" else 0.3)
    assert torch.cuda.is_available(), "bench_kmeans_l1.py measures on a GPU"
    from flink_ml_amd.ops import kmeans as kk

    shapes = sweep(a.sweep) if a.shapes is None else [
        (s.split(":")[0],) + tuple(int(v) for v in s.split(":")[1:]) for s in a.shapes.split(",")]
    name = "l1_ab.jsonl" if a.sweep == "main" else "l1_ab_crossover.jsonl"
    path = a.out or os.path.join(ROOT, "profiles", "r26", name)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        for dt, n, D, k in shapes:
            X, C = make_input(dt, n, D, k)
            cb = kk.CentroidBuffers(k, D, X.device, torch.float64 if dt == "fp64" else torch.float32)
            lab = {s: torch.empty(n, dtype=torch.int32, device=X.device) for s in ("new", "old")}

            def assign(side):
                kk.L1 = new_mode if side == "new" else False
                kk.assign(X, cb, "manhattan", lab[side])

            def round_(side, rnd):
                kk.L1 = new_mode if side == "new" else False
                rnd.finalize(cb, rnd.run(cb))

            def measure(sides, rec, what):
                """Warm both sides (timed: a slow old side keeps that single call), then new, old, old, new."""
                warm = {s: round(timed(sides[s], min_s=0.0), 4) for s in sides}
                slow = [s for s in sides if warm[s] > a.slow_ms]
                tm = {s: [] for s in sides if s not in slow}
                for s in ("new", "old", "old", "new"):
                    if s in tm:
                        tm[s].append(round(timed(sides[s], min_s=min_s), 4))
                for s in slow:
                    tm[s] = [warm[s]]
                    rec[what + "_note"] = "%s side: one call (the warm-up), not repeated" % s
                rec[what + "_ms"] = tm
                rec[what + "_new_wins_both_orders"] = max(tm["new"]) < min(tm["old"])

            cb.set(C)
            rec = {"dtype": dt, "n": n, "D": D, "k": k, "new_side": "routed" if a.routed else "force"}
            measure({s: (lambda s=s: assign(s)) for s in ("new", "old")}, rec, "assign")
            rec["labels_agree"] = float((lab["new"] == lab["old"]).double().mean())
            rec["new_pair_elements_per_s"] = float("%.4g" % (n * k * D / (max(rec["assign_ms"]["new"]) * 1e-3)))
            if not assign_only:
                # the rounds move the centroids: every timed round starts from wherever the last one
                # ended (same work per round: the grouping and the sums do not depend on the values)
                rounds = {s: kk.KMeansRound(X, k, "manhattan") for s in ("new", "old")}
                measure({s: (lambda s=s: round_(s, rounds[s])) for s in rounds}, rec, "round")
                del rounds
            kk.L1 = True
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            del X, cb, lab
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
