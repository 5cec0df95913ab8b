"""KNN transform in the fp64 parity mode (ops/csrc/knn_wide_f64.hip) on one MI355X.

One ``KnnModel.transform`` under ``dtype_policy("fp64")`` of 10k queries against 100k training rows
at D in {16, 64, 256, 1024, 4096}, k in {5, 16, 32}, and one shape near the route's floor on
queries x training rows: the fused fp64 MFMA kernel (``FMLX_KNN_F64=force``: every supported shape)
against the route before it (``=0``: a library GEMM block, then the radix selection) in one
process, timed new, old, old, new after a warm-up of both, device events around enough repeats to
fill 0.3 s. Each record carries the share of queries on which the two routes predict the same
label, and the new route's achieved FLOP/s (2·nq·n·D over the whole call's time) with its share of
the fp64 MFMA peak.

One JSON line per shape. Usage: python scripts/bench_knn_f64.py [--out FILE] [--shapes nq:n:D:k,...]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_MFMA_FLOPS = 78.6e12  # MI355X dense fp64 matrix peak
SHAPES = ([(10_000, 100_000, D, k) for D in (16, 64, 256, 1024, 4096) for k in (5, 16, 32)]
          + [(1_024, 2_048, 256, 5)])  # 2^21 pairs


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


def randn_rows(n, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((n, D), dtype=torch.float64, device="cuda")
    for r0 in range(0, n, 1 << 16):
        X[r0:r0 + (1 << 16)] = torch.randn((min(1 << 16, n - r0), D), generator=g, device="cuda", dtype=torch.float64)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="nq:n:D:k,... (default: the documented sweep)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn_f64.py measures on a GPU"
    from flink_ml_amd import Table
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import Knn
    from flink_ml_amd.ops import knn as ko

    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    path = a.out or os.path.join(ROOT, "profiles", "r24", "knn_f64_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    data = {}
    with open(path, "w") as out, dtype_policy("fp64"):
        for nq, n, D, k in shapes:
            if data.get("key") != (nq, n, D):
                data.clear()
                torch.cuda.empty_cache()
                train = Table({"features": randn_rows(n, D, 3),
                               "label": torch.randint(0, 10, (n,), device="cuda").double()})
                data.update(key=(nq, n, D), model=Knn().fit(train), Q=Table({"features": randn_rows(nq, D, 5)}))
                del train
            model = data["model"].set_k(k)
            pred = {}

            def run(side):
                ko.F64 = "force" if side == "new" else "0"
                pred[side] = model.transform(data["Q"])[0].column("prediction")

            for s in ("new", "old"):  # warm
                run(s)
            agree = float((pred["new"] == pred["old"]).double().mean())
            tm = {"new": [], "old": []}
            for s in ("new", "old", "old", "new"):
                tm[s].append(round(timed(lambda: run(s)), 4))
            ko.F64 = "1"
            flops = 2.0 * nq * n * D / (min(tm["new"]) * 1e-3)
            rec = {"nq": nq, "n": n, "D": D, "k": k, "transform_ms": tm, "labels_agree": agree,
                   "new_wins_both_orders": max(tm["new"]) < min(tm["old"]), "new_flops": flops,
                   "new_share_of_fp64_mfma_peak": round(flops / PEAK_FP64_MFMA_FLOPS, 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            # fp64 on both sides: the routes differ in summation order only
            assert agree >= 0.9999, "the two routes predict other labels on %.4f %% of the queries" % (100 - 100 * agree)


if __name__ == "__main__":
    main()
