"""KNN predict on dense fp32 rows wider than 128 (ops/csrc/knn_wide.hip) on one MI355X.

One ``knn_predict`` (distances, top-k, vote) of 10k queries against 100k training rows at
D in {256, 768, 1024, 2048}, k in {5, 16, 64}, and of 100k queries against 1M rows at D = 256, k = 10:
the K-tiled fused kernel (``FMLX_KNN_WIDE=force``: every supported shape) against the routes before
it (``=0``: a library GEMM block, then the top-k scan for k <= 16 or the radix selection above) in
one process, timed new, old, old, new after a warm-up of both, device events around enough repeats
to fill 0.3 s. Each record carries the share of queries on which the two routes predict the same
label, and the new route's achieved FLOP/s (2·nq·n·D over the whole call's time) with its share of
the fp32 MFMA peak.

One JSON line per shape. Usage: python scripts/bench_knn_wide.py [--out FILE] [--shapes nq:n:D:k,...]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_FLOPS = 157.3e12  # MI355X dense fp32 matrix peak
SHAPES = [(10_000, 100_000, D, k) for D in (256, 768, 1024, 2048) for k in (5, 16, 64)] + [(100_000, 1_000_000, 256, 10)]


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
    X = torch.empty((n, D), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 1 << 16):
        X[r0:r0 + (1 << 16)] = torch.randn((min(1 << 16, n - r0), D), generator=g, device="cuda")
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="nq:n:D:k,... (default: the documented sweep)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn_wide.py measures on a GPU"
    from flink_ml_amd.models.knn import knn_predict
    from flink_ml_amd.ops import knn as ko

    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    path = a.out or os.path.join(ROOT, "profiles", "r21", "knn_wide_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    data = {}
    with open(path, "w") as out:
        for nq, n, D, k in shapes:
            if data.get("key") != (nq, n, D):
                data.clear()
                torch.cuda.empty_cache()
                T = randn_rows(n, D, 3)
                data.update(key=(nq, n, D), Q=randn_rows(nq, D, 5), T=T, tn=(T * T).sum(1),
                            lab=torch.randint(0, 10, (n,), device="cuda").double())
                data["classes"] = torch.unique(data["lab"])
            pred = {}

            def run(side):
                ko.WIDE = "force" if side == "new" else "0"
                assert ko.fused_wide_supported(k, n, D, None, data["T"])
                pred[side] = knn_predict(data["Q"], data["T"], data["tn"], data["lab"], k, classes=data["classes"],
                                         Tc=data["T"])

            for s in ("new", "old"):  # warm
                run(s)
            agree = float((pred["new"] == pred["old"]).double().mean())
            tm = {"new": [], "old": []}
            for s in ("new", "old", "old", "new"):
                tm[s].append(round(timed(lambda: run(s)), 4))
            ko.WIDE = "1"
            flops = 2.0 * nq * n * D / (min(tm["new"]) * 1e-3)
            rec = {"nq": nq, "n": n, "D": D, "k": k, "predict_ms": tm, "labels_agree": agree,
                   "new_wins_both_orders": max(tm["new"]) < min(tm["old"]), "new_flops": flops,
                   "new_share_of_fp32_mfma_peak": round(flops / PEAK_FP32_MFMA_FLOPS, 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
