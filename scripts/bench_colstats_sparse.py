"""Column statistics of CSR feature columns (ops/csrc/colstats_csr.hip) on one GPU.

``--part sweep``: the CSR route against the route before it at shapes both hold, 100,000 rows,
D = 1,024 and 16,384, densities 0.1 / 1 / 5 / 20 %, fp32 values:

* ``colstats`` (StandardScaler / MinMaxScaler / VarianceThresholdSelector): ``to_dense`` in fp32 +
  ``column_stats`` against ``column_stats_csr``;
* ``group`` (ANOVATest with 3 classes): ``to_dense`` in fp64 + ``group_colstats`` against
  ``group_colstats_csr``.

Each side is the whole call, its one-time work included (``to_dense``; the column-major copy). Both
are warmed, then timed csr, dense, dense, csr (host clock around calls that end in a device
synchronise), and their sums compared. ``FMLX_COLSTATS_CSR=auto`` takes the CSR route up to the
highest density at which it wins in both orders at both widths (``ops.features.COLSTATS_CSR_CROSSOVER``).

``--part large``: ``StandardScaler.fit`` on 1,000,000 x 262,144 with 64 stored values per row (no
dense form exists: 1 TB in fp32): ms per fit and the peak device memory above the inputs.

One JSON line per measurement. Usage:
python scripts/bench_colstats_sparse.py --part sweep|large [--out FILE] [--n N]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_sparse import once, timed, uniform_csr  # noqa: E402


def strided_csr(n, D, L, seed):
    """Rows of L distinct columns start + i·stride mod D (stride odd), values N(1.5, 1), fp32."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    start = torch.randint(0, D, (n, 1), generator=g, device="cuda")
    stride = torch.randint(0, D // 2, (n, 1), generator=g, device="cuda") * 2 + 1
    idx = ((start + torch.arange(L, device="cuda")[None, :] * stride) % D).to(torch.int32).reshape(-1)
    val = torch.randn(n * L, generator=g, device="cuda") + 1.5
    return SparseColumn(torch.arange(0, n * L + 1, L, dtype=torch.int64, device="cuda"), idx, val, D)


def rel_diff(a, b) -> float:
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def sweep(a, out):
    from flink_ml_amd.ops import features as fo

    n = a.n or 100_000
    for D in [int(s) for s in a.Ds.split(",")]:
        for density in [float(s) for s in a.densities.split(",")]:
            X = uniform_csr(n, D, density, 7)
            nnz = int(X.indices.numel())
            gidx = (torch.arange(n, device="cuda") % 3).to(torch.int32)
            sides = {
                "colstats": (lambda: fo.column_stats_csr(X)["sum"],
                             lambda: fo.column_stats(X.to_dense(torch.float32))["sum"]),
                "group": (lambda: fo.group_colstats_csr(X, gidx, 3)[0],
                          lambda: fo.group_colstats(X.to_dense(torch.float64), gidx, 3)[0]),
            }
            for what, (csr, dense) in sides.items():
                diff = rel_diff(csr(), dense())  # warm, and the same sums
                torch.cuda.synchronize()
                t = {"csr": [], "dense": []}
                for side in ("csr", "dense", "dense", "csr"):
                    t[side].append(round(timed(csr if side == "csr" else dense), 3))
                rec = {"part": "sweep", "what": what, "n": n, "D": D, "density": density, "nnz": nnz, "csr_ms": t["csr"],
                       "dense_ms": t["dense"], "csr_wins_both_orders": max(t["csr"]) < min(t["dense"]),
                       "sums_max_rel_diff": diff}
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del X, sides
            torch.cuda.empty_cache()


def large(a, out):
    from flink_ml_amd import Table
    from flink_ml_amd.models import StandardScaler
    from flink_ml_amd.ops import features as fo

    n, D, L = a.n or 1_000_000, 262_144, 64
    fit = lambda t: StandardScaler().set_input_col("features").fit(t)  # noqa: E731
    fit(Table({"features": strided_csr(1000, D, L, 1)}))  # warm: code objects, the sort's first launches
    X = strided_csr(n, D, L, 11)
    t = Table({"features": X})
    assert fo.csr_stats_route(X, X.values.device)
    torch.cuda.synchronize()
    dev = X.values.device
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = [round(once(lambda: fit(t))[0], 3) for _ in range(3)]
    peak = torch.cuda.max_memory_allocated(dev) - base
    copy_ms = [round(once(lambda: fo._column_major(X))[0], 3) for _ in range(2)]
    rec = {"part": "large", "what": "StandardScaler.fit", "n": n, "D": D, "nnz": int(X.indices.numel()),
           "fit_ms": ms, "column_major_copy_ms": copy_ms, "peak_bytes_above_inputs": int(peak),
           "input_bytes": int(X.indices.numel()) * 8 + (n + 1) * 8, "dense_fp32_bytes": n * D * 4}
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweep", "large"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--Ds", default="1024,16384")
    ap.add_argument("--densities", default="0.001,0.01,0.05,0.2")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_colstats_sparse.py measures on a GPU"
    path = a.out or os.path.join(ROOT, "profiles", "r17", "colstats_csr_%s.jsonl" % a.part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        (sweep if a.part == "sweep" else large)(a, out)


if __name__ == "__main__":
    main()
