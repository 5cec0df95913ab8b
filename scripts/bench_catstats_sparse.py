"""Contingency tables of CSR feature columns (ops/csrc/catstats_csr.hip) on one GPU.

``--part sweep``: the CSR route against the route before it at shapes both hold, 100,000 rows,
D = 1,024 and 16,384, densities 0.1 / 1 / 5 / 20 %, fp32 values 1 … 4 (small counts), 3 labels:

* ``counts``: ``value_label_counts_csr`` against ``to_dense`` in fp64 + ``value_label_counts`` (what
  ``FMLX_COLSTATS_CSR=0`` runs), each with its table brought to the host;
* ``chisq``: ``ChiSqTest.compute`` under ``FMLX_COLSTATS_CSR=1`` against ``=0`` (the host finish is
  the same on both sides).

Both sides are warmed, then timed csr, dense, dense, csr (host clock around calls that end on the
host), and compared. ``FMLX_COLSTATS_CSR=auto`` takes the CSR route up to the highest density at
which it wins in both orders at both widths in both measures (``ops.catstats.CATSTATS_CSR_CROSSOVER``).

``--part large``: ``ChiSqTest.compute`` on 1,000,000 x 262,144 with 64 stored values per row (no
dense form exists: 2.1 TB in fp64): ms per call, the table kernels alone, and the peak device memory
above the inputs.

One JSON line per measurement. Usage:
python scripts/bench_catstats_sparse.py --part sweep|large [--out FILE] [--n N]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_colstats_sparse import strided_csr  # noqa: E402
from scripts.bench_kmeans_sparse import once, timed, uniform_csr  # noqa: E402


def small_counts(X, seed):
    """The column with its values replaced by the counts 1 … 4 (fp32)."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    val = torch.randint(1, 5, (int(X.indices.numel()),), generator=g, device="cuda").float()
    return SparseColumn(X.indptr, X.indices, val, X.size)


def sweep(a, out):
    from flink_ml_amd import Table
    from flink_ml_amd.models import ChiSqTest
    from flink_ml_amd.ops import catstats
    from flink_ml_amd.ops import features as fo

    n, L = a.n or 100_000, 3

    def chisq(t, route):
        fo.COLSTATS_CSR_ROUTE = route
        return ChiSqTest().compute(t)

    for D in [int(s) for s in a.Ds.split(",")]:
        for density in [float(s) for s in a.densities.split(",")]:
            X = small_counts(uniform_csr(n, D, density, 7), 8)
            nnz = int(X.indices.numel())
            y = (torch.arange(n, device="cuda") % L).double()
            li = (torch.arange(n, device="cuda") % L)
            t = Table({"features": X, "label": y})
            sides = {
                "counts": (lambda: catstats.value_label_counts_csr(X, li, L).numpy(),
                           lambda: catstats.value_label_counts(X.to_dense(torch.float64), li, L)),
                "chisq": (lambda: chisq(t, "1"), lambda: chisq(t, "0")),
            }
            for what, (csr, dense) in sides.items():
                r_csr, r_dense = csr(), dense()  # warm, and the same results
                if what == "chisq":
                    same = r_csr == r_dense
                else:
                    cf, _, cnt, _ = r_csr
                    c, _, slots = r_dense
                    same = bool(np.array_equal(np.concatenate([c[j][:, slots[j]].T for j in range(D)]), cnt)) and \
                        cf[-1] == cnt.shape[0]
                del r_csr, r_dense
                tm = {"csr": [], "dense": []}
                for side in ("csr", "dense", "dense", "csr"):
                    tm[side].append(round(timed(csr if side == "csr" else dense), 3))
                rec = {"part": "sweep", "what": what, "n": n, "D": D, "density": density, "nnz": nnz, "csr_ms": tm["csr"],
                       "dense_ms": tm["dense"], "csr_wins_both_orders": max(tm["csr"]) < min(tm["dense"]),
                       "results_equal": bool(same)}
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del X, t, sides
            torch.cuda.empty_cache()


def large(a, out):
    from flink_ml_amd import Table
    from flink_ml_amd.models import ChiSqTest
    from flink_ml_amd.ops import catstats

    n, D, per_row, L = a.n or 1_000_000, 262_144, 64, 3
    warm = small_counts(strided_csr(1000, D, per_row, 1), 2)
    ChiSqTest().compute(Table({"features": warm, "label": (torch.arange(1000, device="cuda") % L).double()}))
    X = small_counts(strided_csr(n, D, per_row, 11), 12)
    y = (torch.arange(n, device="cuda") % L).double()
    t = Table({"features": X, "label": y})
    assert catstats.catstats_csr_route(X, X.values.device)
    torch.cuda.synchronize()
    dev = X.values.device
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = [round(once(lambda: ChiSqTest().compute(t))[0], 3) for _ in range(3)]
    peak = torch.cuda.max_memory_allocated(dev) - base
    li = (torch.arange(n, device="cuda") % L)
    table_ms = [round(once(lambda: catstats.value_label_counts_csr(X, li, L))[0], 3) for _ in range(3)]
    rc = catstats.value_label_counts_csr(X, li, L)
    rec = {"part": "large", "what": "ChiSqTest.compute", "n": n, "D": D, "nnz": int(X.indices.numel()),
           "compute_ms": ms, "table_kernels_ms": table_ms, "table_rows": int(rc.values.numel()),
           "peak_bytes_above_inputs": int(peak), "input_bytes": int(X.indices.numel()) * 8 + (n + 1) * 8,
           "dense_fp64_bytes": n * D * 8}
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
    assert torch.cuda.is_available(), "bench_catstats_sparse.py measures on a GPU"
    path = a.out or os.path.join(ROOT, "profiles", "r18", "catstats_csr_%s.jsonl" % a.part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        (sweep if a.part == "sweep" else large)(a, out)


if __name__ == "__main__":
    main()
