"""Interaction with sparse inputs on one GPU: the CSR route (ops/csrc/interaction_csr.hip,
``FMLX_INTERACTION_CSR=1``) against the route that densifies the inputs, crosses them into a dense
fp64 [n, Π D_c] matrix and turns it back into CSR (``=0``).

``--part shapes``: ``Interaction.transform`` on one-hot(100) × one-hot(100) and one-hot(1000) ×
one-hot(1000) at 1M rows and dense(16) × sparse(4096, 32 stored) at 100,000 rows. A shape whose
dense route fails (its intermediate does not fit) records the failure instead of a time.

``--part sweep``: 100,000 rows of sparse(64) × sparse(64), both columns at the same density, so
the output's density is its square; ``FMLX_INTERACTION_CSR=auto`` takes the CSR route up to the
highest output density at which it wins in both run orders (``ops.blas.INTERACTION_CSR_CROSSOVER``).

Each shape is warmed on both routes, then timed csr, dense, dense, csr (host clock around calls
that end on the host), and the two results' dense images compared where both exist. One JSON line
per shape. Usage: python scripts/bench_interaction_sparse.py --part shapes|sweep [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_sparse import timed, uniform_csr  # noqa: E402


def onehot(n, D, seed):
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.randint(0, D, (n,), generator=g, device="cuda", dtype=torch.int32)
    return SparseColumn(torch.arange(n + 1, device="cuda"), idx, torch.ones(n, device="cuda"), D)


def fixed_csr(n, D, k, seed):
    """n rows of k distinct sorted columns each, values U(0.5, 1.5) fp32."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.rand((n, D), generator=g, device="cuda").topk(k, dim=1).indices.sort(dim=1).values
    val = torch.rand(n * k, generator=g, device="cuda") + 0.5
    return SparseColumn(torch.arange(n + 1, device="cuda") * k, idx.reshape(-1).to(torch.int32), val, D)


def transform(cols, route):
    from flink_ml_amd import Table
    from flink_ml_amd.models.feature import Interaction
    from flink_ml_amd.ops import blas

    blas.INTERACTION_CSR_ROUTE = route
    names = ["c%d" % i for i in range(len(cols))]
    out = Interaction().set_input_cols(*names).set_output_col("out").transform(Table(dict(zip(names, cols))))[0]
    return out.column("out")


def measure(name, cols, check_dense=True):
    n = len(cols[0]) if not isinstance(cols[0], torch.Tensor) else cols[0].shape[0]
    sides = {"csr": lambda: transform(cols, "1"), "dense": lambda: transform(cols, "0")}
    got = sides["csr"]()  # warm
    rec = {"shape": name, "n": n, "size": got.size, "entries": int(got.values.numel()),
           "density": got.values.numel() / (n * got.size), "dense_intermediate_bytes": n * got.size * 8}
    try:
        want = sides["dense"]()
        if check_dense:
            rec["same_dense_image"] = bool(torch.equal(got.to_dense(), want.to_dense()))
        del want
    except Exception as e:  # the intermediate does not fit (torch.OutOfMemoryError), or a torch limit on its size
        rec["dense_failure"] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
    del got
    torch.cuda.empty_cache()
    tm = {"csr": [], "dense": []}
    for side in ("csr", "dense", "dense", "csr"):
        if side == "csr" or "dense_failure" not in rec:
            tm[side].append(round(timed(sides[side], max_reps=10), 3))
    rec.update(csr_ms=tm["csr"], dense_ms=tm["dense"],
               csr_wins_both_orders=bool(tm["dense"]) and max(tm["csr"]) < min(tm["dense"]))
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["shapes", "sweep"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--densities", default="0.05,0.1,0.2,0.3,0.5,0.7,0.85,1.0")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_interaction_sparse.py measures on a GPU"
    path = a.out or os.path.join(ROOT, "profiles", "r27", "interaction_csr_%s.jsonl" % a.part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        if a.part == "shapes":
            n = a.n or 1_000_000
            jobs = [("onehot100_x_onehot100", lambda: [onehot(n, 100, 1), onehot(n, 100, 2)], False),
                    ("onehot1000_x_onehot1000", lambda: [onehot(n, 1000, 3), onehot(n, 1000, 4)], False),
                    ("dense16_x_sparse4096_32", lambda: [torch.rand((n // 10, 16), device="cuda") + 0.5,
                                                         fixed_csr(n // 10, 4096, 32, 5)], False)]
        else:
            n = a.n or 100_000
            jobs = [("sparse64_x_sparse64_d%g" % d, lambda d=d: [uniform_csr(n, 64, d, 6), uniform_csr(n, 64, d, 7)],
                     True) for d in [float(s) for s in a.densities.split(",")]]
        for name, make, check in jobs:
            line = json.dumps(measure(name, make(), check))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
