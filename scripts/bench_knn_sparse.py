"""Knn on CSR feature columns (ops/csrc/knn_csr.hip) on one GPU.

``--part sweep``: ``KnnModel.transform`` on the CSR route (``FMLX_KNN_CSR=1``) against the route
that densifies (``=0``: the training set as a dense matrix, a library GEMM per query block) at a
shape both hold: 100,000 training rows x 4,096 columns, 1,024 queries of the same density, fp32,
densities 0.1 / 1 / 5 / 20 %, k = 5 (the top-k scan kernel) and k = 100 (the radix-select kernel).
Both models are fitted and warmed (their states, the column-major copy and the dense matrix, are
one-time costs reported beside the timings), then timed csr, dense, dense, csr (host clock around
calls that end on the host) and their predictions compared. ``FMLX_KNN_CSR=auto`` takes the CSR
route up to the highest density at which it wins in both orders at both k
(``ops.knn.CSR_CROSSOVER``).

``--part large``: the CSR route alone at HashingTF's width, 100,000 training rows x 262,144 and
10,000 queries of about 100 draws per row with Zipf(1.1) columns (a row's duplicate draws removed),
k = 5 and 100: ms per transform, the products kernel and the selection kernel alone over the same
query blocks, the one-time costs and the peak device memory. No dense form exists there (105 GB in
fp32).

``--tile``: the products kernel's tile (one of ``ops.knn.CSR_TILE_ROWS_BUILT``), for the products
timing of ``--part large``.

One JSON line per measurement. Usage:
python scripts/bench_knn_sparse.py --part sweep|large [--out FILE] [--n N] [--nq NQ] [--ks 5,100]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_kmeans_sparse import once, timed, uniform_csr, zipf_csr  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def fitted(X, y, route):
    """(model with its state built, fit ms, state ms) under ``FMLX_KNN_CSR=route``."""
    from flink_ml_amd import Table
    from flink_ml_amd.models.knn import Knn
    from flink_ml_amd.ops import knn as knn_ops

    knn_ops.CSR_ROUTE = route
    fit_ms, model = once(lambda: Knn().fit(Table({"features": X, "label": y})))
    state_ms, _ = once(model._model_state)
    return model, fit_ms, state_ms


def predict(model, t, k, route):
    from flink_ml_amd.ops import knn as knn_ops

    knn_ops.CSR_ROUTE = route
    return model.set_k(k).transform(t)[0].column("prediction").cpu()


def sweep(a, out):
    from flink_ml_amd import Table
    from flink_ml_amd.models import knn as mknn

    n, nq, D = a.n or 100_000, a.nq or 1024, a.D
    for density in [float(s) for s in a.densities.split(",")]:
        X, Q = uniform_csr(n, D, density, 7), uniform_csr(nq, D, density, 8)
        y = (torch.arange(n, device="cuda") % 7).double()
        t = Table({"features": Q})
        csr, fit_csr, state_csr = fitted(X, y, "1")
        dense, fit_dense, state_dense = fitted(X, y, "0")
        assert isinstance(csr._model_state(), mknn._CsrState) and not isinstance(dense._model_state(), mknn._CsrState)
        for k in [int(s) for s in a.ks.split(",")]:
            sides = {"csr": lambda: predict(csr, t, k, "1"), "dense": lambda: predict(dense, t, k, "0")}
            p_csr, p_dense = sides["csr"](), sides["dense"]()  # warm
            agree = float((p_csr == p_dense).double().mean())  # (fp32 products in two orders: near ties may differ)
            tm = {"csr": [], "dense": []}
            for side in ("csr", "dense", "dense", "csr"):
                tm[side].append(round(timed(sides[side], max_reps=10), 3))
            emit(out, {"part": "sweep", "n": n, "nq": nq, "D": D, "density": density, "nnz": int(X.indices.numel()),
                       "k": k, "csr_ms": tm["csr"], "dense_ms": tm["dense"],
                       "csr_wins_both_orders": max(tm["csr"]) < min(tm["dense"]), "predictions_agree": agree,
                       "one_time_ms": {"csr_fit": round(fit_csr, 1), "csr_state": round(state_csr, 1),
                                       "dense_fit": round(fit_dense, 1), "dense_state": round(state_dense, 1)}})
        del X, Q, t, csr, dense, sides
        torch.cuda.empty_cache()


def large(a, out):
    from flink_ml_amd import Table
    from flink_ml_amd.models import knn as mknn
    from flink_ml_amd.ops import knn as knn_ops
    from flink_ml_amd.ops.csr import csr_arrays
    from flink_ml_amd.table import SparseColumn

    n, nq, D, draws = a.n or 100_000, a.nq or 10_000, 262_144, 100
    warm, _, _ = fitted(zipf_csr(1000, D, draws, 1), (torch.arange(1000, device="cuda") % 7).double(), "1")
    predict(warm, Table({"features": zipf_csr(100, D, draws, 2)}), 5, "1")
    X, Q = zipf_csr(n, D, draws, 11), zipf_csr(nq, D, draws, 12)
    y = (torch.arange(n, device="cuda") % 7).double()
    t = Table({"features": Q})
    dev = X.values.device
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    model, fit_ms, state_ms = fitted(X, y, "1")
    st = model._model_state()
    assert isinstance(st, mknn._CsrState)
    cm, tn = st.cm, st.tnorm
    Qk = SparseColumn(*csr_arrays(Q, cm.acc), D)
    qn = knn_ops.csr_sqnorm(Qk, cm.acc)
    for k in [int(s) for s in a.ks.split(",")]:
        ms = [round(once(lambda: predict(model, t, k, "1"))[0], 3) for _ in range(3)]
        if k <= knn_ops.ROUTE_MAX_K:
            qb, select = knn_ops.query_block(n), knn_ops.topk_from_products
        else:
            qb, select = knn_ops.select_query_block(n, tn.element_size()), knn_ops.select_topk
        G = torch.empty((min(qb, nq), n), dtype=cm.acc, device=dev)
        blocks = [(s, min(nq, s + qb)) for s in range(0, nq, qb)]
        tile = a.tile or knn_ops.CSR_TILE_ROWS[cm.acc]
        prod = [round(once(lambda: [knn_ops.csr_products(Qk, cm, s, e, out=G[:e - s], tile=tile) for s, e in blocks])[0], 3)
                for _ in range(3)]
        sel = [round(once(lambda: [select(G[:e - s], qn[s:e], tn, k) for s, e in blocks])[0], 3) for _ in range(3)]
        peak = torch.cuda.max_memory_allocated(dev) - base
        emit(out, {"part": "large", "n": n, "nq": nq, "D": D, "train_nnz": int(X.indices.numel()),
                   "query_nnz": int(Q.indices.numel()), "longest_column": int((cm.colptr[1:] - cm.colptr[:-1]).max()),
                   "k": k, "query_block": qb, "tile_rows": tile, "transform_ms": ms, "products_ms": prod,
                   "selection_ms": sel, "fit_ms": round(fit_ms, 1), "column_major_ms": round(state_ms, 1),
                   "peak_bytes_above_inputs": int(peak), "dense_fp32_bytes": n * D * 4})
        del G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweep", "large"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--nq", type=int, default=0)
    ap.add_argument("--D", type=int, default=4096)
    ap.add_argument("--ks", default="5,100")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--densities", default="0.001,0.01,0.05,0.2")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn_sparse.py measures on a GPU"
    path = a.out or os.path.join(ROOT, "profiles", "r19", "knn_csr_%s.jsonl" % a.part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        (sweep if a.part == "sweep" else large)(a, out)


if __name__ == "__main__":
    main()
