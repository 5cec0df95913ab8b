"""KMeans on CSR feature columns (ops/csrc/kmeans_csr.hip) on one GPU.

``--part sweep``: the CSR round against the round on the densified matrix (``FMLX_KMEANS_CSR=0``:
the path before the CSR kernels) at a shape both hold, 100,000 x 16,384 fp32, k = 10 and 100,
densities 0.1 / 1 / 5 / 20 %. A round is ``run`` + ``finalize`` of the round object ``kmeans_lloyd``
drives (one rank: no all-reduce); where the dense round does not take the width (its row sums hold
at most 1,024 columns) the two assigns are compared instead (``"what": "assign"``; ``--D 1024`` is
the widest shape whose whole rounds compare). Both rounds are warmed, then timed csr, dense, dense, csr (host
clock around calls that end in a device synchronise). The one-time costs (the column-major copy of
the CSR round, ``to_dense`` of the dense one) are reported beside them. ``FMLX_KMEANS_CSR=auto``
takes the CSR path below the highest density at which it wins in both orders
(``ops.kmeans.CSR_CROSSOVER``).

``--part large``: the CSR path alone at 1,000,000 x 262,144, about 100 entries per row with
Zipf(1.1) columns (a row's duplicate draws removed), k = 10 and 100: ms per round and the split
assign / column sums / finalize (device events around each launcher, in a run of their own), with
the bytes each must move.

One JSON line per measurement. Usage:
python scripts/bench_kmeans_sparse.py --part sweep|large [--out FILE] [--n N] [--ks 10,100]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, min_s=0.3, max_reps=20):
    """ms per call: one call, then as many as fill ``min_s`` (the clock is the host's)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    reps = min(max_reps, int(min_s / max(first, 1e-6)))
    if reps < 2:
        return first * 1e3
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def uniform_csr(n, D, density, seed):
    """A SparseColumn of the given density (uniform columns, values U(0.5, 1.5), fp32)."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    idx, step = [], max(1, (1 << 28) // D)
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        r, c = torch.nonzero(torch.rand((m, D), generator=g, device="cuda") < density, as_tuple=True)
        ptr[r0 + 1:r0 + m + 1] = torch.bincount(r, minlength=m)
        idx.append(c.to(torch.int32))
    ptr = torch.cumsum(ptr, 0)
    idx = torch.cat(idx)
    val = torch.rand(idx.numel(), generator=g, device="cuda") + 0.5
    return SparseColumn(ptr, idx, val, D)


def zipf_csr(n, D, draws, seed):
    """Rows of ``draws`` Zipf(1.1)-like columns min(floor(u^-10) - 1, D - 1) (the continuous
    approximation of the Zipf tail), duplicates within a row removed."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)
    ptrs, idx, step = [torch.zeros(1, dtype=torch.int64, device="cuda")], [], 1 << 18
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        u = torch.rand((m, draws), generator=g, device="cuda", dtype=torch.float64).clamp_min(1e-12)
        cols = torch.clamp(torch.floor(u ** -10.0) - 1, max=D - 1).to(torch.int64)
        cols = torch.sort(cols, dim=1).values
        keep = torch.ones_like(cols, dtype=torch.bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
        ptrs.append(keep.sum(1))
        idx.append(cols[keep].to(torch.int32))
    ptr = torch.cumsum(torch.cat(ptrs), 0)
    idx = torch.cat(idx)
    val = torch.rand(idx.numel(), generator=g, device="cuda") + 0.5
    return SparseColumn(ptr, idx, val, D)


def init_rows(X, k):
    """The first k rows, dense fp64 on the host."""
    C = torch.zeros(k, X.size, dtype=torch.float64)
    ptr = X.indptr[: k + 1].cpu()
    for i in range(k):
        s, e = int(ptr[i]), int(ptr[i + 1])
        C[i, X.indices[s:e].cpu().long()] = X.values[s:e].cpu().double()
    return C


def sweep(a, out):
    from flink_ml_amd.ops import kmeans as kk

    n, D = a.n or 100_000, a.D
    for density in [float(s) for s in a.densities.split(",")]:
        X = uniform_csr(n, D, density, 7)
        nnz = int(X.indices.numel())
        dense_ms, Xd = once(lambda: X.to_dense(torch.float32))
        for k in [int(s) for s in a.ks.split(",")]:
            C = init_rows(X, k)
            cbs = kk.SparseCentroidBuffers(k, D, X.device, torch.float32)
            cbd = kk.CentroidBuffers(k, D, X.device, torch.float32)
            copy_ms, rs = once(lambda: kk.SparseKMeansRound(X, k, "euclidean"))
            rd = kk.KMeansRound(Xd, k, "euclidean")

            what = "round"
            try:  # the dense round sums rows of at most 1,024 columns: wider, only the assign compares
                rd.run(cbd)
                torch.cuda.synchronize()
            except RuntimeError:
                what = "assign"

            def csr():
                cbs.set(C)
                if what == "assign":
                    kk.assign_csr(rs.X, cbs, "euclidean", rs.labels)
                else:
                    rs.finalize(cbs, rs.run(cbs))

            def dense():
                cbd.set(C)
                if what == "assign":
                    kk.assign(Xd, cbd, "euclidean", rd.labels)
                else:
                    rd.finalize(cbd, rd.run(cbd))

            def sets():
                cbs.set(C)
                cbd.set(C)

            csr(), dense()  # warm
            torch.cuda.synchronize()
            same = float((rs.labels == rd.labels).double().mean())
            set_ms = timed(sets) / 2  # the host-side centroid reset inside every timed call
            t = {"csr": [], "dense": []}
            for side in ("csr", "dense", "dense", "csr"):
                t[side].append(round(timed(csr if side == "csr" else dense), 3))
            rec = {"part": "sweep", "what": what, "n": n, "D": D, "k": k, "density": density, "nnz": nnz, "csr_ms": t["csr"],
                   "dense_ms": t["dense"], "centroid_reset_ms_each": round(set_ms, 3),
                   "csr_wins_both_orders": max(t["csr"]) < min(t["dense"]), "labels_equal_frac": same,
                   "column_major_copy_ms": round(copy_ms, 3), "to_dense_ms": round(dense_ms, 3)}
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            del rs, rd, cbs, cbd
        del X, Xd
        torch.cuda.empty_cache()


def large(a, out):
    from flink_ml_amd.ops import kmeans as kk

    n, D = a.n or 1_000_000, 262_144
    X = zipf_csr(n, D, a.draws, 11)
    nnz = int(X.indices.numel())
    col = torch.bincount(X.indices.long(), minlength=D)
    for k in [int(s) for s in a.ks.split(",")]:
        C = init_rows(X, k)
        cb = kk.SparseCentroidBuffers(k, D, X.device, torch.float32)
        cb.set(C)
        copy_ms, rnd = once(lambda: kk.SparseKMeansRound(X, k, "euclidean"))

        def one():
            rnd.finalize(cb, rnd.run(cb))

        one()
        cb.set(C)
        round_ms = [round(timed(one, max_reps=10), 3) for _ in range(2)]
        cb.set(C)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        split = []
        for _ in range(5):
            ev[0].record()
            kk.assign_csr(rnd.X, cb, "euclidean", rnd.labels)
            ev[1].record()
            rnd.colsum()
            ev[2].record()
            rnd.finalize(cb, rnd.payload)
            ev[3].record()
            torch.cuda.synchronize()
            split.append([round(ev[i].elapsed_time(ev[i + 1]), 3) for i in range(3)])
        kp, es = cb.kp, 4
        rec = {"part": "large", "n": n, "D": D, "k": k, "kp": kp, "nnz": nnz, "nnz_per_row": round(nnz / n, 1),
               "longest_column": int(col.max()), "long_columns": rnd.nlong, "segments": rnd.nsegs,
               "round_ms": round_ms, "assign_colsum_finalize_ms": split, "column_major_copy_ms": round(copy_ms, 3),
               # what each kernel must move: the gathered image rows + its streams
               "assign_bytes": nnz * kp * es + nnz * (4 + es) + n * (8 + 4),
               "colsum_bytes": nnz * (4 + es + 4) + D * kp * es + n * 4,
               "finalize_bytes": 2 * D * kp * es}
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        del rnd, cb
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweep", "large"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--densities", default="0.001,0.01,0.05,0.2")
    ap.add_argument("--D", type=int, default=16_384, help="width of the sweep")
    ap.add_argument("--draws", type=int, default=150, help="Zipf draws per row before duplicates are removed")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kmeans_sparse.py measures on a GPU"
    path = a.out or os.path.join(ROOT, "profiles", "r12", "kmeans_csr_%s.jsonl" % a.part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        (sweep if a.part == "sweep" else large)(a, out)


if __name__ == "__main__":
    main()
