"""Bindings for ``csrc/knn.hip``: KNN predict's distances + per-query top-k (K13).

Two device paths, both with ``KnnModel.predictLabel`` (reference ``KnnModel.java:154-194``)
semantics — the k nearest training points per query, nearest first, ties to the lower index:

* ``fused_topk(Q, pack, k)`` (D ≤ 128, k ≤ 64): ONE kernel computes the distances on the fp32
  matrix cores and keeps the top-k in registers; the nq×n distance block never reaches HBM.
  ``TrainPack`` is the training matrix pre-arranged once per model for the kernel's tile copy.
* ``topk_from_products(G, qn, tn, k)`` (any D, k ≤ 32): takes an fp32 product block
  ``G = Q·Tᵀ`` from a library GEMM and scans it once (the fallback for D > 128).

``csr_products(Q, cm, q0, q1)`` (``csrc/knn_csr.hip``) forms that product block from two CSR
operands instead, a block of query rows and the training set's column-major copy, for sparse
feature columns that are not densified (``csr_route``, ``FMLX_KNN_CSR``).
"""
from __future__ import annotations

import os

import torch

from . import native

FUSED_MAX_K = 64
FUSED_MAX_D = 128
# the shortest training segment worth a block (in 64-row tiles) and the most segments tried
FUSED_MIN_TILES = 16
FUSED_MAX_SEGMENTS = 64
_SLOTS = {}


def _slots(k: int, dp: int, device) -> int:
    """Fused-kernel blocks resident at once on the device (occupancy × CUs)."""
    key = (k, dp, str(device))
    if key not in _SLOTS:
        per_cu = native.kernels().fmlx_knn_fused_blocks_per_cu(k, dp)
        _SLOTS[key] = max(1, per_cu) * torch.cuda.get_device_properties(device).multi_processor_count
    return _SLOTS[key]


def fused_supported(k: int, n: int, d: int, device) -> bool:
    return (torch.device(device).type == "cuda" and 1 <= k <= FUSED_MAX_K and k <= n < 2 ** 31 - 128
            and 1 <= d <= FUSED_MAX_D)


class TrainPack:
    """Training points as the fused kernel's LDS image, one block of floats per 64-row tile
    (built once per model, on the device): ``[sub 2][h 2][r 32][dp + 4]`` with
    ``T[64·t + 32·sub + r][2·s + h]`` at ``s`` (zero padded: D to 2·dp, dp = ceil(D/2) rounded up
    to 4, and 4 pad columns that keep the kernel's LDS reads conflict-free), then the tile's 64
    squared norms in a 256-float block, so the kernel stages a tile with plain 1-KiB LDS-DMA copies."""

    def __init__(self, T: torch.Tensor, tnorm: torch.Tensor):
        n, d = T.shape
        self.n, self.d = int(n), int(d)
        self.dp = -(-(-(-d // 2)) // 4) * 4
        self.nt = -(-n // 64)
        dev = T.device
        self.Tt = torch.zeros((self.nt, 128 * (self.dp + 4) + 256), dtype=torch.float32, device=dev)
        self._Tp = torch.zeros((self.nt * 64, 2 * self.dp), dtype=torch.float32, device=dev)
        self._tn = torch.zeros(self.nt * 64, dtype=torch.float32, device=dev)
        self.refresh(T, tnorm)

    def refresh(self, T: torch.Tensor, tnorm: torch.Tensor) -> "TrainPack":
        """Re-fills the pack in place from new values of the same shape (device copies only, so
        it can run inside a captured graph — KMeans re-packs its centroids every round)."""
        nt, dp, n, d = self.nt, self.dp, self.n, self.d
        self._Tp[:n, :d].copy_(T)
        rows = self.Tt[:, :128 * (dp + 4)].view(nt, 2, 2, 32, dp + 4)
        rows[..., :dp].copy_(self._Tp.view(nt, 2, 32, dp, 2).permute(0, 1, 4, 2, 3))
        self._tn[:n].copy_(tnorm)
        self.Tt[:, 128 * (dp + 4):128 * (dp + 4) + 64].copy_(self._tn.view(nt, 64))
        return self


def fused_segments(nq: int, n: int, k: int, slots: int) -> int:
    """Training segments per query block. Cost model in tile units: the blocks run in
    ceil(blocks / slots) rounds of (tiles per segment + a list fill of ~1 + k/16 tiles); a bad
    split strands a mostly empty last round (782 query blocks × 2 segments on 512 slots ran 4
    rounds for 3.05 rounds of work), so every S up to the cap is scored and the cheapest wins."""
    bq = -(-nq // 128)
    nt = -(-n // 64)
    smax = int(max(1, min(FUSED_MAX_SEGMENTS, nt // FUSED_MIN_TILES, 256)))
    fill = 1.0 + k / 16.0
    best, best_cost = 1, None
    for S in range(1, smax + 1):
        cost = -(-(bq * S) // slots) * (-(-nt // S) + fill)
        if best_cost is None or cost < best_cost * 0.995:
            best, best_cost = S, cost
    return best


def fused_topk(Q: torch.Tensor, pack: "TrainPack", k: int, with_dist: bool = False, segments: int = 0):
    """k nearest training points of every row of ``Q`` [nq, D] (fp32) in one fused kernel."""
    nq, d = Q.shape
    if Q.dtype != torch.float32 or d != pack.d or not fused_supported(k, pack.n, d, Q.device):
        raise ValueError("knn fused: bad inputs Q=%s %s, D=%d, n=%d, k=%d" % (tuple(Q.shape), Q.dtype, pack.d,
                                                                              pack.n, k))
    if Q.stride(1) != 1:
        Q = Q.contiguous()
    S = int(segments) or fused_segments(nq, pack.n, k, _slots(k, pack.dp, Q.device))
    idx = torch.empty((nq, k), dtype=torch.int32, device=Q.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=Q.device) if with_dist else None
    ws_d = torch.empty(nq * S * k, dtype=torch.float32, device=Q.device) if S > 1 else None
    ws_i = torch.empty(nq * S * k, dtype=torch.int32, device=Q.device) if S > 1 else None
    native.call("fmlx_knn_fused", native.ptr(Q), Q.stride(0), nq, d, native.ptr(pack.Tt), pack.n, pack.dp, k, S,
                native.ptr(idx), native.ptr(dist), native.ptr(ws_d), native.ptr(ws_i), native.stream_ptr(Q.device))
    return (idx, dist) if with_dist else idx

MAX_K = 32
# KnnModel routes k above this to the sort path: the per-lane insertion lists get long enough that
# insertions, not HBM, bound the scan (measured: k=32 is ~5x slower than addmm+topk; k<=16 is
# 2-3.4x faster — README "KNN")
ROUTE_MAX_K = 16
# G block budget (bytes): large enough to amortise the per-block GEMM/vote launches, small
# enough to bound the transient memory
G_BLOCK_BYTES = 512 << 20


def supported(k: int, n: int, device) -> bool:
    return torch.device(device).type == "cuda" and 1 <= k <= MAX_K and k <= n < 2 ** 31 - 1


def query_block(n: int) -> int:
    b = G_BLOCK_BYTES // max(1, 4 * n)
    return int(min(16384, max(1024, b // 4 * 4)))


# waves wanted per launch and the shortest column segment worth a wave. Few, long segments win:
# every segment pays ~k·ln(L/k) insertions before its bound settles (sweep on MI355X: 2048 waves
# beat 4096/8192/16384 by 10-60%)
TARGET_WAVES = int(os.environ.get("FMLX_KNN_WAVES", "2048"))
MIN_SEGMENT = 2048


def segments(nq: int, n: int) -> int:
    """Column segments per query row so a launch has enough waves in flight."""
    want = -(-TARGET_WAVES // max(1, nq))
    return int(max(1, min(want, n // MIN_SEGMENT, 256)))


def topk_from_products(G: torch.Tensor, qn: torch.Tensor, tn: torch.Tensor, k: int, with_dist: bool = False):
    """k nearest columns of every row of ``G`` under ``sqrt(|qn_r + tn_c − 2·G_rc|)``."""
    nq, n = G.shape
    if not (G.dtype == torch.float32 and qn.dtype == torch.float32 and tn.dtype == torch.float32):
        raise TypeError("knn top-k expects fp32 products and norms")
    if G.stride(1) != 1 or qn.numel() != nq or tn.numel() != n or not supported(k, n, G.device):
        raise ValueError("knn top-k: bad shapes G=%s qn=%s tn=%s k=%d" % (tuple(G.shape), tuple(qn.shape),
                                                                         tuple(tn.shape), k))
    qn, tn = qn.contiguous(), tn.contiguous()
    idx = torch.empty((nq, k), dtype=torch.int32, device=G.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=G.device) if with_dist else None
    S = segments(nq, n)
    ws_d = torch.empty(nq * S * k, dtype=torch.float32, device=G.device) if S > 1 else None
    ws_i = torch.empty(nq * S * k, dtype=torch.int32, device=G.device) if S > 1 else None
    native.call("fmlx_knn_topk", native.ptr(G), G.stride(0), nq, n, S, native.ptr(qn), native.ptr(tn), k,
                native.ptr(idx), native.ptr(dist), native.ptr(ws_d), native.ptr(ws_i), native.stream_ptr(G.device))
    return (idx, dist) if with_dist else idx


# ---- any k, fp32 or fp64: radix selection over a library-GEMM product block (csrc/knn_select.hip)
SELECT_MAX_K = 8192  # csrc/knn_select.hip SEL_KMAX (the k winners are sorted in LDS)
SELECT_BLOCK_BYTES = 1 << 30


def select_supported(k: int, n: int, dtype, device) -> bool:
    return (torch.device(device).type == "cuda" and dtype in (torch.float32, torch.float64)
            and 1 <= k <= SELECT_MAX_K and k <= n < 2 ** 31 - 1)


def select_query_block(n: int, es: int) -> int:
    """Queries per product block: the [block, n] block within SELECT_BLOCK_BYTES."""
    return int(max(1, min(1 << 16, SELECT_BLOCK_BYTES // max(1, es * n))))


def select_topk(G: torch.Tensor, qn: torch.Tensor, tn: torch.Tensor, k: int) -> torch.Tensor:
    """int32 [nq, k]: the k nearest columns of every row of ``G`` under ``|qn_r + tn_c − 2·G_rc|``,
    nearest first, ties to the lower column (``KnnModel.java:154-194``) — any k up to
    SELECT_MAX_K, fp32 or fp64 (one 1024-thread block per row: radix passes, then a sort of the k)."""
    nq, n = G.shape
    dt = G.dtype
    if dt not in (torch.float32, torch.float64) or qn.dtype != dt or tn.dtype != dt:
        raise TypeError("knn select expects fp32 or fp64 products and norms of one dtype")
    if G.stride(1) != 1 or qn.numel() != nq or tn.numel() != n or not select_supported(k, n, dt, G.device):
        raise ValueError("knn select: bad shapes G=%s qn=%s tn=%s k=%d" % (tuple(G.shape), tuple(qn.shape),
                                                                          tuple(tn.shape), k))
    qn, tn = qn.contiguous(), tn.contiguous()
    idx = torch.empty((nq, k), dtype=torch.int32, device=G.device)
    if nq:
        native.call("fmlx_knn_select", int(dt == torch.float64), native.ptr(G), G.stride(0), nq, n, native.ptr(qn),
                    native.ptr(tn), int(k), native.ptr(idx), k, native.stream_ptr(G.device))
    return idx


# ---- CSR feature columns (csrc/knn_csr.hip): the product block of two CSR operands
# FMLX_KNN_CSR: "0" = a SparseColumn is densified (the path before the CSR kernel), "1" = the CSR
# route whenever csr_supported, "auto" = the CSR route when the dense training matrix n·D·elem
# would exceed the HBM budget or the training set's density nnz / (n·D) is at most CSR_CROSSOVER.
CSR_ROUTE = os.environ.get("FMLX_KNN_CSR", "auto")
# training rows per block of the products kernel (32 KiB of LDS accumulators), and every tile
# the library is built with (32 KiB and 8 KiB)
CSR_TILE_ROWS = {torch.float32: 8192, torch.float64: 4096}
CSR_TILE_ROWS_BUILT = {torch.float32: (2048, 8192), torch.float64: (1024, 4096)}
# the highest density of the measured sweep (100,000 training rows x 4,096, 1,024 queries, fp32,
# k = 5 and 100; scripts/bench_knn_sparse.py, profiles/r19/INDEX.md) at which the CSR transform beat
# the densified one in both run orders for both k: 5.2 / 5.7 ms against 7.4 / 8.0 ms at 5 %; at
# 20 % the dense route wins 9x (67 ms against 7.5 ms). Measured on the GPU only: the host route
# follows the same constant unmeasured.
CSR_CROSSOVER = 0.05


def csr_supported(X, device) -> bool:
    """The CSR route takes this training column: 32-bit rows / entries / indices and, on a GPU, the
    column-major copy and its sort scratch within the HBM budget (on the host the route is the
    torch formulation)."""
    from ..table import SparseColumn

    device = torch.device(device)
    if not isinstance(X, SparseColumn):
        return False
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    if n < 1 or D < 1 or n >= 2 ** 31 or nnz >= 2 ** 31 or D >= 2 ** 31:
        return False
    if device.type != "cuda":
        return True
    from ..common.outofcore import hbm_budget

    budget = hbm_budget(device)
    es = 8 if X.values.dtype == torch.float64 else 4
    need = nnz * (4 + es) * 2 + 16 * nnz + 8 * (n + D)
    return budget is None or need <= budget


def csr_route(X, device) -> bool:
    """Whether a sparse training column takes the CSR route (``CSR_ROUTE``)."""
    if CSR_ROUTE == "0" or not csr_supported(X, device):
        return False
    if CSR_ROUTE == "1":
        return True
    from .. import config
    from ..common.outofcore import hbm_budget

    device = torch.device(device)
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    budget = hbm_budget(device) if device.type == "cuda" else None
    if budget is not None and n * D * torch.empty(0, dtype=config.compute_dtype()).element_size() > budget:
        return True
    return nnz <= CSR_CROSSOVER * n * D


class TorchColumnMajor:
    """``ColumnMajor`` (ops/csr.py) formed by torch's stable sort, on the column's own device: the
    host route's inverted index. An index outside [0, D) raises."""

    def __init__(self, X):
        self.n, self.D = len(X), X.size
        idx = X.indices.long()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.D):
            raise ValueError("sparse feature index out of range [0, size)")
        ptr = X.indptr.long()
        rows = torch.repeat_interleave(torch.arange(self.n, device=idx.device), ptr[1:] - ptr[:-1])
        order = torch.sort(idx, stable=True).indices
        self.colptr = torch.zeros(self.D + 1, dtype=torch.int64, device=idx.device)
        self.colptr[1:] = torch.cumsum(torch.bincount(idx, minlength=self.D), 0)
        self.crow = rows[order].to(torch.int32)
        self.cval = X.values[order]
        self.nnz = int(idx.numel())


def has_duplicate_index(cm) -> bool:
    """Whether a row of the column-major copy ``cm`` stores an index twice: equal neighbouring rows
    inside a column (the products kernel needs the rows of a column distinct)."""
    if cm.nnz < 2:
        return False
    crow = cm.crow[: cm.nnz]
    same = crow[1:] == crow[:-1]
    starts = cm.colptr[1:-1]
    starts = starts[(starts > 0) & (starts < cm.nnz)]
    same[starts - 1] = False  # neighbours across a column boundary
    return bool(same.any().item())


def torch_products_csr(Q, T, dtype=torch.float64) -> torch.Tensor:
    """``G[r, t] = Σ_e v_e · T[t, c_e]`` of two CSR columns as one index-add over the (query entry,
    training entry) pairs that share a column, query entries in stored order: the host route and the
    tests' second opinion. ``T``: a SparseColumn or its ``TorchColumnMajor``."""
    cm = T if isinstance(T, TorchColumnMajor) else TorchColumnMajor(T)
    if Q.size != cm.D:
        raise ValueError("Vector size mismatched.")
    nq, n = len(Q), cm.n
    dev = cm.crow.device
    G = torch.zeros(nq * n, dtype=dtype, device=dev)
    qi = Q.indices.to(dev).long()
    if qi.numel() == 0 or cm.nnz == 0:
        return G.view(nq, n)
    if int(qi.min()) < 0 or int(qi.max()) >= cm.D:
        raise ValueError("sparse feature index out of range [0, size)")
    qp = Q.indptr.to(dev).long()
    qrow = torch.repeat_interleave(torch.arange(nq, device=dev), qp[1:] - qp[:-1])
    lens = cm.colptr[qi + 1] - cm.colptr[qi]
    ent = torch.repeat_interleave(torch.arange(qi.numel(), device=dev), lens)  # the pair's query entry
    first = torch.cumsum(lens, 0) - lens
    pos = cm.colptr[qi][ent] + (torch.arange(ent.numel(), device=dev) - first[ent])
    prod = Q.values.to(device=dev, dtype=dtype)[ent] * cm.cval[pos].to(dtype)
    G.index_add_(0, qrow[ent] * n + cm.crow[pos].long(), prod)
    return G.view(nq, n)


def csr_sqnorm(X, dtype=torch.float64, err: torch.Tensor = None) -> torch.Tensor:
    """Σv² per row of a SparseColumn in stored-entry order, accumulated in fp64, as ``dtype`` (fp32
    or fp64). On the GPU an index outside [0, size) adds nothing and sets ``err`` when given."""
    n = len(X)
    dev = X.values.device
    if dev.type != "cuda":
        v = X.values.to(torch.float64)
        ptr = X.indptr.long()
        rows = torch.repeat_interleave(torch.arange(n), ptr[1:] - ptr[:-1])
        return torch.zeros(n, dtype=torch.float64).index_add_(0, rows, v * v).to(dtype)
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("knn csr: norms are fp32 or fp64")
    from .csr import csr_arrays

    indptr, idx, val = csr_arrays(X, torch.float64 if X.values.dtype == torch.float64 else torch.float32)
    out = torch.empty(n, dtype=dtype, device=dev)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    native.call("fmlx_knn_csr_sqnorm", int(val.dtype == torch.float64), int(dtype == torch.float64), native.ptr(indptr),
                native.ptr(idx), native.ptr(val), n, X.size, native.ptr(out), native.ptr(err), native.stream_ptr(dev))
    return out


def csr_products(Q, cm, q0: int, q1: int, out: torch.Tensor = None, tile: int = None) -> torch.Tensor:
    """``G [q1 - q0, n]`` for the query rows [q0, q1) of a device SparseColumn ``Q`` (values in
    ``cm``'s dtype) against the training set's ``ColumnMajor`` ``cm``, every element summed in the
    query row's stored-entry order. A bad index is skipped and sets ``cm.err``
    (``ops.kmeans.check_csr_error``). ``tile``: one of ``CSR_TILE_ROWS_BUILT`` (the result does not
    depend on it)."""
    nq, n, dt = int(q1) - int(q0), cm.n, cm.acc
    if Q.size != cm.D:
        raise ValueError("Vector size mismatched.")
    if not (0 <= q0 <= q1 <= len(Q)) or Q.values.dtype != dt or not Q.values.is_cuda:
        raise ValueError("knn csr products: rows [%d, %d) of %d, values %s against %s" % (q0, q1, len(Q),
                                                                                         Q.values.dtype, dt))
    tile = int(CSR_TILE_ROWS[dt] if tile is None else tile)
    if tile not in CSR_TILE_ROWS_BUILT[dt]:
        raise ValueError("knn csr products: no kernel with a tile of %d rows" % tile)
    if out is None:
        out = torch.empty((nq, n), dtype=dt, device=cm.crow.device)
    if out.dtype != dt or out.shape != (nq, n) or out.stride(1) != 1:
        raise ValueError("knn csr products: bad output block %s %s" % (tuple(out.shape), out.dtype))
    if nq and n:
        qptr, qidx = Q.indptr, Q.indices
        if qptr.dtype != torch.int64 or qidx.dtype != torch.int32 or not qptr.is_contiguous():
            raise ValueError("knn csr products: the query column is not in kernel form (ops.csr.csr_arrays)")
        native.call("fmlx_knn_csr_products", int(dt == torch.float64), native.ptr(qptr), native.ptr(qidx),
                    native.ptr(Q.values), int(q0), nq, cm.D, native.ptr(cm.colptr), native.ptr(cm.crow),
                    native.ptr(cm.cval), n, cm.nnz, tile, native.ptr(out), out.stride(0), native.ptr(cm.err),
                    native.stream_ptr(cm.crow.device))
    return out
