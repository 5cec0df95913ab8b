"""Bindings for ``csrc/kmeans.hip`` plus the host reference (exact reference semantics, fp64).

``assign`` = findClosest for every row (K8); ``KMeansRound`` = one Lloyd step on the rank's
partition producing the all-reduce payload ``[k·D sums | k counts]`` (K9), deterministic.
"""
from __future__ import annotations

import math

import os

import numpy as np
import torch

from . import native
from .csr import ColumnMajor
from .csr import csr_arrays as _csr_arrays

# rows grouped by cluster with the hand-written STABLE counting sort (csrc/groupsort.hip
# st_*: per-tile histograms, column scan, ordered scatter — rows of a cluster stay in row order,
# so the centroid sums are bit-reproducible) for k <= 2048; larger k takes the arrival-order
# counting sort (sums reproducible to rounding), or the stable radix sort of sort.hip when
# FMLX_DETERMINISTIC=1. GROUP_SORT=False forces the radix sort (A/B and tests).
GROUP_SORT = True
DETERMINISTIC = os.environ.get("FMLX_DETERMINISTIC", "0") == "1"

METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2}
CHUNK = 256
# (A split round — part p's grouping + gather-sum on a side stream under part p + 1's assign —
# measured 3.98-4.06 vs 3.77-3.86 ms/iter unsplit at the 12.5M x 128, k = 1024 shard and was removed
# in round 5: the assign fills every CU and the gather-sum beside it slows it more than it hides;
# profiles/r4/kmeans_assign_lds_split_ab.jsonl.)
MFMA_KS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16)


def mfma_ks(D: int) -> int:
    """Padded number of 16-wide K steps for the MFMA assign kernel (0 if D is too wide)."""
    need = (D + 15) // 16
    for ks in MFMA_KS:
        if ks >= need:
            return ks
    return 0


# MFMA assign schedule (fmlx_kmeans_set_sched): 1 = the pipelined kernel for D = 64/128 (norms in
# the matrix core, LDS-DMA centroid ring, B fragments one tile ahead; other widths take the plain
# loop), 0 = the plain loop everywhere (A/B and tests). FMLX_KMEANS_SCHED overrides. 12.5M x 128,
# k = 1024 on one MI355X: 3.53 ms (plain) → 3.18 ms (pipelined); the other variants measured over
# rounds 2-4 were removed in round 5 (history in csrc/kmeans.hip).
ASSIGN_SCHED = int(os.environ.get("FMLX_KMEANS_SCHED", "1"))
_sched_applied = None


def set_assign_sched(mode: int) -> None:
    global _sched_applied
    native.call("fmlx_kmeans_set_sched", int(mode))
    _sched_applied = int(mode)


def mfma_ok(X: torch.Tensor, metric: str) -> bool:
    return (X.device.type == "cuda" and X.dtype == torch.bfloat16 and metric == "euclidean"
            and X.stride(1) == 1 and X.stride(0) % 2 == 0 and X.data_ptr() % 4 == 0 and mfma_ks(X.shape[1]) > 0)


class CentroidBuffers:
    """Device-side centroid representations consumed by the assign kernels."""

    def __init__(self, k: int, D: int, device, acc_dtype):
        self.k, self.D = k, D
        self.kpad = max(32, (k + 31) // 32 * 32)
        self.KS = mfma_ks(D) or (D + 15) // 16
        self.DP = self.KS * 16
        self.cent = torch.zeros((k, D), dtype=acc_dtype, device=device)
        self.cnorm = torch.zeros(k, dtype=acc_dtype, device=device)          # ‖c‖ (acc dtype)
        self.Cb = torch.zeros((self.kpad, self.DP), dtype=torch.bfloat16, device=device)
        self.cnorm_b = torch.full((self.kpad,), float("inf"), dtype=torch.float32, device=device)  # ‖c_bf16‖²
        # the pipelined MFMA assign's B_aug rows (‖c‖² split into three bf16s), rebuilt from
        # cnorm_b by every assign launch
        self.baug = torch.empty(self.kpad * 2, dtype=torch.int32, device=device)
        self.weights = torch.zeros(k, dtype=torch.float64, device=device)
        self._pack = None

    def set(self, centroids: torch.Tensor) -> None:
        # the k x D representations are formed on the host and copied over once (a fit's initial
        # centroids come from the host anyway): on the device the norm / pow / scatter ops would
        # each load their torch code object at first use, ~10-40 ms apiece in a fresh process
        c = torch.as_tensor(centroids).detach().to(device="cpu", dtype=self.cent.dtype)
        cb = c.to(torch.bfloat16)
        Cb = torch.zeros((self.kpad, self.DP), dtype=torch.bfloat16)
        Cb[: self.k, : self.D] = -2 * cb  # the MFMA assign consumes −2·c (exact in bf16)
        nb = torch.full((self.kpad,), float("inf"), dtype=torch.float32)
        nb[: self.k] = (cb.float() * cb.float()).sum(1)
        self.cent.copy_(c)
        self.cnorm.copy_(torch.linalg.vector_norm(c.to(torch.float64), dim=1).to(self.cent.dtype))
        self.Cb.copy_(Cb)
        self.cnorm_b.copy_(nb)
        self._pack = None

    def fp32_pack(self):
        """The current centroids as the fused KNN kernel's training pack (fp32). Refreshed in place
        on every call: the finalize kernel rewrites ``cent`` on the device, and inside a captured
        round the refresh replays with it."""
        c = self.cent.to(torch.float32)
        if self._pack is None:
            from . import knn as knn_ops

            self._pack = knn_ops.TrainPack(c, (c * c).sum(1))
        else:
            self._pack.refresh(c, (c * c).sum(1))
        return self._pack


# fp32 euclidean assign from GEMM_ASSIGN_MIN_ROWS rows: "fused" = the fused KNN kernel with k = 1
# (D <= 128; 1M x 100, k=10: 9.24 ms per 10-round fit vs 9.69 through the GEMM), "gemm" = library
# GEMM + argmin for few centroids; small inputs take the one-launch wave-per-row kernel (the
# fused path's pack refresh + merge launches cost more than they save there)
FP32_ASSIGN = os.environ.get("FMLX_KMEANS_FP32_ASSIGN", "fused")
GEMM_ASSIGN_MAX_K = 64       # fp32 euclidean assign through a library GEMM up to this many centroids
GEMM_ASSIGN_ROWS = 1 << 22   # rows per GEMM chunk (bounds the n×k distance block)
GEMM_ASSIGN_MIN_ROWS = 1 << 18  # below this the one-launch wave kernel wins (the GEMM path is ~6 launches)


def assign(X: torch.Tensor, cb: CentroidBuffers, metric: str, out: torch.Tensor = None) -> torch.Tensor:
    """Index of the closest centroid for every row (reference ``DistanceMeasure.findClosest``)."""
    n, D = X.shape
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=X.device)
    if n == 0:
        return out
    if X.device.type != "cuda":
        return torch_assign(X, cb.cent, metric).to(torch.int32)
    if mfma_ok(X, metric):
        if _sched_applied is None:
            set_assign_sched(ASSIGN_SCHED)
        native.call("fmlx_kmeans_assign_bf16", native.ptr(X), X.stride(0), n, D, cb.KS, native.ptr(cb.Cb),
                    native.ptr(cb.cnorm_b), cb.kpad, native.ptr(out), native.ptr(cb.baug), native.stream_ptr(X.device))
        return out
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float32)
    X = X if X.stride(1) == 1 else X.contiguous()
    if X.dtype == torch.float32 and metric == "euclidean" and FP32_ASSIGN == "fused" and n >= GEMM_ASSIGN_MIN_ROWS:
        from . import knn as knn_ops

        if knn_ops.fused_supported(1, cb.k, D, X.device):
            # the fused KNN kernel with k = 1: fp32 MFMA distances with the argmin in registers
            # (ties → lower centroid index, NaN never wins), no n×k block in HBM
            pack = cb.fp32_pack()
            out.copy_(knn_ops.fused_topk(X, pack, 1).view(-1))
            return out
    if X.dtype == torch.float32 and metric == "euclidean" and cb.k <= GEMM_ASSIGN_MAX_K and n >= GEMM_ASSIGN_MIN_ROWS:
        # few centroids: the distance "GEMM" X·Cᵀ is one bandwidth-bound library GEMM (fp32
        # accumulate) plus an n×k argmin; the wave-per-row kernel is latency-bound at this shape
        C = cb.cent.to(torch.float32)
        cn2 = (C * C).sum(1)
        for r0 in range(0, n, GEMM_ASSIGN_ROWS):
            Xc = X[r0:r0 + GEMM_ASSIGN_ROWS]
            # ‖c‖² − 2x·c: the per-row ‖x‖² does not move the argmin (no n×D temporary for it)
            d = torch.addmm(cn2.unsqueeze(0), Xc, C.t(), alpha=-2.0)
            d.nan_to_num_(nan=float("inf"))  # NaN distances never win, like torch_assign / the kernels
            out[r0:r0 + Xc.shape[0]] = torch.argmin(d, dim=1).to(torch.int32)  # first (lowest) index on ties
        return out
    C = cb.cent.to(X.dtype).contiguous()
    cn = cb.cnorm.to(X.dtype).contiguous()
    native.call("fmlx_kmeans_assign_generic", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, D,
                native.ptr(C), native.ptr(cn), cb.k, METRICS[metric], native.ptr(out), native.stream_ptr(X.device))
    return out


def torch_assign(X: torch.Tensor, C: torch.Tensor, metric: str) -> torch.Tensor:
    """Host reference of findClosest (EuclideanDistanceMeasure.java:53-73 incl. pruning order)."""
    X = X.to(torch.float64)
    C = C.to(device=X.device, dtype=torch.float64)
    if X.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64)
    if metric == "euclidean":
        pn = torch.linalg.vector_norm(X, dim=1)
        cn = torch.linalg.vector_norm(C, dim=1)
        d2 = torch.clamp(pn[:, None] * pn[:, None] + (cn * cn)[None, :] - 2.0 * (X @ C.T), min=0.0)
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
        return torch.argmin(d2, dim=1)  # argmin returns the first minimum: lowest index on ties
    if metric == "manhattan":
        d = torch.cdist(X, C, p=1)
    else:
        d = 1.0 - (X @ C.T) / torch.linalg.vector_norm(X, dim=1)[:, None] / torch.linalg.vector_norm(C, dim=1)[None, :]
    return torch.argmin(d, dim=1)


class KMeansRound:
    """One Lloyd iteration on a device-resident partition: assign → ordered chunk sums →
    per-cluster sums/counts. ``payload`` is the fixed-size all-reduce buffer."""

    def __init__(self, X: torch.Tensor, k: int, metric: str):
        self.X = X
        self.n, self.D = X.shape
        self.k = k
        self.metric = metric
        dev = X.device
        self.acc = torch.float64 if X.dtype == torch.float64 else torch.float32
        self.labels = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.max_chunks = (self.n + CHUNK - 1) // CHUNK + k
        self.partial = torch.zeros((self.max_chunks, self.D), dtype=self.acc, device=dev)
        self.payload = torch.zeros(k * self.D + k, dtype=self.acc, device=dev)
        self.zero_i64 = torch.zeros(1, dtype=torch.int64, device=dev)
        self.fast = (dev.type == "cuda" and X.dtype == torch.bfloat16 and self.D in (8, 16, 32, 64, 128, 256, 512)
                     and X.stride(1) == 1 and X.stride(0) % 8 == 0 and X.data_ptr() % 16 == 0)
        lib = native.kernels() if dev.type == "cuda" else None
        self.stable = dev.type == "cuda" and GROUP_SORT and k <= lib.fmlx_group_stable_max_keys()
        self.group = (dev.type == "cuda" and GROUP_SORT and not self.stable and not DETERMINISTIC
                      and k <= lib.fmlx_group_max_keys())
        if dev.type == "cuda":
            self.offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
            self.chunk_off = torch.zeros(k + 1, dtype=torch.int64, device=dev)
            self.order32 = torch.empty(self.n, dtype=torch.int32, device=dev)
        if self.stable:
            self.gscratch = torch.empty(max(1, int(lib.fmlx_group_stable_scratch(self.n, k))), dtype=torch.int32,
                                        device=dev)
        elif self.group:
            self.gcounts = torch.zeros(k, dtype=torch.int32, device=dev)  # re-zeroed by the scan kernel
            self.gcursor = torch.zeros(k, dtype=torch.int32, device=dev)
        if dev.type == "cuda" and not self.stable and not self.group:
            # more keys than the counting sort's LDS histograms hold: the stable segmented LSD radix
            # sort (radix.hip, one segment) over ceil(log2 k) bits, buffers allocated once
            from . import glm as _glm

            self.bits = max(1, int(k - 1).bit_length())
            self.iota = torch.arange(self.n, dtype=torch.int32, device=dev)
            self.sort_keys = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.sort_vals = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.sort_keys_alt = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.sort_vals_alt = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.sort_scratch = torch.empty(_glm.seg_sort_scratch([0, self.n], self.bits), dtype=torch.int32,
                                            device=dev)
            odd = _glm.seg_sort_passes(self.bits) & 1
            self.keys_sorted = self.sort_keys_alt if odd else self.sort_keys
            self.order32 = self.sort_vals_alt if odd else self.sort_vals

    def run(self, cb: CentroidBuffers) -> torch.Tensor:
        X = self.X
        if self.n == 0:
            self.payload.zero_()
            return self.payload
        assign(X, cb, self.metric, self.labels)
        stream = native.stream_ptr(X.device)
        if self.stable:
            # stable counting sort by cluster + cluster / chunk offsets (groupsort.hip st_*)
            native.call("fmlx_group_by_key_stable", native.ptr(self.labels), self.n, self.k, CHUNK,
                        native.ptr(self.gscratch), native.ptr(self.offsets), native.ptr(self.chunk_off),
                        native.ptr(self.order32), stream)
        elif self.group:
            # counting sort by cluster + cluster / chunk offsets, no library sort (groupsort.hip)
            native.call("fmlx_group_by_key", native.ptr(self.labels), self.n, self.k, CHUNK, native.ptr(self.gcounts),
                        native.ptr(self.gcursor), native.ptr(self.offsets), native.ptr(self.chunk_off),
                        native.ptr(self.order32), stream)
        else:
            from . import glm as _glm

            self.sort_keys.copy_(self.labels)
            self.sort_vals.copy_(self.iota)
            _glm.seg_sort(self.sort_keys, self.sort_vals, [0, self.n], [0], self.bits, self.sort_keys_alt,
                          self.sort_vals_alt, self.sort_scratch)
            # cluster boundaries on the device (no host sync: the round is hipGraph-capturable)
            native.call("fmlx_kmeans_offsets", native.ptr(self.keys_sorted), self.n, self.k, native.ptr(self.offsets),
                        native.ptr(self.chunk_off), stream)
        offsets, chunk_off = self.offsets, self.chunk_off
        if self.fast:
            native.call("fmlx_kmeans_chunk_sum_bf16v", native.ptr(X), X.stride(0), self.D, native.ptr(self.order32),
                        native.ptr(offsets), native.ptr(chunk_off), self.k, self.max_chunks, native.ptr(self.partial),
                        stream)
        else:
            order = self.order32.to(torch.int64)
            Xs = X if X.dtype in (torch.bfloat16, torch.float32, torch.float64) else X.to(torch.float32)
            native.call("fmlx_kmeans_chunk_sum", native.dtype_code(Xs.dtype), native.ptr(Xs), Xs.stride(0), self.D,
                        native.ptr(order), native.ptr(offsets), native.ptr(chunk_off), self.k, self.max_chunks,
                        native.ptr(self.partial), stream)
        native.call("fmlx_kmeans_cluster_sum", int(self.acc == torch.float64), native.ptr(self.partial), self.D,
                    native.ptr(offsets), native.ptr(chunk_off), self.k, native.ptr(self.payload),
                    native.stream_ptr(X.device))
        return self.payload

    def finalize(self, cb: CentroidBuffers, payload: torch.Tensor) -> None:
        native.call("fmlx_kmeans_finalize", int(self.acc == torch.float64), native.ptr(payload), self.D, self.k,
                    native.ptr(cb.cent), native.ptr(cb.weights), native.ptr(cb.Cb), cb.DP, native.ptr(cb.cnorm_b),
                    native.ptr(cb.cnorm), native.stream_ptr(self.X.device))


def torch_round_payload(X: torch.Tensor, C: torch.Tensor, metric: str) -> torch.Tensor:
    """Host reference for one round's [sums | counts] (CentroidsUpdateAccumulator, KMeans.java:269-300)."""
    k, D = C.shape
    X = X.to(torch.float64)
    out = torch.zeros(k * D + k, dtype=torch.float64)
    if X.shape[0] == 0:
        return out
    lab = torch_assign(X, C, metric)
    sums = torch.zeros((k, D), dtype=torch.float64).index_add_(0, lab, X)
    out[: k * D] = sums.reshape(-1)
    out[k * D:] = torch.bincount(lab, minlength=k).to(torch.float64)
    return out


def torch_finalize(payload: torch.Tensor, k: int, D: int):
    sums = payload[: k * D].reshape(k, D)
    counts = payload[k * D:]
    cent = sums * (1.0 / counts)[:, None]  # scal(1/count): 0 rows → NaN like the reference
    return cent, counts


def group_by_key(keys: torch.Tensor, k: int, chunk: int = 0, stable: bool = False):
    """Rows grouped by an int32 key in [0, k) on the device (csrc/groupsort.hip counting sort):
    returns (order int32 [m], offsets int64 [k + 1], chunk_off int64 [k + 1] or None), where
    ``order[offsets[c]:offsets[c+1]]`` are the rows with key c (in row order with ``stable``,
    k ≤ ``fmlx_group_stable_max_keys()``; otherwise in arrival order, k ≤ ``fmlx_group_max_keys()``)
    and m = offsets[k] (keys outside [0, k) are dropped)."""
    dev = keys.device
    n = keys.numel()
    keys = keys.to(torch.int32).contiguous()
    if stable:
        lib = native.kernels()
        scratch = torch.empty(max(1, int(lib.fmlx_group_stable_scratch(n, int(k)))), dtype=torch.int32, device=dev)
        offsets = torch.empty(k + 1, dtype=torch.int64, device=dev)
        chunk_off = torch.empty(k + 1, dtype=torch.int64, device=dev) if chunk > 0 else None
        order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        native.call("fmlx_group_by_key_stable", native.ptr(keys), n, int(k), int(chunk), native.ptr(scratch),
                    native.ptr(offsets), native.ptr(chunk_off), native.ptr(order), native.stream_ptr(dev))
        m = int(offsets[k].item())
        return order[:m], offsets, chunk_off
    counts = torch.zeros(k, dtype=torch.int32, device=dev)
    cursor = torch.empty(k, dtype=torch.int32, device=dev)
    offsets = torch.empty(k + 1, dtype=torch.int64, device=dev)
    chunk_off = torch.empty(k + 1, dtype=torch.int64, device=dev) if chunk > 0 else None
    order = torch.empty(n, dtype=torch.int32, device=dev)
    native.call("fmlx_group_by_key", native.ptr(keys), n, int(k), int(chunk), native.ptr(counts), native.ptr(cursor),
                native.ptr(offsets), native.ptr(chunk_off), native.ptr(order), native.stream_ptr(dev))
    m = int(offsets[k].item())
    return order[:m], offsets, chunk_off


# ------------------------------------------------------------------------------------------------
# CSR feature columns (csrc/kmeans_csr.hip): assign / Lloyd round without an n x D matrix
# ------------------------------------------------------------------------------------------------
# FMLX_KMEANS_CSR: "0" = a SparseColumn is densified (the path before the CSR kernels), "1" = the
# CSR path whenever csr_supported, "auto" = the CSR path when the densified matrix would exceed the
# HBM budget or the density nnz / (n·D) is at most CSR_CROSSOVER.
CSR_ROUTE = os.environ.get("FMLX_KMEANS_CSR", "auto")
# the highest density of the measured sweep (100,000 rows, k = 10 and 100; scripts/
# bench_kmeans_sparse.py, profiles/r12/INDEX.md) at which the CSR round beat the densified one in
# both run orders for both k: at 20 % the dense round wins at k = 10
CSR_CROSSOVER = 0.05
# columns of the column-major copy longer than this are summed in segments of this length, one
# wave each, and their partial sums added in segment order (text columns are Zipf-distributed: one
# wave per column would run as long as the most frequent term)
CSR_COL_SEGMENT = 4096
CSR_MAX_K = 1024


def csr_kp(k: int) -> int:
    """Lanes per row of the centroid image: k rounded up to a power of two (<= 64), above that to
    64 · {1, 2, 4, 8, 16} (the accumulators a lane holds)."""
    kp = 1
    while kp < k:
        kp *= 2
    return kp


def _elem(dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def csr_supported(X, k: int, device) -> bool:
    """The CSR kernels take this column: a GPU, k <= 1024, 32-bit rows / entries, and the centroid
    image, the payload and the column-major copy within the HBM budget."""
    from ..table import SparseColumn

    device = torch.device(device)
    if device.type != "cuda" or not isinstance(X, SparseColumn):
        return False
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    if not (1 <= k <= CSR_MAX_K) or D < 1 or n >= 2 ** 31 or nnz >= 2 ** 31 or D >= 2 ** 31:
        return False
    from ..common.outofcore import hbm_budget

    budget = hbm_budget(device)
    es = 8 if X.values.dtype == torch.float64 else 4
    need = 2 * D * csr_kp(k) * es + nnz * (4 + es) * 2 + 16 * nnz + 8 * (n + D)
    return budget is None or need <= budget


def csr_route(X, k: int, device) -> bool:
    """Whether a SparseColumn takes the CSR path (``CSR_ROUTE``)."""
    if CSR_ROUTE == "0" or not csr_supported(X, k, device):
        return False
    if CSR_ROUTE == "1":
        return True
    from .. import config
    from ..common.outofcore import hbm_budget

    n, D, nnz = len(X), X.size, int(X.indices.numel())
    budget = hbm_budget(device)
    if budget is not None and n * D * _elem(config.compute_dtype()) > budget:
        return True
    return nnz <= CSR_CROSSOVER * n * D


def csr_features(table, col: str, k: int):
    """The feature column as a device-resident ``SparseColumn`` (values in the accumulation dtype)
    when it is one and takes the CSR path, else None (the caller densifies as before)."""
    from .. import config
    from ..table import SparseColumn

    c = table.column(col)
    dev = config.compute_device()
    if not isinstance(c, SparseColumn) or not csr_route(c, k, dev):
        return None
    return config.features_for_compute(table, col, allow_sparse=True)


class SparseCentroidBuffers:
    """The centroid image of the CSR kernels: centroid-minor ``Ct[D][kp]`` (padding lanes 0), the
    per-centroid norms ``[‖c‖ | ‖c‖² | ‖c‖₁]`` and the weights. ``cent`` is its [k, D] view."""

    def __init__(self, k: int, D: int, device, acc_dtype):
        self.k, self.D = int(k), int(D)
        self.kp = csr_kp(self.k)
        self.Ct = torch.zeros((self.D, self.kp), dtype=acc_dtype, device=device)
        self.norms = torch.zeros((3, self.kp), dtype=acc_dtype, device=device)
        self.weights = torch.zeros(self.k, dtype=torch.float64, device=device)
        # finalize: block b folds rows [b·rpb, (b + 1)·rpb) of the image, then one ordered add
        self.rpb = max(256, -(-self.D // 1024))
        self.nb = -(-self.D // self.rpb)
        self.part = torch.zeros((self.nb, 2, self.kp), dtype=acc_dtype, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)

    @property
    def cent(self) -> torch.Tensor:
        return self.Ct[:, : self.k].t()

    def set(self, centroids: torch.Tensor) -> None:
        # formed on the host and copied over once, like CentroidBuffers.set
        c = torch.as_tensor(centroids).detach().to(device="cpu", dtype=torch.float64)
        Ct = torch.zeros((self.D, self.kp), dtype=self.Ct.dtype)
        Ct[:, : self.k] = c.t().to(self.Ct.dtype)
        c = Ct[:, : self.k].t().to(torch.float64)
        norms = torch.zeros((3, self.kp), dtype=torch.float64)
        norms[1, : self.k] = (c * c).sum(1)
        norms[0, : self.k] = norms[1, : self.k].sqrt()
        norms[2, : self.k] = c.abs().sum(1)
        self.Ct.copy_(Ct)
        self.norms.copy_(norms.to(self.norms.dtype))


def check_csr_error(*holders) -> None:
    """Raises for a feature index outside [0, D) seen by a CSR kernel (the entry was skipped)."""
    bad = 0
    for h in holders:
        bad |= int(h.err.item())
    if bad:
        raise ValueError("sparse feature index out of range [0, size)")


def assign_csr(X, cb: SparseCentroidBuffers, metric: str, out: torch.Tensor = None) -> torch.Tensor:
    """``assign`` for a device-resident ``SparseColumn``; a bad index sets ``cb.err``."""
    n = len(X)
    dev = cb.Ct.device
    if X.size != cb.D:
        raise ValueError("vector size %d does not match the centroids' %d" % (X.size, cb.D))
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    indptr, idx, val = _csr_arrays(X, cb.Ct.dtype)
    native.call("fmlx_kmeans_csr_assign", int(cb.Ct.dtype == torch.float64), native.ptr(indptr), native.ptr(idx),
                native.ptr(val), n, cb.D, native.ptr(cb.Ct), cb.kp, cb.k, native.ptr(cb.norms), METRICS[metric],
                native.ptr(out), native.ptr(cb.err), native.stream_ptr(dev))
    return out


class SparseKMeansRound:
    """One Lloyd iteration on a device-resident CSR partition: assign → per-column sums through the
    column-major copy (built here, once per fit) → ``payload`` = ``[D·kp sums | k counts]``."""

    def __init__(self, X, k: int, metric: str):
        dev = X.values.device
        self.n, self.D, self.k, self.metric = len(X), X.size, int(k), metric
        self.kp = csr_kp(self.k)
        # the column-major copy (ops/csr.py): built once per fit, a column's entries in row order
        cm = self.cm = ColumnMajor(X, int(CSR_COL_SEGMENT))
        self.acc, self.nnz, self.seg, self.err = cm.acc, cm.nnz, cm.seg, cm.err
        self.indptr, self.idx, self.val = cm.indptr, cm.idx, cm.val
        self.X = type(X)(self.indptr, self.idx, self.val, self.D)
        self.colptr, self.crow, self.cval = cm.colptr, cm.crow, cm.cval
        self.nlong, self.long_col, self.long_seg0 = cm.nlong, cm.long_col, cm.long_seg0
        self.nsegs, self.seg_col, self.seg_k = cm.nsegs, cm.seg_col, cm.seg_k
        self.labels = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.payload = torch.zeros(self.D * self.kp + self.k, dtype=self.acc, device=dev)
        self.counts = torch.zeros(self.k, dtype=torch.int32, device=dev)  # re-zeroed by every round
        self.partial = torch.zeros(max(self.nsegs, 1) * self.kp, dtype=self.acc, device=dev)

    def run(self, cb: SparseCentroidBuffers) -> torch.Tensor:
        assign_csr(self.X, cb, self.metric, self.labels)
        return self.colsum()

    def colsum(self) -> torch.Tensor:
        """The centroid update of the current ``labels`` into ``payload``."""
        native.call("fmlx_kmeans_csr_colsum", int(self.acc == torch.float64), native.ptr(self.colptr),
                    native.ptr(self.crow), native.ptr(self.cval), native.ptr(self.labels), self.n, self.D, self.kp,
                    self.k, self.seg, self.nlong, native.ptr(self.long_col), native.ptr(self.long_seg0), self.nsegs,
                    native.ptr(self.seg_col), native.ptr(self.seg_k), native.ptr(self.partial),
                    native.ptr(self.counts), native.ptr(self.payload), native.stream_ptr(self.payload.device))
        return self.payload

    def finalize(self, cb: SparseCentroidBuffers, payload: torch.Tensor) -> None:
        native.call("fmlx_kmeans_csr_finalize", int(self.acc == torch.float64), native.ptr(payload), self.D, self.kp,
                    self.k, native.ptr(cb.Ct), native.ptr(cb.norms), native.ptr(cb.weights), native.ptr(cb.part),
                    cb.rpb, cb.nb, native.stream_ptr(payload.device))


def _csr_rows(X) -> torch.Tensor:
    indptr = X.indptr.to(torch.int64)
    n = len(X)
    return torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1],
                                   output_size=int(X.indices.numel()))


def torch_dist_csr(X, C: torch.Tensor, metric: str) -> torch.Tensor:
    """Host reference: the [n, k] fp64 distances of ``torch_assign`` (squared for euclidean) for a
    ``SparseColumn``, through torch's sparse-CSR ``@``: no n x D array is formed."""
    import warnings

    n, D = len(X), X.size
    dev = X.values.device
    indptr, idx, val = X.indptr.to(torch.int64), X.indices.to(torch.int64), X.values.to(torch.float64)
    C = C.to(device=dev, dtype=torch.float64)
    rows = _csr_rows(X)
    cn = torch.linalg.vector_norm(C, dim=1)
    pn = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, rows, val * val).sqrt()
    if metric == "manhattan":
        d = C.abs().sum(1)[None, :].repeat(n, 1)
        Ct = C.t().contiguous()
        for s in range(0, int(idx.numel()), 1 << 16):
            cj = Ct[idx[s:s + (1 << 16)]]
            d.index_add_(0, rows[s:s + (1 << 16)], (val[s:s + (1 << 16), None] - cj).abs() - cj.abs())
        return d
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dot = torch.sparse_csr_tensor(indptr, idx, val, size=(n, D)) @ C.t().contiguous()
    if metric == "euclidean":
        return torch.clamp(pn[:, None] * pn[:, None] + (cn * cn)[None, :] - 2.0 * dot, min=0.0)
    return 1.0 - dot / pn[:, None] / cn[None, :]


def torch_assign_csr(X, C: torch.Tensor, metric: str) -> torch.Tensor:
    """``torch_assign`` for a ``SparseColumn`` (fp64, no n x D array)."""
    if len(X) == 0:
        return torch.zeros(0, dtype=torch.int64)
    d = torch_dist_csr(X, C, metric)
    if metric == "euclidean":
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return torch.argmin(d, dim=1)


def torch_round_payload_csr(X, C: torch.Tensor, metric: str, labels: torch.Tensor = None) -> torch.Tensor:
    """``torch_round_payload`` for a ``SparseColumn``: ``[k·D sums | k counts]`` in fp64 (of the given
    ``labels`` instead of the reference assignment when passed; labels outside [0, k) add nothing)."""
    k, D = C.shape
    dev = X.values.device
    out = torch.zeros(k * D + k, dtype=torch.float64, device=dev)
    if len(X) == 0:
        return out
    lab = (torch_assign_csr(X, C, metric) if labels is None else labels.to(dev)).to(torch.int64)
    ok = (lab >= 0) & (lab < k)
    el = lab[_csr_rows(X)]
    eok = (el >= 0) & (el < k)
    out.index_add_(0, el[eok] * D + X.indices.to(torch.int64)[eok], X.values.to(torch.float64)[eok])
    out[k * D:] = torch.bincount(lab[ok], minlength=k).to(torch.float64)
    return out
