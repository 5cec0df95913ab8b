"""Device contingency statistics (``csrc/catstats.hip``): sorted distinct values, label indices
and (feature, value, label) counts for NaiveBayes (K22) and ChiSqTest (K20), with no library
sort / unique / bincount. Integer-valued columns with a small value range (the categorical
case) are counted straight into an LDS-privatised table; anything else goes through the stable
64-bit radix sort of each column (``ops/sorting.py``) and a distinct-id scan.

All functions take CUDA tensors; the CPU reference of every result is the torch code in
``models/stats.py`` / ``models/naive_bayes.py``.

A CSR feature column (``SparseColumn``) is counted from its stored entries alone
(``csrc/catstats_csr.hip``, ``value_label_counts_csr``): one radix sort of (column, value) keys, a
run scan, an integer count per run and label, and the zero row of every column from the label
totals. The result is a ragged table (``RaggedCounts``) instead of [d, L, Vmax]; the same functions
run on CPU tensors through a numpy formulation over the CSR arrays (``torch_value_label_counts_csr``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import native, sorting

# integer tables up to this many cells are counted directly (value range × labels × features)
MAX_TABLE = 1 << 27
# integer labels / values are histogrammed directly up to this range
MAX_INT_RANGE = 1 << 24
SORT_SEGMENTS = 32  # columns per segmented sort call (radix.hip RS_MAXS)


def _mat(X: torch.Tensor) -> torch.Tensor:
    if X.dim() == 1:
        X = X.reshape(-1, 1)
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    if X.stride(1) != 1:
        X = X.contiguous()
    return X


def flags(X: torch.Tensor) -> Tuple[float, float, bool]:
    """(min, max, any non-integer or non-finite) of all elements of X (device reduction)."""
    X = _mat(X)
    n, d = X.shape
    if n * d == 0:
        return float("inf"), float("-inf"), False
    dev = X.device
    part = torch.empty(3 * 1024, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    native.call("fmlx_cs_flags", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, d, native.ptr(part),
                native.ptr(out), native.stream_ptr(dev))
    mn, mx, non = out.cpu().tolist()
    return mn, mx, non != 0.0


CODE_COUNTS_MAX_V = 4096  # dictionary sizes of the one-pass count kernel (csrc/hash.hip cv_tfdf_kernel)
CODE_COUNTS_SEG = 4096  # codes per pseudo-document (the kernel's unit of work per wave)


def code_counts_first(codes: torch.Tensor, V: int):
    """(count, first position) per dictionary code in [0, V) of a device int32 code column, host
    int64 arrays, in one pass of the CountVectorizer tf kernel over fixed-size segments (the
    column cut into pseudo-documents; their document frequencies are not used). None when V is
    beyond the kernel's LDS tables."""
    n = codes.shape[0]
    if not codes.is_cuda or V < 1 or V > CODE_COUNTS_MAX_V or n >= (1 << 32):
        return None
    dev = codes.device
    codes = codes.to(torch.int32).contiguous()
    seg = CODE_COUNTS_SEG
    nd = max(1, -(-n // seg))
    off = torch.from_numpy(np.minimum(np.arange(nd + 1, dtype=np.int64) * seg, n)).to(dev)
    out = torch.zeros(3 * V, dtype=torch.int64, device=dev)  # count | (unused) | first
    out[2 * V:] = n
    if n:
        native.call("fmlx_cv_tfdf", native.ptr(codes), native.ptr(off), nd, V, native.ptr(out), native.ptr(out[V:]),
                    native.ptr(out[2 * V:]), native.stream_ptr(dev))
    h = out.cpu().numpy().reshape(3, V)
    return h[0], h[2]


SMALL_DISTINCT_TABLE_MAX = 2048  # LDS hash-set slots (csrc/catstats.hip small_distinct_kernel)


def bounded_distinct_counts(X: torch.Tensor, cap: int):
    """Per column of a device fp64 matrix: the number of distinct values (NaN one value, −0 == +0)
    when it is at most ``cap``, else cap + 1 — one early-exit hash-set pass (a continuous column
    stops after a few hundred rows). None when cap is too large for the LDS table."""
    X = _mat(X)
    if X.dtype != torch.float64:
        X = X.to(torch.float64)
    if X.stride(1) != 1:
        X = X.contiguous()
    n, d = X.shape
    S = 1
    while S < 2 * cap + 256:
        S <<= 1
    if cap < 1 or S > SMALL_DISTINCT_TABLE_MAX or d > 65535:
        return None
    dev = X.device
    gtab = torch.full((d * S,), -1, dtype=torch.int64, device=dev)
    ints = torch.zeros(2 * d, dtype=torch.int32, device=dev)  # counts | overflow flags
    if n and d:
        native.call("fmlx_cs_small_distinct", native.ptr(X), X.stride(0), n, d, int(cap), S, native.ptr(gtab),
                    native.ptr(ints), native.ptr(ints[d:]), native.stream_ptr(dev))
    h = ints.cpu().numpy()
    return np.where(h[d:] != 0, cap + 1, h[:d]).astype(np.int64)


def int_hist(v: torch.Tensor, lo: int, R: int) -> torch.Tensor:
    """int32 counts of the integer values lo … lo + R − 1 of the 1-D tensor ``v`` (device)."""
    dev = v.device
    if v.dtype not in (torch.float32, torch.float64, torch.int32):
        v = v.to(torch.float64)
    v = v.reshape(-1, 1).contiguous()
    counts = torch.zeros(max(1, R), dtype=torch.int32, device=dev)
    if v.shape[0]:
        native.call("fmlx_cs_ihist", native.dtype_code(v.dtype), native.ptr(v), 1, v.shape[0], 0, int(lo), int(R),
                    native.ptr(counts), native.stream_ptr(dev))
    return counts[:R]


def distinct_codes(X: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Per column j of X [n, d]: the sorted distinct values (fp64, device; −0 folded into +0, NaN
    last) and every row's index into them: codes int32 [d, n]."""
    X = _mat(X)
    n, d = X.shape
    dev = X.device
    codes = torch.empty((d, n), dtype=torch.int32, device=dev)
    vals: List[torch.Tensor] = []
    tile = int(native.kernels().fmlx_cs_tile())
    for j0 in range(0, d, SORT_SEGMENTS):
        nc = min(SORT_SEGMENTS, d - j0)
        m = n * nc
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        rows = torch.empty(m, dtype=torch.int32, device=dev)
        orand = torch.tensor([0, -1], dtype=torch.int64, device=dev)
        native.call("fmlx_cs_col_keys", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, j0, nc,
                    native.ptr(keys), native.ptr(rows), native.ptr(orand), native.stream_ptr(dev))
        lo, hi = sorting.bit_range(orand)
        keys, rows = sorting.sort_u64(keys, rows, [c * n for c in range(nc + 1)], lo, hi)
        nt = max(1, -(-m // tile))
        tcnt = torch.empty(nt + 1, dtype=torch.int64, device=dev)
        uval = torch.empty(max(1, m), dtype=torch.float64, device=dev)
        ucol = torch.empty(max(1, m), dtype=torch.int32, device=dev)
        colfirst = torch.zeros(nc, dtype=torch.int64, device=dev)
        native.call("fmlx_cs_distinct", native.ptr(keys), native.ptr(rows), n, nc, j0, native.ptr(tcnt), 0,
                    native.ptr(codes[j0:j0 + nc]), native.ptr(uval), native.ptr(ucol), native.ptr(colfirst),
                    native.stream_ptr(dev))
        if n == 0:
            vals += [torch.empty(0, dtype=torch.float64, device=dev) for _ in range(nc)]
            continue
        first = colfirst.cpu().tolist() + [int(tcnt[nt].item())]
        vals += [uval[first[c]:first[c + 1]] for c in range(nc)]
    return codes, vals


def sorted_unique(v: torch.Tensor) -> torch.Tensor:
    """Sorted distinct values of a 1-D tensor (fp64): a presence histogram for small-range
    integers, else the sorted-column distinct pass."""
    v = v.reshape(-1)
    if v.numel() == 0:
        return torch.empty(0, dtype=torch.float64, device=v.device)
    mn, mx, non = flags(v)
    if not non and mx - mn + 1 <= MAX_INT_RANGE:
        cnt = int_hist(v, int(mn), int(mx - mn) + 1)
        present = np.nonzero(cnt.cpu().numpy())[0]
        return torch.as_tensor(present + int(mn), dtype=torch.float64).to(v.device)
    return distinct_codes(v)[1][0]


def label_index(y: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int32 index of every y in the sorted ``labels`` (a binary search per row)."""
    return torch.searchsorted(labels.to(torch.float64), y.reshape(-1).to(torch.float64)).to(torch.int32)


def label_counts(li: torch.Tensor, L: int) -> torch.Tensor:
    """int64 rows per label index 0 … L − 1."""
    return int_hist(li.to(torch.int32), 0, L).to(torch.int64)


def int_table(X: torch.Tensor, li: torch.Tensor, L: int, vmin: int, V: int) -> torch.Tensor:
    """int32 [d, L, V] counts of the integer values vmin … vmin + V − 1 per (feature, label
    index) — one pass over X (LDS-privatised table when d·L·V fits)."""
    X = _mat(X)
    n, d = X.shape
    dev = X.device
    counts = torch.zeros(max(1, d * L * V), dtype=torch.int32, device=dev)
    if n and d:
        native.call("fmlx_cs_hist", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, d,
                    native.ptr(li.to(torch.int32).contiguous()), L, int(vmin), int(V), native.ptr(counts),
                    native.stream_ptr(dev))
    return counts[:d * L * V].reshape(d, L, V)


def value_label_counts(X: torch.Tensor, li: torch.Tensor, L: int,
                       int_range: Optional[Tuple[float, float]] = None):
    """(feature, distinct value, label) counts of one rank's rows.

    Returns (counts int64 [d, L, Vmax] numpy, per-feature sorted distinct values as numpy fp64,
    per-feature slots of those values in the last axis). ``int_range`` = (min, max) when X is
    known to hold integers (the caller's flags, possibly all-reduced): the direct table path."""
    X = _mat(X)
    n, d = X.shape
    dev = X.device
    li = li.to(torch.int32).contiguous()
    if int_range is None:
        mn, mx, non = flags(X)
        int_range = None if non else (mn, mx)
    if int_range is not None and n and (int_range[1] - int_range[0] + 1) * L * d <= MAX_TABLE:
        vmin = int(int_range[0])
        V = int(int_range[1]) - vmin + 1
        c = int_table(X, li, L, vmin, V).cpu().numpy().astype(np.int64)
        present = c.sum(1) > 0
        slots = [np.nonzero(present[j])[0] for j in range(d)]
        return c, [(sl + vmin).astype(np.float64) for sl in slots], slots
    codes, vals = distinct_codes(X)
    Vn = [int(v.numel()) for v in vals]
    Vmax = max([1] + Vn)
    coloff = torch.arange(d, dtype=torch.int64, device=dev) * Vmax
    counts = torch.zeros(max(1, d * Vmax * L), dtype=torch.int32, device=dev)
    native.call("fmlx_cs_chist", native.ptr(codes), n, d, native.ptr(coloff), native.ptr(li), L, native.ptr(counts),
                native.stream_ptr(dev))
    c = counts[:d * Vmax * L].reshape(d, Vmax, L).permute(0, 2, 1).cpu().numpy().astype(np.int64)
    return c, [v.cpu().numpy() for v in vals], [np.arange(V) for V in Vn]


def global_value_label_counts(X: torch.Tensor, li: torch.Tensor, L: int):
    """(feature, distinct value, label) counts over ALL ranks on the native kernels — the keyed
    count of ``ChiSqTest.java:127-155`` / ``NaiveBayes.java:95-103`` without a keyed shuffle:

    * integer features whose [d, L, V] table (value range from the all-reduced min / max) has at
      most MAX_TABLE cells: one ``int_table`` pass per rank, then ONE all-reduce of the dense table;
    * otherwise every rank takes its per-column sorted distinct values (``value_label_counts``:
      radix sort + distinct pass), the ranks' value lists are all-gathered (padded to the longest,
      the padding repeating a real value of the column) and their union per column is one more
      ``distinct_codes`` pass; each rank places its local counts at their union slots (a host
      binary search over the small per-column lists) and one all-reduce sums the tables.

    Returns (counts float64 [d, L, Vmax] numpy, per-feature sorted distinct values (numpy fp64),
    per-feature slots of those values in the last axis) — the shape ``value_label_counts`` returns
    on one rank."""
    from ..parallel import comm

    X = _mat(X)
    n, d = X.shape
    dev = X.device
    mn, mx, non = flags(X) if n else (float("inf"), float("-inf"), False)
    f = comm.all_reduce(torch.tensor([-mn, mx, float(non)], dtype=torch.float64, device=dev), "max").tolist()
    mn, mx, non = -f[0], f[1], f[2] != 0.0
    if not non and mx >= mn and (mx - mn + 1) * L * d <= MAX_TABLE:
        vmin, V = int(mn), int(mx - mn) + 1
        cnt = comm.all_reduce_sum(int_table(X, li, L, vmin, V).to(torch.float64)) if n else \
            comm.all_reduce_sum(torch.zeros((d, L, V), dtype=torch.float64, device=dev))
        counts = cnt.cpu().numpy()
        present = counts.sum(1) > 0
        slots = [np.nonzero(present[j])[0] for j in range(d)]
        return counts, [(sl + vmin).astype(np.float64) for sl in slots], slots
    if n:
        c_loc, vals_loc, slots_loc = value_label_counts(X, li, L, int_range=None)
    else:
        c_loc, vals_loc, slots_loc = np.zeros((d, L, 1), np.int64), [np.zeros(0)] * d, [np.zeros(0, np.int64)] * d
    vl = np.array([len(v) for v in vals_loc], dtype=np.int64)
    M = int(comm.all_reduce(torch.tensor([int(vl.max()) if d else 0], dtype=torch.int64, device=dev), "max")[0])
    M = max(M, 1)
    pad = np.zeros((M, d), dtype=np.float64)
    for j in range(d):
        if vl[j]:
            pad[:vl[j], j] = vals_loc[j]
    # (the gathered blocks carry each rank's list lengths in a last row)
    blk = torch.from_numpy(np.concatenate([pad, vl[None, :].astype(np.float64)], 0)).to(dev)
    gathered = comm.all_gather_tensor(blk)
    G = torch.stack(gathered)                   # [world, M + 1, d]
    lens = G[:, M, :].cpu().numpy().astype(np.int64)  # [world, d]
    vals_g = G[:, :M, :]
    rows = torch.arange(M, device=dev)[None, :, None]
    valid = rows < torch.as_tensor(lens, device=dev)[:, None, :]
    # padding repeats a real value of its column (the first one of the first rank holding one)
    first_r = np.argmax(lens > 0, axis=0)
    fill = vals_g[torch.as_tensor(first_r, device=dev), 0, torch.arange(d, device=dev)]
    U = torch.where(valid, vals_g, fill[None, None, :]).reshape(-1, d)
    _, union = distinct_codes(U)
    union = [u.cpu().numpy() if int(lens[:, j].sum()) else np.zeros(0) for j, u in enumerate(union)]
    Umax = max([1] + [len(u) for u in union])
    T = np.zeros((d, L, Umax), dtype=np.float64)
    for j in range(d):
        if vl[j]:
            pos = np.searchsorted(union[j], vals_loc[j])
            T[j][:, pos] = c_loc[j][:, slots_loc[j]]
    T = comm.all_reduce_sum(torch.from_numpy(T).to(dev)).cpu().numpy()
    return T, union, [np.arange(len(u)) for u in union]


# ------------------------------------------------------------------------------------------------
# CSR feature columns (csrc/catstats_csr.hip): the same counts without an n x D matrix
# ------------------------------------------------------------------------------------------------
# The route is under FMLX_COLSTATS_CSR (ops/features.py): "0" densifies, "1" always takes it, "auto"
# takes it when the densified matrix would exceed the HBM budget or the density nnz / (n·D) is at
# most CATSTATS_CSR_CROSSOVER. The dense contingency route fills an fp64 n x D matrix and counts
# every cell, so the column statistics' constant does not transfer: this one is the highest density
# of a sweep of its own (100,000 rows, D = 1,024 and 16,384, densities 0.1 / 1 / 5 / 20 %;
# scripts/bench_catstats_sparse.py, profiles/r18/INDEX.md) at which the CSR route won in both run
# orders at both widths, for the tables alone and for ChiSqTest.compute. It won at every measured
# density, so the constant is the sweep's highest one; nothing above 20 % was measured.
CATSTATS_CSR_CROSSOVER = 0.2


class RaggedCounts:
    """Contingency tables of all features as one ragged table: feature j's sorted distinct values are
    ``values[colfirst[j]:colfirst[j + 1]]`` (fp64; −0 folded into +0, NaN last) and ``counts[u, l]``
    the rows of label index l that hold value u; ``n_label[l]`` the rows per label. ``paths``: the
    count kernel's tiles that went through LDS / global atomics; ``err``: the CSR error word."""

    __slots__ = ("colfirst", "values", "counts", "n_label", "paths", "err")

    def __init__(self, colfirst, values, counts, n_label, paths=None, err=None):
        self.colfirst, self.values, self.counts, self.n_label = colfirst, values, counts, n_label
        self.paths, self.err = paths, err

    def numpy(self):
        """(colfirst int64 [D + 1], values fp64 [U], counts int64 [U, L], n_label int64 [L]) on the host."""
        return (self.colfirst.cpu().numpy().astype(np.int64), self.values.cpu().numpy(),
                self.counts.cpu().numpy().astype(np.int64), self.n_label.cpu().numpy().astype(np.int64))


class StoredCounts:
    """The stored entries' part of a table, before the zero rows: distinct (column, value) pairs in
    sorted order, ``ucol[U]`` (int32), ``uval[U]`` (fp64), ``cnt[U, L]``."""

    __slots__ = ("ucol", "uval", "cnt", "paths", "err")

    def __init__(self, ucol, uval, cnt, paths=None, err=None):
        self.ucol, self.uval, self.cnt, self.paths, self.err = ucol, uval, cnt, paths, err


def catstats_csr_route(X, device) -> bool:
    """Whether the contingency counts of a ``SparseColumn`` take the CSR path."""
    from . import features as fo
    from ..table import SparseColumn

    if fo.COLSTATS_CSR_ROUTE == "0" or not isinstance(X, SparseColumn):
        return False
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    if n >= 2 ** 31 or nnz >= 2 ** 31 - 1 or D >= 2 ** 31 or D < 1:
        return False
    if fo.COLSTATS_CSR_ROUTE == "1":
        return True
    device = torch.device(device)
    if device.type == "cuda":
        from .. import config
        from ..common.outofcore import hbm_budget

        budget = hbm_budget(device)
        if budget is not None and n * D * torch.empty(0, dtype=config.compute_dtype()).element_size() > budget:
            return True
    return nnz <= CATSTATS_CSR_CROSSOVER * n * D


def _np_stored(col: np.ndarray, val: np.ndarray, L: int, lab: np.ndarray = None, W: np.ndarray = None):
    """Distinct (column, value) pairs of entries in sorted order and their counts per label: one per
    entry at its label index ``lab``, or the entry's row of ``W`` [m, L]."""
    v = val.astype(np.float64) + 0.0  # −0 → +0
    order = np.lexsort((v, col))      # (NaN sorts last)
    c, v = col[order], v[order]
    m = c.shape[0]
    head = np.ones(m, dtype=bool)
    head[1:] = (c[1:] != c[:-1]) | ~((v[1:] == v[:-1]) | (np.isnan(v[1:]) & np.isnan(v[:-1])))
    gid = np.cumsum(head) - 1
    U = int(gid[-1]) + 1 if m else 0
    if W is None:
        cnt = np.bincount(gid * L + lab[order], minlength=U * L).reshape(U, L).astype(np.int64)
    else:
        cnt = np.zeros((U, L), dtype=np.int64)
        np.add.at(cnt, gid, W[order])
    return c[head].astype(np.int32), v[head], cnt


def _np_zero_merge(ucol, uval, cnt, D: int, n_label: np.ndarray):
    """The final table of stored counts: per column the zero row n_label − Σ of its other rows, added
    to a stored zero's row, inserted at its sorted place when any row does not store the column."""
    L = n_label.shape[0]
    stored = np.zeros(D, dtype=np.int64)
    np.add.at(stored, ucol, cnt.sum(1))
    has_zero = np.zeros(D, dtype=bool)
    has_zero[ucol[uval == 0.0]] = True
    ins = np.nonzero(~has_zero & (stored < int(n_label.sum())))[0].astype(np.int32)
    col = np.concatenate([ucol, ins])
    val = np.concatenate([uval, np.zeros(ins.shape[0])])
    out = np.concatenate([cnt, np.zeros((ins.shape[0], L), dtype=np.int64)])
    order = np.lexsort((val, col))
    col, val, out = col[order], val[order], out[order]
    colfirst = np.searchsorted(col, np.arange(D + 1)).astype(np.int64)
    z = np.nonzero(val == 0.0)[0]
    others = out.copy()
    others[z] = 0
    run = np.concatenate([np.zeros((1, L), dtype=np.int64), np.cumsum(others, 0)])
    jz = col[z]
    out[z] = n_label[None, :] - (run[colfirst[jz + 1]] - run[colfirst[jz]])
    return colfirst, val, out


def _np_entries(X, li, L: int):
    """(column, value, label index) of the entries of a host ``SparseColumn``; raises for a column
    outside [0, size); entries of rows without a label index in [0, L) are dropped."""
    n = len(X)
    col = X.indices.cpu().numpy().astype(np.int64)
    if col.size and (col.min() < 0 or col.max() >= X.size):
        raise ValueError("sparse feature index out of range [0, size)")
    ptr = X.indptr.cpu().numpy().astype(np.int64)
    lab = np.repeat(np.asarray(li.cpu().numpy(), dtype=np.int64), ptr[1:] - ptr[:-1]) if n else np.zeros(0, np.int64)
    val = X.values.cpu().numpy()
    ok = (lab >= 0) & (lab < L)
    return col[ok], val[ok], lab[ok]


def _ragged_from_np(colfirst, val, out, n_label, device="cpu", paths=None, err=None) -> RaggedCounts:
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return RaggedCounts(t(colfirst), t(val), t(out), t(n_label), paths, err)


def torch_value_label_counts_csr(X, li: torch.Tensor, L: int) -> RaggedCounts:
    """``value_label_counts_csr`` from the CSR arrays alone on the host (numpy, no n x D array): the
    CPU path of the route and the oracle of the kernels. Raises for an index outside [0, size)."""
    col, val, lab = _np_entries(X, li, L)
    n_label = np.bincount(np.asarray(li.cpu().numpy(), dtype=np.int64), minlength=L)[:L].astype(np.int64)
    ucol, uval, cnt = _np_stored(col, val, L, lab)
    return _ragged_from_np(*_np_zero_merge(ucol, uval, cnt, X.size, n_label), n_label)


def _value_ranks(val: torch.Tensor):
    """(vid uint32-in-int32 [m], gval fp64): every fp64 value's rank among the distinct values (one
    sort of the 64-bit value keys; the value 0 is always one of them) and the values by rank."""
    dev, m = val.device, int(val.numel())
    keys = torch.empty(m + 1, dtype=torch.int64, device=dev)
    pay = torch.empty(m + 1, dtype=torch.int32, device=dev)
    orand = torch.tensor([0, -1], dtype=torch.int64, device=dev)
    stream = native.stream_ptr(dev)
    native.call("fmlx_ccsr_vkeys", native.ptr(val), m, native.ptr(keys), native.ptr(pay), native.ptr(orand), stream)
    lo, hi = sorting.bit_range(orand)
    keys, pay = sorting.sort_u64(keys, pay, [0, m + 1], lo, hi)
    tile = int(native.kernels().fmlx_ccsr_tile())
    tcnt = torch.empty(-(-(m + 1) // tile) + 1, dtype=torch.int64, device=dev)
    vid = torch.empty(max(1, m), dtype=torch.int32, device=dev)
    gval = torch.empty(m + 1, dtype=torch.float64, device=dev)
    native.call("fmlx_ccsr_vids", native.ptr(keys), native.ptr(pay), m, native.ptr(tcnt), native.ptr(vid),
                native.ptr(gval), stream)
    return vid, gval


def _count_runs(keys, pay, orand, total: int, L: int, W, gval, err) -> Optional[StoredCounts]:
    """Sort (column, k32) keys, scan their runs and count per run and label. None when the table
    would pass MAX_TABLE cells."""
    dev = keys.device
    stream = native.stream_ptr(dev)
    lo, hi = sorting.bit_range(orand)
    keys, pay = sorting.sort_u64(keys, pay, [0, total], lo, hi)
    tile = int(native.kernels().fmlx_ccsr_tile())
    nt = -(-total // tile)
    tcnt = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    native.call("fmlx_ccsr_runs", native.ptr(keys), total, native.ptr(tcnt), stream)
    U = int(tcnt[nt].item())
    if U * L > MAX_TABLE:
        return None
    cnt = torch.zeros((U, L), dtype=torch.int32, device=dev)
    ucol = torch.empty(U, dtype=torch.int32, device=dev)
    uval = torch.empty(U, dtype=torch.float64, device=dev)
    paths = torch.zeros(2, dtype=torch.int32, device=dev)
    if U:
        native.call("fmlx_ccsr_count", native.ptr(keys), native.ptr(pay), total, native.ptr(tcnt), L, native.ptr(W),
                    native.ptr(gval), native.ptr(cnt), native.ptr(ucol), native.ptr(uval), native.ptr(paths), stream)
    return StoredCounts(ucol, uval, cnt, paths, err)


def _empty_stored(L: int, dev) -> StoredCounts:
    return StoredCounts(torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float64, device=dev),
                        torch.zeros((0, L), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev))


def stored_counts_csr(X, li: torch.Tensor, L: int) -> Optional[StoredCounts]:
    """Counts per (column, stored value, label index) of a ``SparseColumn`` on its device, before the
    zero rows. An index outside [0, size) is skipped and sets ``err`` (``ops.kmeans.check_csr_error``)
    on the GPU and raises on the CPU. None when the table would pass MAX_TABLE cells."""
    dev = X.values.device
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    if dev.type != "cuda":
        col, val, lab = _np_entries(X, li, L)
        ucol, uval, cnt = _np_stored(col, val, L, lab)
        if cnt.size > MAX_TABLE:
            return None
        return StoredCounts(torch.from_numpy(ucol), torch.from_numpy(uval), torch.from_numpy(cnt))
    if nnz == 0 or n == 0:
        return _empty_stored(L, dev)
    indptr = X.indptr.to(torch.int64).contiguous()
    idx = X.indices.to(torch.int32).contiguous()
    li = li.to(device=dev, dtype=torch.int32).contiguous()
    if X.values.dtype == torch.float32:
        val, vid, gval = X.values.contiguous(), None, None
    else:
        val = None
        vid, gval = _value_ranks(X.values.to(torch.float64).contiguous())
    keys = torch.empty(nnz, dtype=torch.int64, device=dev)
    pay = torch.empty(nnz, dtype=torch.int32, device=dev)
    orand = torch.tensor([0, -1], dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    native.call("fmlx_ccsr_keys", native.ptr(indptr), native.ptr(idx), native.ptr(val), native.ptr(vid), native.ptr(li),
                n, D, L, native.ptr(keys), native.ptr(pay), native.ptr(orand), native.ptr(err), native.stream_ptr(dev))
    return _count_runs(keys, pay, orand, nnz, L, None, gval, err)


def merge_stored_counts(col: torch.Tensor, val: torch.Tensor, W: torch.Tensor, D: int) -> Optional[StoredCounts]:
    """One table of several: rows (col[m], val[m], W[m, L]) with repeated (column, value) pairs summed
    by the same sort + run pass, the rows' counts as weights."""
    dev, m, L = val.device, int(val.numel()), int(W.shape[1])
    if dev.type != "cuda":
        ucol, uval, cnt = _np_stored(col.numpy().astype(np.int64), val.numpy(), L, W=W.numpy().astype(np.int64))
        return StoredCounts(torch.from_numpy(ucol), torch.from_numpy(uval), torch.from_numpy(cnt))
    if m == 0:
        return _empty_stored(L, dev)
    vid, gval = _value_ranks(val.to(torch.float64).contiguous())
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    pay = torch.empty(m, dtype=torch.int32, device=dev)
    orand = torch.tensor([0, -1], dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    native.call("fmlx_ccsr_ekeys", native.ptr(col.to(torch.int32).contiguous()), native.ptr(vid), m, D, native.ptr(keys),
                native.ptr(pay), native.ptr(orand), native.ptr(err), native.stream_ptr(dev))
    return _count_runs(keys, pay, orand, m, L, W.to(torch.int32).contiguous(), gval, err)


def zero_merge(st: StoredCounts, D: int, n_label: torch.Tensor) -> Optional[RaggedCounts]:
    """The final ragged table of stored counts and the label totals (int64 [L]). None when it would
    pass MAX_TABLE cells."""
    dev = st.uval.device
    L = int(n_label.numel())
    if dev.type != "cuda":
        out = _np_zero_merge(st.ucol.numpy(), st.uval.numpy(), st.cnt.numpy().astype(np.int64), D,
                             n_label.numpy().astype(np.int64))
        return None if out[2].size > MAX_TABLE else _ragged_from_np(*out, n_label.numpy().astype(np.int64))
    U = int(st.uval.numel())
    stream = native.stream_ptr(dev)
    n_label = n_label.to(device=dev, dtype=torch.int64).contiguous()
    gf = torch.empty(D + 1, dtype=torch.int64, device=dev)
    flag = torch.empty(D, dtype=torch.int32, device=dev)
    zr = torch.empty(D, dtype=torch.int32, device=dev)
    colfirst = torch.empty(D + 1, dtype=torch.int64, device=dev)
    native.call("fmlx_ccsr_columns", native.ptr(st.ucol), native.ptr(st.uval), native.ptr(st.cnt), U, D, L,
                int(n_label.sum().item()), native.ptr(gf), native.ptr(flag), native.ptr(zr), native.ptr(colfirst), stream)
    Uo = int(colfirst[D].item())
    if Uo * L > MAX_TABLE:
        return None
    values = torch.empty(Uo, dtype=torch.float64, device=dev)
    out = torch.empty((Uo, L), dtype=torch.int32, device=dev)
    native.call("fmlx_ccsr_merge", native.ptr(st.ucol), native.ptr(st.uval), native.ptr(st.cnt), U, D, L, native.ptr(gf),
                native.ptr(flag), native.ptr(zr), native.ptr(colfirst), native.ptr(n_label), native.ptr(values),
                native.ptr(out), stream)
    return RaggedCounts(colfirst, values, out, n_label, st.paths, st.err)


def _n_label(li: torch.Tensor, L: int) -> torch.Tensor:
    if li.is_cuda:
        return label_counts(li, L) if li.numel() else torch.zeros(L, dtype=torch.int64, device=li.device)
    return torch.bincount(li.to(torch.int64), minlength=L)[:L]


def value_label_counts_csr(X, li: torch.Tensor, L: int, check: bool = True) -> Optional[RaggedCounts]:
    """(feature, distinct value, label) counts of a ``SparseColumn`` on its device as a ragged table,
    the rows that store nothing in a column counting as the value 0. Exact (integer counts). None
    when the table would pass MAX_TABLE cells: the caller densifies. ``check``: raise for an index
    outside [0, size) (else the entry is skipped and ``err`` set)."""
    if X.values.device.type != "cuda":
        return torch_value_label_counts_csr(X, li, L)
    st = stored_counts_csr(X, li, L)
    res = zero_merge(st, X.size, _n_label(li.to(X.values.device), L)) if st is not None else None
    if check and st is not None:
        from .kmeans import check_csr_error

        check_csr_error(st)
    return res


def global_value_label_counts_csr(X, li: torch.Tensor, L: int) -> Optional[RaggedCounts]:
    """``value_label_counts_csr`` over ALL ranks: every rank's stored-entry table and label totals,
    the tables all-gathered (padded to the longest) and merged by the same sort + run pass with the
    counts as weights, then the zero rows from the all-reduced label totals. No keyed shuffle, no
    library sort; every rank ends with the same table."""
    from ..parallel import comm

    dev = X.values.device
    li = li.to(dev)
    st = stored_counts_csr(X, li, L)
    # (too large a table or a bad index on one rank: every rank learns it before the next collective)
    bad = 1.0 if st is not None and st.err is not None and int(st.err.item()) else 0.0
    over = comm.all_reduce(torch.tensor([0.0 if st is not None else 1.0, bad], dtype=torch.float64, device=dev), "max")
    if float(over[1]) != 0.0:
        raise ValueError("sparse feature index out of range [0, size)")
    if float(over[0]) != 0.0:
        return None
    n_label = comm.all_reduce_sum(_n_label(li, L).to(torch.float64)).to(torch.int64)
    U = int(st.uval.numel())
    M = max(1, int(comm.all_reduce(torch.tensor([float(U)], dtype=torch.float64, device=dev), "max")[0]))
    blk = torch.zeros((M + 1, L + 2), dtype=torch.float64, device=dev)  # (col, value, counts); last row: U
    blk[:U, 0] = st.ucol.to(torch.float64)
    blk[:U, 1] = st.uval
    blk[:U, 2:] = st.cnt.to(torch.float64)
    blk[M, 0] = U
    G = [g.to(dev) for g in comm.all_gather_tensor(blk)]
    rows = torch.cat([g[:int(g[M, 0].item())] for g in G])
    merged = merge_stored_counts(rows[:, 0].to(torch.int32), rows[:, 1].contiguous(), rows[:, 2:].to(torch.int64), X.size)
    return zero_merge(merged, X.size, n_label) if merged is not None else None


# ------------------------------------------------------------------------------------------------
# NaiveBayes prediction on a CSR column (csrc/catstats_csr.hip nb_csr_predict)
# ------------------------------------------------------------------------------------------------
NB_NONE = 2 ** 31 - 1  # "no unseen value"


def torch_nb_csr_predict(X, off: torch.Tensor, vflat: torch.Tensor, delta: torch.Tensor, base: torch.Tensor):
    """``nb_csr_predict`` in torch over the CSR arrays alone (the CPU path): a vectorised binary
    search of every entry's value in its feature's value list, the deltas added in stored-entry
    order (``index_add_`` on the host), first maximum."""
    n, D = len(X), X.size
    idx = X.indices.to(torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= D):
        raise ValueError("sparse feature index out of range [0, size)")
    v = X.values.to(torch.float64)
    lo, hi = off[idx].clone(), off[idx + 1].clone()
    end = hi.clone()
    top = max(int(vflat.numel()) - 1, 0)
    vpad = vflat if vflat.numel() else torch.zeros(1, dtype=torch.float64, device=vflat.device)
    while bool((lo < hi).any()):
        act = lo < hi
        mid = (lo + hi) // 2
        less = vpad[mid.clamp(max=top)] < v
        lo = torch.where(act & less, mid + 1, lo)
        hi = torch.where(act & ~less, mid, hi)
    found = (lo < end) & (vpad[lo.clamp(max=top)] == v)
    unseen = int(idx[~found].min()) if bool((~found).any()) else NB_NONE
    ptr = X.indptr.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, device=v.device), ptr[1:] - ptr[:-1], output_size=int(idx.numel()))
    score = base[None, :].repeat(n, 1)
    score.index_add_(0, rows[found], delta[lo[found]])
    return torch.argmax(score, dim=1).to(torch.int32), unseen


def nb_csr_predict(X, off: torch.Tensor, vflat: torch.Tensor, delta: torch.Tensor, base: torch.Tensor):
    """(index of the first maximal score per row (int32), lowest feature with an unseen value or
    ``NB_NONE``) of a ``SparseColumn`` on the model's device. ``off`` [>= size + 1] / ``vflat``: the
    features' sorted values; ``delta`` [ΣV, L]: log-probabilities relative to each feature's value 0;
    ``base`` [L]. Raises ValueError for an index outside [0, size)."""
    dev = delta.device
    if dev.type != "cuda":
        return torch_nb_csr_predict(X, off, vflat, delta, base)
    from .csr import csr_arrays
    from .kmeans import check_csr_error

    n, D, L = len(X), X.size, int(base.numel())
    indptr, idx, val = csr_arrays(X, torch.float64)
    pred = torch.zeros(n, dtype=torch.int32, device=dev)
    unseen = torch.full((1,), NB_NONE, dtype=torch.int32, device=dev)
    holder = StoredCounts(None, None, None, None, torch.zeros(1, dtype=torch.int32, device=dev))
    if n and D:
        native.call("fmlx_nb_csr_predict", native.ptr(indptr), native.ptr(idx), native.ptr(val), n, D,
                    native.ptr(off.to(torch.int64).contiguous()), native.ptr(vflat.contiguous()),
                    native.ptr(delta.contiguous()), native.ptr(base.to(torch.float64).contiguous()), L, native.ptr(pred),
                    native.ptr(unseen), native.ptr(holder.err), native.stream_ptr(dev))
    check_csr_error(holder)
    return pred, int(unseen.item())
