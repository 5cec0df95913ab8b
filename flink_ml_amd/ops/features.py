"""Device ops shared by the feature transformers (``csrc/colstats.hip``) with torch fallbacks on CPU.

``column_stats`` is the K15 single-pass column reduction (sum, Σx², min, max) and
``affine_cols`` the K16 fused per-column ``(x - sub) * mul + add``; both work on the rank's
partition and the estimators all-reduce the fixed-size statistics across ranks.
``column_stats_csr`` / ``group_colstats_csr`` give the same statistics of a ``SparseColumn`` from
its CSR arrays (``csrc/colstats_csr.hip`` over the column-major copy of ``ops/csr.py``; on the CPU
the ``torch_*`` formulations), without an n x d matrix.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import native


def column_stats(X: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Per-column sum, sumsq, min, max (fp64) of a dense [n, d] tensor on the rank."""
    n, d = X.shape
    dev = X.device
    if n == 0:
        inf = float("inf")
        return {"sum": torch.zeros(d, dtype=torch.float64, device=dev),
                "sumsq": torch.zeros(d, dtype=torch.float64, device=dev),
                "min": torch.full((d,), inf, dtype=torch.float64, device=dev),
                "max": torch.full((d,), -inf, dtype=torch.float64, device=dev), "count": 0}
    if dev.type == "cuda" and X.dtype in (torch.float32, torch.float64, torch.bfloat16) and X.stride(1) == 1:
        nb = max(1, min(1024, (n + 1023) // 1024))
        part = torch.empty((nb, 4, d), dtype=torch.float64, device=dev)
        res = torch.empty((4, d), dtype=torch.float64, device=dev)
        native.call("fmlx_colstats", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, d, native.ptr(part),
                    nb, native.ptr(res), native.stream_ptr(dev))
        return {"sum": res[0], "sumsq": res[1], "min": res[2], "max": res[3], "count": n}
    Xd = X.to(torch.float64)
    return {"sum": Xd.sum(0), "sumsq": (Xd * Xd).sum(0), "min": Xd.min(0).values, "max": Xd.max(0).values,
            "count": n}


def affine_cols(X: torch.Tensor, sub: Optional[torch.Tensor] = None, mul: Optional[torch.Tensor] = None,
                add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(x - sub) * mul + add`` per column; output fp64 on CPU, fp32/fp64 on GPU."""
    n, d = X.shape
    dev = X.device
    prep = lambda v: None if v is None else v.to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
    sub, mul, add = prep(sub), prep(mul), prep(add)
    if dev.type == "cuda" and X.dtype in (torch.float32, torch.float64, torch.bfloat16) and X.stride(1) == 1:
        out_dt = torch.float64 if X.dtype == torch.float64 else torch.float32
        out = torch.empty((n, d), dtype=out_dt, device=dev)
        if n:
            native.call("fmlx_affine_cols", native.dtype_code(X.dtype), native.dtype_code(out_dt), native.ptr(X),
                        X.stride(0), n, d, native.ptr(sub), native.ptr(mul), native.ptr(add), native.ptr(out),
                        native.stream_ptr(dev))
        return out
    out = X.to(torch.float64)
    if sub is not None:
        out = out - sub
    if mul is not None:
        out = out * mul
    if add is not None:
        out = out + add
    return out


MAX_GROUPS = 32


def group_colstats(X: torch.Tensor, gidx: Optional[torch.Tensor] = None, G: int = 1,
                   w: Optional[torch.Tensor] = None):
    """Per-group weighted column sums S[G, d] = Σ_{group(r)=g} w_r·x_r, plus Σx and Σx² (all fp64)
    in one pass (``csrc/groupstats.hip`` on the GPU, G <= 32)."""
    n, d = X.shape
    dev = X.device
    if (dev.type == "cuda" and 1 <= G <= MAX_GROUPS and X.dtype in (torch.float32, torch.float64, torch.bfloat16)
            and X.stride(1) == 1 and n > 0):
        nb = max(1, min(1024, (n + 2047) // 2048))
        part = torch.empty((nb, (G + 2) * d), dtype=torch.float64, device=dev)
        res = torch.empty(((G + 2) * d,), dtype=torch.float64, device=dev)
        g = gidx.to(device=dev, dtype=torch.int32).contiguous() if gidx is not None else None
        ww = w.to(device=dev, dtype=torch.float64).contiguous() if w is not None else None
        native.call("fmlx_group_colstats", native.dtype_code(X.dtype), native.ptr(X), X.stride(0), n, d, native.ptr(g),
                    G, native.ptr(ww), native.ptr(part), nb, native.ptr(res), native.stream_ptr(dev))
        return res[:G * d].reshape(G, d), res[G * d:(G + 1) * d], res[(G + 1) * d:]
    Xd = X.to(torch.float64)
    wx = Xd * w.to(dev, torch.float64)[:, None] if w is not None else Xd
    if gidx is None:
        S = wx.sum(0, keepdim=True).expand(G, d).clone() if G == 1 else None
    else:
        S = torch.zeros((G, d), dtype=torch.float64, device=dev).index_add_(0, gidx.to(dev).long(), wx)
    return S, Xd.sum(0), (Xd * Xd).sum(0)


# ------------------------------------------------------------------------------------------------
# CSR feature columns (csrc/colstats_csr.hip): the same statistics without an n x D matrix
# ------------------------------------------------------------------------------------------------
# FMLX_COLSTATS_CSR: "0" = a SparseColumn is densified (the path before the CSR kernel), "1" = the
# CSR path for every sparse column, "auto" = the CSR path when the densified matrix would exceed the
# HBM budget (GPU only) or the density nnz / (n·D) is at most COLSTATS_CSR_CROSSOVER. The rule is the
# same on CPU and GPU; ranks may route differently (both routes all-reduce the same vectors).
COLSTATS_CSR_ROUTE = os.environ.get("FMLX_COLSTATS_CSR", "auto")
# the highest density of the measured sweep (100,000 rows, D = 1,024 and 16,384; scripts/
# bench_colstats_sparse.py, profiles/r17/INDEX.md) at which the CSR route (copy included) beat
# to_dense + the dense kernel in both run orders at both widths: at 5 % the fp32 to_dense +
# colstats wins at D = 1,024 (the per-group route against the fp64 to_dense wins through 20 %)
COLSTATS_CSR_CROSSOVER = 0.01


def csr_stats_route(X, device) -> bool:
    """Whether the column statistics of a ``SparseColumn`` take the CSR path (``COLSTATS_CSR_ROUTE``)."""
    from ..table import SparseColumn

    if COLSTATS_CSR_ROUTE == "0" or not isinstance(X, SparseColumn):
        return False
    n, D, nnz = len(X), X.size, int(X.indices.numel())
    if n >= 2 ** 31 or nnz >= 2 ** 31 or D >= 2 ** 31:
        return False
    if COLSTATS_CSR_ROUTE == "1":
        return True
    device = torch.device(device)
    if device.type == "cuda":
        from .. import config
        from ..common.outofcore import hbm_budget

        budget = hbm_budget(device)
        if budget is not None and n * D * torch.empty(0, dtype=config.compute_dtype()).element_size() > budget:
            return True
    return nnz <= COLSTATS_CSR_CROSSOVER * n * D


def _csr_entries(X):
    """(column, fp64 value) of every entry; raises for a column outside [0, size)."""
    idx, v = X.indices.to(torch.int64), X.values.to(torch.float64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= X.size):
        raise ValueError("sparse feature index out of range [0, size)")
    return idx, v


def torch_column_stats_csr(X) -> Dict[str, torch.Tensor]:
    """``column_stats`` of a ``SparseColumn`` from its CSR arrays alone (fp64; no n x D array), the
    rows that store nothing in a column counting as zeros; plus ``stored``, the entries per column.
    A NaN never wins a min / max, as in the kernels."""
    n, D, dev = len(X), X.size, X.values.device
    idx, v = _csr_entries(X)
    zero = torch.zeros(D, dtype=torch.float64, device=dev)
    inf = torch.full((D,), float("inf"), dtype=torch.float64, device=dev)
    nan = torch.isnan(v)
    mn = inf.scatter_reduce(0, idx, torch.where(nan, inf[:1], v), "amin")
    mx = (-inf).scatter_reduce(0, idx, torch.where(nan, -inf[:1], v), "amax")
    stored = torch.bincount(idx, minlength=D)
    implicit = stored < n
    mn = torch.where(implicit & (zero < mn), zero, mn)
    mx = torch.where(implicit & (zero > mx), zero, mx)
    return {"sum": zero.clone().index_add_(0, idx, v), "sumsq": zero.clone().index_add_(0, idx, v * v), "min": mn,
            "max": mx, "count": n, "stored": stored}


def torch_group_colstats_csr(X, gidx: Optional[torch.Tensor] = None, G: int = 1, w: Optional[torch.Tensor] = None):
    """``group_colstats`` of a ``SparseColumn`` from its CSR arrays alone (fp64; no n x D array).
    ``gidx`` None: one group; a row whose group is outside [0, G) adds to no group."""
    n, D, dev = len(X), X.size, X.values.device
    idx, v = _csr_entries(X)
    indptr = X.indptr.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:] - indptr[:-1], output_size=int(idx.numel()))
    wv = v * w.to(device=dev, dtype=torch.float64)[rows] if w is not None else v
    g = gidx.to(device=dev, dtype=torch.int64)[rows] if gidx is not None else torch.zeros_like(idx)
    ok = (g >= 0) & (g < G)
    S = torch.zeros(G * D, dtype=torch.float64, device=dev).index_add_(0, g[ok] * D + idx[ok], wv[ok])
    zero = torch.zeros(D, dtype=torch.float64, device=dev)
    return S.reshape(G, D), zero.clone().index_add_(0, idx, v), zero.clone().index_add_(0, idx, v * v)


def colstats_csr_windows(cm, gidx: Optional[torch.Tensor] = None, G: int = 1, w: Optional[torch.Tensor] = None):
    """The kernel over a column-major copy ``cm`` (``ops.csr.ColumnMajor``), one launch per window
    of ``MAX_GROUPS`` groups: ``(S[G, D], Σx, Σx², min, max, stored)``. A bad index of the copy is
    skipped, not raised (``cm.err``; ``group_colstats_csr`` / ``column_stats_csr`` raise)."""
    dev = cm.cval.device
    D, G = cm.D, int(G)
    if G < 1 or (gidx is None and G != 1):
        raise ValueError("G groups need a group index per row")
    g = gidx.to(device=dev, dtype=torch.int32).contiguous() if gidx is not None else None
    ww = w.to(device=dev, dtype=torch.float64).contiguous() if w is not None else None
    if (g is not None and g.numel() != cm.n) or (ww is not None and ww.numel() != cm.n):
        raise ValueError("one group / weight per row")
    partial = torch.empty(max(cm.nsegs, 1) * 37, dtype=torch.float64, device=dev)
    stored = torch.empty(D, dtype=torch.int64, device=dev)
    S, res = [], None
    for g0 in range(0, G, MAX_GROUPS):
        Gw = min(MAX_GROUPS, G - g0)
        res = torch.empty((Gw + 4, D), dtype=torch.float64, device=dev)
        native.call("fmlx_colstats_csr", int(cm.acc == torch.float64), native.ptr(cm.colptr), native.ptr(cm.crow),
                    native.ptr(cm.cval), native.ptr(g), native.ptr(ww), cm.n, cm.nnz, D, g0, Gw, cm.seg, cm.nlong,
                    native.ptr(cm.long_col), native.ptr(cm.long_seg0), cm.nsegs, native.ptr(cm.seg_col),
                    native.ptr(cm.seg_k), native.ptr(partial), native.ptr(res), native.ptr(stored),
                    native.stream_ptr(dev))
        S.append(res[:Gw])
    return (S[0] if len(S) == 1 else torch.cat(S)), res[-4], res[-3], res[-2], res[-1], stored


def _column_major(X):
    from .csr import ColumnMajor

    return X if isinstance(X, ColumnMajor) else ColumnMajor(X)


def group_colstats_csr(X, gidx: Optional[torch.Tensor] = None, G: int = 1, w: Optional[torch.Tensor] = None):
    """``group_colstats`` for a ``SparseColumn`` (or its ``ColumnMajor`` copy): ``(S[G, D], Σx, Σx²)``
    in fp64, deterministic. G > 32 runs the kernel once per window of 32 groups over the same copy.
    On the CPU the torch formulation. Raises ValueError for an index outside [0, size)."""
    from .csr import ColumnMajor
    from .kmeans import check_csr_error

    if not isinstance(X, ColumnMajor) and (X.values.device.type != "cuda" or X.size < 1):
        return torch_group_colstats_csr(X, gidx, G, w)
    cm = _column_major(X)
    S, sm, sq, _, _, _ = colstats_csr_windows(cm, gidx, G, w)
    check_csr_error(cm)
    return S, sm, sq


def column_stats_csr(X) -> Dict[str, torch.Tensor]:
    """``column_stats`` for a ``SparseColumn`` (or its ``ColumnMajor`` copy) without densifying:
    sum, sumsq, min, max (fp64; rows that store nothing in a column count as zeros), ``count`` =
    the rows (empty ones included) and ``stored`` = the entries per column."""
    from .csr import ColumnMajor
    from .kmeans import check_csr_error

    if not isinstance(X, ColumnMajor) and (X.values.device.type != "cuda" or X.size < 1):
        return torch_column_stats_csr(X)
    cm = _column_major(X)
    _, sm, sq, mn, mx, stored = colstats_csr_windows(cm)
    check_csr_error(cm)
    return {"sum": sm, "sumsq": sq, "min": mn, "max": mx, "count": cm.n, "stored": stored}
