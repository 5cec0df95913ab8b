"""The column-major copy of a device-resident CSR feature column, shared by the kernels that reduce
a ``SparseColumn`` per column without an n x D matrix (``csrc/kmeans_csr.hip``: the centroid
update; ``csrc/colstats_csr.hip``: the column statistics).

Built once per fit on the device: (column, entry id) of every entry through the stable segmented
radix sort (``ops.glm.seg_sort``: one segment, ceil(log2 D) key bits), so a column's entries stay in
row order and every per-column sum has one fixed order. A column longer than the segment length is
reduced in segments, one wave each, whose partials fold in segment order (text columns are
Zipf-distributed: one wave per column would run as long as the most frequent term).
"""
from __future__ import annotations

import torch

from . import native


def csr_arrays(X, dtype):
    return (X.indptr.to(torch.int64).contiguous(), X.indices.to(torch.int32).contiguous(),
            X.values.to(dtype).contiguous())


class ColumnMajor:
    """``colptr[D + 1]`` (int64), ``crow[nnz]`` (int32, the row of each entry), ``cval[nnz]`` (fp32
    or fp64) and the tables of the columns longer than ``seg`` entries: ``long_col[nlong]``,
    ``long_seg0[nlong + 1]`` (first segment of each), ``seg_col`` / ``seg_k[nsegs]`` (column and
    ordinal of each segment). ``indptr`` / ``idx`` / ``val`` are the row-major arrays it was built
    from. An index outside [0, D) is skipped (row -1) and sets ``err``: ``check_csr_error``."""

    def __init__(self, X, seg: int = None):
        from . import glm as _glm
        from . import kmeans as _km

        dev = X.values.device
        self.n, self.D = len(X), X.size
        self.acc = torch.float64 if X.values.dtype == torch.float64 else torch.float32
        self.indptr, self.idx, self.val = csr_arrays(X, self.acc)
        self.nnz = nnz = int(self.idx.numel())
        self.seg = int(_km.CSR_COL_SEGMENT if seg is None else seg)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.colptr = torch.zeros(self.D + 1, dtype=torch.int64, device=dev)
        self.crow = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        self.cval = torch.empty(max(nnz, 1), dtype=self.acc, device=dev)
        stream = native.stream_ptr(dev)
        if nnz:
            # (column, entry id) through the stable segmented radix sort: one segment, ceil(log2 D)
            # key bits; a column's entries stay in row order
            bits = max(1, int(self.D - 1).bit_length())
            keys = torch.empty(nnz, dtype=torch.int32, device=dev)
            ids = torch.empty(nnz, dtype=torch.int32, device=dev)
            erow = torch.empty(nnz, dtype=torch.int32, device=dev)
            native.call("fmlx_kmeans_csr_prepare", native.ptr(self.indptr), native.ptr(self.idx), self.n, self.D,
                        native.ptr(keys), native.ptr(ids), native.ptr(erow), native.ptr(self.err), stream)
            keys, ids = _glm.seg_sort(keys, ids, [0, nnz], [0], bits)
            native.call("fmlx_kmeans_csr_colptr", native.ptr(keys), nnz, self.D, native.ptr(self.colptr), stream)
            native.call("fmlx_kmeans_csr_gather", int(self.acc == torch.float64), native.ptr(ids), native.ptr(erow),
                        native.ptr(self.val), nnz, native.ptr(self.crow), native.ptr(self.cval), stream)
            del keys, ids, erow  # the sort scratch goes with them
        # columns longer than a segment: (column, first segment) and the per-segment table
        lens = self.colptr[1:] - self.colptr[:-1]
        long_col = torch.nonzero(lens > self.seg).reshape(-1)
        self.nlong = int(long_col.numel())
        nseg = (lens[long_col] + self.seg - 1) // self.seg
        self.long_seg0 = torch.zeros(self.nlong + 1, dtype=torch.int64, device=dev)
        self.long_seg0[1:] = torch.cumsum(nseg, 0)
        self.nsegs = int(self.long_seg0[-1].item())
        self.long_col = long_col.to(torch.int32)
        self.seg_col = torch.repeat_interleave(self.long_col, nseg, output_size=self.nsegs)
        self.seg_k = (torch.arange(self.nsegs, device=dev)
                      - torch.repeat_interleave(self.long_seg0[:-1], nseg, output_size=self.nsegs)).to(torch.int32)
