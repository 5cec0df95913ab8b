"""MinHash signatures (``csrc/minhash.hip``) with an exact int64 numpy path on CPU, and the search
over them (``csrc/lsh_join.hip``): the similarity join, pair distances and the neighbour filter.

``minhash(X, a, b)`` returns fp64 [n, K] with K = numHashTables * numHashFunctionsPerTable, the
reference ``MinHashLSHModelData.hashFunction`` values flattened table-major.

``similarity_join`` / ``pair_jaccard`` / ``nearest`` run the HIP kernels on device tensors and a
torch formulation (``*_torch``) on CPU tensors, with ``FMLX_LSH_NATIVE=0``, and for input whose
equality or membership the kernels do not decide: signatures holding NaN, ±inf or −0.0, and CSR
rows whose indices are not strictly increasing. Both give the same rows, order and distances.
"""
from __future__ import annotations

import os
from typing import Tuple

import numpy as np
import torch

from ..table import SparseColumn
from . import native
from . import sorting

HASH_PRIME = 2038074743


def to_csr_sets(X) -> SparseColumn:
    """Nonzero pattern of a dense tensor or SparseColumn (``Vector.toSparse().indices``)."""
    if isinstance(X, SparseColumn):
        nz = X.values != 0
        if bool(nz.all()):
            return X
        rows = torch.repeat_interleave(torch.arange(len(X), device=X.values.device),
                                       (X.indptr[1:] - X.indptr[:-1]).to(X.values.device))[nz]
        indptr = torch.zeros(len(X) + 1, dtype=torch.int64, device=X.values.device)
        indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=len(X)), 0)
        return SparseColumn(indptr, X.indices[nz], X.values[nz], X.size)
    nzr, nzc = torch.nonzero(X, as_tuple=True)
    indptr = torch.zeros(X.shape[0] + 1, dtype=torch.int64, device=X.device)
    indptr[1:] = torch.cumsum(torch.bincount(nzr, minlength=X.shape[0]), 0)
    return SparseColumn(indptr, nzc.to(torch.int32), X[nzr, nzc].to(torch.float64), X.shape[1])


def minhash(X, coef_a, coef_b) -> torch.Tensor:
    sets = to_csr_sets(X)
    n = len(sets)
    indptr = sets.indptr.to(torch.int64)
    if n and bool(((indptr[1:] - indptr[:-1]) == 0).any()):
        raise ValueError("Must have at least 1 non zero entry.")
    dev = sets.values.device
    K = len(coef_a)
    if dev.type == "cuda":
        a = torch.as_tensor(np.asarray(coef_a, dtype=np.int32), device=dev)
        b = torch.as_tensor(np.asarray(coef_b, dtype=np.int32), device=dev)
        ind = sets.indices.to(device=dev, dtype=torch.int32).contiguous()
        ip = indptr.to(dev).contiguous()
        out = torch.empty((n, K), dtype=torch.float64, device=dev)
        native.call("fmlx_minhash_csr", native.ptr(ip), native.ptr(ind) if ind.numel() else None, n, K,
                    native.ptr(a), native.ptr(b), native.ptr(out), native.stream_ptr(dev))
        return out
    ind = sets.indices.cpu().numpy().astype(np.int64)
    ip = indptr.cpu().numpy()
    a = np.asarray(coef_a, dtype=np.int64)
    b = np.asarray(coef_b, dtype=np.int64)
    if n == 0:
        return torch.zeros((0, K), dtype=torch.float64)
    h = ((1 + ind)[:, None] * a[None, :] + b[None, :]) % HASH_PRIME
    out = np.minimum.reduceat(h, ip[:-1], axis=0)
    return torch.from_numpy(out.astype(np.float64))


def jaccard_distance(x_idx: np.ndarray, y_idx: np.ndarray) -> float:
    """``MinHashLSHModelData.keyDistance``: 1 - |x ∩ y| / |x ∪ y| over nonzero index sets."""
    if len(x_idx) + len(y_idx) == 0:
        raise ValueError("The union of two input sets must have at least 1 elements")
    inter = len(np.intersect1d(x_idx, y_idx, assume_unique=True))
    return 1.0 - inter / (len(x_idx) + len(y_idx) - inter)


# ------------------------------------------------------------------ search: the torch formulation
EMPTY_UNION = "The union of two input sets must have at least 1 elements"


def _row_keys(sets: SparseColumn) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row id per nnz, sorted key row*d + col) for membership tests."""
    dev = sets.values.device
    rows = torch.repeat_interleave(torch.arange(len(sets), device=dev), (sets.indptr[1:] - sets.indptr[:-1]).to(dev))
    return rows, rows * sets.size + sets.indices.to(dev).long()


def pair_jaccard_torch(sa: SparseColumn, sb: SparseColumn, ia: torch.Tensor, ib: torch.Tensor) -> torch.Tensor:
    """Jaccard distance of set pairs (sa[ia[p]], sb[ib[p]]), vectorised over all nnz of the A side."""
    dev = ia.device
    if ia.numel() == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev)
    a_ptr, b_ptr = sa.indptr.to(dev), sb.indptr.to(dev)
    la = (a_ptr[ia + 1] - a_ptr[ia])
    lb = (b_ptr[ib + 1] - b_ptr[ib])
    # expand every pair by its A-side nnz, look the column up in B's row-keyed sorted index
    pid = torch.repeat_interleave(torch.arange(ia.numel(), device=dev), la)
    off = torch.arange(pid.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(la, 0) - la, la)
    cols = sa.indices.to(dev).long()[a_ptr[ia][pid] + off]
    d = max(sa.size, sb.size)
    _, bkeys = _row_keys(SparseColumn(sb.indptr, sb.indices, sb.values, d))
    bkeys_sorted, _ = torch.sort(bkeys)
    q = ib[pid] * d + cols
    pos = torch.clamp(torch.searchsorted(bkeys_sorted, q), max=max(bkeys_sorted.numel() - 1, 0))
    hit = (bkeys_sorted[pos] == q) if bkeys_sorted.numel() else torch.zeros_like(q, dtype=torch.bool)
    inter = torch.zeros(ia.numel(), dtype=torch.float64, device=dev).index_add_(0, pid, hit.to(torch.float64))
    union = (la + lb).to(torch.float64) - inter
    if bool((union <= 0).any()):
        raise ValueError(EMPTY_UNION)
    return 1.0 - inter / union


def similarity_join_torch(ha: torch.Tensor, hb: torch.Tensor, sa: SparseColumn, sb: SparseColumn,
                          threshold: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Join on (table, signature) via ``unique(dim=0)`` group ids, the candidate pairs of all tables
    deduplicated, Jaccard distance <= threshold; rows in ascending (ia, ib)."""
    dev = ha.device
    na, nb = ha.shape[0], hb.shape[0]
    pairs = []
    for tb in range(ha.shape[1]):
        allk = torch.cat([ha[:, tb], hb[:, tb]])
        _, g = torch.unique(allk, dim=0, return_inverse=True)
        ga, gb = g[:na], g[na:]
        ob = torch.argsort(gb, stable=True)
        gbs = gb[ob]
        lo = torch.searchsorted(gbs, ga)
        hi = torch.searchsorted(gbs, ga, right=True)
        cnt = hi - lo
        ia = torch.repeat_interleave(torch.arange(na, device=dev), cnt)
        off = torch.arange(ia.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        ib = ob[lo[ia] + off]
        pairs.append(ia * nb + ib)
    keys = torch.unique(torch.cat(pairs)) if pairs else torch.zeros(0, dtype=torch.int64, device=dev)
    ia, ib = torch.div(keys, nb, rounding_mode="floor"), keys % nb if nb else keys
    dist = pair_jaccard_torch(sa, sb, ia, ib)
    keep = dist <= threshold
    return ia[keep], ib[keep], dist[keep]


def nearest_torch(H: torch.Tensor, kh: torch.Tensor, sets: SparseColumn, kset: SparseColumn,
                  k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    cand = (H == kh[None]).all(dim=2).any(dim=1)
    idx = torch.nonzero(cand, as_tuple=True)[0]
    dist = pair_jaccard_torch(kset, sets, torch.zeros_like(idx), idx)
    order = torch.argsort(dist, stable=True)[:k]
    return idx[order], dist[order]


# ------------------------------------------------------------------ search: csrc/lsh_join.hip
# words of the kernels' int64 state block (lsh_join.hip ST_*)
_ST_BADVAL, _ST_OR, _ST_AND, _ST_ERROR, _ST_UNSORTED, _ST_TOTAL, _ST_WORDS = 0, 1, 2, 3, 4, 5, 8
_ERR_EMPTY_UNION, _ERR_ROW_RANGE = 1, 2
_MAX_ROWS = (1 << 31) - 1


def _native(*xs) -> bool:
    """The kernels take this call: every tensor on a GPU and FMLX_LSH_NATIVE not 0."""
    if os.environ.get("FMLX_LSH_NATIVE", "1") == "0":
        return False
    for x in xs:
        ts = (x.indptr, x.indices, x.values) if isinstance(x, SparseColumn) else (x,)
        if any(t.device.type != "cuda" for t in ts):
            return False
    return True


def _signatures_ok(*hs) -> bool:
    return all(h.dim() == 3 and h.dtype == torch.float64 for h in hs)


def _new_state(dev) -> torch.Tensor:
    st = [0] * _ST_WORDS
    st[_ST_AND] = -1
    return torch.tensor(st, dtype=torch.int64, device=dev)


def _csr(sets: SparseColumn, st: torch.Tensor):
    """(indptr int64, indices int32) of the sets, and their sortedness check launched into ``st``."""
    ptr = sets.indptr.to(torch.int64).contiguous()
    ind = sets.indices.to(torch.int32).contiguous()
    native.call("fmlx_lsh_sorted_check", native.ptr(ptr), native.ptr(ind), len(sets), ind.numel(), native.ptr(st),
                native.stream_ptr(st.device))
    return ptr, ind


def _scan(cnt: torch.Tensor, st: torch.Tensor) -> torch.Tensor:
    """int64 [n + 1] exclusive offsets of int32 counts; the total also lands in ``st[_ST_TOTAL]``."""
    n = cnt.numel()
    off = torch.empty(n + 1, dtype=torch.int64, device=cnt.device)
    scratch = torch.empty(int(native.kernels().fmlx_lsh_scan_scratch(n)), dtype=torch.int64, device=cnt.device)
    native.call("fmlx_lsh_scan", native.ptr(cnt), n, native.ptr(off), native.ptr(scratch),
                st.data_ptr() + 8 * _ST_TOTAL, native.stream_ptr(cnt.device))
    return off


def _raise_for(err: int) -> None:
    if err & _ERR_ROW_RANGE:
        raise IndexError("pair_jaccard: a pair names a row outside its set column")
    if err & _ERR_EMPTY_UNION:
        raise ValueError(EMPTY_UNION)


def _empty_join(dev):
    z = torch.zeros(0, dtype=torch.int64, device=dev)
    return z, z.clone(), torch.zeros(0, dtype=torch.float64, device=dev)


def similarity_join(ha: torch.Tensor, hb: torch.Tensor, sa: SparseColumn, sb: SparseColumn, threshold: float, *,
                    chunk: int = 1 << 22, key_bits: int = 63) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pairs (ia, ib, dist) of rows of A and B that share a signature in some table and whose sets'
    Jaccard distance is <= threshold, in ascending (ia, ib): int64, int64, fp64 on the inputs' device.

    ``ha`` / ``hb``: fp64 [n, tables, funcs]; ``sa`` / ``sb``: the rows' sets (CSR). At most ``chunk``
    candidate pairs are in flight at a time; ``key_bits`` (1..63) narrows the bucket keys (tests force
    key collisions with it: the result does not depend on it)."""
    if not (_native(ha, hb, sa, sb) and _signatures_ok(ha, hb) and ha.shape[1:] == hb.shape[1:]
            and ha.shape[0] == len(sa) and hb.shape[0] == len(sb)):
        return similarity_join_torch(ha, hb, sa, sb, threshold)
    dev = ha.device
    na, nb, T, F = ha.shape[0], hb.shape[0], ha.shape[1], ha.shape[2]
    if na > _MAX_ROWS or nb > _MAX_ROWS:
        raise ValueError("similarity_join: at most 2^31 - 1 rows per side (%d, %d)" % (na, nb))
    L = na + nb
    if L > _MAX_ROWS:
        raise ValueError("similarity_join: at most 2^31 - 1 entries per table segment (%d)" % L)
    if not 1 <= key_bits <= 63 or chunk < 1:
        raise ValueError("similarity_join: key_bits in 1..63 and chunk >= 1")
    if na == 0 or nb == 0 or T == 0 or F == 0:
        return _empty_join(dev)
    ha, hb = ha.contiguous(), hb.contiguous()
    stream = native.stream_ptr(dev)
    st = _new_state(dev)
    a_ptr, a_idx = _csr(sa, st)
    b_ptr, b_idx = _csr(sb, st)
    # (a) bucket keys, table-major: table t is entries [t·L, (t + 1)·L), A's rows then B's
    N = T * L
    keys = torch.empty(N, dtype=sorting.U64, device=dev)
    rows = torch.empty(N, dtype=torch.int32, device=dev)
    for h, n, side, base in ((ha, na, 0, 0), (hb, nb, 1, na)):
        native.call("fmlx_lsh_keys", native.ptr(h), n, T, F, side, key_bits, L, base, native.ptr(keys),
                    native.ptr(rows), native.ptr(st), stream)
    host = st.cpu().tolist()
    if host[_ST_BADVAL] or host[_ST_UNSORTED]:
        return similarity_join_torch(ha, hb, sa, sb, threshold)
    # (b) one sort per run of tables (32 segments and 2^31 - 1 entries per sort)
    bit_lo, bit_hi = sorting.bit_range(torch.tensor(host[_ST_OR:_ST_AND + 1], dtype=torch.int64))
    per_run = max(1, min(32, _MAX_ROWS // L))
    sk, sr = [], []
    for t0 in range(0, T, per_run):
        t1 = min(T, t0 + per_run)
        k, r = sorting.sort_u64(keys[t0 * L:t1 * L], rows[t0 * L:t1 * L], [i * L for i in range(t1 - t0 + 1)],
                                bit_lo, bit_hi)
        sk.append(k)
        sr.append(r)
    skeys = sk[0] if len(sk) == 1 else torch.cat(sk)
    srows = sr[0] if len(sr) == 1 else torch.cat(sr)
    del keys, rows, sk, sr
    # (c) candidates per A entry, their offsets, the total
    cnt = torch.empty(N, dtype=torch.int32, device=dev)
    lo = torch.empty(N, dtype=torch.int32, device=dev)
    native.call("fmlx_lsh_count", native.ptr(skeys), N, L, native.ptr(cnt), native.ptr(lo), stream)
    off = _scan(cnt, st)
    del cnt, skeys
    C = int(st[_ST_TOTAL].item())
    if C == 0:
        return _empty_join(dev)
    # (d) the candidates chunk by chunk: survivors appended behind the chunk's cursor
    nchunk = -(-C // chunk)
    cur = torch.zeros(_ST_WORDS + nchunk, dtype=torch.int64, device=dev)  # state words, then one cursor per chunk
    cap = min(chunk, C)
    out_key = torch.empty(cap, dtype=sorting.U64, device=dev)
    out_dist = torch.empty(cap, dtype=torch.float64, device=dev)
    part_k, part_d = [], []
    for i in range(nchunk):
        c0, c1 = i * chunk, min(C, (i + 1) * chunk)
        native.call("fmlx_lsh_emit", native.ptr(srows), native.ptr(off), native.ptr(lo), N, L, c0, c1, native.ptr(ha),
                    native.ptr(hb), na, nb, T, F, native.ptr(a_ptr), native.ptr(a_idx), native.ptr(b_ptr),
                    native.ptr(b_idx), float(threshold), cur.data_ptr() + 8 * (_ST_WORDS + i), native.ptr(out_key),
                    native.ptr(out_dist), native.ptr(cur), stream)
        got = cur.cpu().tolist()  # (the chunk's survivor count: the buffer is reused by the next chunk)
        _raise_for(got[_ST_ERROR])
        kept = got[_ST_WORDS + i]
        if kept:
            part_k.append(out_key[:kept].clone())
            part_d.append(out_dist[:kept].clone())
    del out_key, out_dist, off, lo, srows
    if not part_k:
        return _empty_join(dev)
    # (e) every pair is there once: a sort by (a, b) fixes the order whatever the append order was
    pk = part_k[0] if len(part_k) == 1 else torch.cat(part_k)
    pd = part_d[0] if len(part_d) == 1 else torch.cat(part_d)
    S = pk.numel()
    if S > _MAX_ROWS:
        raise ValueError("similarity_join: at most 2^31 - 1 result pairs (%d)" % S)
    pos = torch.arange(S, dtype=torch.int32, device=dev)
    pk, pos = sorting.sort_u64(pk, pos, [0, S], 0, (nb - 1).bit_length())
    pk, pos = sorting.sort_u64(pk, pos, [0, S], 32, 32 + (na - 1).bit_length())
    ia = torch.empty(S, dtype=torch.int64, device=dev)
    ib = torch.empty(S, dtype=torch.int64, device=dev)
    dist = torch.empty(S, dtype=torch.float64, device=dev)
    native.call("fmlx_lsh_gather", native.ptr(pk), native.ptr(pos), native.ptr(pd), S, native.ptr(ia), native.ptr(ib),
                native.ptr(dist), stream)
    return ia, ib, dist


def pair_jaccard(sa: SparseColumn, sb: SparseColumn, ia: torch.Tensor, ib: torch.Tensor) -> torch.Tensor:
    """fp64 Jaccard distances of the set pairs (sa[ia[p]], sb[ib[p]])."""
    if not _native(sa, sb, ia, ib):
        return pair_jaccard_torch(sa, sb, ia, ib)
    dev = ia.device
    P = ia.numel()
    if P == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev)
    st = _new_state(dev)
    a_ptr, a_idx = _csr(sa, st)
    b_ptr, b_idx = _csr(sb, st)
    ia64, ib64 = ia.to(torch.int64).contiguous(), ib.to(torch.int64).contiguous()
    dist = torch.empty(P, dtype=torch.float64, device=dev)
    native.call("fmlx_lsh_pair_jaccard", native.ptr(a_ptr), native.ptr(a_idx), len(sa), native.ptr(b_ptr),
                native.ptr(b_idx), len(sb), native.ptr(ia64), native.ptr(ib64), P, native.ptr(dist), native.ptr(st), 0,
                native.stream_ptr(dev))
    host = st.cpu().tolist()
    if host[_ST_UNSORTED]:
        return pair_jaccard_torch(sa, sb, ia, ib)
    _raise_for(host[_ST_ERROR])
    return dist


def nearest(H: torch.Tensor, kh: torch.Tensor, sets: SparseColumn, kset: SparseColumn,
            k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` rows nearest to the key among those sharing a signature with it in some table:
    (row ids int64, distances fp64), ordered by (distance, row). ``H``: fp64 [n, tables, funcs] of
    the rows, ``kh``: [tables, funcs] of the key, ``sets`` / ``kset``: their sets (``kset``: one row)."""
    if not (_native(H, kh, sets, kset) and _signatures_ok(H) and kh.dtype == torch.float64
            and kh.shape == H.shape[1:] and H.shape[0] == len(sets) and len(kset) == 1 and H.shape[1] * H.shape[2] > 0):
        return nearest_torch(H, kh, sets, kset, k)
    dev = H.device
    n, T, F = H.shape
    if n > _MAX_ROWS:
        raise ValueError("nearest: at most 2^31 - 1 rows (%d)" % n)
    H, kh = H.contiguous(), kh.contiguous()
    stream = native.stream_ptr(dev)
    st = _new_state(dev)
    s_ptr, s_idx = _csr(sets, st)
    k_ptr, k_idx = _csr(kset, st)
    flag = torch.empty(n, dtype=torch.int32, device=dev)
    native.call("fmlx_lsh_match", native.ptr(H), n, T, F, native.ptr(kh), native.ptr(flag), native.ptr(st), stream)
    off = _scan(flag, st)
    host = st.cpu().tolist()
    if host[_ST_BADVAL] or host[_ST_UNSORTED]:
        return nearest_torch(H, kh, sets, kset, k)
    M = host[_ST_TOTAL]
    if M == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    idx = torch.empty(M, dtype=torch.int64, device=dev)
    native.call("fmlx_lsh_compact", native.ptr(flag), native.ptr(off), n, M, native.ptr(idx), stream)
    dist = torch.empty(M, dtype=torch.float64, device=dev)
    native.call("fmlx_lsh_pair_jaccard", native.ptr(k_ptr), native.ptr(k_idx), 1, native.ptr(s_ptr), native.ptr(s_idx),
                n, None, native.ptr(idx), M, native.ptr(dist), native.ptr(st), 1, stream)
    _raise_for(int(st[_ST_ERROR].item()))
    # distances in [0, 1] order like their bit patterns (bits 0..61); the sort is stable and the
    # compacted rows ascend, so ties stay in row order
    sk, sv = sorting.sort_u64(dist.view(sorting.U64), torch.arange(M, dtype=torch.int32, device=dev), [0, M], 0, 62)
    return idx[sv[:k].long()], sk[:k].view(torch.float64)
