"""Knn on CSR feature columns on the GPU (ops/csrc/knn_csr.hip): the product block of two CSR
operands, the row norms, and the stage on them.

Shape (per value dtype, from ``ops.knn.CSR_TILE_ROWS``): n = TILE + TILE // 4 + 3 training rows (a
second, ragged tile whose second wave quarter is ragged), D = 300, 70 queries. ``train_column`` /
``query_column``: column 0 is stored in every training row but the empty one (row 5), so it crosses
every quarter and tile; columns 290 … 299 are stored by no training row; query row 3 is empty, query
row 0 has 130 entries (three broadcast batches) and stores the unused column 295; indices are
unique and unsorted inside a row. ``kind="int"``: integer values in [-4, 4] without 0, so that every
product, norm and squared distance is an integer below 2^24 (exact in fp32 and fp64, many equal
distances); ``kind="normal"``: N(0, 1) values rounded to fp32."""
import functools
import gc

import numpy as np
import pytest
import torch

from flink_ml_amd.ops import knn as knn_ops
from flink_ml_amd.table import SparseColumn

pytestmark = pytest.mark.gpu

D, NQ, USED = 300, 70, 290
DTYPES = [torch.float32, torch.float64]
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def n_train(dtype) -> int:
    tile = knn_ops.CSR_TILE_ROWS[dtype]
    return tile + tile // 4 + 3


def _values(rs, m, kind):
    if kind == "int":
        return (rs.randint(1, 5, m) * rs.choice([-1, 1], m)).astype(np.float64)
    return rs.normal(0.0, 1.0, m).astype(np.float32).astype(np.float64)


def _column(rows, kind, seed) -> SparseColumn:
    rs = np.random.RandomState(seed)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    return SparseColumn(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(_values(rs, idx.shape[0], kind)), D)


@functools.lru_cache(maxsize=None)
def train_column(n, kind) -> SparseColumn:
    rs = np.random.RandomState(21)
    order = np.argsort(rs.rand(n, USED - 1), axis=1)[:, :32] + 1  # distinct columns 1 … 289, unsorted
    lens = rs.randint(1, 33, n)
    rows = []
    for i in range(n):
        r = order[i, :lens[i]]
        rows.append(np.zeros(0, np.int64) if i == 5 else (np.append(r, 0) if i % 2 else np.insert(r, 0, 0)))
    return _column(rows, kind, 22)


@functools.lru_cache(maxsize=None)
def query_column(kind) -> SparseColumn:
    rs = np.random.RandomState(31)
    rows = []
    for i in range(NQ):
        L = 130 if i == 0 else (0 if i == 3 else int(rs.randint(1, 65)))
        r = rs.permutation(USED)[:L]
        if i == 0:
            r[17] = 295  # a column no training row stores
        rows.append(r)
    return _column(rows, kind, 32)


def labels_of(n):
    return torch.from_numpy(np.random.RandomState(4).randint(0, 4, n).astype(np.float64))


def absolute(X: SparseColumn) -> SparseColumn:
    return SparseColumn(X.indptr, X.indices, X.values.abs(), X.size)


@functools.lru_cache(maxsize=None)
def host_products(n, kind, magnitudes=False) -> torch.Tensor:
    """fp64 on the host (the index-add formulation); ``magnitudes``: Σ|v·w| instead."""
    Q, T = query_column(kind), train_column(n, kind)
    return knn_ops.torch_products_csr(absolute(Q), absolute(T)) if magnitudes else knn_ops.torch_products_csr(Q, T)


def device_column(X: SparseColumn, dtype) -> SparseColumn:
    from flink_ml_amd.ops.csr import csr_arrays

    return SparseColumn(*csr_arrays(X.to(device="cuda"), dtype), X.size)


@functools.lru_cache(maxsize=None)
def device_operands(dtype, kind):
    from flink_ml_amd.ops.csr import ColumnMajor

    cm = ColumnMajor(device_column(train_column(n_train(dtype), kind), dtype))
    assert int(cm.err.item()) == 0 and not knn_ops.has_duplicate_index(cm)
    return device_column(query_column(kind), dtype), cm


def test_shape_has_the_cases():
    for dtype in DTYPES:
        n, tile = n_train(dtype), knn_ops.CSR_TILE_ROWS[dtype]
        assert tile < n < 2 * tile and (n - tile) % (tile // 4) == 3 and (n - tile) // (tile // 4) == 1
        T = train_column(n, "int")
        lens = T.indptr[1:] - T.indptr[:-1]
        assert int(lens[5]) == 0 and int((lens == 0).sum()) == 1
        assert int((T.indices == 0).sum()) == n - 1 and int(T.indices.max()) < USED
    Q = query_column("int")
    ql = Q.indptr[1:] - Q.indptr[:-1]
    assert int(ql[0]) == 130 and int(ql[3]) == 0 and int((Q.indices == 295).sum()) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_products_integer_data_bitwise(dtype):
    _need_gpu()
    Q, cm = device_operands(dtype, "int")
    G = knn_ops.csr_products(Q, cm, 0, NQ)
    want = host_products(n_train(dtype), "int")
    assert float(want.abs().max()) < 2 ** 24 and float(want.abs().max()) > 16
    assert G.dtype == dtype and torch.equal(G.cpu().double(), want)
    assert int(cm.err.item()) == 0
    assert not G[3].any() and not G[:, 5].any()  # the empty query row, the empty training row


@pytest.mark.parametrize("dtype", DTYPES)
def test_products_normal_data_within_the_rounding_bound(dtype):
    """|G − G64| ≤ (m + 2)·u·Σ|v·w| per element, m the query row's entry count, u the unit roundoff of
    the value dtype: the rounding bound of m products and m adds (a fused multiply-add rounds once where
    they round twice). G64 is the host's fp64 index-add over the same pairs in the same order; for fp32
    its own error (m·2^-53·Σ|v·w|) is far inside the two spare units. Every element is checked."""
    _need_gpu()
    n = n_train(dtype)
    Q, cm = device_operands(dtype, "normal")
    G = knn_ops.csr_products(Q, cm, 0, NQ).cpu().double()
    G64, S = host_products(n, "normal"), host_products(n, "normal", True)
    Qh = query_column("normal")
    m = (Qh.indptr[1:] - Qh.indptr[:-1]).double()[:, None]
    excess = (G - G64).abs() - (m + 2) * U[dtype] * S
    print("largest |G - G64| / ((m + 2) u S): %.3g" % float(((G - G64).abs() / ((m + 2) * U[dtype] * S).clamp_min(1e-300)).max()))
    assert bool((excess <= 0).all())
    assert float(S.max()) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_products_bitwise_reproducible(dtype):
    """Run to run, across query blocks and across every tile the library is built with."""
    _need_gpu()
    Q, cm = device_operands(dtype, "normal")
    n = n_train(dtype)
    G = knn_ops.csr_products(Q, cm, 0, NQ).clone()
    assert torch.equal(knn_ops.csr_products(Q, cm, 0, NQ), G)
    for block in (1, 7, 64):
        out = torch.full((NQ, n), float("nan"), dtype=dtype, device="cuda")
        for s in range(0, NQ, block):
            e = min(NQ, s + block)
            knn_ops.csr_products(Q, cm, s, e, out=out[s:e])
        assert torch.equal(out, G), block
    tiles = knn_ops.CSR_TILE_ROWS_BUILT[dtype]
    assert knn_ops.CSR_TILE_ROWS[dtype] in tiles and len(tiles) > 1
    for tile in tiles:
        assert torch.equal(knn_ops.csr_products(Q, cm, 0, NQ, tile=tile), G), tile
    # a padded output block (row stride > n) is written in place
    wide = torch.zeros((NQ, n + 5), dtype=dtype, device="cuda")
    knn_ops.csr_products(Q, cm, 0, NQ, out=wide[:, :n])
    assert torch.equal(wide[:, :n], G) and not wide[:, n:].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sqnorm(dtype):
    """fp64 accumulation in stored-entry order. Integer data: bitwise the fp64 sum. Normal data: the
    values are fp32 numbers, so their squares are exact in fp64, and the kernel's sum and the
    reference's are both m-term fp64 sums of them: |s − s_ref| ≤ 2·(m + 2)·2^-53·Σv², plus one rounding
    of the result, 2^-24·Σv², for an fp32 output."""
    _need_gpu()
    n = n_train(dtype)
    for kind in ("int", "normal"):
        Th = train_column(n, kind)
        T = device_column(Th, dtype)
        want = knn_ops.csr_sqnorm(Th, torch.float64)
        rows = torch.repeat_interleave(torch.arange(n), Th.indptr[1:] - Th.indptr[:-1])
        assert torch.equal(want, torch.zeros(n, dtype=torch.float64).index_add_(0, rows, Th.values ** 2))
        m = (Th.indptr[1:] - Th.indptr[:-1]).double()
        for out in DTYPES:
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = knn_ops.csr_sqnorm(T, out, err=err)
            assert got.dtype == out and int(err.item()) == 0
            if kind == "int":
                assert torch.equal(got.cpu().double(), want)
            else:
                bound = 2 * (m + 2) * 2.0 ** -53 * want + (2.0 ** -24 * want if out == torch.float32 else 0.0)
                assert bool(((got.cpu().double() - want).abs() <= bound).all())


@functools.lru_cache(maxsize=None)
def host_neighbours(n):
    """fp64 on the host, from the dense matrices: the training points in (distance, index) order."""
    T, Q = train_column(n, "int"), query_column("int")
    Td, Qd = T.to_dense(torch.float64), Q.to_dense(torch.float64)
    d2 = (Qd * Qd).sum(1)[:, None] + (Td * Td).sum(1)[None, :] - 2.0 * Qd @ Td.t()
    assert float(d2.max()) < 2 ** 24 and bool((d2 == d2.round()).all())
    return torch.sort(torch.sqrt(d2.abs()), dim=1, stable=True).indices


@pytest.mark.parametrize("policy", ["fp32", "fp64"])
def test_stage_end_to_end_equals_host_and_dense_route(policy, monkeypatch):
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import knn as mknn
    from flink_ml_amd.models.knn import Knn

    dtype = torch.float32 if policy == "fp32" else torch.float64
    n = n_train(dtype)
    T, Q, y = train_column(n, "int"), query_column("int"), labels_of(n)
    order = host_neighbours(n)
    classes = torch.unique(y)
    ks = [1, 5, 100, n]
    assert ks[1] <= knn_ops.ROUTE_MAX_K < ks[2] <= knn_ops.SELECT_MAX_K
    with dtype_policy(policy):
        monkeypatch.setattr(knn_ops, "CSR_ROUTE", "1")
        model = Knn().fit(Table({"features": T, "label": y}))
        st = model._model_state()
        assert isinstance(st, mknn._CsrState) and st.cm.acc == dtype and st.tnorm.dtype == dtype
        monkeypatch.setattr(knn_ops, "CSR_ROUTE", "0")
        dense = Knn().fit(Table({"features": T, "label": y}))
        assert not isinstance(dense._model_state(), mknn._CsrState)
        for k in ks:
            want_idx = order[:, :k]
            want = np.asarray(mknn.knn_vote(y[want_idx], classes))
            monkeypatch.setattr(knn_ops, "CSR_ROUTE", "1")
            idx = torch.cat(list(mknn.knn_topk_csr(Q.to(device="cuda"), st, k)))
            assert torch.equal(idx.cpu(), want_idx), k
            got = np.asarray(model.set_k(k).transform(Table({"features": Q}))[0].column("prediction").cpu())
            assert np.array_equal(got, want), k
            monkeypatch.setattr(knn_ops, "CSR_ROUTE", "0")
            old = np.asarray(dense.set_k(k).transform(Table({"features": Q}))[0].column("prediction").cpu())
            assert np.array_equal(old, want), k
    assert bool((order[:, 0] != order[0, 0]).any())


def test_bounded_memory_at_hashingtf_width(monkeypatch):
    """2,000 x 262,144 in fp32 is 2.1 GB densified; fit and transform stay under a tenth of it (the
    peak above what earlier tests of the process still hold, such as the GEMM library's workspace)."""
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.models import knn as mknn
    from flink_ml_amd.models.knn import Knn
    from flink_ml_amd.ops import native

    n, nq, wide, L, k = 2000, 500, 1 << 18, 30, 5
    native.kernels()
    rs = np.random.RandomState(8)

    def column(rows, seed):
        r = np.random.RandomState(seed)
        # half of a row's columns among the first 256 (rows share columns), distinct inside a row
        lo = np.argsort(r.rand(rows, 256), axis=1)[:, :L // 2]
        hi = 256 + (r.randint(0, (wide - 256) // L, (rows, L - L // 2)) * L + np.arange(L - L // 2)[None, :])
        idx = np.concatenate([lo, hi], axis=1)
        idx = np.take_along_axis(idx, np.argsort(r.rand(rows, L), axis=1), axis=1).astype(np.int32).reshape(-1)
        val = (r.randint(1, 5, rows * L) * r.choice([-1, 1], rows * L)).astype(np.float64)
        return SparseColumn(torch.arange(0, rows * L + 1, L, dtype=torch.int64), torch.from_numpy(idx),
                            torch.from_numpy(val), wide)

    T, Q = column(n, 9), column(nq, 10)
    assert int(T.indices.max()) > wide // 2
    y = torch.from_numpy(rs.randint(0, 3, n).astype(np.float64))
    G = knn_ops.torch_products_csr(Q, T)
    d2 = knn_ops.csr_sqnorm(Q)[:, None] + knn_ops.csr_sqnorm(T)[None, :] - 2.0 * G
    idx = torch.sort(torch.sqrt(d2.abs()), dim=1, stable=True).indices[:, :k]
    want = np.asarray(mknn.knn_vote(y[idx], torch.unique(y)))
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "auto")
    monkeypatch.setenv("FMLX_HBM_BUDGET", "1G")  # the dense training matrix does not fit: the memory criterion
    dev = torch.device("cuda")
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)  # what earlier tests of the process still hold (their cached operands)
    model = Knn().set_k(k).fit(Table({"features": T, "label": y}))
    got = np.asarray(model.transform(Table({"features": Q}))[0].column("prediction").cpu())
    peak = torch.cuda.max_memory_allocated(dev) - base
    print("peak: %.1f MiB above %.1f MiB held before, of %.1f MiB dense" % (peak / 2 ** 20, base / 2 ** 20,
                                                                        n * wide * 4 / 2 ** 20))
    assert isinstance(model._model_state(), mknn._CsrState)
    assert peak < n * wide * 4 // 10
    assert np.array_equal(got, want) and len(set(want.tolist())) > 1


def with_entry(X, row, index, value=1.0):
    at = int(X.indptr[row + 1])
    ptr = X.indptr.clone()
    ptr[row + 1:] += 1
    idx = torch.cat([X.indices[:at], torch.tensor([index], dtype=X.indices.dtype), X.indices[at:]])
    val = torch.cat([X.values[:at], torch.tensor([value], dtype=X.values.dtype), X.values[at:]])
    return SparseColumn(ptr, idx, val, X.size)


def test_bad_index_sets_the_error_word_and_is_skipped(monkeypatch):
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.models.knn import Knn
    from flink_ml_amd.ops.csr import ColumnMajor
    from flink_ml_amd.ops.kmeans import check_csr_error

    dtype = torch.float32
    n = n_train(dtype)
    Q, cm0 = device_operands(dtype, "int")
    G = knn_ops.csr_products(Q, cm0, 0, NQ).clone()
    cm = ColumnMajor(device_column(train_column(n, "int"), dtype))  # (an error word of its own)
    for bad in (D, -1, 2 ** 31 - 1):
        cm.err.zero_()
        Qbad = device_column(with_entry(with_entry(query_column("int"), 0, bad), 40, bad), dtype)
        got = knn_ops.csr_products(Qbad, cm, 0, NQ)
        torch.cuda.synchronize()
        assert int(cm.err.item()) == 1
        assert torch.equal(got, G)  # the entry was skipped
        with pytest.raises(ValueError, match="out of range"):
            check_csr_error(cm)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert torch.equal(knn_ops.csr_sqnorm(Qbad, torch.float64, err=err), knn_ops.csr_sqnorm(Q, torch.float64))
        assert int(err.item()) == 1
    # the stage: a bad training index at fit, a bad query index and a wrong size at transform
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "1")
    T, y = train_column(n, "int"), labels_of(n)
    with pytest.raises(ValueError, match="out of range"):
        Knn().fit(Table({"features": with_entry(T, 9, D), "label": y}))
    model = Knn().fit(Table({"features": T, "label": y}))
    with pytest.raises(ValueError, match="out of range"):
        model.transform(Table({"features": with_entry(query_column("int"), 2, D + 3)}))
    Qh = query_column("int")
    with pytest.raises(ValueError, match="Vector size mismatched."):
        model.transform(Table({"features": SparseColumn(Qh.indptr, Qh.indices, Qh.values, D + 1)}))
    torch.cuda.synchronize()
    want = model.transform(Table({"features": Qh}))[0].column("prediction")
    assert want.shape[0] == NQ
