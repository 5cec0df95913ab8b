"""Knn on CSR feature columns without densifying, on the host (gloo for two ranks): the model that
holds the CSR training set (``models.knn.CsrPackedFeatures``), the torch formulation of the product
block (``ops.knn.torch_products_csr``) and the routing knob ``FMLX_KNN_CSR`` (``ops.knn.CSR_ROUTE``).

Data (``int_column``): unique, unsorted indices per row, at most 64 of them, integer values in
[-4, 4] without 0; every 13th row empty. Every product, norm and squared distance is then an integer
below 2^24: the routes must agree exactly, and equal distances are common, so the tie rule (the
earlier training point wins) is exercised."""
import functools
import os

import numpy as np
import pytest
import torch

from flink_ml_amd import Table
from flink_ml_amd.linalg.vectors import DenseMatrix
from flink_ml_amd.models import knn as mknn
from flink_ml_amd.models.knn import Knn, KnnModel
from flink_ml_amd.ops import knn as knn_ops
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd
from tests.test_colstats_csr import on_cpu

N, NQ, D = 60, 20, 300


def int_column(n, D, seed, max_len=64, empty_every=13) -> SparseColumn:
    rs = np.random.RandomState(seed)
    ptr, cols, vals = [0], [], []
    for i in range(n):
        L = 0 if empty_every and i % empty_every == empty_every - 1 else int(rs.randint(1, max_len + 1))
        # half of the draws from the first 200 columns (rows then share columns at any width)
        c = rs.permutation(np.unique(np.concatenate([rs.randint(0, min(D, 200), L // 2), rs.randint(0, D, L - L // 2)])))
        v = rs.randint(1, 5, c.shape[0]) * rs.choice([-1, 1], c.shape[0])
        cols.append(np.asarray(c, np.int32))
        vals.append(v.astype(np.float64))
        ptr.append(ptr[-1] + c.shape[0])
    return SparseColumn(torch.tensor(ptr, dtype=torch.int64), torch.from_numpy(np.concatenate(cols).astype(np.int32)),
                        torch.from_numpy(np.concatenate(vals)), D)


def labels_of(n, seed=4):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 3, n).astype(np.float64))


@functools.lru_cache(maxsize=None)
def data(D=D):
    """(training column, labels, query column); the narrow queries share columns with the training
    rows (low-numbered columns are drawn more often through the second call's range)."""
    return int_column(N, D, 1), labels_of(N), int_column(NQ, D, 2)


def no_dense(self, *a, **k):
    raise AssertionError("SparseColumn.to_dense called")


def fit(X, y, route, monkeypatch, k=5):
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", route)
    return Knn().set_k(k).fit(Table({"features": X, "label": y}))


def predict(model, Q, k=None):
    if k is not None:
        model.set_k(k)
    return np.asarray(model.transform(Table({"features": Q}))[0].column("prediction").cpu())


def host_reference(X, y, Q, k):
    """fp64 on the host from the dense matrices: squared distances, a stable sort, the vote."""
    Xd, Qd = X.to_dense(torch.float64), Q.to_dense(torch.float64)
    d2 = (Qd * Qd).sum(1)[:, None] + (Xd * Xd).sum(1)[None, :] - 2.0 * Qd @ Xd.t()
    idx = torch.sort(torch.sqrt(d2.abs()), dim=1, stable=True).indices[:, :min(k, len(X))]
    return idx, np.asarray(mknn.knn_vote(y[idx], torch.unique(y)))


def test_torch_products_csr_is_the_dense_product():
    X, _, Q = data()
    G = knn_ops.torch_products_csr(Q, X)
    assert G.dtype == torch.float64 and G.shape == (NQ, N)
    assert torch.equal(G, Q.to_dense(torch.float64) @ X.to_dense(torch.float64).t())
    assert torch.equal(knn_ops.csr_sqnorm(X, torch.float64), (X.to_dense() ** 2).sum(1))
    assert G.abs().max() > 0 and int((X.indptr[1:] == X.indptr[:-1]).sum()) == N // 13


def test_no_dense_matrix_is_ever_made(monkeypatch):
    """At HashingTF's default width neither fit nor transform may form an n x D matrix."""
    wide = 1 << 18
    X, y, Q = data(wide)
    with on_cpu():
        monkeypatch.setattr(SparseColumn, "to_dense", no_dense)
        model = fit(X, y, "1", monkeypatch)
        packed = model.get_model_data()[0].column("packedFeatures")[0]
        assert isinstance(packed, mknn.CsrPackedFeatures) and isinstance(packed, DenseMatrix)
        assert (packed.num_rows, packed.num_cols) == (wide, N)
        pred = predict(model, Q)
        assert isinstance(model._model_state(), mknn._CsrState)
    assert int(X.indices.max()) > 1 << 17 and pred.shape == (NQ,) and set(pred.tolist()) <= {0.0, 1.0, 2.0}
    # the same neighbours from the CSR arrays alone: products through a dict per training row
    rows = [dict(zip(X.indices[int(X.indptr[i]):int(X.indptr[i + 1])].tolist(),
                     X.values[int(X.indptr[i]):int(X.indptr[i + 1])].tolist())) for i in range(N)]
    tn = np.array([sum(v * v for v in r.values()) for r in rows])
    want = []
    for q in range(NQ):
        s, e = int(Q.indptr[q]), int(Q.indptr[q + 1])
        qi, qv = Q.indices[s:e].tolist(), Q.values[s:e].tolist()
        g = np.array([sum(v * r.get(c, 0.0) for c, v in zip(qi, qv)) for r in rows])
        d = np.sqrt(np.abs(sum(v * v for v in qv) + tn - 2.0 * g))
        idx = torch.from_numpy(np.argsort(d, kind="stable")[:5])
        want.append(float(mknn.knn_vote(y[idx][None, :], torch.unique(y))[0]))
    assert pred.tolist() == want


@pytest.mark.parametrize("k", [1, 5, N])
def test_csr_route_equals_dense_route(k, monkeypatch):
    X, y, Q = data()
    with on_cpu():
        dense = fit(X, y, "0", monkeypatch, k)
        assert type(dense.get_model_data()[0].column("packedFeatures")[0]) is DenseMatrix
        want = predict(dense, Q)
        csr = fit(X, y, "1", monkeypatch, k)
        got = predict(csr, Q)
        assert isinstance(csr._model_state(), mknn._CsrState)
        idx = torch.cat(list(mknn.knn_topk_csr(Q, csr._model_state(), k)))
    ref_idx, ref_pred = host_reference(X, y, Q, k)
    assert np.array_equal(got, want) and np.array_equal(got, ref_pred)
    assert torch.equal(idx, ref_idx)
    if k == 5:  # the data does tie: some query has two training points at one distance among its first k + 1
        Xd, Qd = X.to_dense(), Q.to_dense()
        d2 = torch.cdist(Qd, Xd).pow(2).round()
        top = torch.sort(d2, dim=1).values[:, :k + 1]
        assert bool((top[:, 1:] == top[:, :-1]).any())
        assert len(set(want.tolist())) > 1


def data_bytes(path):
    out = {}
    for root, _, names in os.walk(os.path.join(path, "data")):
        for nm in sorted(names):
            with open(os.path.join(root, nm), "rb") as f:
                out[nm] = f.read()
    return out


def test_save_writes_the_dense_bytes_and_load_predicts_the_same(monkeypatch, tmp_path):
    X, y, Q = data()
    with on_cpu():
        dense = fit(X, y, "0", monkeypatch)
        csr = fit(X, y, "1", monkeypatch)
        assert isinstance(csr.get_model_data()[0].column("packedFeatures")[0], mknn.CsrPackedFeatures)
        want = predict(csr, Q)
        dense.save(str(tmp_path / "dense"))
        csr.save(str(tmp_path / "csr"))
        a, b = data_bytes(str(tmp_path / "dense")), data_bytes(str(tmp_path / "csr"))
        assert a and a == b
        loaded = KnnModel.load(str(tmp_path / "csr"))
        assert type(loaded.get_model_data()[0].column("packedFeatures")[0]) is DenseMatrix
        assert np.array_equal(predict(loaded, Q), want)
        assert not isinstance(loaded._model_state(), mknn._CsrState)
        # a dense query column against the CSR-backed model: the dense route
        assert np.array_equal(predict(csr, Q.to_dense(torch.float64)), want)


def model_arrays(model):
    packed, norms, labels = model.model_data_rows()[0]
    c = packed.csr
    return (c.indptr.cpu().numpy(), c.indices.cpu().numpy(), c.values.cpu().numpy(), c.size,
            np.asarray(norms.values), np.asarray(labels.values))


def _two_rank_worker(rank, world):
    from flink_ml_amd.ops import knn as knn_ops

    knn_ops.CSR_ROUTE = "1"  # (this process is the rank's own)
    X, y, Q = data()
    lo, hi = (0, 23) if rank == 0 else (23, N)
    model = Knn().set_k(5).fit(Table({"features": X.slice(lo, hi), "label": y[lo:hi]}))
    return model_arrays(model), predict(model, Q)


def test_two_ranks_equal_one_rank(monkeypatch):
    X, y, Q = data()
    with on_cpu():
        one = fit(X, y, "1", monkeypatch)
        ref, want = model_arrays(one), predict(one, Q)
    for arrays, pred in run_spmd(_two_rank_worker, 2):
        for a, b in zip(arrays, ref):
            assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype
        assert np.array_equal(pred, want)


def with_entry(X, row, index, value=1.0):
    """``X`` with one more entry at the end of ``row``."""
    at = int(X.indptr[row + 1])
    ptr = X.indptr.clone()
    ptr[row + 1:] += 1
    idx = torch.cat([X.indices[:at], torch.tensor([index], dtype=X.indices.dtype), X.indices[at:]])
    val = torch.cat([X.values[:at], torch.tensor([value], dtype=X.values.dtype), X.values[at:]])
    return SparseColumn(ptr, idx, val, X.size)


def test_errors(monkeypatch):
    X, y, Q = data()
    with on_cpu():
        for bad in (D, D + 7, -1):
            with pytest.raises(ValueError, match="out of range"):
                fit(with_entry(X, 3, bad), y, "1", monkeypatch)
        model = fit(X, y, "1", monkeypatch)
        for bad in (D, -1):
            with pytest.raises(ValueError, match="out of range"):
                predict(model, with_entry(Q, 5, bad))
        for size in (D - 1, D + 1):
            with pytest.raises(ValueError, match="Vector size mismatched."):
                predict(model, SparseColumn(Q.indptr, Q.indices.clamp(max=D - 2), Q.values, size))


def test_duplicated_training_index_keeps_the_dense_route(monkeypatch):
    X, y, Q = data()
    row = 7
    dup = with_entry(X, row, int(X.indices[int(X.indptr[row])]), 3.0)
    with on_cpu():
        want = predict(fit(dup, y, "0", monkeypatch), Q)
        model = fit(dup, y, "1", monkeypatch)
        assert isinstance(model.get_model_data()[0].column("packedFeatures")[0], mknn.CsrPackedFeatures)
        assert not isinstance(model._model_state(), mknn._CsrState)
        assert np.array_equal(predict(model, Q), want)
    # a duplicated index in a query row is taken as it is stored: both entries count
    cm = knn_ops.TorchColumnMajor(X)
    assert not knn_ops.has_duplicate_index(cm) and knn_ops.has_duplicate_index(knn_ops.TorchColumnMajor(dup))
    q2 = with_entry(Q, 0, int(Q.indices[0]), 2.0)
    G, G2 = knn_ops.torch_products_csr(Q, cm), knn_ops.torch_products_csr(q2, cm)
    col = X.to_dense()[:, int(Q.indices[0])]
    assert torch.equal(G2[0], G[0] + 2.0 * col) and torch.equal(G2[1:], G[1:])


def _column_with(nnz: int, n=100, D=100) -> SparseColumn:
    cells = torch.arange(nnz)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(cells // D, minlength=n), 0)
    return SparseColumn(ptr, (cells % D).to(torch.int32), torch.ones(nnz, dtype=torch.float64), D)


def test_routing(monkeypatch):
    cpu = torch.device("cpu")
    monkeypatch.setattr(knn_ops, "CSR_CROSSOVER", 0.05)
    below, above = _column_with(500), _column_with(501)
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "0")
    assert not knn_ops.csr_route(below, cpu) and not knn_ops.csr_route(above, cpu)
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "1")
    assert knn_ops.csr_route(below, cpu) and knn_ops.csr_route(above, cpu)
    assert not knn_ops.csr_supported(torch.zeros(3, 3), cpu) and not knn_ops.csr_route(torch.zeros(3, 3), cpu)
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "auto")
    assert knn_ops.csr_route(below, cpu) and not knn_ops.csr_route(above, cpu)
    monkeypatch.setattr(knn_ops, "CSR_CROSSOVER", 0.0)  # only the memory criterion routes
    assert not knn_ops.csr_route(_column_with(1), cpu)
    assert set(knn_ops.CSR_TILE_ROWS) == {torch.float32, torch.float64}
    for dt, tile in knn_ops.CSR_TILE_ROWS.items():
        assert tile in knn_ops.CSR_TILE_ROWS_BUILT[dt] and tile % 256 == 0
    # under "0" the stage densifies, as before
    monkeypatch.setattr(knn_ops, "CSR_ROUTE", "0")
    monkeypatch.setattr(SparseColumn, "to_dense", no_dense)
    X, y, _ = data()
    with on_cpu(), pytest.raises(AssertionError, match="to_dense"):
        Knn().fit(Table({"features": X, "label": y}))
