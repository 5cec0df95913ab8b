"""Contingency tables of CSR feature columns without densifying (ops/catstats.py: the numpy
formulation over the CSR arrays, the routing knob) and the stages on them (ChiSqTest,
UnivariateFeatureSelector with categorical features and labels, NaiveBayes fit and predict), on the
host.

Input (``make_input``, the structure of tests/test_colstats_csr_gpu.make_input): every 97th row empty;
columns min(zipf(1.1) - 1, D - 1) plus uniform ones, unique per row; values min(geometric(0.5), 6),
every 53rd entry 0.0, every 211th -2.5, every 307th -0.0; labels (7 i + randint(0, 3)) % 3. The cut
used here is 1,500 x 400; the handmade 130 x 70 column adds an all-stored column with no zero
category (column 0), stored zeros (column 2) and an empty column (column 3).

Counts are integers: every comparison of tables, statistics, p-values and model bytes is exact."""
import functools
import io

import numpy as np
import pytest
import torch

from flink_ml_amd import Table
from flink_ml_amd.models import stats as mstats
from flink_ml_amd.ops import catstats
from flink_ml_amd.ops import features as fo
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd
from tests.test_colstats_csr import _gap_threshold, on_cpu

N_CUT, D_CUT = 1500, 400


def make_input(n, D, seed=5, nan_every=0):
    """(indptr, indices, values) as numpy arrays; see the module docstring."""
    rs = np.random.RandomState(seed)
    ptr, cols = [0], []
    for i in range(n):
        if i % 97 == 96:
            ptr.append(ptr[-1])
            continue
        L = int(rs.randint(1, 65))
        c = np.concatenate([np.minimum(rs.zipf(1.1, L) - 1, D - 1), rs.randint(0, D, max(1, L // 2))])
        _, first = np.unique(c, return_index=True)
        cols.append(c[np.sort(first)])  # unique, unsorted
        ptr.append(ptr[-1] + cols[-1].shape[0])
    cols = np.concatenate(cols).astype(np.int32)
    vals = np.minimum(rs.geometric(0.5, cols.shape[0]), 6).astype(np.float64)
    e = np.arange(cols.shape[0])
    vals[e % 53 == 52] = 0.0
    vals[e % 211 == 210] = -2.5
    vals[e % 307 == 306] = -0.0
    if nan_every:
        vals[e % nan_every == nan_every - 1] = np.nan
    return np.asarray(ptr, np.int64), cols, vals


def class_labels(n, seed=9):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(((7 * np.arange(n) + rs.randint(0, 3, n)) % 3).astype(np.float64))


@functools.lru_cache(maxsize=None)
def generated(n=N_CUT, D=D_CUT, nan_every=0) -> SparseColumn:
    ptr, idx, val = make_input(n, D, nan_every=nan_every)
    return SparseColumn(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(val), D)


@functools.lru_cache(maxsize=None)
def handmade_counts() -> SparseColumn:
    """The 130 x 70 layout of tests/test_colstats_csr_gpu.handmade with categorical values: column 0
    in every row (values 1 … 3: no zero category), column 1 negative in the even rows, column 2 stored
    zeros (+0.0 and -0.0), column 3 empty, small counts elsewhere, the last column included."""
    n, D = 130, 70
    rs = np.random.RandomState(3)
    ptr, cols, vals = [0], [], []
    for i in range(n):
        c, v = [0], [float(rs.randint(1, 4))]
        if i % 2 == 0:
            c.append(1)
            v.append(-float(rs.randint(1, 3)))
        if i % 3 == 0:
            c.append(2)
            v.append(0.0 if i % 2 else -0.0)
        extra = np.unique(rs.randint(4, D, 6))
        if i % 5 == 0:
            extra = np.union1d(extra, [D - 1])
        c += extra.tolist()
        v += np.minimum(rs.geometric(0.5, extra.shape[0]), 4).astype(np.float64).tolist()
        order = rs.permutation(len(c))
        cols.append(np.asarray(c)[order])
        vals.append(np.asarray(v)[order])
        ptr.append(ptr[-1] + len(c))
    return SparseColumn(torch.tensor(ptr, dtype=torch.int64), torch.from_numpy(np.concatenate(cols).astype(np.int32)),
                        torch.from_numpy(np.concatenate(vals)), D)


def dense_tables(Xd: torch.Tensor, li: torch.Tensor, L: int):
    """The dense CPU route's tables (models/stats.py ChiSqTest on one host rank): per feature the
    sorted distinct values and the [V, L] counts."""
    vals, tabs = [], []
    for j in range(Xd.shape[1]):
        v = torch.unique(Xd[:, j])
        vi = torch.searchsorted(v, Xd[:, j].contiguous())
        vals.append(v.numpy())
        tabs.append(torch.bincount(vi * L + li, minlength=v.numel() * L).reshape(-1, L).numpy())
    return vals, tabs


def assert_equals_dense(rc, Xd, li, L):
    colfirst, values, counts, n_label = rc.numpy()
    vals, tabs = dense_tables(Xd, li, L)
    assert colfirst.shape[0] == Xd.shape[1] + 1 and colfirst[0] == 0 and colfirst[-1] == values.shape[0]
    assert np.array_equal(np.diff(colfirst), [v.shape[0] for v in vals])
    assert np.array_equal(values, np.concatenate(vals))  # (-0.0 == 0.0)
    assert not np.signbit(values).any() or values.min() < 0  # no -0.0 is left
    assert not np.signbit(values[values == 0.0]).any()
    assert np.array_equal(counts, np.concatenate(tabs))
    assert np.array_equal(n_label, np.bincount(li.numpy(), minlength=L))


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("which", ["handmade", "generated"])
def test_csr_formulation_equals_dense_tables(which, L):
    X = handmade_counts() if which == "handmade" else generated()
    n = len(X)
    li = (class_labels(n).long() if L == 3 else torch.zeros(n, dtype=torch.int64))
    Xd = X.to_dense(torch.float64)
    rc = catstats.torch_value_label_counts_csr(X, li, L)
    assert_equals_dense(rc, Xd, li, L)
    colfirst, values, counts, _ = rc.numpy()
    if which == "handmade":
        assert values[colfirst[0]:colfirst[1]].min() >= 1.0          # all stored, no zero category
        assert np.array_equal(values[colfirst[3]:colfirst[4]], [0.0])  # the empty column: one zero row
        assert counts[colfirst[3]].sum() == n
        z2 = colfirst[2] + np.searchsorted(values[colfirst[2]:colfirst[3]], 0.0)
        assert values[z2] == 0.0 and counts[z2].sum() == n             # stored ±0 merged with the implicit zeros
    else:
        assert int((X.indptr[1:] == X.indptr[:-1]).sum()) == n // 97
        assert (values == -2.5).any() and (X.values == 0.0).any()


def test_csr_formulation_edge_cases():
    e = lambda n: SparseColumn(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),  # noqa: E731
                               torch.zeros(0, dtype=torch.float64), 4)
    c0, v0, t0, _ = catstats.torch_value_label_counts_csr(e(0), torch.zeros(0, dtype=torch.int64), 2).numpy()
    assert np.array_equal(c0, [0] * 5) and v0.size == 0 and t0.shape == (0, 2)
    c1, v1, t1, n1 = catstats.torch_value_label_counts_csr(e(3), torch.tensor([0, 1, 1]), 2).numpy()
    assert np.array_equal(c1, [0, 1, 2, 3, 4]) and not v1.any() and np.array_equal(t1, [[1, 2]] * 4)
    assert np.array_equal(n1, [1, 2])
    nan = SparseColumn(torch.tensor([0, 1, 2, 3]), torch.tensor([1, 1, 1], dtype=torch.int32),
                       torch.tensor([float("nan"), 2.0, float("nan")], dtype=torch.float64), 2)
    c2, v2, t2, _ = catstats.torch_value_label_counts_csr(nan, torch.tensor([0, 0, 1]), 2).numpy()
    assert np.array_equal(c2, [0, 1, 3]) and v2[1] == 2.0 and np.isnan(v2[2])  # NaN: one value, last
    assert np.array_equal(t2, [[2, 1], [1, 0], [1, 1]])
    bad = SparseColumn(torch.tensor([0, 1]), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.float64), 4)
    with pytest.raises(ValueError):
        catstats.torch_value_label_counts_csr(bad, torch.zeros(1, dtype=torch.int64), 1)


# ------------------------------------------------------------------------------------------------
# stage level
# ------------------------------------------------------------------------------------------------
def model_bytes(model) -> bytes:
    from flink_ml_amd.io.serialization import DataOutput

    out = DataOutput(io.BytesIO())
    type(model).encode_record(out, model.model_data_rows()[0])
    return out.stream.getvalue()


def run_stages(features, y, fpr=None, smoothing=1.0):
    """ChiSqTest, the categorical selector, NaiveBayes fit and predict on one feature column."""
    from flink_ml_amd.models import ChiSqTest, NaiveBayes, UnivariateFeatureSelector

    t = Table({"features": features, "label": y})
    out = {}
    out["p"], out["dof"], out["stat"] = ChiSqTest().compute(t)
    out["fpr"] = _gap_threshold(out["p"]) if fpr is None else fpr
    sel = UnivariateFeatureSelector().set_feature_type("categorical").set_label_type("categorical") \
        .set_selection_mode("fpr").set_selection_threshold(out["fpr"])
    out["ufs"] = sorted(sel.fit(t).get_model_data()[0].rows()[0][0])
    model = NaiveBayes().set_smoothing(smoothing).fit(t)
    out["model"] = model
    out["model_bytes"] = model_bytes(model)
    out["pred"] = np.asarray(model.transform(t)[0].column("prediction").cpu())
    return out


def no_dense(self, *a, **k):
    raise AssertionError("SparseColumn.to_dense called")


@pytest.mark.parametrize("as_vectors", [False, True])
def test_stages_on_sparse_column_without_densifying(as_vectors, monkeypatch):
    X = generated()
    y = class_labels(N_CUT)
    with on_cpu():
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "0")
        ref = run_stages(X.to_dense(torch.float64), y)
        monkeypatch.setattr(SparseColumn, "to_dense", no_dense)
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
        features = [X.row(i) for i in range(N_CUT)] if as_vectors else X
        got = run_stages(features, y, ref["fpr"])
    assert got["p"] == ref["p"] and got["dof"] == ref["dof"] and got["stat"] == ref["stat"]
    assert got["ufs"] == ref["ufs"] and 0 < len(ref["ufs"]) < D_CUT
    assert got["model_bytes"] == ref["model_bytes"]
    assert np.array_equal(got["pred"], ref["pred"])
    assert len(set(ref["pred"].tolist())) > 1


def test_unseen_value_names_the_dense_routes_feature(monkeypatch):
    from flink_ml_amd.models import NaiveBayes

    X = handmade_counts()
    n = len(X)
    y = class_labels(n)
    with on_cpu():
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
        model = NaiveBayes().fit(Table({"features": X, "label": y}))
        # column 0 has no zero category in the model: a row that does not store it is unseen there;
        # the changed value in column 40 is unseen too, and the lower feature is named
        keep = torch.ones(X.indices.numel(), dtype=torch.bool)
        at = int(torch.nonzero(X.indices[int(X.indptr[5]):int(X.indptr[6])] == 0)[0]) + int(X.indptr[5])
        keep[at] = False
        ptr = X.indptr.clone()
        ptr[6:] -= 1
        vals = X.values.clone()
        c40 = int(torch.nonzero(X.indices == 40)[0])
        vals[c40] = 17.0
        for Xbad, feature in ((SparseColumn(X.indptr, X.indices, vals, X.size), 40),
                              (SparseColumn(ptr, X.indices[keep], vals[keep], X.size), 0)):
            for route in ("1", "0"):
                monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", route)
                with pytest.raises(RuntimeError, match="Feature %d of the input" % feature):
                    model.transform(Table({"features": Xbad}))


def old_chisq_finish(Vn, flat, L):
    """The per-feature finish ChiSqTest had before the batched one."""
    from scipy import stats as sps

    p_out, dof_out, stat_out, off = [], [], [], 0
    for V in Vn:
        obs = flat[off:off + V * L].reshape(V, L)
        off += V * L
        n = obs.sum()
        exp = np.outer(obs.sum(1), obs.sum(0)) / n
        stat = float(((obs - exp) ** 2 / exp).sum())
        dof = (V - 1) * (L - 1)
        if dof == 0:
            stat, p = 0.0, 1.0
        else:
            p = 1.0 - float(sps.chi2.cdf(stat, dof))
        p_out.append(mstats._round11(p))
        dof_out.append(dof)
        stat_out.append(mstats._round11(stat))
    return p_out, dof_out, stat_out


def test_batched_statistics_bitwise_equal_per_feature():
    rs = np.random.RandomState(1)
    for L in (1, 2, 3, 5, 40):
        Vn = np.concatenate([rs.randint(1, 41, 300), [1, 2, 40, 40, 173]])  # (173: a group of one table)
        rs.shuffle(Vn)
        scale = rs.choice([3, 50, 4000, 10 ** 6], Vn.shape[0])
        flat = np.concatenate([rs.poisson(s, V * L) + 1 for V, s in zip(Vn, scale)]).astype(np.float64)
        stat = mstats.chisq_statistics(Vn, flat, L)
        off = np.concatenate([[0], np.cumsum(Vn * L)])
        for j, V in enumerate(Vn):
            if V > 1 and L > 1:
                one = mstats.chisq_statistic_one(flat[off[j]:off[j + 1]].reshape(V, L))
                assert stat[j].tobytes() == np.float64(one).tobytes(), (V, L)
        old_batch, mstats.CHISQ_BATCH_CELLS = mstats.CHISQ_BATCH_CELLS, 1000  # a group split into several batches
        try:
            assert mstats.chisq_statistics(Vn, flat, L).tobytes() == stat.tobytes()
        finally:
            mstats.CHISQ_BATCH_CELLS = old_batch
        got, ref = mstats.chisq_finish(Vn, flat, L), old_chisq_finish(Vn.tolist(), flat, L)
        for g, r in zip(got, ref):
            assert np.asarray(g, dtype=np.float64).tobytes() == np.asarray(r, dtype=np.float64).tobytes()


def _column_with(nnz: int, n=100, D=100) -> SparseColumn:
    cells = torch.arange(nnz)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(cells // D, minlength=n), 0)
    return SparseColumn(ptr, (cells % D).to(torch.int32), torch.ones(nnz, dtype=torch.float64), D)


def test_routing(monkeypatch):
    cpu = torch.device("cpu")
    at = int(catstats.CATSTATS_CSR_CROSSOVER * 100 * 100)
    assert at >= 1
    below, above = _column_with(at), _column_with(at + 1)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "0")
    assert not catstats.catstats_csr_route(below, cpu) and not catstats.catstats_csr_route(above, cpu)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
    assert catstats.catstats_csr_route(below, cpu) and catstats.catstats_csr_route(above, cpu)
    assert not catstats.catstats_csr_route(torch.zeros(3, 3), cpu)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "auto")
    assert catstats.catstats_csr_route(below, cpu) and not catstats.catstats_csr_route(above, cpu)
    monkeypatch.setattr(catstats, "CATSTATS_CSR_CROSSOVER", 0.5)
    assert catstats.catstats_csr_route(_column_with(5000), cpu) and not catstats.catstats_csr_route(_column_with(5001), cpu)
    # the stages follow the knob: under "0" a sparse column is densified
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "0")
    monkeypatch.setattr(SparseColumn, "to_dense", no_dense)
    from flink_ml_amd.models import ChiSqTest

    with on_cpu(), pytest.raises(AssertionError, match="to_dense"):
        ChiSqTest().compute(Table({"features": handmade_counts(), "label": class_labels(130)}))


def test_smoothing_zero_model_predicts_as_before(monkeypatch):
    """log(0) in theta: the model keeps the dense route, and predicts what it predicted."""
    X = handmade_counts()
    y = class_labels(len(X))
    with on_cpu():
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "0")
        ref = run_stages(X.to_dense(torch.float64), y, smoothing=0.0)
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
        got = run_stages(X, y, ref["fpr"], smoothing=0.0)
        assert got["model"]._csr_state() is None
    assert got["model_bytes"] == ref["model_bytes"]
    assert np.array_equal(got["pred"], ref["pred"])


def _two_rank_worker(rank, world):
    from flink_ml_amd.models import ChiSqTest
    from flink_ml_amd.ops import catstats
    from flink_ml_amd.ops import features as fo

    fo.COLSTATS_CSR_ROUTE = "1"  # (this process is the rank's own)
    X, y = generated(), class_labels(N_CUT)
    lo, hi = (0, N_CUT // 2) if rank == 0 else (N_CUT // 2, N_CUT)
    Xr, yr = X.slice(lo, hi), y[lo:hi]
    rc = catstats.global_value_label_counts_csr(Xr, yr.long(), 3)
    return rc.numpy(), ChiSqTest().compute(Table({"features": Xr, "label": yr}))


def test_two_ranks_give_the_one_rank_tables():
    X, y = generated(), class_labels(N_CUT)
    ref = catstats.torch_value_label_counts_csr(X, y.long(), 3).numpy()
    with on_cpu():
        from flink_ml_amd.models import ChiSqTest

        chi_ref = ChiSqTest().compute(Table({"features": X.to_dense(torch.float64), "label": y}))
    for tabs, chi in run_spmd(_two_rank_worker, 2):
        for a, b in zip(tabs, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert tuple(chi) == tuple(chi_ref)
