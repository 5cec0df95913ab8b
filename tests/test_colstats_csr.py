"""Column statistics of CSR feature columns without densifying (ops/features.py: the fp64 torch
formulations, the routing knob) and the stages that fit through them (StandardScaler, MinMaxScaler,
VarianceThresholdSelector, ANOVATest, FValueTest, UnivariateFeatureSelector), on the host.

Input: 500 x 300 at 5 % density, every 37th row empty; the augmented input adds column 300, stored
in every row with values in [1, 2), and column 301, negative values in the even rows.

Sums are compared within 4·(m_j + 1)·2^-53·Σ|terms_j| (m_j: the column's stored count), the
worst-case distance of two fp64 summation orders of the same terms."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from flink_ml_amd import Table
from flink_ml_amd.ops import features as fo
from flink_ml_amd.parallel import context as pctx
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd

N, D0 = 500, 300


@contextlib.contextmanager
def on_cpu():
    old = pctx._CTX
    pctx.set_context(pctx.SPMDContext(device=torch.device("cpu")))
    try:
        yield
    finally:
        pctx.set_context(old)


@functools.lru_cache(maxsize=None)
def host_column(augmented: bool) -> SparseColumn:
    rs = np.random.RandomState(11)
    mask = rs.rand(N, D0) < 0.05
    mask[36::37] = False
    vals = rs.normal(0.5, 1.0, (N, D0))
    D = D0 + 2 if augmented else D0
    ptr, cols, data = [0], [], []
    for i in range(N):
        c = np.nonzero(mask[i])[0]
        v = vals[i, c]
        if augmented:
            c = np.concatenate([c, [D0]])
            v = np.concatenate([v, [1.0 + rs.rand()]])
            if i % 2 == 0:
                c = np.concatenate([c, [D0 + 1]])
                v = np.concatenate([v, [-0.25 - rs.rand()]])
        cols.append(c)
        data.append(v)
        ptr.append(ptr[-1] + c.shape[0])
    return SparseColumn(torch.tensor(ptr, dtype=torch.int64), torch.from_numpy(np.concatenate(cols).astype(np.int32)),
                        torch.from_numpy(np.concatenate(data)), D)


def sum_bound(X: SparseColumn, gidx=None, G=1, w=None):
    """The bound of the module docstring for (S, Σx, Σx²)."""
    Xa = SparseColumn(X.indptr, X.indices, X.values.abs(), X.size)
    S, sm, sq = fo.torch_group_colstats_csr(Xa, gidx, G, None if w is None else w.abs())
    m = torch.bincount(X.indices.long(), minlength=X.size).double()
    f = 4.0 * (m + 1.0) * 2.0 ** -53
    return f[None, :] * S, f * sm, f * sq


def within(got, ref, bound):
    err = (got.double().cpu() - ref.double().cpu()).abs()
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("augmented", [False, True])
def test_oracle_matches_dense_formulation(augmented):
    X = host_column(augmented)
    Xd = X.to_dense(torch.float64)
    n, D = Xd.shape
    assert int((X.indptr[1:] == X.indptr[:-1]).sum()) == (0 if augmented else N // 37)
    ref, got = fo.column_stats(Xd), fo.torch_column_stats_csr(X)
    assert got["count"] == ref["count"] == n
    assert torch.equal(got["stored"], (Xd != 0).sum(0))
    assert torch.equal(got["min"], ref["min"]) and torch.equal(got["max"], ref["max"])
    _, bs, bq = sum_bound(X)
    within(got["sum"], ref["sum"], bs)
    within(got["sumsq"], ref["sumsq"], bq)
    if augmented:
        assert float(got["min"][D0]) >= 1.0 and int(got["stored"][D0]) == n
        assert float(got["max"][D0 + 1]) == 0.0 and float(got["min"][D0 + 1]) < 0.0
        assert int(got["stored"][D0 + 1]) == n // 2
    g = torch.Generator().manual_seed(2)
    w = torch.randn(n, generator=g, dtype=torch.float64)
    gidx = torch.randint(0, 5, (n,), generator=g)
    for gi, G, ww in ((None, 1, w), (gidx, 5, None)):
        Sr, smr, sqr = fo.group_colstats(Xd, gi, G, ww)
        S, sm, sq = fo.torch_group_colstats_csr(X, gi, G, ww)
        bS, bs, bq = sum_bound(X, gi, G, ww)
        assert S.shape == (G, D)
        within(S, Sr, bS)
        within(sm, smr, bs)
        within(sq, sqr, bq)


def test_oracle_edge_cases():
    e = fo.torch_column_stats_csr(SparseColumn(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                               torch.zeros(0, dtype=torch.float64), 4))
    assert e["count"] == 0 and bool((e["min"] == float("inf")).all()) and bool((e["max"] == -float("inf")).all())
    z = fo.torch_column_stats_csr(SparseColumn(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                               torch.zeros(0, dtype=torch.float64), 4))
    assert z["count"] == 3
    for k in ("sum", "sumsq", "min", "max"):
        assert not bool(z[k].any())
    bad = SparseColumn(torch.tensor([0, 1]), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.float64), 4)
    with pytest.raises(ValueError):
        fo.torch_column_stats_csr(bad)
    with pytest.raises(ValueError):
        fo.column_stats_csr(bad)
    with pytest.raises(ValueError):
        fo.group_colstats_csr(bad)


def _gap_threshold(values) -> float:
    """The middle of the widest gap between the sorted finite values: no tie decides a selection."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    v = v[np.isfinite(v)]
    i = int(np.argmax(np.diff(v)))
    assert v[i + 1] > v[i]
    return float((v[i] + v[i + 1]) / 2)


def _labels():
    g = torch.Generator().manual_seed(4)
    return (torch.arange(N) % 3).double(), torch.randn(N, generator=g, dtype=torch.float64)


def fit_stages(features, y_class, y_cont, var_threshold=None, fpr=None):
    """The six stages' results on one feature column; thresholds from the results when None."""
    from flink_ml_amd.models import (ANOVATest, FValueTest, MinMaxScaler, StandardScaler, UnivariateFeatureSelector,
                                     VarianceThresholdSelector)

    tc = Table({"features": features, "label": y_class})
    tr = Table({"features": features, "label": y_cont})
    out = {}
    mean, std = StandardScaler().set_input_col("features").fit(tc).get_model_data()[0].rows()[0]
    out["mean"], out["std"] = mean.values, std.values
    mn, mx = MinMaxScaler().set_input_col("features").fit(tc).get_model_data()[0].rows()[0]
    out["min"], out["max"] = mn.values, mx.values
    n = len(y_class)
    var = out["std"] ** 2 * (n - 1) / n
    out["var_threshold"] = _gap_threshold(var) if var_threshold is None else var_threshold
    out["var_idx"] = sorted(VarianceThresholdSelector().set_input_col("features").set_variance_threshold(
        out["var_threshold"]).fit(tc).get_model_data()[0].rows()[0][1])
    pa, _, fa = ANOVATest().compute(tc)
    pf, _, ff = FValueTest().compute(tr)
    out["anova_f"], out["fvalue_f"] = np.asarray(fa), np.asarray(ff)
    out["fpr"] = (_gap_threshold(pa), _gap_threshold(pf)) if fpr is None else fpr
    for name, lt, t, th in (("ufs_anova", "categorical", tc, out["fpr"][0]), ("ufs_fvalue", "continuous", tr, out["fpr"][1])):
        sel = UnivariateFeatureSelector().set_feature_type("continuous").set_label_type(lt).set_selection_mode("fpr") \
            .set_selection_threshold(th)
        out[name] = sorted(sel.fit(t).get_model_data()[0].rows()[0][0])
    return out


def compare_stages(got, ref, rtol):
    for k in ("mean", "std", "anova_f", "fvalue_f"):
        assert np.allclose(got[k], ref[k], rtol=rtol, atol=0.0, equal_nan=True), k
    assert np.array_equal(got["min"], ref["min"]) and np.array_equal(got["max"], ref["max"])
    for k in ("var_idx", "ufs_anova", "ufs_fvalue"):
        assert got[k] == ref[k], k
        assert 0 < len(ref[k]) < len(ref["mean"])  # the selection selects, and not everything


@pytest.mark.parametrize("as_vectors", [False, True])
def test_stages_fit_sparse_column_without_densifying(as_vectors, monkeypatch):
    X = host_column(True)
    yc, yr = _labels()
    with on_cpu():
        ref = fit_stages(X.to_dense(torch.float64), yc, yr)

        def no_dense(self, *a, **k):
            raise AssertionError("SparseColumn.to_dense called")

        monkeypatch.setattr(SparseColumn, "to_dense", no_dense)
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
        features = [X.row(i) for i in range(N)] if as_vectors else X
        got = fit_stages(features, yc, yr, ref["var_threshold"], ref["fpr"])
    compare_stages(got, ref, 1e-9)


def _column_with(nnz: int, n=100, D=100) -> SparseColumn:
    cells = torch.arange(nnz)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(cells // D, minlength=n), 0)
    return SparseColumn(ptr, (cells % D).to(torch.int32), torch.ones(nnz, dtype=torch.float64), D)


def test_routing(monkeypatch):
    cpu = torch.device("cpu")
    at = int(fo.COLSTATS_CSR_CROSSOVER * 100 * 100)
    below, above = _column_with(at), _column_with(at + 1)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "0")
    assert not fo.csr_stats_route(below, cpu) and not fo.csr_stats_route(above, cpu)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "1")
    assert fo.csr_stats_route(below, cpu) and fo.csr_stats_route(above, cpu)
    assert not fo.csr_stats_route(torch.zeros(3, 3), cpu)
    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "auto")
    assert fo.csr_stats_route(below, cpu) and not fo.csr_stats_route(above, cpu)
    monkeypatch.setattr(fo, "COLSTATS_CSR_CROSSOVER", 0.5)
    assert fo.csr_stats_route(_column_with(5000), cpu) and not fo.csr_stats_route(_column_with(5001), cpu)


def _two_rank_worker(rank, world):
    from flink_ml_amd.models import ANOVATest
    from flink_ml_amd.models.feature import scalers
    from flink_ml_amd.ops import features as fo

    fo.COLSTATS_CSR_ROUTE = "1"  # (this process is the rank's own)
    X = host_column(True)
    yc, _ = _labels()
    lo, hi = (0, N // 2) if rank == 0 else (N // 2, N)
    t = Table({"features": X.slice(lo, hi), "label": yc[lo:hi]})
    s = scalers._stats(t, "features")
    return {k: (v if isinstance(v, int) else v.numpy()) for k, v in s.items()}, np.asarray(ANOVATest().compute(t)[2])


def test_two_ranks_give_the_one_rank_statistics():
    X = host_column(True)
    yc, _ = _labels()
    ref = fo.torch_column_stats_csr(X)
    _, bs, bq = sum_bound(X)
    with on_cpu():
        from flink_ml_amd.models import ANOVATest

        f_ref = np.asarray(ANOVATest().compute(Table({"features": X.to_dense(torch.float64), "label": yc}))[2])
    for s, f in run_spmd(_two_rank_worker, 2):
        assert s["count"] == N
        assert np.array_equal(s["min"], ref["min"].numpy()) and np.array_equal(s["max"], ref["max"].numpy())
        within(torch.from_numpy(s["sum"]), ref["sum"], bs)
        within(torch.from_numpy(s["sumsq"]), ref["sumsq"], bq)
        assert np.allclose(f, f_ref, rtol=1e-9, atol=0.0, equal_nan=True)
