"""The CSR column-statistics kernel (csrc/colstats_csr.hip) against the fp64 torch formulations of
ops/features.py, and the stages that fit through it against the same stages on the host.

Input (the generator documented in tests/test_kmeans_csr_gpu.py): rows of 1-64 draws (every 97th
row empty); columns min(zipf(1.1) - 1, D - 1) plus max(1, L // 2) uniform ones, unique per row;
values N(1.5, 1); n = 12,000, D = 5,000 and 2^20. The head column holds most rows: three segments
of CSR_COL_SEGMENT entries. The oracle sees the values rounded to the dtype the device holds.

Sums are compared within 4·(m_j + 1)·2^-53·Σ|terms_j| (m_j: the column's stored count), the
worst-case distance of two fp64 summation orders of the same terms; stored, min and max exactly."""
import functools

import numpy as np
import pytest
import torch

from flink_ml_amd import Table
from flink_ml_amd.ops import features as fo
from flink_ml_amd.ops import kmeans as kk
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd
from tests.test_colstats_csr import fit_stages, on_cpu, sum_bound, within

pytestmark = pytest.mark.gpu

N, D_SMALL, D_WIDE = 12000, 5000, 1 << 20
DTYPES = [torch.float32, torch.float64]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_input(n, D, seed=5):
    """(indptr, indices, values) as numpy arrays; see the module docstring."""
    rs = np.random.RandomState(seed)
    ptr, cols, vals = [0], [], []
    for i in range(n):
        if i % 97 == 96:
            ptr.append(ptr[-1])
            continue
        L = int(rs.randint(1, 65))
        c = np.concatenate([np.minimum(rs.zipf(1.1, L) - 1, D - 1), rs.randint(0, D, max(1, L // 2))])
        _, first = np.unique(c, return_index=True)
        c = c[np.sort(first)]  # unique, unsorted
        cols.append(c)
        vals.append(rs.normal(1.5, 1.0, c.shape[0]))
        ptr.append(ptr[-1] + c.shape[0])
    return np.asarray(ptr, np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(vals)


@functools.lru_cache(maxsize=None)
def host_column(D: int, dtype=torch.float64) -> SparseColumn:
    """The input on the host, its values rounded to ``dtype`` (held as fp64)."""
    ptr, idx, val = make_input(N, D)
    X = SparseColumn(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(val).to(dtype).double(), D)
    longest = int(torch.bincount(X.indices.long(), minlength=D).max())
    assert longest > 2 * kk.CSR_COL_SEGMENT  # the head column is summed in three segments
    return X


def handmade(dtype=torch.float64) -> SparseColumn:
    """130 x 70: column 0 in every row with values >= 1, column 1 negative in the even rows, column 2
    stored zeros, column 3 empty, random entries elsewhere, the last column included."""
    n, D = 130, 70
    rs = np.random.RandomState(3)
    ptr, cols, vals = [0], [], []
    for i in range(n):
        c, v = [0], [1.0 + rs.rand()]
        if i % 2 == 0:
            c.append(1)
            v.append(-0.5 - rs.rand())
        if i % 3 == 0:
            c.append(2)
            v.append(0.0)
        extra = np.unique(rs.randint(4, D, 6))
        if i % 5 == 0:
            extra = np.union1d(extra, [D - 1])
        c += extra.tolist()
        v += rs.normal(0.0, 2.0, extra.shape[0]).tolist()
        order = rs.permutation(len(c))
        cols.append(np.asarray(c)[order])
        vals.append(np.asarray(v)[order])
        ptr.append(ptr[-1] + len(c))
    return SparseColumn(torch.tensor(ptr, dtype=torch.int64), torch.from_numpy(np.concatenate(cols).astype(np.int32)),
                        torch.from_numpy(np.concatenate(vals)).to(dtype).double(), D)


def on_device(X: SparseColumn, dtype) -> SparseColumn:
    return X.to(device=torch.device("cuda"), dtype=dtype)


def groups_and_weights(n, G, weighted):
    g = torch.Generator().manual_seed(100 + G)
    gidx = torch.randint(0, G, (n,), generator=g).to(torch.int32) if G > 1 else None
    w = torch.randn(n, generator=g, dtype=torch.float64) if weighted else None
    return gidx, w


def check_against_oracle(Xh: SparseColumn, dtype, G, weighted):
    from flink_ml_amd.ops.csr import ColumnMajor

    gidx, w = groups_and_weights(len(Xh), G, weighted)
    cm = ColumnMajor(on_device(Xh, dtype))
    S, sm, sq, mn, mx, stored = fo.colstats_csr_windows(cm, gidx, G, w)
    kk.check_csr_error(cm)
    ref = fo.torch_column_stats_csr(Xh)
    assert torch.equal(stored.cpu(), ref["stored"])
    assert torch.equal(mn.cpu(), ref["min"]) and torch.equal(mx.cpu(), ref["max"])
    Sr, smr, sqr = fo.torch_group_colstats_csr(Xh, gidx, G, w)
    bS, bs, bq = sum_bound(Xh, gidx, G, w)
    assert S.shape == (G, Xh.size)
    within(S, Sr, bS)
    within(sm, smr, bs)
    within(sq, sqr, bq)
    return cm


CASES = [(1, True), (3, False), (32, False), (40, False)]  # G = 40: two windows of the kernel


@pytest.mark.parametrize("G,weighted", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [D_SMALL, D_WIDE])
def test_kernel_matches_fp64_oracle(D, dtype, G, weighted):
    _need_gpu()
    cm = check_against_oracle(host_column(D, dtype), dtype, G, weighted)
    assert cm.nlong == 6 and cm.nsegs >= 6 + 2  # six columns exceed a segment, the head column twice


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_handmade_columns(dtype):
    _need_gpu()
    Xh = handmade(dtype)
    for G, weighted in CASES:
        check_against_oracle(Xh, dtype, G, weighted)
    s = fo.column_stats_csr(on_device(Xh, dtype))
    n, D = len(Xh), Xh.size
    assert s["count"] == n and int(s["stored"][0]) == n and float(s["min"][0]) >= 1.0
    assert float(s["max"][1]) == 0.0 and float(s["min"][1]) < 0.0 and int(s["stored"][1]) == n // 2
    assert int(s["stored"][2]) == -(-n // 3) and float(s["min"][2]) == 0.0 == float(s["max"][2])
    assert int(s["stored"][3]) == 0
    for k in ("sum", "sumsq", "min", "max"):
        assert float(s[k][3]) == 0.0
    assert int(s["stored"][D - 1]) >= n // 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_no_entries_and_no_rows(dtype):
    _need_gpu()
    dev = torch.device("cuda")
    empty = lambda n: SparseColumn(torch.zeros(n + 1, dtype=torch.int64, device=dev),  # noqa: E731
                                   torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=dtype, device=dev), 7)
    z = fo.column_stats_csr(empty(5))
    assert z["count"] == 5 and not bool(z["stored"].any())
    for k in ("sum", "sumsq", "min", "max"):
        assert z[k].shape == (7,) and not bool(z[k].any())
    e = fo.column_stats_csr(empty(0))
    assert e["count"] == 0 and not bool(e["sum"].any()) and not bool(e["sumsq"].any())
    assert bool((e["min"] == float("inf")).all()) and bool((e["max"] == -float("inf")).all())
    S, sm, sq = fo.group_colstats_csr(empty(5), torch.zeros(5, dtype=torch.int32), 3)
    assert S.shape == (3, 7) and not bool(S.any()) and not bool(sm.any()) and not bool(sq.any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_reproducible(dtype):
    _need_gpu()
    from flink_ml_amd.ops.csr import ColumnMajor

    Xh = host_column(D_SMALL, dtype)
    gidx, w = groups_and_weights(N, 40, True)
    a = fo.colstats_csr_windows(ColumnMajor(on_device(Xh, dtype)), gidx, 40, w)
    b = fo.colstats_csr_windows(ColumnMajor(on_device(Xh, dtype)), gidx, 40, w)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        if x.is_floating_point():
            assert torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


def test_bad_index_raises_and_other_columns_stand():
    _need_gpu()
    from flink_ml_amd.ops.csr import ColumnMajor

    Xh = host_column(D_SMALL).slice(0, 300)
    at = int(Xh.indptr[150])
    idx = Xh.indices.clone()
    idx[at] = D_SMALL  # one past the last column
    bad = SparseColumn(Xh.indptr, idx, Xh.values, D_SMALL)
    keep = torch.ones(idx.numel(), dtype=torch.bool)
    keep[at] = False
    ptr = Xh.indptr.clone()
    ptr[151:] -= 1
    rest = SparseColumn(ptr, Xh.indices[keep], Xh.values[keep], D_SMALL)  # the column without that entry
    cm = ColumnMajor(on_device(bad, torch.float64))
    S, sm, sq, mn, mx, stored = fo.colstats_csr_windows(cm)
    ref = fo.torch_column_stats_csr(rest)
    assert torch.equal(stored.cpu(), ref["stored"])
    assert torch.equal(mn.cpu(), ref["min"]) and torch.equal(mx.cpu(), ref["max"])
    _, bs, bq = sum_bound(rest)
    within(sm, ref["sum"], bs)
    within(sq, ref["sumsq"], bq)
    with pytest.raises(ValueError):
        kk.check_csr_error(cm)
    with pytest.raises(ValueError):
        fo.column_stats_csr(on_device(bad, torch.float64))
    with pytest.raises(ValueError):
        fo.group_colstats_csr(on_device(bad, torch.float64))
    # the device is intact: the good column goes through
    assert fo.column_stats_csr(on_device(Xh, torch.float64))["count"] == 300


# ------------------------------------------------------------------------------------------------
# stage level
# ------------------------------------------------------------------------------------------------
FLOAT_KEYS = ("mean", "std", "anova_f", "fvalue_f")
SET_KEYS = ("var_idx", "ufs_anova", "ufs_fvalue")


def _stage_labels():
    g = torch.Generator().manual_seed(4)
    return (torch.arange(N) % 3).double(), torch.randn(N, generator=g, dtype=torch.float64)


def rel_err(got, ref) -> float:
    """The largest relative error over the finite, nonzero reference entries; NaNs must coincide."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    m = np.isfinite(ref) & (ref != 0)
    return float((np.abs(got[m] - ref[m]) / np.abs(ref[m])).max())


def _gpu_stages(route, ref, monkeypatch_route):
    from flink_ml_amd.config import dtype_policy

    monkeypatch_route(route)
    yc, yr = _stage_labels()
    with dtype_policy("fp64"):
        return fit_stages(host_column(D_SMALL), yc, yr, ref["var_threshold"], ref["fpr"])


@functools.lru_cache(maxsize=None)
def stage_runs():
    """The six stages on the host in fp64 on the densified table (the reference), and on the GPU
    through the CSR route and through the dense route; the routes' largest relative errors."""
    old = fo.COLSTATS_CSR_ROUTE

    def set_route(r):
        fo.COLSTATS_CSR_ROUTE = r

    try:
        yc, yr = _stage_labels()
        with on_cpu():
            set_route("0")
            ref = fit_stages(host_column(D_SMALL).to_dense(torch.float64), yc, yr)
        csr = _gpu_stages("1", ref, set_route)
        dense = _gpu_stages("0", ref, set_route)
    finally:
        set_route(old)
    errs = {k: (rel_err(csr[k], ref[k]), rel_err(dense[k], ref[k])) for k in FLOAT_KEYS}
    return ref, csr, dense, errs


def stage_limit(errs, k) -> float:
    """At most 8x the dense route's error, and never below 1e-12: both routes are fp64 sums of at
    most 12,000 equal terms in different orders."""
    return max(8.0 * errs[k][1], 1e-12)


def test_stages_csr_route_as_accurate_as_dense_route():
    _need_gpu()
    ref, csr, dense, errs = stage_runs()
    for k in FLOAT_KEYS:
        print("stage-level %s: csr route %.3e, dense route %.3e (relative, against the fp64 host run)"
              % (k, errs[k][0], errs[k][1]))
    for k in FLOAT_KEYS:
        assert errs[k][0] <= stage_limit(errs, k), (k, errs[k])
    for got in (csr, dense):
        assert np.array_equal(got["min"], ref["min"]) and np.array_equal(got["max"], ref["max"])
        for k in SET_KEYS:
            assert got[k] == ref[k], k
    for k in SET_KEYS:
        assert 0 < len(ref[k]) < D_SMALL


def test_fits_bounded_memory_at_wide_columns(monkeypatch):
    """2,000 x 2^20 with 3 classes, device-resident, the knob at auto: densified it is 8.4 GB in fp32
    (16.8 GB in fp64 for ANOVATest); each fit stays under n·D·4 / 16 = 524 MB above its inputs."""
    _need_gpu()
    from flink_ml_amd.models import ANOVATest, StandardScaler
    from flink_ml_amd.ops import native

    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "auto")
    n, D, L = 2000, D_WIDE, 32
    dev = torch.device("cuda")
    native.kernels()
    g = torch.Generator().manual_seed(3)
    start = torch.randint(0, D, (n, 1), generator=g)
    stride = torch.randint(0, D // 2, (n, 1), generator=g) * 2 + 1  # odd: the L columns of a row are distinct
    idx = ((start + torch.arange(L)[None, :] * stride) % D).to(torch.int32).reshape(-1)
    val = torch.randn(n * L, generator=g) + 1.5
    X = SparseColumn(torch.arange(0, n * L + 1, L, dtype=torch.int64), idx, val, D).to(device=dev, dtype=torch.float32)
    t = Table({"features": X, "label": (torch.arange(n) % 3).double().to(dev)})
    limit = n * D * 4 // 16
    for name, fit in (("StandardScaler.fit", lambda: StandardScaler().set_input_col("features").fit(t)),
                      ("ANOVATest.transform", lambda: ANOVATest().transform(t))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fit()
        peak = torch.cuda.max_memory_allocated(dev) - base
        print("%s: peak above the inputs %.1f MiB" % (name, peak / 2 ** 20))
        assert peak < limit, name
    assert len(out[0].get_list("fValues")[0].values) == D


def _two_rank_worker(rank, world):
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import ANOVATest, StandardScaler
    from flink_ml_amd.ops import features as fo

    fo.COLSTATS_CSR_ROUTE = "1"  # (this process is the rank's own)
    yc, _ = _stage_labels()
    X = host_column(D_SMALL)
    lo, hi = (0, N // 2) if rank == 0 else (N // 2, N)
    t = Table({"features": X.slice(lo, hi), "label": yc[lo:hi]})
    with dtype_policy("fp64"):
        mean, std = StandardScaler().set_input_col("features").fit(t).get_model_data()[0].rows()[0]
        f = np.asarray(ANOVATest().compute(t)[2])
    return mean.values, std.values, f


def test_two_ranks_sharing_the_gpu_equal_one_rank():
    _need_gpu()
    _, csr, _, errs = stage_runs()
    res = run_spmd(_two_rank_worker, 2, env={"FMLX_DEVICE": "cuda:0", "FMLX_XGMI": "0"}, timeout=300)
    for mean, std, f in res:
        for k, got in (("mean", mean), ("std", std), ("anova_f", f)):
            e = rel_err(got, csr[k])
            print("two ranks %s: %.3e against one rank" % (k, e))
            assert e <= stage_limit(errs, k), (k, e)
    for a, b in zip(res[0], res[1]):
        assert a.tobytes() == b.tobytes()
