"""The CSR contingency kernels and the NaiveBayes CSR predict kernel (csrc/catstats_csr.hip) against
the numpy formulation over the CSR arrays (ops/catstats.py), and ChiSqTest, the categorical
UnivariateFeatureSelector and NaiveBayes on the GPU through the CSR route against the same stages on
the host on the densified table.

Input: tests/test_catstats_csr.make_input at n = 12,000, D = 5,000 and 2^20 (small counts, stored
zeros, -0.0, -2.5; a handful of NaN in the kernel-level tests only), and the handmade 130 x 70 column.
The head column's most frequent value is a run of more than two tiles of the count kernel. Counts are
integers: tables are compared exactly. Every value of the generator is exact in fp32, so one oracle
serves both dtypes."""
import functools

import numpy as np
import pytest
import torch

from flink_ml_amd import Table
from flink_ml_amd.ops import catstats
from flink_ml_amd.ops import features as fo
from flink_ml_amd.ops import kmeans as kk
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd
from tests.test_catstats_csr import class_labels, generated, handmade_counts, run_stages
from tests.test_colstats_csr import on_cpu

pytestmark = pytest.mark.gpu

N, D_SMALL, D_WIDE = 12000, 5000, 1 << 20
DTYPES = [torch.float32, torch.float64]
NAN_EVERY = 40009  # a handful of NaN entries among ~540,000


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def kernel_column(D: int) -> SparseColumn:
    return handmade_counts() if D == 70 else generated(N, D, NAN_EVERY)


def label_index(n: int, L: int) -> torch.Tensor:
    if L == 3:
        return class_labels(n).long()
    return torch.from_numpy((np.arange(n) * 7 + np.random.RandomState(L).randint(0, L, n)) % L)


@functools.lru_cache(maxsize=None)
def oracle(D: int, L: int):
    X = kernel_column(D)
    return catstats.torch_value_label_counts_csr(X, label_index(len(X), L), L).numpy()


def assert_tables_equal(rc, ref):
    got = rc.numpy()
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1], equal_nan=True)
    assert not np.signbit(got[1][got[1] == 0.0]).any()
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])


@pytest.mark.parametrize("L", [1, 3, 40])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [70, D_SMALL, D_WIDE])
def test_kernel_equals_csr_formulation(D, dtype, L):
    _need_gpu()
    X = kernel_column(D)
    n = len(X)
    ref = oracle(D, L)
    rc = catstats.value_label_counts_csr(X.to(device=torch.device("cuda"), dtype=dtype), label_index(n, L).cuda(), L)
    assert rc.colfirst.dtype == torch.int64 and rc.values.dtype == torch.float64
    assert_tables_equal(rc, ref)
    lds_tiles, atomic_tiles = rc.paths.cpu().tolist()
    assert lds_tiles + atomic_tiles > 0
    if D != 70:
        assert lds_tiles > 0  # (the head columns' long runs: few ids per tile)
        tile = int(catstats.native.kernels().fmlx_ccsr_tile())
        assert np.isnan(ref[1]).any()
        # stored runs: the rows of a nonzero value count exactly its entries
        longest = int(oracle(D, 1)[2][oracle(D, 1)[1] != 0.0].max())
        assert longest > 2 * tile, (longest, tile)
        if L == 40:  # the tail's tiles span more ids x labels than the LDS table holds
            assert atomic_tiles > 0 and tile * L > int(catstats.native.kernels().fmlx_ccsr_lds_ints())
        assert lds_tiles + atomic_tiles == -(-int(X.indices.numel()) // tile)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_no_entries_and_no_rows(dtype):
    _need_gpu()
    dev = torch.device("cuda")
    empty = lambda n: SparseColumn(torch.zeros(n + 1, dtype=torch.int64, device=dev),  # noqa: E731
                                   torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=dtype, device=dev), 7)
    c, v, t, nl = catstats.value_label_counts_csr(empty(5), torch.tensor([0, 1, 1, 0, 1], device=dev), 2).numpy()
    assert np.array_equal(c, np.arange(8)) and not v.any() and np.array_equal(t, [[2, 3]] * 7) and np.array_equal(nl, [2, 3])
    c, v, t, nl = catstats.value_label_counts_csr(empty(0), torch.zeros(0, dtype=torch.int64, device=dev), 2).numpy()
    assert not c.any() and v.size == 0 and t.shape == (0, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_index_is_skipped_and_raises(dtype):
    _need_gpu()
    dev = torch.device("cuda")
    Xh = generated(N, D_SMALL, NAN_EVERY).slice(0, 300)
    li = label_index(300, 3)
    at = int(Xh.indptr[150])
    idx = Xh.indices.clone()
    idx[at] = D_SMALL  # one past the last column
    bad = SparseColumn(Xh.indptr, idx, Xh.values, D_SMALL)
    keep = torch.ones(idx.numel(), dtype=torch.bool)
    keep[at] = False
    ptr = Xh.indptr.clone()
    ptr[151:] -= 1
    rest = SparseColumn(ptr, Xh.indices[keep], Xh.values[keep], D_SMALL)  # the column without that entry
    rc = catstats.value_label_counts_csr(bad.to(device=dev, dtype=dtype), li.cuda(), 3, check=False)
    assert_tables_equal(rc, catstats.torch_value_label_counts_csr(rest, li, 3).numpy())
    with pytest.raises(ValueError):
        kk.check_csr_error(rc)
    with pytest.raises(ValueError):
        catstats.value_label_counts_csr(bad.to(device=dev, dtype=dtype), li.cuda(), 3)
    # the device is intact: the good column goes through
    good = catstats.value_label_counts_csr(Xh.to(device=dev, dtype=dtype), li.cuda(), 3)
    assert_tables_equal(good, catstats.torch_value_label_counts_csr(Xh, li, 3).numpy())


# ------------------------------------------------------------------------------------------------
# stage level
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_runs():
    """The stages on the host on the densified 12,000 x 5,000 table, and on the GPU through the CSR
    route (SparseColumn.to_dense raising)."""
    from flink_ml_amd.config import dtype_policy

    X, y = generated(N, D_SMALL), class_labels(N)
    old, old_dense = fo.COLSTATS_CSR_ROUTE, SparseColumn.to_dense
    try:
        with on_cpu():
            fo.COLSTATS_CSR_ROUTE = "0"
            ref = run_stages(X.to_dense(torch.float64), y)
        fo.COLSTATS_CSR_ROUTE = "1"

        def no_dense(self, *a, **k):
            raise AssertionError("SparseColumn.to_dense called")

        SparseColumn.to_dense = no_dense
        with dtype_policy("fp64"):
            got = run_stages(X, y, ref["fpr"])
    finally:
        fo.COLSTATS_CSR_ROUTE, SparseColumn.to_dense = old, old_dense
    return ref, got


def test_stages_through_csr_route_match_host():
    _need_gpu()
    ref, got = stage_runs()
    assert got["dof"] == ref["dof"]
    for k in ("stat", "p"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        print("ChiSqTest %s: largest difference %.3e" % (k, float(np.abs(g - r).max())))
        assert np.allclose(g, r, rtol=1e-12, atol=1e-11)
    assert got["ufs"] == ref["ufs"] and 0 < len(ref["ufs"]) < D_SMALL
    th_g, pi_g, lab_g = got["model"].model_data_rows()[0]
    th_r, pi_r, lab_r = ref["model"].model_data_rows()[0]
    assert np.array_equal(lab_g.values, lab_r.values) and np.array_equal(pi_g.values, pi_r.values)
    for mg, mr in zip(th_g, th_r):
        for a, b in zip(mg, mr):
            assert list(a.keys()) == list(b.keys())
            assert np.allclose(list(a.values()), list(b.values()), rtol=1e-12, atol=0.0)


def host_scores():
    """Host scores of the training table under the host model: (scores [n, L], Σ|terms| [n, L])."""
    ref, _ = stage_runs()
    X = generated(N, D_SMALL)
    with on_cpu():
        vals, offs, table, pi, _ = ref["model"]._model_state()
        Xd = X.to_dense(torch.float64)
        cols = torch.empty((N, D_SMALL), dtype=torch.int64)
        for j in range(D_SMALL):
            cols[:, j] = offs[j] + torch.searchsorted(vals[j], Xd[:, j].contiguous())
        sc, ab = [], []
        for s in range(0, N, 1000):
            g = table[:, cols[s:s + 1000]]
            sc.append(g.sum(dim=2).t() + pi[None, :])
            ab.append(g.abs().sum(dim=2).t() + pi.abs()[None, :])
    return torch.cat(sc).numpy(), torch.cat(ab).numpy()


def test_naive_bayes_predicts_training_table_like_host():
    """The two routes sum a row's terms in different orders: predictions must agree wherever the
    host's top-two margin exceeds 2·(D + 2·m_i + 2)·2^-53·3·max_l Σ|terms| (m_i: the row's stored
    entries), which at most 0.1 % of the rows may fail to."""
    _need_gpu()
    ref, got = stage_runs()
    X = generated(N, D_SMALL)
    scores, absum = host_scores()
    top = np.sort(scores, axis=1)
    margin = top[:, -1] - top[:, -2]
    m = (X.indptr[1:] - X.indptr[:-1]).numpy()
    bound = 2.0 * (D_SMALL + 2 * m + 2) * 2.0 ** -53 * 3 * absum.max(axis=1)
    decided = margin > bound
    print("smallest margin %.3e, largest bound %.3e, rows under the bound %d" % (margin.min(), bound.max(), int((~decided).sum())))
    assert (~decided).mean() <= 0.001
    assert np.array_equal(got["pred"][decided], ref["pred"][decided])
    assert len(set(ref["pred"].tolist())) > 1


def test_unseen_value_names_the_dense_routes_feature(monkeypatch):
    _need_gpu()
    _, got = stage_runs()
    X = generated(N, D_SMALL).slice(0, 500)
    vals = X.values.clone()
    present = torch.unique(X.indices)
    lowest = int(present[40])
    for c in (int(present[300]), lowest, int(present[900])):
        vals[int(torch.nonzero(X.indices == c)[0])] = 17.0
    t = Table({"features": SparseColumn(X.indptr, X.indices, vals, D_SMALL)})
    msgs = []
    for route in ("1", "0"):
        monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", route)
        with pytest.raises(RuntimeError) as ei:
            got["model"].transform(t)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] == "Feature %d of the input contains a value unseen in training." % lowest


def _two_rank_worker(rank, world):
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import ChiSqTest
    from flink_ml_amd.ops import catstats
    from flink_ml_amd.ops import features as fo

    fo.COLSTATS_CSR_ROUTE = "1"  # (this process is the rank's own)
    X, y = generated(N, D_SMALL), class_labels(N)
    lo, hi = (0, N // 2) if rank == 0 else (N // 2, N)
    Xr, yr = X.slice(lo, hi), y[lo:hi]
    dev = torch.device("cuda")
    rc = catstats.global_value_label_counts_csr(Xr.to(device=dev), yr.long().to(dev), 3)
    with dtype_policy("fp64"):
        chi = ChiSqTest().compute(Table({"features": Xr, "label": yr}))
    return rc.numpy(), chi


def test_two_ranks_sharing_the_gpu_equal_one_rank():
    _need_gpu()
    _, got = stage_runs()
    X, y = generated(N, D_SMALL), class_labels(N)
    one = catstats.value_label_counts_csr(X.to(device=torch.device("cuda")), y.long().cuda(), 3).numpy()
    for tabs, chi in run_spmd(_two_rank_worker, 2, env={"FMLX_DEVICE": "cuda:0", "FMLX_XGMI": "0"}, timeout=300):
        for a, b in zip(tabs, one):
            assert np.array_equal(a, b)
        assert tuple(chi) == (got["p"], got["dof"], got["stat"])


def test_chisq_bounded_memory_at_wide_columns(monkeypatch):
    """2,000 x 2^20 with 3 labels, device-resident fp32, the knob at auto: densified it is 16.8 GB in
    fp64; the test stays under n·D·4 / 16 = 500 MiB above its inputs."""
    _need_gpu()
    from flink_ml_amd.models import ChiSqTest
    from flink_ml_amd.ops import native

    monkeypatch.setattr(fo, "COLSTATS_CSR_ROUTE", "auto")
    n, D, L = 2000, D_WIDE, 32
    dev = torch.device("cuda")
    native.kernels()
    g = torch.Generator().manual_seed(3)
    start = torch.randint(0, D, (n, 1), generator=g)
    stride = torch.randint(0, D // 2, (n, 1), generator=g) * 2 + 1  # odd: the L columns of a row are distinct
    idx = ((start + torch.arange(L)[None, :] * stride) % D).to(torch.int32).reshape(-1)
    val = torch.randint(1, 5, (n * L,), generator=g).float()
    Xh = SparseColumn(torch.arange(0, n * L + 1, L, dtype=torch.int64), idx, val, D)
    yh = (torch.arange(n) % 3).double()
    t = Table({"features": Xh.to(device=dev, dtype=torch.float32), "label": yh.to(dev)})
    limit = n * D * 4 // 16
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = ChiSqTest().transform(t)
    peak = torch.cuda.max_memory_allocated(dev) - base
    print("ChiSqTest.transform: peak above the inputs %.1f MiB" % (peak / 2 ** 20))
    assert peak < limit
    dof = out[0].get_list("degreesOfFreedom")[0]
    colfirst = catstats.torch_value_label_counts_csr(Xh, yh.long(), 3).numpy()[0]
    assert len(dof) == D and dof == ((np.diff(colfirst) - 1) * 2).tolist()
