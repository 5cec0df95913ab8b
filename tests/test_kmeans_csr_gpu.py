"""KMeans on CSR feature columns (csrc/kmeans_csr.hip) against the fp64 host references of
ops/kmeans.py: assign, the deterministic column-sum round, finalize, the fit (eager and hipGraph,
one and two ranks), the stage routing, bounded memory and bad indices.

Input: rows of 1-64 draws (every 97th row empty); columns min(zipf(1.1) - 1, D - 1) plus
max(1, L // 2) uniform ones, unique per row; values N(1.5, 1); n = 4,000, D = 2^20. Centroids are
one fp64 Lloyd step from the first k non-empty rows."""
import functools

import numpy as np
import pytest
import torch

from flink_ml_amd.ops import kmeans as kk
from flink_ml_amd.table import SparseColumn
from tests.spmd import run_spmd

pytestmark = pytest.mark.gpu

N, D_WIDE, D_SMALL = 4000, 1 << 20, 5000
METRICS = ["euclidean", "manhattan", "cosine"]


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
def host_column(n=N, D=D_WIDE, seed=5) -> SparseColumn:
    ptr, idx, val = make_input(n, D, seed)
    return SparseColumn(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(val), D)


def first_rows(X: SparseColumn, k: int) -> torch.Tensor:
    """The first k non-empty rows, dense fp64 [k, D]."""
    lens = X.indptr[1:] - X.indptr[:-1]
    rows = torch.nonzero(lens > 0).reshape(-1)[:k]
    C = torch.zeros(k, X.size, dtype=torch.float64)
    for i, r in enumerate(rows.tolist()):
        s, e = int(X.indptr[r]), int(X.indptr[r + 1])
        C[i, X.indices[s:e].long()] = X.values[s:e].double()
    return C


@functools.lru_cache(maxsize=None)
def centroids(D: int, k: int) -> torch.Tensor:
    X = host_column(N, D)
    C, _ = kk.torch_finalize(kk.torch_round_payload_csr(X, first_rows(X, k), "euclidean"), k, D)
    return C


@functools.lru_cache(maxsize=None)
def ref_dist(D: int, k: int, metric: str) -> torch.Tensor:
    return kk.torch_dist_csr(host_column(N, D), centroids(D, k), metric)


_BUFFERS = {}


def buffers(D, k, dtype):
    key = (D, k, dtype)
    if key not in _BUFFERS:
        _BUFFERS.clear()  # one image at a time (2^20 x 128 fp64 is 1 GiB)
        cb = kk.SparseCentroidBuffers(k, D, torch.device("cuda"), dtype)
        cb.set(centroids(D, k))
        _BUFFERS[key] = cb
    return _BUFFERS[key]


def device_column(X: SparseColumn, dtype) -> SparseColumn:
    return X.to(device=torch.device("cuda"), dtype=dtype)


def check_labels(got: torch.Tensor, d: torch.Tensor, metric: str, tol: float):
    """``got`` against the fp64 distances ``d`` [n, k]: a row may differ from the argmin only when
    its distance is within tol·(1 + |best|) of the best (which bounds the best / second-best gap);
    at most 1 % of the rows may; a row whose distances are all NaN gets -1 (0 for euclidean)."""
    got = got.cpu().long()
    nan_row = torch.isnan(d).all(1)
    dd = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    best, ref = dd.min(1)
    ref = torch.where(nan_row, torch.full_like(ref, 0 if metric == "euclidean" else -1), ref)
    diff = got != ref
    assert not bool((diff & nan_row).any())
    assert int(got.min()) >= -1 and int(got.max()) < d.shape[1]
    assert not bool((got[~nan_row] < 0).any())
    if bool(diff.any()):
        rows = torch.nonzero(diff).reshape(-1)
        gap = dd[rows, got[rows]] - best[rows]
        print("differing rows: %d, largest gap %.3e" % (rows.numel(), float(gap.max())))
        assert bool((gap <= tol * (1 + best[rows].abs())).all()), float(gap.max())
    assert float(diff.double().mean()) <= 0.01


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("D,k", [(D_WIDE, 10), (D_WIDE, 70), (D_SMALL, 257)])
def test_assign_csr_matches_fp64_reference(D, k, dtype, metric):
    """One lane group (k = 10), two accumulators (70) and several (257)."""
    _need_gpu()
    cb = buffers(D, k, dtype)
    got = kk.assign_csr(device_column(host_column(N, D), dtype), cb, metric)
    kk.check_csr_error(cb)
    check_labels(got, ref_dist(D, k, metric), metric, 1e-4 if dtype == torch.float32 else 1e-9)


@pytest.mark.parametrize("metric", METRICS)
def test_assign_csr_equals_dense_generic_kernel(metric):
    """fp64 labels equal ``assign`` on the densified matrix, the -1 of empty rows under cosine
    included."""
    _need_gpu()
    n, D, k = 3000, D_SMALL, 10
    X = host_column(n, D)
    C = kk.torch_finalize(kk.torch_round_payload_csr(X, first_rows(X, k), "euclidean"), k, D)[0]
    dev = torch.device("cuda")
    cbs = kk.SparseCentroidBuffers(k, D, dev, torch.float64)
    cbs.set(C)
    cbd = kk.CentroidBuffers(k, D, dev, torch.float64)
    cbd.set(C)
    got = kk.assign_csr(device_column(X, torch.float64), cbs, metric)
    want = kk.assign(X.to_dense(torch.float64, dev), cbd, metric)
    assert torch.equal(got, want)
    empty = (X.indptr[1:] == X.indptr[:-1])
    assert int(empty.sum()) >= n // 97
    if metric == "cosine":
        assert bool((got.cpu()[empty] == -1).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("seg", [256, None])
def test_round_payload_deterministic_and_matches_torch(seg, dtype, monkeypatch):
    """Column 0 (most rows hold it) is summed in many segments at CSR_COL_SEGMENT = 256."""
    _need_gpu()
    if seg is not None:
        monkeypatch.setattr(kk, "CSR_COL_SEGMENT", seg)
    D, k = D_WIDE, 10
    Xh = host_column(N, D)
    col0 = int((Xh.indices == 0).sum())
    assert col0 > 3000  # > 11 segments of 256
    C = centroids(D, k).clone()
    C[k - 1] = 50.0  # never the closest: an empty cluster
    dev = torch.device("cuda")
    cb = kk.SparseCentroidBuffers(k, D, dev, dtype)
    cb.set(C)
    X = device_column(Xh, dtype)
    rnd = kk.SparseKMeansRound(X, k, "euclidean")
    assert rnd.seg == (seg or kk.CSR_COL_SEGMENT)
    if seg:
        assert rnd.nlong >= 1 and rnd.nsegs >= -(-col0 // 256) >= 12
    else:
        assert rnd.nlong == 0  # every column within one default segment
    kp = cb.kp

    def check(C_now):
        p1 = rnd.run(cb).clone()
        p2 = rnd.run(cb).clone()
        assert torch.equal(p1.view(torch.uint8), p2.view(torch.uint8))  # bit-identical
        lab = rnd.labels.cpu().long()
        got = p1.cpu().double()
        assert torch.equal(got[D * kp:], torch.bincount(lab, minlength=k).double())
        ref = kk.torch_round_payload_csr(Xh, C_now, "euclidean", labels=lab)
        img = got[: D * kp].reshape(D, kp)
        assert not bool(img[:, k:].any())  # padding lanes zero
        rtol, atol = (1e-5, 1e-3) if dtype == torch.float32 else (1e-12, 0.0)
        sums = img[:, :k].t()
        assert torch.allclose(sums, ref[: k * D].reshape(k, D), rtol=rtol, atol=atol)
        used = torch.zeros(D, dtype=torch.bool)
        used[Xh.indices.long()] = True
        assert not bool(sums[:, ~used].any())  # columns without an entry: exact zeros
        return p1, lab, ref

    p1, lab, ref = check(C)
    assert int((lab == k - 1).sum()) == 0
    rnd.finalize(cb, p1)
    kk.check_csr_error(cb, rnd)
    cent, w = cb.cent.cpu().double(), cb.weights.cpu()
    assert bool(torch.isnan(cent[k - 1]).all()) and float(w[k - 1]) == 0.0
    want_c, want_w = kk.torch_finalize(ref, k, D)
    assert torch.equal(w, want_w)
    assert torch.allclose(cent[: k - 1], want_c[: k - 1], rtol=1e-5 if dtype == torch.float32 else 1e-12,
                          atol=1e-5 if dtype == torch.float32 else 1e-12)
    nr = cb.norms.cpu().double()
    c = cent[: k - 1]
    rt = 1e-5 if dtype == torch.float32 else 1e-12
    assert torch.allclose(nr[1, : k - 1], (c * c).sum(1), rtol=rt) and torch.allclose(nr[2, : k - 1], c.abs().sum(1), rtol=rt)
    assert torch.allclose(nr[0, : k - 1], (c * c).sum(1).sqrt(), rtol=rt)
    # the payload buffer is reused: a second round after finalize rewrites every column, the ones
    # without an entry as zeros
    rnd.payload.fill_(123.0)
    check(cent)


def _fit_input(k):
    Xh = host_column(N, D_WIDE)
    return Xh, first_rows(Xh, k).numpy()


def _host_lloyd(Xh, init, rounds, metric="euclidean"):
    k, D = init.shape
    C = torch.as_tensor(init, dtype=torch.float64)
    for _ in range(rounds):
        d = kk.torch_dist_csr(Xh, C, metric)
        two = torch.topk(torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d), 2, dim=1, largest=False).values
        # no tie can hide a failure: every row's best / second-best gap is far above fp64 rounding
        assert bool((two[:, 1] - two[:, 0] > 1e-9 * (1 + two[:, 0].abs())).all())
        C, w = kk.torch_finalize(kk.torch_round_payload_csr(Xh, C, metric), k, D)
    return C, w


def test_fit_fp64_matches_host_lloyd_eager_and_graph(monkeypatch):
    _need_gpu()
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models.kmeans import kmeans_lloyd

    k, rounds = 7, 5
    Xh, init = _fit_input(k)
    C_ref, w_ref = _host_lloyd(Xh, init, rounds)
    with dtype_policy("fp64"):
        X = device_column(Xh, torch.float64)
        monkeypatch.setenv("FMLX_HIPGRAPH", "0")
        c0, w0 = kmeans_lloyd(X, init, rounds, "euclidean")
        monkeypatch.setenv("FMLX_HIPGRAPH", "1")
        c1, w1 = kmeans_lloyd(X, init, rounds, "euclidean")
    assert c0.tobytes() == c1.tobytes() and w0.tobytes() == w1.tobytes()
    assert np.array_equal(w0, w_ref.numpy())
    assert np.allclose(c0, C_ref.numpy(), rtol=1e-9, atol=0.0, equal_nan=True)
    assert not np.isnan(c0).any()


def _two_rank_worker(rank, world, k, rounds):
    import torch

    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models.kmeans import kmeans_lloyd

    Xh, init = _fit_input(k)
    half = N // 2
    part = Xh.slice(0, half) if rank == 0 else Xh.slice(half, N)
    with dtype_policy("fp64"):
        c, w = kmeans_lloyd(part.to(device=torch.device("cuda:0"), dtype=torch.float64), init, rounds, "euclidean")
    return c, w


def test_fit_two_ranks_equals_one_rank():
    _need_gpu()
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models.kmeans import kmeans_lloyd

    k, rounds = 7, 5
    Xh, init = _fit_input(k)
    with dtype_policy("fp64"):
        c1, w1 = kmeans_lloyd(device_column(Xh, torch.float64), init, rounds, "euclidean")
    res = run_spmd(_two_rank_worker, 2, k, rounds, env={"FMLX_DEVICE": "cuda:0", "FMLX_XGMI": "0"}, timeout=300)
    for c, w in res:
        assert np.array_equal(w, w1)
        assert np.allclose(c, c1, rtol=1e-9, atol=0.0)
    assert res[0][0].tobytes() == res[1][0].tobytes()


def test_fit_bounded_memory_at_hashingtf_width():
    """8,192 x 262,144 (HashingTF's default width): densified it is 8.6 GB in fp32; the CSR fit
    stays under 1 GiB above its inputs."""
    _need_gpu()
    from flink_ml_amd.models.kmeans import kmeans_lloyd
    from flink_ml_amd.ops import native

    n, D, k, L = 8192, 262144, 10, 32
    dev = torch.device("cuda")
    native.kernels()
    g = torch.Generator().manual_seed(3)
    start = torch.randint(0, D, (n, 1), generator=g)
    stride = torch.randint(0, D // 2, (n, 1), generator=g) * 2 + 1  # odd: the L columns of a row are distinct
    idx = ((start + torch.arange(L)[None, :] * stride) % D).to(torch.int32).reshape(-1)
    val = torch.randn(n * L, generator=g) + 1.5
    Xh = SparseColumn(torch.arange(0, n * L + 1, L, dtype=torch.int64), idx, val, D)
    init = first_rows(Xh, k).numpy()
    X = Xh.to(device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    c, w = kmeans_lloyd(X, init, 2, "euclidean")
    peak = torch.cuda.max_memory_allocated(dev) - base
    print("peak above the inputs: %.1f MiB" % (peak / 2 ** 20))
    assert peak < (1 << 30)
    assert c.shape == (k, D) and float(w.sum()) == n


def _docs():
    a = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta"]
    b = ["one", "two", "three", "four", "five", "six", "seven", "eight"]
    rs = np.random.RandomState(1)
    docs, group = [], []
    for i in range(60):
        vocab = a if i % 2 == 0 else b
        docs.append(" ".join(rs.choice(vocab, 6)))
        group.append(i % 2)
    return docs, group


def test_stage_text_pipeline_separates_vocabularies(monkeypatch, tmp_path):
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.models import HashingTF, KMeans, KMeansModel, Tokenizer

    monkeypatch.setattr(kk, "CSR_ROUTE", "1")
    docs, group = _docs()
    t = Table.from_rows([(d,) for d in docs], ["text"])
    t = Tokenizer().set_input_col("text").set_output_col("words").transform(t)[0]
    t = HashingTF().set_input_col("words").set_output_col("features").transform(t)[0]
    assert isinstance(t.column("features"), SparseColumn) and t.column("features").size == 262144
    calls = []
    real = kk.SparseKMeansRound
    monkeypatch.setattr(kk, "SparseKMeansRound", lambda *a: calls.append(1) or real(*a))
    model = KMeans().set_k(2).set_seed(STAGE_SEED).set_max_iter(5).fit(t)
    assert calls  # the CSR round ran
    pred = torch.as_tensor(model.transform(t)[0].column("prediction")).cpu().tolist()
    assert len({(g, p) for g, p in zip(group, pred)}) == 2 and len(set(pred)) == 2
    p = str(tmp_path / "km")
    model.save(p)
    loaded = KMeansModel.load(p)
    assert np.array_equal(loaded.centroids(), model.centroids())
    assert torch.as_tensor(loaded.transform(t)[0].column("prediction")).cpu().tolist() == pred


STAGE_SEED = 2


def test_models_predict_sparse_column_like_dense_route(monkeypatch):
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.models import KMeansModel, OnlineKMeansModel
    from flink_ml_amd.models.kmeans import kmeans_model_data_table

    n, D, k = 3000, D_SMALL, 10
    Xh = host_column(n, D)
    C = kk.torch_finalize(kk.torch_round_payload_csr(Xh, first_rows(Xh, k), "euclidean"), k, D)[0].numpy()
    md = kmeans_model_data_table(C, np.ones(k))
    t = Table({"features": Xh})
    from flink_ml_amd.config import dtype_policy

    with dtype_policy("fp64"):
        for cls in (KMeansModel, OnlineKMeansModel):
            out = {}
            for route in ("0", "1"):
                monkeypatch.setattr(kk, "CSR_ROUTE", route)
                model = cls().set_model_data(md)
                if cls is KMeansModel:
                    model.set_k(k)
                out[route] = torch.as_tensor(model.transform(t)[0].column("prediction")).cpu()
            assert out["0"].dtype == out["1"].dtype == torch.int64
            assert torch.equal(out["0"], out["1"]), cls.__name__


def test_bad_index_raises_value_error(monkeypatch):
    _need_gpu()
    from flink_ml_amd import Table
    from flink_ml_amd.models import KMeans, KMeansModel
    from flink_ml_amd.models.kmeans import kmeans_model_data_table

    monkeypatch.setattr(kk, "CSR_ROUTE", "1")
    n, D, k = 300, D_SMALL, 3
    Xh = host_column(n, D)
    idx = Xh.indices.clone()
    idx[int(Xh.indptr[150])] = D  # one past the last column
    bad = Table({"features": SparseColumn(Xh.indptr, idx, Xh.values, D)})
    with pytest.raises(ValueError):
        KMeans().set_k(k).set_max_iter(2).fit(bad)
    model = KMeansModel().set_model_data(kmeans_model_data_table(first_rows(Xh, k).numpy(), np.ones(k))).set_k(k)
    with pytest.raises(ValueError):
        model.transform(bad)
    # the device is intact: the same calls on the good column succeed
    good = Table({"features": Xh})
    assert len(model.transform(good)[0].column("prediction")) == n
    KMeans().set_k(k).set_max_iter(2).fit(good)
