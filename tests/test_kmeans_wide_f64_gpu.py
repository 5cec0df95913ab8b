"""KMeans on dense fp64 rows of 16 <= D <= 4096 (ops/csrc/kmeans_wide_f64.hip: the K-tiled fp64 MFMA
assign and the wide gather-sum) against plain torch fp64 on the CPU:
d = max(0, ‖x‖² + ‖c‖² − 2·x·c), argmin (first minimum, NaN keys never win)."""
import numpy as np
import pytest
import torch

from flink_ml_amd.ops import kmeans as kk

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _wide_kernel_at_every_supported_shape(monkeypatch):
    """``assign`` leaves some shapes to the routes that measured faster (``kk.wide64_route``);
    here every shape the kernel supports goes to it."""
    monkeypatch.setattr(kk, "WIDE", "force")


def _data(n, D, k, seed=0):
    """Rows clustered on k random centroids: a row's best / second-best key gap is >= 1.4·(1 + |best|)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(seed * 100003 + D * 31 + k)
    C = torch.randn((k, D), generator=g, dtype=torch.float64)
    X = C[torch.arange(n) % k] + 0.05 * torch.randn((n, D), generator=g, dtype=torch.float64)
    return X, C


def _dist(X, C):
    d = torch.clamp((X * X).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * X @ C.T, min=0.0)
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)


def _assign(X, C):
    cb = kk.CentroidBuffers(C.shape[0], C.shape[1], torch.device("cuda"), torch.float64)
    cb.set(C)
    assert kk.mfma_wide_f64_ok(X, "euclidean")
    return kk.assign(X, cb, "euclidean").cpu().long()


@pytest.mark.parametrize("k", [5, 17, 65, 130])
@pytest.mark.parametrize("n,D", [(300, 16), (300, 18), (300, 130), (300, 1000), (300, 1024), (300, 4096), (1, 1000)])
def test_exact_labels_on_separated_data(n, D, k):
    X, C = _data(n, D, k)
    assert torch.equal(_assign(X.cuda(), C), torch.argmin(_dist(X, C), 1))


@pytest.mark.parametrize("j", [0, 37])
def test_equal_keys_take_the_lowest_index(j):
    """Duplicates of one centroid across lane groups, accumulator elements, tiles and macro-tiles."""
    X, C = _data(300, 130, 200)
    for o in (1, 4, 16, 64):
        C[j + o] = C[j]
    g = torch.Generator().manual_seed(j)
    X[:] = C[j] + 0.05 * torch.randn(X.shape, generator=g, dtype=torch.float64)
    assert bool((_assign(X.cuda(), C) == j).all())


def test_nan_never_wins_and_no_label_past_k():
    X, C = _data(300, 130, 5)
    C[2] = float("nan")
    X[7, 100] = float("nan")
    lab = _assign(X.cuda(), C)
    assert torch.equal(lab, torch.argmin(_dist(X, C), 1))
    assert int(lab[7]) == 0 and not bool((lab == 2).any()) and int(lab.max()) < 5


def test_unseparated_data_within_the_near_tie_rule():
    """The reference against itself with the products in a permuted column order stays inside both
    conditions on this input: all 3000 labels equal, so the largest excess over the minimum is 0."""
    g = torch.Generator().manual_seed(4)
    X = torch.randn((3000, 1000), generator=g, dtype=torch.float64)
    C = torch.randn((257, 1000), generator=g, dtype=torch.float64)
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lab, d = _assign(X.cuda(), C), _dist(X, C)
    ref = torch.argmin(d, 1)
    dsel, dref = d.gather(1, lab[:, None]).squeeze(1), d.gather(1, ref[:, None]).squeeze(1)
    print("labels equal %.6f, largest excess %.3g" % (float((lab == ref).double().mean()), float((dsel - dref).max())))
    assert torch.all((lab == ref) | ((dsel - dref).abs() <= 1e-12 * (1 + dref.abs())))
    assert (lab == ref).double().mean() >= 0.999


@pytest.mark.parametrize("D", [130, 1000])
def test_rows_inside_a_wider_buffer(D):
    X, C = _data(300, D, 17)
    buf = torch.full((300, D + 2), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :D] = X.cuda()
    assert buf[:, :D].stride(0) == D + 2
    assert torch.equal(_assign(buf[:, :D], C), _assign(X.cuda(), C))
    odd = torch.zeros((300, D + 1), dtype=torch.float64, device="cuda")[:, :D]
    assert not kk.mfma_wide_f64_ok(odd, "euclidean")  # today's route


@pytest.mark.parametrize("D", [130, 1030, 4096])
def test_round_sums_counts_reproducible_and_graph_replay(D):
    from flink_ml_amd.utils import graphs

    n, k = 300, 5
    X, C = _data(n, D, k)
    Xd = X.cuda()

    def fresh():
        cb = kk.CentroidBuffers(k, D, Xd.device, torch.float64)
        cb.set(C)
        rnd = kk.KMeansRound(Xd, k, "euclidean")
        assert rnd.wide64 and not rnd.wide32 and not rnd.wide and not rnd.fast
        return cb, rnd

    cb, rnd = fresh()
    got = rnd.run(cb).clone()
    lab = rnd.labels.cpu().long()
    assert torch.equal(lab, torch.argmin(_dist(X, C), 1))
    sums = torch.zeros((k, D), dtype=torch.float64).index_add_(0, lab, X)
    # near-zero sums: each side's error is at most γ_60·Σ|x| <= 60·1.1e-16·(60·5) = 2e-12
    assert torch.allclose(got[: k * D].cpu().reshape(k, D), sums, rtol=1e-12, atol=4e-12)
    assert torch.equal(got[k * D:].cpu(), torch.bincount(lab, minlength=k).double())
    assert torch.equal(rnd.run(cb), got)  # bitwise
    for _ in range(3):
        rnd.finalize(cb, rnd.run(cb))
    cb2, rnd2 = fresh()
    gr = graphs.capture(lambda: rnd2.finalize(cb2, rnd2.run(cb2)), Xd.device)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cb2.cent, cb.cent) and torch.equal(rnd2.labels, rnd.labels)


def test_fit_and_transform_on_a_wide_fp64_column(monkeypatch):
    from flink_ml_amd import Table, config
    from flink_ml_amd.models.kmeans import KMeans, kmeans_lloyd, sample_rows

    X, C = _data(400, 1030, 4)
    t = Table({"features": X.cuda()})
    est = KMeans().set_k(4).set_max_iter(5).set_seed(6)  # a seed whose initial rows are one per cluster
    init = sample_rows(X.cuda(), 4, est.get_seed())
    assert sorted(kk.torch_assign(torch.as_tensor(init), C, "euclidean").tolist()) == [0, 1, 2, 3]
    with config.dtype_policy("fp64"):
        model = est.fit(t)
        ref_c, _ = kmeans_lloyd(X, init, 5, "euclidean")
        # separated data: the labels agree every round, only the summation order of 100 rows differs
        # (near-zero means: each side's error is at most γ_100·max|x| <= 1.1e-14·5 = 5.5e-14)
        assert np.allclose(model.centroids(), ref_c, rtol=1e-12, atol=2e-13)
        pred = model.transform(t)[0].column("prediction").cpu()
        assert torch.equal(pred, kk.torch_assign(X, torch.as_tensor(ref_c), "euclidean"))
        monkeypatch.setattr(kk, "WIDE", False)
        with pytest.raises(RuntimeError, match=r"fmlx_kmeans_chunk_sum failed with error -3$"):
            est.fit(t)
