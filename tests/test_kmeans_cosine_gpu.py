"""KMeans under cosine distance on the wide MFMA assigns (ops/csrc/kmeans_wide.hip, kmeans_wide_f32.hip,
kmeans_wide_f64.hip, the cosine instantiations) against fp64 on the operands as the kernels see them:
d = 1 − x·c/‖x‖/‖c‖, first minimum, NaN never wins, −1 for a row without a winner."""
import contextlib

import numpy as np
import pytest
import torch

from flink_ml_amd.ops import kmeans as kk

pytestmark = pytest.mark.gpu

# dtype → rows' dtype, accumulation dtype, the predicate, bits of the accumulator's mantissa,
# tie offsets (the existing tie tests'), pitch padding, (rtol, atol) of the round's sums
DT = {"bf16": (torch.bfloat16, torch.float32, kk.mfma_wide_ok, 23, (1, 32, 64, 128), 8, (1e-5, 1e-3)),
      "fp32": (torch.float32, torch.float32, kk.mfma_wide_f32_ok, 23, (1, 32, 64, 128), 4, (1e-5, 1e-3)),
      "fp64": (torch.float64, torch.float64, kk.mfma_wide_f64_ok, 52, (1, 4, 16, 64), 2, (1e-12, 4e-12))}
SHAPES = [("bf16", D) for D in (64, 72, 264, 1000, 4096)] + [("fp32", D) for D in (132, 160, 1000, 4096)] + [
    ("fp64", D) for D in (16, 18, 130, 1000)]


@pytest.fixture(autouse=True)
def _wide_kernel_at_every_supported_shape(monkeypatch):
    monkeypatch.setattr(kk, "WIDE", "force")


def _data(dt, n, D, k, seed=0):
    """Rows s_i·(c_(i mod k) + 0.05·noise) with 1/2 <= s_i <= 2; the centroids handed to the kernel are
    the c_j scaled by factors spanning two decades (rounded as the kernel reads them)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(seed * 100003 + D * 31 + k)
    C0 = torch.randn((k, D), generator=g, dtype=torch.float64)
    s = 2.0 ** (2 * torch.rand((n, 1), generator=g, dtype=torch.float64) - 1)
    X = (s * (C0[torch.arange(n) % k] + 0.05 * torch.randn((n, D), generator=g, dtype=torch.float64))).to(DT[dt][0])
    C = C0 * 10.0 ** (2 * torch.rand((k, 1), generator=g, dtype=torch.float64) - 1)
    return X, C.to(DT[dt][0]).double()


def _ref(X, C):
    X = X.double()
    d = 1.0 - X @ C.T / torch.linalg.vector_norm(X, dim=1)[:, None] / torch.linalg.vector_norm(C, dim=1)[None, :]
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return d, torch.where((d < float("inf")).any(1), torch.argmin(d, 1), -1)


def _assign(dt, X, C, metric="cosine"):
    cb = kk.CentroidBuffers(C.shape[0], C.shape[1], torch.device("cuda"), DT[dt][1])
    cb.set(C)
    assert not kk.WIDE or DT[dt][2](X, metric)
    return kk.assign(X, cb, metric).cpu().long()


@pytest.mark.parametrize("k", [5, 33, 129, 300])
@pytest.mark.parametrize("dt,D,n", [(dt, D, 300) for dt, D in SHAPES] + [(dt, 1000, 1) for dt in DT])
def test_exact_labels_on_separated_data(dt, D, n, k):
    X, C = _data(dt, n, D, k)
    d, ref = _ref(X, C)
    if k > 1:
        two = torch.topk(d, 2, dim=1, largest=False).values
        assert float((two[:, 1] - two[:, 0]).min()) > max(0.05, 100 * D * 2.0 ** -DT[dt][3])
    if n > 1:  # a euclidean kernel does not pass
        assert bool((kk.torch_assign(X, C, "euclidean") != ref).any())
    assert torch.equal(_assign(dt, X.cuda(), C), ref)


@pytest.mark.parametrize("j", [0, 37])
@pytest.mark.parametrize("dt,D", [("bf16", 264), ("fp32", 132), ("fp64", 130)])
def test_equal_keys_take_the_lowest_index(dt, D, j):
    """Copies of one centroid, some scaled by a power of two (dot and norm scale exactly: equal keys)."""
    X, C = _data(dt, 300, D, 200)
    for o, e in zip(DT[dt][4], (0, 1, -2, 3)):
        C[j + o] = C[j] * 2.0 ** e
    g = torch.Generator().manual_seed(j)
    X[:] = (C[j] * (1 + 0.05 * torch.randn(X.shape, generator=g, dtype=torch.float64))).to(X.dtype)
    assert bool((_assign(dt, X.cuda(), C) == j).all())


@pytest.mark.parametrize("dt,D", [("bf16", 72), ("fp32", 160), ("fp64", 18)])
def test_degenerate_rows_and_centroids(dt, D, monkeypatch):
    X, C = _data(dt, 300, D, 5)
    C[1] = 0.0
    C[2, D // 2] = float("nan")
    X[3] = 0.0
    X[7, D - 1] = float("nan")
    X[11, 0] = float("inf")
    lab = _assign(dt, X.cuda(), C)
    assert lab[[3, 7, 11]].tolist() == [-1, -1, -1] and int(lab.max()) < 5
    assert not bool(((lab == 1) | (lab == 2)).any()) and torch.equal(lab, _ref(X, C)[1])
    monkeypatch.setattr(kk, "WIDE", False)
    assert torch.equal(lab, _assign(dt, X.cuda(), C))  # the generic route


@pytest.mark.parametrize("dt", list(DT))
def test_unseparated_data_within_the_accumulation_bound(dt):
    g = torch.Generator().manual_seed(4)
    X = torch.randn((3000, 1000), generator=g, dtype=torch.float64).to(DT[dt][0])
    C = torch.randn((257, 1000), generator=g, dtype=torch.float64)
    C = (C * 10.0 ** (2 * torch.rand((257, 1), generator=g, dtype=torch.float64) - 1)).to(DT[dt][0]).double()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tol = 1000 * 2.0 ** -DT[dt][3]
    d, ref = _ref(X, C)
    shaken = torch.argmin(d + tol * (2 * torch.rand(d.shape, generator=g, dtype=torch.float64) - 1), 1)
    assert (shaken != ref).double().mean() <= 0.01  # the cap holds for the reference under that perturbation
    lab = _assign(dt, X.cuda(), C)
    excess = d.gather(1, lab[:, None]).squeeze(1) - d.gather(1, ref[:, None]).squeeze(1)
    print("labels differ %.6f, largest excess %.3g (bound %.3g)" % (float((lab != ref).double().mean()),
                                                                     float(excess.max()), tol))
    assert torch.all((lab == ref) | (excess <= tol)) and (lab != ref).double().mean() <= 0.01


@pytest.mark.parametrize("dt,D", [("bf16", 72), ("bf16", 1000), ("fp32", 132), ("fp32", 1000), ("fp64", 18),
                                  ("fp64", 1000)])
def test_rows_inside_a_wider_buffer(dt, D):
    X, C = _data(dt, 300, D, 33)
    buf = torch.full((300, D + DT[dt][5]), float("nan"), dtype=X.dtype, device="cuda")
    buf[:, :D] = X.cuda()
    assert buf[:, :D].stride(0) != D
    assert torch.equal(_assign(dt, buf[:, :D], C), _assign(dt, X.cuda(), C))


@pytest.mark.parametrize("dt,D", [(dt, D) for dt in DT for D in (520, 1032, 4096)] + [("bf16", 264)])
def test_round_sums_counts_reproducible_and_graph_replay(dt, D):
    from flink_ml_amd.utils import graphs

    n, k = 300, 5
    X, C = _data(dt, n, D, k)
    Xd = X.cuda()

    def fresh(metric="cosine"):
        cb = kk.CentroidBuffers(k, D, Xd.device, DT[dt][1])
        cb.set(C)
        rnd = kk.KMeansRound(Xd, k, metric)
        assert [rnd.wide, rnd.wide32, rnd.wide64] == [dt == "bf16" and not rnd.fast, dt == "fp32", dt == "fp64"]
        return cb, rnd

    cb, rnd = fresh()
    got = rnd.run(cb).clone()
    lab = rnd.labels.cpu().long()
    assert torch.equal(lab, _ref(X, C)[1])
    sums = torch.zeros((k, D), dtype=torch.float64).index_add_(0, lab, X.double())
    rtol, atol = DT[dt][6]
    assert torch.allclose(got[: k * D].cpu().double().reshape(k, D), sums, rtol=rtol, atol=atol)
    assert torch.equal(got[k * D:].cpu().double(), torch.bincount(lab, minlength=k).double())
    assert torch.equal(rnd.run(cb), got)  # bitwise
    for _ in range(3):
        rnd.finalize(cb, rnd.run(cb))
    cb2, rnd2 = fresh()
    gr = graphs.capture(lambda: rnd2.finalize(cb2, rnd2.run(cb2)), Xd.device)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cb2.cent, cb.cent) and torch.equal(cb2.Cb, cb.Cb) and torch.equal(rnd2.labels, rnd.labels)
    if D == 1032:  # the gather-sums serve every metric
        cb3, rnd3 = fresh("manhattan")
        want = kk.torch_round_payload(X, cb3.cent.cpu(), "manhattan")
        assert torch.allclose(rnd3.run(cb3).cpu().double(), want, rtol=rtol, atol=atol)


@pytest.mark.parametrize("dt,tol", [("fp32", 1e-5), ("bf16", 2.0 ** -8)])
def test_fit_and_transform_on_a_wide_column(dt, tol, monkeypatch):
    from flink_ml_amd import Table, config
    from flink_ml_amd.models.kmeans import KMeans, kmeans_lloyd, sample_rows

    X, C = _data(dt, 400, 1032, 4)
    t = Table({"features": X.cuda()})
    est = KMeans().set_distance_measure("cosine").set_k(4).set_max_iter(5).set_seed(6)
    init = sample_rows(X.cuda(), 4, est.get_seed())
    assert sorted(kk.torch_assign(torch.as_tensor(init), C, "cosine").tolist()) == [0, 1, 2, 3]  # one per cluster
    with config.dtype_policy("fp32") if dt == "fp32" else contextlib.nullcontext():
        model = est.fit(t)
        ref_c, _ = kmeans_lloyd(X.double(), init, 5, "cosine")
        assert np.allclose(model.centroids(), ref_c, rtol=tol, atol=tol)
        pred = model.transform(t)[0].column("prediction").cpu()
        assert torch.equal(pred, kk.torch_assign(X, torch.as_tensor(ref_c), "cosine"))
        monkeypatch.setattr(kk, "WIDE", False)
        with pytest.raises(RuntimeError, match=r"fmlx_kmeans_chunk_sum failed with error -3$"):
            est.fit(t)
