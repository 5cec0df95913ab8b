"""KMeans under manhattan distance on the tiled assign (ops/csrc/kmeans_l1.hip) against fp64
``torch.cdist(p=1)`` on the operands as the kernel reads them (rows widened exactly, centroids rounded
to the buffer dtype): first strict minimum, NaN and inf never win, −1 for a row without a winner."""
import contextlib

import numpy as np
import pytest
import torch

from flink_ml_amd.ops import kmeans as kk
from flink_ml_amd.ops import native

pytestmark = pytest.mark.gpu

# dtype → rows' dtype, accumulation dtype, entry point, p (the accumulator's 2^-p), pitch padding,
# (rtol, atol) of the round's sums
DT = {"bf16": (torch.bfloat16, torch.float32, "fmlx_kmeans_assign_l1_bf16", 24, 8, (1e-5, 1e-3)),
      "fp32": (torch.float32, torch.float32, "fmlx_kmeans_assign_l1_f32", 24, 4, (1e-5, 1e-3)),
      "fp64": (torch.float64, torch.float64, "fmlx_kmeans_assign_l1_f64", 53, 2, (1e-12, 4e-12))}
SHAPES = [("fp32", D) for D in (4, 36, 132, 1000, 4096)] + [("bf16", D) for D in (8, 72, 264, 1000, 4096)] + [
    ("fp64", D) for D in (2, 18, 130, 1000)]
# copies of a centroid: in the same thread's tile (16), across the threads of a row in one wave (1)
# and in another wave (8), across macro-tiles (64 for fp64, 128)
TIE_OFFSETS = (1, 8, 16, 64, 128)


@pytest.fixture(autouse=True)
def _l1_kernel_at_every_supported_shape(monkeypatch):
    monkeypatch.setattr(kk, "L1", "force")


def _data(dt, n, D, k, seed=1):
    """Rows c_(i mod k) + 0.05·noise; the centroids handed to the kernel are the c_j, every odd one
    moved by 0.6·D along the first coordinate (far in L2, still nearest in L1 once D is large), rounded
    to the centroid buffer's dtype."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(seed * 100003 + D * 31 + k)
    C = torch.randn((k, D), generator=g, dtype=torch.float64)
    X = (C[torch.arange(n) % k] + 0.05 * torch.randn((n, D), generator=g, dtype=torch.float64)).to(DT[dt][0])
    C[1::2, 0] += 0.6 * D
    return X, C.to(DT[dt][1]).double()


def _ref(X, C):
    d = torch.cdist(X.double(), C, p=1)
    return d, kk._first_strict_min(d)


def _assign(dt, X, C):
    cb = kk.CentroidBuffers(C.shape[0], C.shape[1], torch.device("cuda"), DT[dt][1])
    cb.set(C)
    assert not kk.L1 or kk.l1_ok(X, "manhattan")
    return kk.assign(X, cb, "manhattan").cpu().long()


@pytest.mark.parametrize("k", [5, 33, 129, 300])
@pytest.mark.parametrize("dt,D,n", [(dt, D, 300) for dt, D in SHAPES] + [(dt, 1000, 1) for dt in DT])
def test_exact_labels_on_separated_data(dt, D, n, k):
    X, C = _data(dt, n, D, k)
    d, ref = _ref(X, C)
    two = torch.topk(d, 2, dim=1, largest=False).values
    assert bool((two[:, 1] - two[:, 0] > 100 * D * 2.0 ** -DT[dt][3] * two[:, 0]).all())
    if n > 1:  # a euclidean kernel does not pass
        assert bool((kk.torch_assign(X, C, "euclidean") != ref).any())
    assert torch.equal(_assign(dt, X.cuda(), C), ref)


@pytest.mark.parametrize("j", [0, 37])
@pytest.mark.parametrize("dt,D", [("bf16", 264), ("fp32", 132), ("fp64", 130)])
def test_equal_keys_take_the_lowest_index(dt, D, j):
    X, C = _data(dt, 300, D, 200)
    for o in TIE_OFFSETS:
        C[j + o] = C[j]
    g = torch.Generator().manual_seed(j)
    X[:] = (C[j] + 0.05 * torch.randn(X.shape, generator=g, dtype=torch.float64)).to(X.dtype)
    assert bool((_assign(dt, X.cuda(), C) == j).all())


@pytest.mark.parametrize("dt,D", [("bf16", 72), ("fp32", 36), ("fp64", 18)])
def test_degenerate_rows_and_centroids(dt, D, monkeypatch):
    X, C = _data(dt, 300, D, 5)
    C[1, D - 1] = float("inf")
    C[2, D // 2] = float("nan")
    X[3] = 0.0
    X[7, D - 1] = float("nan")
    X[11, 0] = float("inf")
    lab = _assign(dt, X.cuda(), C)
    assert lab[[7, 11]].tolist() == [-1, -1] and 0 <= int(lab[3]) < 5 and int(lab.max()) < 5
    assert not bool(((lab == 1) | (lab == 2)).any()) and torch.equal(lab, _ref(X, C)[1])
    monkeypatch.setattr(kk, "L1", False)
    assert torch.equal(lab, _assign(dt, X.cuda(), C))  # the generic route


@pytest.mark.parametrize("dt", list(DT))
def test_unseparated_data_within_the_accumulation_bound(dt):
    """Σ of D non-negative terms, each one rounded subtraction, in any order: a relative error of at
    most (D + 2)·2^-p per key to first order, so a label other than the reference's costs at most twice
    that of its own distance."""
    g = torch.Generator().manual_seed(4)
    X = torch.randn((3000, 1000), generator=g, dtype=torch.float64).to(DT[dt][0])
    C = torch.randn((257, 1000), generator=g, dtype=torch.float64).to(DT[dt][1]).double()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rel = 2 * (1000 + 2) * 2.0 ** -DT[dt][3]
    d, ref = _ref(X, C)
    shaken = torch.argmin(d * (1 + rel * (2 * torch.rand(d.shape, generator=g, dtype=torch.float64) - 1)), 1)
    assert (shaken != ref).double().mean() <= 0.01  # the cap holds for the reference under that perturbation
    lab = _assign(dt, X.cuda(), C)
    dl, dr = d.gather(1, lab[:, None]).squeeze(1), d.gather(1, ref[:, None]).squeeze(1)
    print("labels differ %.6f, largest excess %.3g of the bound" % (float((lab != ref).double().mean()),
                                                                    float(((dl - dr) / (rel * dl)).max())))
    assert torch.all((lab == ref) | (dl - dr <= rel * dl)) and (lab != ref).double().mean() <= 0.01


@pytest.mark.parametrize("dt,D", [("bf16", 8), ("bf16", 1000), ("fp32", 4), ("fp32", 1000), ("fp64", 2),
                                  ("fp64", 1000)])
def test_rows_inside_a_wider_buffer(dt, D):
    X, C = _data(dt, 300, D, 33)
    buf = torch.full((300, D + DT[dt][4]), float("nan"), dtype=X.dtype, device="cuda")
    buf[:, :D] = X.cuda()
    assert buf[:, :D].stride(0) != D
    assert torch.equal(_assign(dt, buf[:, :D], C), _assign(dt, X.cuda(), C))


@pytest.mark.parametrize("dt", list(DT))
def test_route_round_reproducible_and_graph_replay(dt, monkeypatch):
    from flink_ml_amd.utils import graphs

    n, k, D = 300, 5, 1032
    X, C = _data(dt, n, D, k)
    Xd = X.cuda()
    seen = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (seen.append((name, a[0])), call(name, *a))[1])

    def fresh():
        cb = kk.CentroidBuffers(k, D, Xd.device, DT[dt][1])
        cb.set(C)
        return cb, kk.KMeansRound(Xd, k, "manhattan")

    cb, rnd = fresh()
    got = rnd.run(cb).clone()
    assert (DT[dt][2], Xd.data_ptr()) in seen and "fmlx_kmeans_assign_generic" not in [s[0] for s in seen]
    rtol, atol = DT[dt][5]
    assert torch.allclose(got.cpu().double(), kk.torch_round_payload(X, C, "manhattan"), rtol=rtol, atol=atol)
    assert torch.equal(rnd.run(cb), got)  # bitwise
    for _ in range(3):
        rnd.finalize(cb, rnd.run(cb))
    cb2, rnd2 = fresh()
    gr = graphs.capture(lambda: rnd2.finalize(cb2, rnd2.run(cb2)), Xd.device)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cb2.cent, cb.cent) and torch.equal(rnd2.labels, rnd.labels)


@pytest.mark.parametrize("dt,tol", [("fp32", 1e-5), ("bf16", 2.0 ** -8)])
def test_fit_and_transform_on_a_wide_column(dt, tol):
    from flink_ml_amd import Table, config
    from flink_ml_amd.models.kmeans import KMeans, kmeans_lloyd, sample_rows

    X, C = _data(dt, 400, 1032, 4)
    t = Table({"features": X.cuda()})
    est = KMeans().set_distance_measure("manhattan").set_k(4).set_max_iter(5).set_seed(6)
    init = sample_rows(X.cuda(), 4, est.get_seed())
    assert sorted(kk.torch_assign(torch.as_tensor(init), C, "manhattan").tolist()) == [0, 1, 2, 3]  # one per cluster
    with config.dtype_policy("fp32") if dt == "fp32" else contextlib.nullcontext():
        model = est.fit(t)
        ref_c, _ = kmeans_lloyd(X.double(), init, 5, "manhattan")
        assert np.allclose(model.centroids(), ref_c, rtol=tol, atol=tol)
        pred = model.transform(t)[0].column("prediction").cpu()
        assert torch.equal(pred, kk.torch_assign(X, torch.as_tensor(ref_c), "manhattan"))
