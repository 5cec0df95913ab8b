"""The K-tiled fused KNN kernel for fp32 rows of 128 < D <= 4096 (``ops/csrc/knn_wide.hip``) against a
plain fp64 reference, and KnnModel's route to it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _int_data(nq, n, d):
    # small integers in [-3, 3]: every product and norm is exact in fp32 up to D = 4096
    # (9 · 4096 < 2^24), so the kernel's ranking must equal the fp64 ranking, ties to the lower index
    g = torch.Generator(device="cpu").manual_seed(nq * 7 + n * 3 + d)
    return (torch.randint(-3, 4, (nq, d), generator=g).double(), torch.randint(-3, 4, (n, d), generator=g).double())


@functools.lru_cache(maxsize=None)
def _ref_fp64(nq, n, d):
    Q, T = _int_data(nq, n, d)
    dist = ((Q * Q).sum(1)[:, None] + (T * T).sum(1)[None, :] - 2.0 * Q @ T.t()).abs().sqrt()
    s = torch.sort(dist, dim=1, stable=True)
    return s.indices[:, :64], s.values[:, :64]


def _wide(Q, T, k, **kw):
    from flink_ml_amd.ops import knn as ko

    tn = (T * T).sum(1).float().cuda()
    return ko.fused_wide_topk(Q.float().cuda(), T.float().cuda(), tn, k, with_dist=True, **kw)


# one chunk plus a tail, whole chunks, one piece past and short of a chunk, many chunks; the widest row
@pytest.mark.parametrize("n,d,k", [(4099, d, k) for d in (132, 256, 260, 380, 1028) for k in (1, 5, 33, 64)]
                         + [(515, 4096, 33)])
def test_wide_exact_vs_fp64(n, d, k):
    idx, dist = _wide(*_int_data(301, n, d), k)
    ridx, rdist = _ref_fp64(301, n, d)
    assert torch.equal(idx.long().cpu(), ridx[:, :k])
    torch.testing.assert_close(dist.double().cpu(), rdist[:, :k], rtol=1e-6, atol=0)


@pytest.mark.parametrize("segments", [1, 2, 5])
@pytest.mark.parametrize("n", [37, 64, 129, 20011])
def test_wide_segments_and_tails(segments, n):
    k = min(9, n)
    Q, T = _int_data(70, n, 132)
    idx, dist = _wide(Q, T, k, segments=segments)
    assert torch.equal(idx.long().cpu(), _ref_fp64(70, n, 132)[0][:, :k])
    idx2, dist2 = _wide(Q, T, k, segments=segments % 5 + 2)  # another split: 3, 4, 2
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)


def _nan_view(X):
    """X as rows inside a wider NaN buffer: pitch D + 4, base 4 floats in, behind a [3:] row slice."""
    buf = torch.full((X.shape[0] + 3, X.shape[1] + 4), float("nan"), dtype=torch.float32, device="cuda")
    buf[3:, 4:] = X
    return buf[3:, 4:]


def test_wide_views_and_refused_shapes():
    from flink_ml_amd.models.knn import knn_predict, knn_vote
    from flink_ml_amd.ops import knn as ko

    Q, T = _int_data(301, 4099, 260)
    q, t, tn = Q.float().cuda(), T.float().cuda(), (T * T).sum(1).float().cuda()
    idx, dist = ko.fused_wide_topk(q, t, tn, 5, with_dist=True)
    vidx, vdist = ko.fused_wide_topk(_nan_view(q), _nan_view(t), tn, 5, with_dist=True)
    assert torch.equal(idx, vidx) and torch.equal(dist, vdist)

    lab = (T[:, 0] > 0).double().cuda()
    ref = knn_vote(lab.cpu()[_ref_fp64(301, 4099, 260)[0][:, :5]], torch.unique(lab.cpu()))
    odd = torch.zeros((4099, 261), dtype=torch.float32, device="cuda")[:, :260].copy_(t)  # a pitch of D + 1
    assert not ko.fused_wide_supported(5, 4099, 260, q, odd)
    assert torch.equal(knn_predict(q, odd, tn, lab, 5).cpu(), ref)
    Q2, T2 = _int_data(301, 4099, 130)  # D % 4 != 0
    assert not ko.fused_wide_supported(5, 4099, 130, Q2.float().cuda(), T2.float().cuda())
    pred = knn_predict(Q2.float().cuda(), T2.float().cuda(), (T2 * T2).sum(1).float().cuda(), lab, 5)
    assert torch.equal(pred.cpu(), knn_vote(lab.cpu()[_ref_fp64(301, 4099, 130)[0][:, :5]], torch.unique(lab.cpu())))


def test_wide_random_floats_and_nan_norm():
    from flink_ml_amd.ops import knn as ko

    D, k = 512, 20
    g = torch.Generator(device="cpu").manual_seed(11)
    Q, T = torch.randn(200, D, generator=g), torch.randn(5000, D, generator=g)
    tn = (T * T).sum(1)
    tn[5] = float("nan")
    idx = ko.fused_wide_topk(Q.cuda(), T.cuda(), tn.cuda(), k).long().cpu()
    assert not (idx == 5).any()
    qn64, tn64 = (Q.double() ** 2).sum(1), (T.double() ** 2).sum(1)
    d2 = (qn64[:, None] + tn64[None, :] - 2.0 * Q.double() @ T.double().t()).abs()
    got = torch.gather(d2, 1, idx)
    d2[:, 5] = float("inf")
    want = torch.sort(d2, dim=1).values[:, :k]
    bound = 2.0 * (D + 4) * 2.0 ** -24 * (qn64[:, None] + tn64[idx])
    assert ((got - want).abs() <= bound).all()


@pytest.mark.parametrize("k", [5, 64])
def test_knn_model_routes_wide(k, monkeypatch):
    from flink_ml_amd import Table
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import Knn
    from flink_ml_amd.models.knn import knn_vote
    from flink_ml_amd.ops import knn as ko
    from flink_ml_amd.table import SparseColumn

    nq, n, D = 301, 4099, 260
    Q, T = _int_data(nq, n, D)
    lab = (T[:, 0] > 0).double() + (T[:, 1] > 0).double()
    ref = knn_vote(lab[_ref_fp64(nq, n, D)[0][:, :k]], torch.unique(lab))
    sparse = SparseColumn(torch.arange(0, nq * D + 1, D), torch.arange(D, dtype=torch.int32).repeat(nq),
                          Q.reshape(-1), D)
    with dtype_policy("fp32"):
        model = Knn().set_k(k).fit(Table({"features": T.cuda(), "label": lab.cuda()}))
        with monkeypatch.context() as m:
            m.setattr(ko, "WIDE", "0")
            old = model.transform(Table({"features": Q.cuda()}))[0].column("prediction").cpu()

        def no_mm(*a, **kw):
            raise AssertionError("library GEMM on the wide KNN route")

        monkeypatch.setattr(torch, "mm", no_mm)
        pred = model.transform(Table({"features": Q.cuda()}))[0].column("prediction").cpu()
        spred = model.transform(Table({"features": sparse}))[0].column("prediction").cpu()
    assert torch.equal(pred.double(), ref.double())
    assert torch.equal(old.double(), ref.double()) and torch.equal(spred.double(), ref.double())
