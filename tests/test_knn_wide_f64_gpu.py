"""The fused fp64 KNN kernel for parity-mode rows of 16 <= D <= 4096 (``ops/csrc/knn_wide_f64.hip``)
against a plain fp64 CPU reference, and KnnModel's route to it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _int_data(nq, n, d, span):
    # integer-valued doubles in [-span, span]. span 2^19: every product, norm and key stays below
    # 2^53 up to D = 4096 (2^38 · 4096 · 4 = 2^52), so the fp64 ranking and distances are exact and a
    # kernel that drops to fp32 anywhere fails. span 3: many ties.
    g = torch.Generator(device="cpu").manual_seed(nq * 7 + n * 3 + d + span)
    return (torch.randint(-span, span + 1, (nq, d), generator=g).double(),
            torch.randint(-span, span + 1, (n, d), generator=g).double())


@functools.lru_cache(maxsize=None)
def _ref(nq, n, d, span):
    Q, T = _int_data(nq, n, d, span)
    dist = ((Q * Q).sum(1)[:, None] + (T * T).sum(1)[None, :] - 2.0 * Q @ T.t()).abs().sqrt()
    s = torch.sort(dist, dim=1, stable=True)
    return s.indices[:, :32], s.values[:, :32]


def _f64(Q, T, k, **kw):
    from flink_ml_amd.ops import knn as ko

    return ko.fused_f64_topk(Q.cuda(), T.cuda(), (T * T).sum(1).cuda(), k, with_dist=True, **kw)


# one chunk, a chunk plus one piece, one piece short of two chunks, two chunks, many chunks plus a
# piece; the widest row; both value ranges at D = 30
@pytest.mark.parametrize("n,d,k,span", [(1031, d, k, 1 << 19) for d in (16, 18, 30, 32, 258) for k in (1, 5, 16, 17, 32)]
                         + [(1031, 30, k, 3) for k in (1, 5, 16, 17, 32)] + [(515, 4096, 17, 1 << 19)])
def test_f64_exact(n, d, k, span):
    idx, dist = _f64(*_int_data(150, n, d, span), k)
    ridx, rdist = _ref(150, n, d, span)
    assert torch.equal(idx.long().cpu(), ridx[:, :k])
    torch.testing.assert_close(dist.cpu(), rdist[:, :k], rtol=1e-15, atol=0)


@pytest.mark.parametrize("segments", [1, 2, 5])
@pytest.mark.parametrize("n", [37, 64, 129, 4099])
def test_f64_segments_and_tails(segments, n):
    k = min(9, n)
    Q, T = _int_data(70, n, 18, 3)
    idx, dist = _f64(Q, T, k, segments=segments)
    assert torch.equal(idx.long().cpu(), _ref(70, n, 18, 3)[0][:, :k])
    idx2, dist2 = _f64(Q, T, k, segments=segments % 5 + 2)  # another split: 3, 4, 2
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)


def _nan_view(X):
    """X as rows inside a wider NaN buffer: pitch D + 2, base 2 doubles in, behind a [3:] row slice."""
    buf = torch.full((X.shape[0] + 3, X.shape[1] + 2), float("nan"), dtype=torch.float64, device="cuda")
    buf[3:, 2:] = X
    return buf[3:, 2:]


def test_f64_views_and_refused_shapes(monkeypatch):
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models.knn import knn_predict, knn_vote
    from flink_ml_amd.ops import knn as ko

    span = 1 << 19
    Q, T = _int_data(150, 1031, 30, span)
    q, t, tn = Q.cuda(), T.cuda(), (T * T).sum(1).cuda()
    idx, dist = ko.fused_f64_topk(q, t, tn, 5, with_dist=True)
    vidx, vdist = ko.fused_f64_topk(_nan_view(q), _nan_view(t), tn, 5, with_dist=True)
    assert torch.equal(idx, vidx) and torch.equal(dist, vdist)

    lab = (T[:, 0] > 0).double().cuda()
    ref = knn_vote(lab.cpu()[_ref(150, 1031, 30, span)[0][:, :5]], torch.unique(lab.cpu()))
    odd = torch.zeros((1031, 31), dtype=torch.float64, device="cuda")[:, :30].copy_(t)  # a pitch of D + 1
    assert not ko.fused_f64_supported(5, 1031, 30, q, odd)
    Q2, T2 = _int_data(150, 1031, 31, span)  # an odd D
    assert not ko.fused_f64_supported(5, 1031, 31, Q2.cuda(), T2.cuda())
    lab2 = (T2[:, 0] > 0).double().cuda()
    ref2 = knn_vote(lab2.cpu()[_ref(150, 1031, 31, span)[0][:, :5]], torch.unique(lab2.cpu()))
    monkeypatch.setattr(ko, "F64", "force")  # knn_predict asks the kernel first and is refused
    with dtype_policy("fp64"):
        assert torch.equal(knn_predict(q, odd, tn, lab, 5).cpu(), ref)
        assert torch.equal(knn_predict(Q2.cuda(), T2.cuda(), (T2 * T2).sum(1).cuda(), lab2, 5).cpu(), ref2)


def test_f64_random_floats_and_nan_norm():
    from flink_ml_amd.ops import knn as ko

    D, k = 512, 20
    g = torch.Generator(device="cpu").manual_seed(11)
    Q, T = torch.randn(200, D, generator=g).double(), torch.randn(5000, D, generator=g).double()
    tn = (T * T).sum(1)
    tn[5] = float("nan")
    idx = ko.fused_f64_topk(Q.cuda(), T.cuda(), tn.cuda(), k).long().cpu()
    assert not (idx == 5).any()
    qn, tn64 = (Q * Q).sum(1), (T * T).sum(1)
    d2 = (qn[:, None] + tn64[None, :] - 2.0 * Q @ T.t()).abs()
    got = torch.gather(d2, 1, idx)
    d2[:, 5] = float("inf")
    want = torch.sort(d2, dim=1).values[:, :k]
    bound = 2.0 * (D + 4) * 2.0 ** -53 * (qn[:, None] + tn64[idx])
    assert ((got - want).abs() <= bound).all()


@pytest.mark.parametrize("k", [5, 32])
def test_knn_model_routes_f64(k, monkeypatch):
    from flink_ml_amd import Table
    from flink_ml_amd.config import dtype_policy
    from flink_ml_amd.models import Knn
    from flink_ml_amd.models.knn import knn_vote
    from flink_ml_amd.ops import knn as ko
    from flink_ml_amd.table import SparseColumn

    assert not ko.f64_route(5, 301, 6000, 150)  # the default setting keeps the select kernel there
    nq, n, D = 301, 4099, 150
    Q, T = _int_data(nq, n, D, 1 << 19)
    lab = (T[:, 0] > 0).double() + (T[:, 1] > 0).double()
    ref = knn_vote(lab[_ref(nq, n, D, 1 << 19)[0][:, :k]], torch.unique(lab))
    sparse = SparseColumn(torch.arange(0, nq * D + 1, D), torch.arange(D, dtype=torch.int32).repeat(nq),
                          Q.reshape(-1), D)
    with dtype_policy("fp64"):
        model = Knn().set_k(k).fit(Table({"features": T.cuda(), "label": lab.cuda()}))
        with monkeypatch.context() as m:
            m.setattr(ko, "F64", "0")
            old = model.transform(Table({"features": Q.cuda()}))[0].column("prediction").cpu()

        def no_mm(*a, **kw):
            raise AssertionError("library GEMM on the fp64 fused KNN route")

        monkeypatch.setattr(ko, "F64", "force")
        monkeypatch.setattr(torch, "mm", no_mm)
        pred = model.transform(Table({"features": Q.cuda()}))[0].column("prediction").cpu()
        spred = model.transform(Table({"features": sparse}))[0].column("prediction").cpu()
    assert torch.equal(pred.double(), ref.double())
    assert torch.equal(old.double(), ref.double()) and torch.equal(spred.double(), ref.double())
