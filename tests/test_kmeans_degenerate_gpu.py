"""KMeans with NaN centroids (what an empty cluster leaves behind), zero / NaN / ±inf rows and rows
without a winner, on every dense assign route, on the round that follows an empty cluster and
through the three groupings, against one fp64 reference of ``DistanceMeasure.findClosest``:

* distances on the operands as the route stores them (rows and centroids rounded to its dtype):
  euclidean max(0, ‖x‖² + ‖c‖² − 2·x·c) with NaN kept, manhattan Σ|x − c|, cosine 1 − x·c/‖x‖/‖c‖;
* a NaN distance counts as +inf (strict '<' never takes it), the first strict minimum wins;
* a row with no distance below +inf gets 0 under euclidean (EuclideanDistanceMeasure: bestIndex = 0)
  and −1 under manhattan and cosine (DistanceMeasure: targetCentroidId = −1);
* a row labelled −1 adds to no sum and no count of the round's payload.

The labels are compared exactly: before any launch the reference asserts that every row's two
smallest distances differ by more than 100·D·2^−m of the magnitude of the key's terms (m = 23 for
fp32 accumulation, 52 for fp64). A dot product of D terms accumulated in that format is off by at
most D·2^−(m+1)·Σ|x_j·c_j| <= D·2^−(m+1)·(‖x‖² + ‖c‖²)/2, so the bound has two decades of slack
for the norms, the summation order and the bf16 kernels' tile bits in the low mantissa. The seeds in
``SEEDS`` are the first ones at which that assertion holds for the case's shape (searched on a CPU).
"""
import pytest
import torch

from flink_ml_amd.ops import kmeans as kk

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
N = 300
INF = float("inf")
NAN = float("nan")
MANT = {torch.bfloat16: 23, torch.float32: 23, torch.float64: 52}  # the accumulator's mantissa bits
ACC = {torch.bfloat16: torch.float32, torch.float32: torch.float32, torch.float64: torch.float64}
ROUND_TOL = {torch.float32: (1e-5, 1e-3), torch.float64: (1e-12, 4e-12)}  # the existing round tests' (rtol, atol)


# ------------------------------------------------------------------------------------ the reference
def ref_distances(X, C, metric, magnitude=False):
    """[n, k] fp64 distances (squared under euclidean), NaN where the reference's are NaN; with
    ``magnitude`` also the sum of the absolute values of the terms each key is formed from."""
    X, C = X.double(), C.double()
    if metric == "manhattan":
        d = (X[:, None, :] - C[None, :, :]).abs().sum(2)
        return (d, d) if magnitude else d
    dot = (X[:, None, :] * C[None, :, :]).sum(2)
    x2, c2 = (X * X).sum(1)[:, None], (C * C).sum(1)[None, :]
    if metric == "euclidean":
        d = x2 + c2 - 2.0 * dot
        d = torch.where(d < 0, torch.zeros_like(d), d)  # Math.max(0.0, d): NaN stays NaN
        mag = x2 + c2 + 2.0 * dot.abs()
    else:
        cos = dot / x2.sqrt() / c2.sqrt()
        d = 1.0 - cos
        mag = 1.0 + cos.abs()
    return (d, mag) if magnitude else d


def ref_assign(X, C, metric):
    d = ref_distances(X, C, metric)
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    lab = torch.argmin(d, dim=1)  # the first minimum
    none = torch.full_like(lab, 0 if metric == "euclidean" else -1)
    return torch.where((d < INF).any(1), lab, none)


def ref_payload(X, labels, k):
    """[k·D sums | k counts] in fp64 of the given labels; a row labelled −1 adds nothing."""
    X = X.double()
    ok = labels >= 0
    sums = torch.zeros((k, X.shape[1]), dtype=torch.float64).index_add_(0, labels[ok], X[ok])
    return torch.cat([sums.reshape(-1), torch.bincount(labels[ok], minlength=k).double()])


def separated(X, C, metric, m):
    """Whether every row's two smallest distances differ by more than 100·D·2^−m of the magnitude of
    their terms (a row with fewer than two distances below +inf has nothing to separate)."""
    d, mag = ref_distances(X, C, metric, magnitude=True)
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    two, idx = torch.topk(d, 2, dim=1, largest=False)
    live = two[:, 1] < INF
    bound = 100.0 * X.shape[1] * 2.0 ** -m * mag.gather(1, idx).max(1).values
    return bool((two[:, 1] - two[:, 0] > bound)[live].all())


# ------------------------------------------------------------------------------------ the data
# (D, k, metric) → the first seed whose data is separated for every dtype the tests use at that shape,
# where that is not seed 0
SEEDS = {(128, 5, "euclidean"): 2, (200, 5, "cosine"): 1, (1025, 5, "euclidean"): 1, (132, 5, "euclidean"): 1,
         (1025, 33, "cosine"): 17}


def clustered(D, k, seed, n=N):
    g = torch.Generator().manual_seed(seed * 100003 + D * 31 + k)
    C = torch.randn((k, D), generator=g, dtype=torch.float64)
    # the coordinate that carries the ±inf elements below: both signs among the centroids, centroid 0
    # negative, so that a key without ‖x‖² is −inf for some centroid other than 0
    C[:, D // 2] = C[:, D // 2].abs() * (2.0 * (torch.arange(k) % 2) - 1.0)
    X = C[torch.arange(n) % k] + 0.05 * torch.randn((n, D), generator=g, dtype=torch.float64)
    return X, C


def degenerate(D, k, dtype, seed):
    """Rows c_(i mod k) + 0.05·noise, then the degenerate rows and centroids; both rounded to ``dtype``."""
    X, C = clustered(D, k, seed)
    X[3] = 0.0
    X[7, D - 1] = NAN
    X[11, D // 2] = INF
    X[13, D // 2] = -INF
    C[2] = NAN  # what an empty cluster leaves
    C[1, D // 3] = NAN
    if k == 33:
        C[4] = 0.0
        C[6, D // 2] = INF
    return X.to(dtype), C.to(dtype).double()


def case_data(D, k, dtype, metric):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    X, C = degenerate(D, k, dtype, SEEDS.get((D, k, metric), 0))
    assert separated(X, C, metric, MANT[dtype])
    ref = ref_assign(X, C, metric)
    # the data does what it is for: no-winner rows, and no label names a NaN centroid
    assert ref[[7, 11, 13]].tolist() == [0 if metric == "euclidean" else -1] * 3
    if metric == "cosine" or k == 33:  # the zero row: no cosine winner; otherwise on the zero centroid
        assert int(ref[3]) == (-1 if metric == "cosine" else 4)
    assert not bool(((ref == 1) | (ref == 2)).any()) and (k != 33 or not bool((ref == 6).any()))
    return X, C, ref


def buffers(C, dtype):
    cb = kk.CentroidBuffers(C.shape[0], C.shape[1], torch.device("cuda"), ACC[dtype])
    cb.set(C)
    return cb


def generic_route(Xd, metric):
    """None of the MFMA, GEMM or fused routes takes these rows: ``fmlx_kmeans_assign_generic``."""
    return not (kk.mfma_ok(Xd, metric) or kk.mfma_wide_ok(Xd, metric) or kk.mfma_wide_f32_ok(Xd, metric)
                or kk.mfma_wide_f64_ok(Xd, metric) or Xd.shape[0] >= kk.GEMM_ASSIGN_MIN_ROWS)


# ------------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("sched,D", [(0, 40), (0, 64), (0, 128), (1, 64), (1, 128)])
def test_assign_narrow_bf16_mfma(sched, D, k):
    X, C, ref = case_data(D, k, torch.bfloat16, "euclidean")
    Xd = X.cuda()
    assert kk.mfma_ok(Xd, "euclidean")
    try:
        kk.set_assign_sched(sched)
        lab = kk.assign(Xd, buffers(C, torch.bfloat16), "euclidean").cpu().long()
    finally:
        kk.set_assign_sched(kk.ASSIGN_SCHED)
    assert torch.equal(lab, ref)


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", [37, 200, 1025])  # wave-per-row (1 and 4 values per lane), thread-per-row
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_assign_generic(dtype, D, metric, k, monkeypatch):
    monkeypatch.setattr(kk, "WIDE", False)
    X, C, ref = case_data(D, k, dtype, metric)
    Xd = X.cuda()
    assert generic_route(Xd, metric)
    assert torch.equal(kk.assign(Xd, buffers(C, dtype), metric).cpu().long(), ref)


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("route", ["gemm", "fused"])
def test_assign_fp32_gemm_and_fused_knn(route, k, monkeypatch):
    from flink_ml_amd.ops import knn as knn_ops

    monkeypatch.setattr(kk, "GEMM_ASSIGN_MIN_ROWS", 1)
    monkeypatch.setattr(kk, "FP32_ASSIGN", route)
    X, C, ref = case_data(100, k, torch.float32, "euclidean")
    Xd = X.cuda()
    assert not kk.mfma_wide_f32_ok(Xd, "euclidean") and k <= kk.GEMM_ASSIGN_MAX_K
    assert knn_ops.fused_supported(1, k, 100, Xd.device)
    assert torch.equal(kk.assign(Xd, buffers(C, torch.float32), "euclidean").cpu().long(), ref)


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("dtype,D,ok", [(torch.bfloat16, 264, kk.mfma_wide_ok), (torch.float32, 132, kk.mfma_wide_f32_ok),
                                        (torch.float64, 130, kk.mfma_wide_f64_ok)])
def test_assign_wide_mfma(dtype, D, ok, k, monkeypatch):
    monkeypatch.setattr(kk, "WIDE", "force")
    X, C, ref = case_data(D, k, dtype, "euclidean")
    Xd = X.cuda()
    assert ok(Xd, "euclidean") and not kk.mfma_ok(Xd, "euclidean")
    assert torch.equal(kk.assign(Xd, buffers(C, dtype), "euclidean").cpu().long(), ref)


# ------------------------------------------------------------------------------------ after an empty cluster
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float32, 37), (torch.float64, 37),
                                     (torch.float32, 1025)])
def test_round_after_an_empty_cluster(dtype, D, monkeypatch):
    """Round 1 leaves cluster 2 empty; ``fmlx_kmeans_finalize`` writes its NaN centroid, −2·c image and
    norms; round 2 reads them and must never choose it. Past D = 1024 the chunk sum refuses the rows
    (−3, as test_gpu_round_row_width_rungs pins), so there the payloads come from the reference sums of
    the device labels and only the assign and the finalize run on the device."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setattr(kk, "WIDE", False)
    k, acc = 5, ACC[dtype]
    X, C = clustered(D, k, 0)
    X = X.to(dtype)
    C[2] = 100.0  # far from every row
    C = C.to(dtype).double()
    Xd = X.cuda()
    cb = buffers(C, dtype)
    rnd = kk.KMeansRound(Xd, k, "euclidean")
    assert not (rnd.wide or rnd.wide32 or rnd.wide64) and (kk.mfma_ok(Xd, "euclidean") or generic_route(Xd, "euclidean"))
    assert kk.mfma_ok(Xd, "euclidean") == (dtype == torch.bfloat16)

    def run_round():
        if D <= 1024:
            return rnd.run(cb).clone()
        with pytest.raises(RuntimeError, match=r"fmlx_kmeans_chunk_sum failed with error -3$"):
            rnd.run(cb)  # (the assign before it wrote rnd.labels)
        return ref_payload(X, rnd.labels.cpu().long(), k).to(acc).cuda()

    def check(Cin, payload):
        Cseen = Cin.to(dtype).double()  # bf16 rows: the MFMA assign reads the bf16 image of the centroids
        assert separated(X, Cseen, "euclidean", MANT[dtype])
        ref = ref_assign(X, Cseen, "euclidean")
        assert torch.equal(rnd.labels.cpu().long(), ref) and not bool((ref == 2).any())
        want, got = ref_payload(X, ref, k), payload.cpu().double()
        rtol, atol = ROUND_TOL[acc]
        assert torch.allclose(got[: k * D], want[: k * D], rtol=rtol, atol=atol)
        assert torch.equal(got[k * D:], want[k * D:]) and float(got[k * D + 2]) == 0.0

    p1 = run_round()
    check(C, p1)
    rnd.finalize(cb, p1)
    cent = cb.cent.cpu().double()
    assert bool(torch.isnan(cent[2]).all()) and float(cb.weights[2]) == 0.0
    assert bool(torch.isfinite(cent[[0, 1, 3, 4]]).all())
    p2 = run_round()
    check(cent, p2)
    rnd.finalize(cb, p2)
    cent2 = cb.cent.cpu().double()
    assert bool(torch.isnan(cent2[2]).all()) and bool(torch.isfinite(cent2[[0, 1, 3, 4]]).all())
    assert cb.weights.cpu().tolist() == p2[k * D:].cpu().double().tolist()


# ------------------------------------------------------------------------------------ the groupings
@pytest.mark.parametrize("k", [5, 8])  # a power of two: the −1 label's low bits are those of key k − 1
@pytest.mark.parametrize("mode", ["stable", "arrival", "radix"])
@pytest.mark.parametrize("metric", ["manhattan", "cosine"])
def test_rows_without_a_winner_through_the_groupings(metric, mode, k, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flink_ml_amd.ops import native

    monkeypatch.setattr(kk, "GROUP_SORT", mode != "radix")
    if mode == "arrival":  # what k > fmlx_group_stable_max_keys() takes
        monkeypatch.setattr(native.kernels(), "fmlx_group_stable_max_keys", lambda: 0)
    n, D = 3000, 20
    X, C = clustered(D, k, SEEDS.get((D, k, metric), 0), n)
    X[torch.arange(17, n, 197)] = 0.0  # 16 zero rows: no winner under cosine
    X[torch.arange(5, n, 211), D - 1] = NAN  # 15 NaN rows: no winner under either metric
    X, C = X.float(), C.float().double()
    assert separated(X, C, metric, 23)
    ref = ref_assign(X, C, metric)
    lost = int((ref < 0).sum())
    assert lost == (31 if metric == "cosine" else 15)
    rnd = kk.KMeansRound(X.cuda(), k, metric)
    assert rnd.stable == (mode == "stable") and rnd.group == (mode == "arrival")
    cb = buffers(C, torch.float32)
    p1 = rnd.run(cb).clone()
    p2 = rnd.run(cb).clone()
    assert torch.equal(rnd.labels.cpu().long(), ref)
    want, got = ref_payload(X, ref, k), p1.cpu().double()
    assert torch.equal(got[k * D:], want[k * D:]) and float(got[k * D:].sum()) == n - lost
    assert torch.allclose(got[: k * D], want[: k * D], rtol=1e-5, atol=1e-3)
    if mode != "arrival":
        assert torch.equal(p1, p2)  # bit-reproducible
    else:
        assert torch.equal(p1[k * D:], p2[k * D:]) and torch.allclose(p1, p2, rtol=1e-6, atol=1e-4)
