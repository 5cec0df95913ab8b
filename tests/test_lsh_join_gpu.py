"""The MinHashLSH search kernels (ops/csrc/lsh_join.hip through ops/lsh.py) against the torch
formulation (FMLX_LSH_NATIVE=0) and plain numpy: pair distances at the lane-group boundaries, the
join over several table shapes, chunking, key collisions, bounded memory, the neighbour filter and
the stage's public methods."""
import numpy as np
import pytest
import torch

from flink_ml_amd import Vectors
from flink_ml_amd.models.feature.lsh import generate_model_data
from flink_ml_amd.ops import lsh as lsh_ops
from flink_ml_amd.table import SparseColumn
from tests.test_feature_lsh import _lsh, _rand_sets

pytestmark = pytest.mark.gpu
HASH_PRIME = lsh_ops.HASH_PRIME


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _csr(rows, d) -> SparseColumn:
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ind = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rows else np.zeros(0, np.int32)
    return SparseColumn(torch.from_numpy(ptr), torch.from_numpy(ind.astype(np.int32)),
                        torch.ones(len(ind), dtype=torch.float64), d)


def _random_rows(rng, n, d, lo, hi):
    return [np.sort(rng.choice(d, size=int(rng.integers(lo, hi)), replace=False)) for _ in range(n)]


def _signatures(sets: SparseColumn, T, F, seed=11) -> torch.Tensor:
    _, _, a, b = generate_model_data(T, F, sets.size, seed)
    return lsh_ops.minhash(sets, a, b).reshape(-1, T, F)


def _torch_path(monkeypatch, fn, *args, **kw):
    """``fn`` under FMLX_LSH_NATIVE=0: the torch formulation on the same (device) tensors."""
    with monkeypatch.context() as m:
        m.setenv("FMLX_LSH_NATIVE", "0")
        return fn(*args, **kw)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.device == w.device
        assert torch.equal(g, w)


def _no_torch_path(monkeypatch):
    """The native calls below must not reach the torch formulation."""
    def boom(*a, **k):
        raise AssertionError("torch formulation on the native path")

    for name in ("similarity_join_torch", "pair_jaccard_torch", "nearest_torch"):
        monkeypatch.setattr(lsh_ops, name, boom)


# ------------------------------------------------------------------------------- pair_jaccard
def test_pair_jaccard_group_and_wave_boundaries(monkeypatch):
    _need_gpu()
    rng = np.random.default_rng(0)
    d = HASH_PRIME
    lens = [1, 15, 16, 17, 63, 64, 65, 300]
    a_rows = [np.sort(rng.choice(2000, size=n, replace=False)) for n in lens]
    b_rows = [np.sort(rng.choice(2000, size=n, replace=False)) for n in lens]
    b_rows += [r.copy() for r in a_rows]                                   # identical sets
    b_rows += [np.arange(5000, 5000 + n) for n in (1, 16, 300)]            # disjoint from every A row
    a_rows.append(np.array([3, 700, HASH_PRIME - 1]))                      # the largest index there is
    b_rows.append(np.array([700, 1999, HASH_PRIME - 1]))
    sa, sb = _csr(a_rows, d).to("cuda"), _csr(b_rows, d).to("cuda")
    ia, ib = np.meshgrid(np.arange(len(a_rows)), np.arange(len(b_rows)), indexing="ij")
    ia = np.concatenate([ia.ravel(), np.full(1000, 7)])                     # one row named by many pairs
    ib = np.concatenate([ib.ravel(), rng.integers(0, len(b_rows), 1000)])
    ia_t, ib_t = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    want = _torch_path(monkeypatch, lsh_ops.pair_jaccard, sa, sb, ia_t, ib_t)
    ref = [lsh_ops.jaccard_distance(a_rows[i], b_rows[j]) for i, j in zip(ia, ib)]
    assert want.cpu().tolist() == ref
    _no_torch_path(monkeypatch)
    got = lsh_ops.pair_jaccard(sa, sb, ia_t, ib_t)
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.equal(got, want)
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0  # identical and disjoint sets are there
    empty = lsh_ops.pair_jaccard(sa, sb, ia_t[:0], ib_t[:0])
    assert empty.shape == (0,) and empty.dtype == torch.float64 and empty.is_cuda


def test_pair_jaccard_errors(monkeypatch):
    _need_gpu()
    sa = _csr([np.array([], dtype=np.int32), np.array([1, 2])], 10).to("cuda")
    one = torch.tensor([1], device="cuda")
    assert lsh_ops.pair_jaccard(sa, sa, one, one).tolist() == [0.0]
    with pytest.raises(ValueError, match="The union of two input sets must have at least 1 elements"):
        lsh_ops.pair_jaccard(sa, sa, one - 1, one - 1)
    with pytest.raises(IndexError):
        lsh_ops.pair_jaccard(sa, sa, one, one + 1)


# ------------------------------------------------------------------------------ similarity_join
@pytest.fixture(scope="module")
def join_sets():
    rng = np.random.default_rng(1)
    a_rows, b_rows = _random_rows(rng, 900, 60, 1, 8), _random_rows(rng, 700, 60, 1, 8)
    return _csr(a_rows, 60), _csr(b_rows, 60)


@pytest.mark.parametrize("T,F", [(4, 2), (5, 1), (3, 3), (40, 1)])
def test_join_matches_torch_path(monkeypatch, join_sets, T, F):
    _need_gpu()
    sa, sb = (s.to("cuda") for s in join_sets)
    ha, hb = _signatures(sa, T, F), _signatures(sb, T, F)
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha, hb, sa, sb, 0.7)
    assert want[0].numel() > 50
    _no_torch_path(monkeypatch)
    got = lsh_ops.similarity_join(ha, hb, sa, sb, 0.7)
    _same(got, want)
    _same(lsh_ops.similarity_join(ha, hb, sa, sb, 0.7), got)  # determinism: a second call, the same tensors
    if (T, F) == (3, 3):  # narrow bucket keys collide; the signatures themselves decide
        _same(lsh_ops.similarity_join(ha, hb, sa, sb, 0.7, key_bits=4), got)
        _same(lsh_ops.similarity_join(ha, hb, sa, sb, 0.7, key_bits=1), got)


@pytest.mark.parametrize("threshold", [0.0, 1.0])
def test_join_threshold_ends(monkeypatch, join_sets, threshold):
    _need_gpu()
    sa, sb = (s.to("cuda") for s in join_sets)
    ha, hb = _signatures(sa, 4, 2), _signatures(sb, 4, 2)
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha, hb, sa, sb, threshold)
    assert want[0].numel() > (1000 if threshold else 5)
    _no_torch_path(monkeypatch)
    _same(lsh_ops.similarity_join(ha, hb, sa, sb, threshold), want)


@pytest.mark.parametrize("na,nb", [(0, 700), (900, 0)])
def test_join_empty_side(monkeypatch, join_sets, na, nb):
    _need_gpu()
    sa, sb = join_sets[0].slice(0, na).to("cuda"), join_sets[1].slice(0, nb).to("cuda")
    ha = _signatures(join_sets[0].to("cuda"), 4, 2)[:na]
    hb = _signatures(join_sets[1].to("cuda"), 4, 2)[:nb]
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha, hb, sa, sb, 0.7)
    _no_torch_path(monkeypatch)
    got = lsh_ops.similarity_join(ha, hb, sa, sb, 0.7)
    _same(got, want)
    assert got[0].numel() == 0


def test_join_exact_duplicates_once(monkeypatch, join_sets):
    """B holds copies of A's rows (and A copies of its own): such a pair matches in every table and
    comes back once."""
    _need_gpu()
    a = join_sets[0]
    rows = [a.indices[int(a.indptr[i]):int(a.indptr[i + 1])].numpy() for i in range(300)]
    sa = _csr(rows + rows[:50], 60).to("cuda")
    sb = _csr(rows[100:250] + rows[100:120], 60).to("cuda")
    ha, hb = _signatures(sa, 4, 2), _signatures(sb, 4, 2)
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha, hb, sa, sb, 0.5)
    _no_torch_path(monkeypatch)
    got = lsh_ops.similarity_join(ha, hb, sa, sb, 0.5)
    _same(got, want)
    keys = (got[0] * len(sb) + got[1]).cpu().numpy()
    assert len(np.unique(keys)) == len(keys)
    assert int((got[2] == 0.0).sum()) >= 150 + 20


def test_join_chunks(monkeypatch):
    """chunk=1000 over 40,000 + candidates, a 200 × 200 bucket across many chunk boundaries."""
    _need_gpu()
    rng = np.random.default_rng(2)
    na, nb = 600, 500
    sa, sb = _csr(_random_rows(rng, na, 64, 2, 12), 64).to("cuda"), _csr(_random_rows(rng, nb, 64, 2, 12), 64).to("cuda")
    ha = torch.from_numpy(rng.integers(0, 40, (na, 2, 1)).astype(np.float64))
    hb = torch.from_numpy(rng.integers(0, 40, (nb, 2, 1)).astype(np.float64))
    ha[:, 0, 0] += 1000.0 + torch.arange(na) * 50  # table 0: nothing matches …
    ha[100:300, 0, 0] = 7.0                        # … but one bucket of 200 × 200
    hb[50:250, 0, 0] = 7.0
    ha, hb = ha.cuda(), hb.cuda()
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha, hb, sa, sb, 1.0)
    assert want[0].numel() >= 40000  # threshold 1.0 keeps every candidate: at least as many candidates
    _no_torch_path(monkeypatch)
    whole = lsh_ops.similarity_join(ha, hb, sa, sb, 1.0)
    _same(whole, want)
    _same(lsh_ops.similarity_join(ha, hb, sa, sb, 1.0, chunk=1000), whole)
    _same(lsh_ops.similarity_join(ha, hb, sa, sb, 1.0, chunk=999), whole)
    part = lsh_ops.similarity_join(ha, hb, sa, sb, 0.6, chunk=1000)
    _same(part, lsh_ops.similarity_join(ha, hb, sa, sb, 0.6))
    _same(part, tuple(x[whole[2] <= 0.6] for x in whole))


def test_join_fallback_flags(monkeypatch, join_sets):
    """−0.0 in a signature and an unsorted set row: the call gives the torch formulation's result."""
    _need_gpu()
    sa, sb = (s.to("cuda") for s in join_sets)
    ha, hb = _signatures(sa, 4, 2), _signatures(sb, 4, 2)
    ha0, hb0 = ha.clone(), hb.clone()
    ha0[:50, 0, :] = 0.0
    hb0[:40, 0, :] = -0.0
    want = _torch_path(monkeypatch, lsh_ops.similarity_join, ha0, hb0, sa, sb, 1.0)
    assert want[0].numel() >= 50 * 40
    _same(lsh_ops.similarity_join(ha0, hb0, sa, sb, 1.0), want)
    longest = int(torch.argmax(sa.indptr[1:] - sa.indptr[:-1]))
    lo, hi = int(sa.indptr[longest]), int(sa.indptr[longest + 1])
    ind = sa.indices.clone()
    ind[lo:hi] = torch.flip(ind[lo:hi], [0])
    sa_u = SparseColumn(sa.indptr, ind, sa.values, sa.size)
    _same(lsh_ops.similarity_join(ha, hb, sa_u, sb, 0.7), lsh_ops.similarity_join(ha, hb, sa, sb, 0.7))
    pairs = torch.tensor([longest] * 3, device="cuda"), torch.tensor([0, 1, 2], device="cuda")
    assert torch.equal(lsh_ops.pair_jaccard(sa_u, sb, *pairs), lsh_ops.pair_jaccard(sa, sb, *pairs))


def test_join_bounded_memory():
    """One table's signature equal for all 4,000 × 4,000 rows: 16 M candidates, of which the planted
    near-duplicates survive, in at most 512 MiB above what was allocated before the call."""
    _need_gpu()
    rng = np.random.default_rng(3)
    n, d, m = 4000, 4096, 32
    a_rows = [np.sort(rng.choice(d, size=m, replace=False)) for _ in range(n)]
    b_rows = [np.sort(rng.choice(d, size=m, replace=False)) for _ in range(n)]
    planted = []
    for q in range(20):  # B row 7 + 150 q: A row 11 + 190 q with 3 of its 32 elements replaced (distance 6 / 35)
        i, j = 11 + 190 * q, 7 + 150 * q
        row = a_rows[i].copy()
        free = np.setdiff1d(np.arange(d), row)
        row[rng.choice(m, size=3, replace=False)] = rng.choice(free, size=3, replace=False)
        b_rows[j] = np.sort(row)
        planted.append((i, j))
    A = torch.zeros((n, d))
    B = torch.zeros((n, d))
    for i in range(n):
        A[i, a_rows[i]] = 1.0
        B[i, b_rows[i]] = 1.0
    inter = (A @ B.T).double()
    dist = 1.0 - inter / (2 * m - inter)
    ei, ej = torch.nonzero(dist <= 0.2, as_tuple=True)
    assert set(planted) <= set(zip(ei.tolist(), ej.tolist()))
    sa, sb = _csr(a_rows, d).to("cuda"), _csr(b_rows, d).to("cuda")
    ha = torch.stack([torch.ones(n), torch.arange(n) * 2.0 + 10], 1).double().reshape(n, 2, 1).cuda()
    hb = torch.stack([torch.ones(n), torch.arange(n) * 2.0 + 11], 1).double().reshape(n, 2, 1).cuda()
    lsh_ops.similarity_join(ha[:8], hb[:8], sa.slice(0, 8), sb.slice(0, 8), 0.2)  # (library and kernels loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ia, ib, got = lsh_ops.similarity_join(ha, hb, sa, sb, 0.2)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print("peak device memory above the inputs: %.1f MiB" % (grown / 2 ** 20))
    pairs = list(zip(ia.tolist(), ib.tolist()))
    assert set(planted) <= set(pairs)
    assert pairs == list(zip(ei.tolist(), ej.tolist()))
    assert got.cpu().tolist() == dist[ei, ej].tolist()
    assert grown <= 512 * 2 ** 20


# -------------------------------------------------------------------------------------- nearest
def test_nearest_matches_torch_path(monkeypatch):
    _need_gpu()
    rng = np.random.default_rng(4)
    d, n = 20000, 3000
    key = np.sort(rng.choice(d, size=40, replace=False))
    rows = _random_rows(rng, n, d, 5, 60)
    spare = np.setdiff1d(np.arange(d), key)[:5]
    for i in range(0, n, 3):       # a third of the rows: the key with its last element replaced → equal distances
        rows[i] = np.sort(np.concatenate([key[:-1], [spare[i % 5]]]))
    for i in range(1, n, 50):
        rows[i] = key.copy()       # distance 0
    sets, kset = _csr(rows, d).to("cuda"), _csr([key], d).to("cuda")
    T, F = 3, 2
    H = torch.from_numpy(rng.integers(100, 10 ** 6, (n, T, F)).astype(np.float64))
    kh = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)
    H[::2, 1] = kh[1]              # every second row shares table 1 with the key, …
    H[5::7, 2] = kh[2]             # … others table 2,
    H[4::9, 0, 0] = kh[0, 0]       # and half a match is none
    H, kh = H.cuda(), kh.cuda()
    cand = int((H == kh[None]).all(2).any(1).sum())
    assert cand > 1500
    for k in (1, 7, 400, cand, cand + 10):  # 400: inside the run of equal distances
        want = _torch_path(monkeypatch, lsh_ops.nearest, H, kh, sets, kset, k)
        with monkeypatch.context() as m:
            _no_torch_path(m)
            got = lsh_ops.nearest(H, kh, sets, kset, k)
        _same(got, want)
        assert got[0].numel() == min(k, cand)
    ties = _torch_path(monkeypatch, lsh_ops.nearest, H, kh, sets, kset, 401)[1]
    assert float(ties[399]) == float(ties[400])  # k = 400 cut through a tie
    # no candidates
    none = lsh_ops.nearest(H, kh + 0.5, sets, kset, 5)
    _same(none, _torch_path(monkeypatch, lsh_ops.nearest, H, kh + 0.5, sets, kset, 5))
    assert none[0].numel() == 0 and none[0].dtype == torch.int64 and none[1].dtype == torch.float64


def test_nearest_key_set_beyond_lds_staging(monkeypatch):
    """A key of 9,000 elements (the kernel stages up to 8,192 in LDS) is read from global memory."""
    _need_gpu()
    rng = np.random.default_rng(5)
    d, n = 30000, 500
    key = np.sort(rng.choice(d, size=9000, replace=False))
    rows = _random_rows(rng, n, d, 20, 400)
    rows[3] = key[:8192].copy()
    rows[4] = key.copy()
    sets, kset = _csr(rows, d).to("cuda"), _csr([key], d).to("cuda")
    H = torch.zeros((n, 2, 1), dtype=torch.float64)
    H[:, 1, 0] = torch.arange(n) % 2
    kh = torch.tensor([[9.0], [1.0]], dtype=torch.float64)
    H, kh = H.cuda(), kh.cuda()
    want = _torch_path(monkeypatch, lsh_ops.nearest, H, kh, sets, kset, 100)
    _no_torch_path(monkeypatch)
    got = lsh_ops.nearest(H, kh, sets, kset, 100)
    _same(got, want)
    assert got[0].numel() == 100 and got[0][0].item() == 3
    assert got[1][0].item() == 1.0 - 8192 / 9000
    # and a key that fits, on the same rows
    kset2 = _csr([key[:8192]], d).to("cuda")
    got2 = lsh_ops.nearest(H, kh, sets, kset2, 5)
    assert got2[0][0].item() == 3 and got2[1][0].item() == 0.0


# ---------------------------------------------------------------------------------------- stage
def _device_tables():
    a, b = _rand_sets(1, 900), _rand_sets(2, 700)
    return a, b, a.to("cuda"), b.to("cuda")


def test_stage_join_and_neighbours_on_device_tables(monkeypatch):
    _need_gpu()
    a, b, ad, bd = _device_tables()
    model = _lsh(4, 2).fit(a)
    ad = model.transform(ad)[0]  # device-resident hashes column
    bd = model.transform(bd)[0]
    key = Vectors.sparse(60, [3, 17, 30, 41], [1.0] * 4)
    want_join = _torch_path(monkeypatch, model.approx_similarity_join, ad, bd, 0.7, "id").rows()
    want_nn = _torch_path(monkeypatch, model.approx_nearest_neighbors, ad, key, 3).select("id", "distCol").rows()
    assert len(want_join) == 2863 and len(want_nn) == 3
    _no_torch_path(monkeypatch)
    join = model.approx_similarity_join(ad, bd, 0.7, "id")
    assert join.column_names == ["datasetA.id", "datasetB.id", "distCol"]
    assert join.rows() == want_join
    assert model.approx_nearest_neighbors(ad, key, 3).select("id", "distCol").rows() == want_nn


def _spmd_keyed_join(rank, world):
    from flink_ml_amd.ops import lsh as ops

    calls = []
    real = ops.pair_jaccard_torch
    ops.pair_jaccard_torch = lambda *a: calls.append(1) or real(*a)
    a, b = _rand_sets(1, 900), _rand_sets(2, 700)
    model = _lsh(4, 2).fit(a)
    join = model.approx_similarity_join(a.partition(rank, world), b.partition(rank, world), 0.7, "id")
    return join.rows(), len(calls)


def test_keyed_join_two_ranks_native_distances(monkeypatch):
    """The 2-rank keyed join, its distances now from the pair kernel, against the one-rank join of
    the torch formulation."""
    _need_gpu()
    from tests.spmd import run_spmd

    a, b, ad, bd = _device_tables()
    want = sorted(_torch_path(monkeypatch, _lsh(4, 2).fit(a).approx_similarity_join, ad, bd, 0.7, "id").rows())
    res = run_spmd(_spmd_keyed_join, 2, env={"FMLX_DEVICE": "cuda:0", "FMLX_XGMI": "0"}, timeout=300)
    assert sorted(r for rows, _ in res for r in rows) == want
    assert [c for _, c in res] == [0, 0]  # no rank computed its distances with the torch formulation


@pytest.mark.parametrize("n,cmax", [(0, 4), (1, 4), (2047, 4), (2048, 4), (2049, 4), (1024 * 2048 + 1, 4),
                                    (20_000, 1 << 20)])
def test_scan_tile_and_pass_edges(n, cmax):
    """fmlx_lsh_scan (int32 counts → int64 exclusive offsets) against torch.cumsum in int64: the
    2048-count tile edge, one tile past a full 1024-tile pass of the one-block scan of the tile
    sums, and counts up to 2^20 whose total exceeds 2^32; off[n] and the state word's total too."""
    _need_gpu()
    g = torch.Generator().manual_seed(n + cmax)
    cnt = torch.randint(0, cmax + 1, (n,), generator=g, dtype=torch.int32)
    want = torch.zeros(n + 1, dtype=torch.int64)
    want[1:] = torch.cumsum(cnt.long(), 0)
    if cmax > 4:
        assert int(want[n]) > 1 << 32
    st = torch.zeros(lsh_ops._ST_WORDS, dtype=torch.int64, device="cuda")
    off = lsh_ops._scan(cnt.cuda(), st)
    assert torch.equal(off.cpu(), want)
    assert int(st[lsh_ops._ST_TOTAL].item()) == int(want[n])
