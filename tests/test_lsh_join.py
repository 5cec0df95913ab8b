"""The MinHashLSH search ops (ops/lsh.py similarity_join / pair_jaccard / nearest) on CPU tensors:
what the stage returned before they existed, a plain numpy reference, and the input that keeps
the torch formulation (unsorted set rows, −0.0 signatures)."""
import hashlib

import numpy as np
import pytest
import torch

from flink_ml_amd import Vectors
from flink_ml_amd.ops import lsh as lsh_ops
from flink_ml_amd.table import SparseColumn
from tests.test_feature_lsh import _lsh, _rand_sets

# approx_similarity_join(a, b, 0.7, "id").rows() and approx_nearest_neighbors(a, KEY, 25) of the
# commit before the ops existed, on the inputs of _case(): row count, sha256 of repr(rows)
JOIN_BEFORE = (2863, "9ff07f5f25a23e10103138e010685fce65c8ce03de9570d436afaa2b4b6c0cf8")
NN_BEFORE = (5, "e9f4b50bd3d378760ea8afd2618644f0aff7515a11cc6e94b0e4a212c4d37a19")
KEY = [3, 17, 30, 41]


def _digest(rows):
    return len(rows), hashlib.sha256(repr(rows).encode()).hexdigest()


@pytest.fixture(scope="module")
def case():
    a, b = _rand_sets(1, 900), _rand_sets(2, 700)
    model = _lsh(4, 2).fit(a)
    sa = SparseColumn.from_vectors(a.get_list("vec"), 60)
    sb = SparseColumn.from_vectors(b.get_list("vec"), 60)
    return a, b, model, sa, sb, model.hash_function(sa), model.hash_function(sb)


def _row(s: SparseColumn, i: int) -> np.ndarray:
    return s.indices[int(s.indptr[i]):int(s.indptr[i + 1])].numpy()


def ref_join(ha, hb, sa, sb, threshold):
    """Per-table signature equality → set of pairs → jaccard_distance, in ascending (ia, ib)."""
    pairs = set()
    for t in range(ha.shape[1]):
        buckets = {}
        for j in range(hb.shape[0]):
            buckets.setdefault(tuple(hb[j, t].tolist()), []).append(j)
        for i in range(ha.shape[0]):
            pairs.update((i, j) for j in buckets.get(tuple(ha[i, t].tolist()), ()))
    out = [(i, j, lsh_ops.jaccard_distance(_row(sa, i), _row(sb, j))) for i, j in sorted(pairs)]
    return [r for r in out if r[2] <= threshold]


def ref_nearest(H, kh, sets, kset, k):
    rows = [i for i in range(H.shape[0]) if any(H[i, t].tolist() == kh[t].tolist() for t in range(H.shape[1]))]
    d = [(lsh_ops.jaccard_distance(_row(kset, 0), _row(sets, i)), i) for i in rows]
    return [(i, x) for x, i in sorted(d)[:k]]


def _key_set(dev="cpu"):
    return SparseColumn(torch.tensor([0, len(KEY)]), torch.tensor(KEY, dtype=torch.int32),
                        torch.ones(len(KEY), dtype=torch.float64), 60).to(dev)


def test_ops_return_what_the_stage_returned(case):
    a, b, model, sa, sb, ha, hb = case
    ia, ib, dist = lsh_ops.similarity_join(ha, hb, sa, sb, 0.7)
    assert ia.dtype == torch.int64 and ib.dtype == torch.int64 and dist.dtype == torch.float64
    ids_a, ids_b = a.get_list("id"), b.get_list("id")
    rows = [(ids_a[i], ids_b[j], d) for i, j, d in zip(ia.tolist(), ib.tolist(), dist.tolist())]
    assert _digest(rows) == JOIN_BEFORE
    assert _digest(model.approx_similarity_join(a, b, 0.7, "id").rows()) == JOIN_BEFORE
    # the pairs' distances again, from pair_jaccard
    assert torch.equal(lsh_ops.pair_jaccard(sa, sb, ia, ib), dist)
    kset = _key_set()
    idx, nd = lsh_ops.nearest(ha, model.hash_function(kset)[0], sa, kset, 25)
    assert idx.dtype == torch.int64 and nd.dtype == torch.float64
    assert _digest([(ids_a[i], d) for i, d in zip(idx.tolist(), nd.tolist())]) == NN_BEFORE
    nn = model.approx_nearest_neighbors(a, Vectors.sparse(60, KEY, [1.0] * 4), 25).select("id", "distCol").rows()
    assert _digest(nn) == NN_BEFORE


def test_ops_match_numpy_reference(case):
    _, _, model, sa, sb, ha, hb = case
    ref = ref_join(ha, hb, sa, sb, 1.0)
    assert len(ref) > 3000
    for threshold in (0.0, 0.5, 0.7, 1.0):
        ia, ib, dist = lsh_ops.similarity_join(ha, hb, sa, sb, threshold)
        assert list(zip(ia.tolist(), ib.tolist(), dist.tolist())) == [r for r in ref if r[2] <= threshold]
    g = torch.Generator().manual_seed(3)
    ia, ib = torch.randint(0, 900, (500,), generator=g), torch.randint(0, 700, (500,), generator=g)
    want = [lsh_ops.jaccard_distance(_row(sa, i), _row(sb, j)) for i, j in zip(ia.tolist(), ib.tolist())]
    assert lsh_ops.pair_jaccard(sa, sb, ia, ib).tolist() == want
    assert lsh_ops.pair_jaccard(sa, sb, ia[:0], ib[:0]).shape == (0,)
    kset = _key_set()
    kh = model.hash_function(kset)[0]
    for k in (1, 3, 25):
        idx, nd = lsh_ops.nearest(ha, kh, sa, kset, k)
        assert list(zip(idx.tolist(), nd.tolist())) == ref_nearest(ha, kh, sa, kset, k)


def _reversed_row(s: SparseColumn, i: int) -> SparseColumn:
    ind = s.indices.clone()
    lo, hi = int(s.indptr[i]), int(s.indptr[i + 1])
    ind[lo:hi] = torch.flip(ind[lo:hi], [0])
    return SparseColumn(s.indptr, ind, s.values, s.size)


def test_unsorted_rows_and_negative_zero_keep_the_torch_path(case):
    _, _, model, sa, sb, ha, hb = case
    longest = int(torch.argmax(sa.indptr[1:] - sa.indptr[:-1]))
    sa_u = _reversed_row(sa, longest)
    assert not torch.equal(sa_u.indices, sa.indices)
    want = lsh_ops.similarity_join_torch(ha, hb, sa, sb, 0.7)
    got = lsh_ops.similarity_join(ha, hb, sa_u, sb, 0.7)  # the same sets, one row listed backwards
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert longest in got[0].tolist()
    # −0.0 == 0.0: rows whose signatures differ only in the zero's sign share a bucket
    ha0, hb0, sa0, sb0 = ha[:150].clone(), hb[:100].clone(), sa.slice(0, 150), sb.slice(0, 100)
    ha0[:, 0, :] = 0.0
    hb0[:, 0, :] = -0.0
    want = ref_join(ha0, hb0, sa0, sb0, 1.0)
    assert len(want) == 150 * 100  # table 0 alone pairs every row with every row
    got = lsh_ops.similarity_join(ha0, hb0, sa0, sb0, 1.0)
    assert list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist())) == want
    assert all(torch.equal(x, y) for x, y in zip(got, lsh_ops.similarity_join_torch(ha0, hb0, sa0, sb0, 1.0)))
    ha0 = ha.clone()
    kset = _key_set()
    kh = model.hash_function(kset)[0].clone()
    kh[1, :] = -0.0
    ha0[:, 1, :] = 0.0
    got = lsh_ops.nearest(ha0, kh, sa_u, kset, 40)
    assert list(zip(got[0].tolist(), got[1].tolist())) == ref_nearest(ha0, kh, sa, kset, 40)
    assert len(got[0]) == 40
