"""KMeans on CSR feature columns: the fp64 host references and the sparse row sample (CPU)."""
import numpy as np
import pytest
import torch

from flink_ml_amd.models.kmeans import sample_rows
from flink_ml_amd.ops import kmeans as kk
from flink_ml_amd.table import SparseColumn

N, D, K = 500, 300, 7
METRICS = ["euclidean", "manhattan", "cosine"]


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    X = torch.randn(N, D, generator=g, dtype=torch.float64)
    X = X * (torch.rand(N, D, generator=g) < 0.05)
    X[::37] = 0.0  # empty rows
    C = torch.randn(K, D, generator=g, dtype=torch.float64) * 0.3
    return X, SparseColumn.from_dense(X), C


@pytest.mark.parametrize("metric", METRICS)
def test_torch_assign_csr_equals_dense(data, metric):
    X, S, C = data
    assert int((S.indptr[1:] == S.indptr[:-1]).sum()) >= N // 37
    assert torch.equal(kk.torch_assign_csr(S, C, metric), kk.torch_assign(X, C, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_torch_round_payload_csr_equals_dense(data, metric):
    X, S, C = data
    got, want = kk.torch_round_payload_csr(S, C, metric), kk.torch_round_payload(X, C, metric)
    assert got.shape == (K * D + K,)
    assert torch.equal(got[K * D:], want[K * D:])
    torch.testing.assert_close(got[: K * D], want[: K * D], rtol=1e-12, atol=1e-12)


def test_torch_round_payload_csr_given_labels(data):
    X, S, C = data
    lab = torch.arange(N) % (K + 1) - 1  # -1 .. K-1: the -1 rows add nothing
    got = kk.torch_round_payload_csr(S, C, "euclidean", labels=lab)
    ok = lab >= 0
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, lab[ok], X[ok])
    torch.testing.assert_close(got[: K * D].reshape(K, D), sums, rtol=1e-12, atol=1e-12)
    assert torch.equal(got[K * D:], torch.bincount(lab[ok], minlength=K).double())


def test_sample_rows_sparse_equals_dense(data):
    X, S, _ = data
    for k, seed in ((K, 3), (N + 5, 9)):
        assert np.array_equal(sample_rows(S, k, seed), sample_rows(X, k, seed))


def test_csr_kp():
    assert [kk.csr_kp(k) for k in (1, 2, 7, 10, 64, 65, 70, 257, 1024)] == [1, 2, 8, 16, 64, 128, 128, 512, 1024]
    for k in (1, 10, 64, 70, 257, 1024):
        kp = kk.csr_kp(k)
        assert kp >= k and ((kp <= 64 and kp & (kp - 1) == 0) or kp % 64 == 0)


def test_csr_route_off_without_gpu(data):
    _, S, _ = data
    assert not kk.csr_supported(S, K, torch.device("cpu"))
    assert not kk.csr_route(S, K, torch.device("cpu"))
