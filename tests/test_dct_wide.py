"""The wide DCT path (ops/csrc/dct_wide.hip, rows of n > 128) without a GPU: the table conventions
of ``ops.dct.wide_tables`` — run through the kernel's algorithm with torch.fft in complex128 —
against a basis whose angles are reduced in integers, and the kernel library's size limits."""
import math
import os

import numpy as np
import pytest
import torch


def exact_basis(n: int) -> torch.Tensor:
    """Orthonormal DCT-II basis M [n, n] (rows = frequencies), fp64, cos(π(2i+1)k/(2n)) with the
    angle reduced exactly: q = (2i+1)·k mod 4n is folded into [0, n] with its sign, so cos sees
    arguments in [0, π/2] only (``dct_matrix`` feeds it up to ≈ πn)."""
    k = torch.arange(n, dtype=torch.int64)[:, None]
    i = torch.arange(n, dtype=torch.int64)[None, :]
    q = ((2 * i + 1) * k) % (4 * n)  # angle πq/(2n), period 4n
    q = torch.where(q > 2 * n, 4 * n - q, q)  # cos(2π − a) = cos a: q in [0, 2n]
    neg = q > n  # cos(π − a) = −cos a: q in [0, n]
    q = torch.where(neg, 2 * n - q, q)
    m = torch.cos(math.pi * q.to(torch.float64) / (2 * n))
    m = torch.where(neg, -m, m)
    m[0] *= math.sqrt(1.0 / n)
    m[1:] *= math.sqrt(2.0 / n)
    return m


def basis_product(X: torch.Tensor, n: int, inverse: bool) -> torch.Tensor:
    """X @ exact_basis(n).T (forward) or X @ exact_basis(n) (inverse), accumulated in extended
    precision and rounded once to fp64. A plain fp64 matmul carries its own summation error of
    about √n·eps·Σ|terms| in an order that depends on the BLAS and its threads: on the all-ones row
    at n = 2047 (y[0] = √n) that alone reaches 5 to 16 of the 16 units the fp64 kernel is allowed."""
    M = exact_basis(n).numpy().astype(np.longdouble)
    out = X.to(torch.float64).numpy().astype(np.longdouble) @ (M if inverse else M.T)
    return torch.from_numpy(out.astype(np.float64))


def _dft(v: torch.Tensor, t: dict, n: int, sign: int) -> torch.Tensor:
    """Σ_j v_j e^{sign·2πijk/n} of every row through the tables: one FFT of length L = n, or the
    chirp convolution over L ≥ 2n − 1 (FFT_L, times B, inverse FFT_L without its 1/L)."""
    L = t["L"]
    if L == n:
        return torch.fft.fft(v) if sign < 0 else torch.fft.ifft(v) * n
    a = torch.zeros(v.shape[0], L, dtype=torch.complex128)
    a[:, :n] = v * t["w"]
    c = torch.fft.ifft(torch.fft.fft(a) * t["B"]) * L
    return c[:, :n] * t["w"]


def fft_dct(X: torch.Tensor, inverse: bool) -> torch.Tensor:
    """The kernel's algorithm on the host in complex128, every factor from ``wide_tables``."""
    from flink_ml_amd.ops.dct import wide_tables

    rows, n = X.shape
    t = wide_tables(n, inverse, torch.float64)
    h = (n + 1) // 2
    X = X.to(torch.float64)
    if not inverse:
        v = torch.empty_like(X)
        v[:, :h] = X[:, 0::2]
        v[:, h:] = X[:, 1::2].flip(1)
        V = _dft(v.to(torch.complex128), t, n, -1)
        return (t["mk"] * V).real
    ym = torch.zeros_like(X)
    ym[:, 1:] = X[:, 1:].flip(1)  # y[n − k], y[n] = 0
    W = t["mk"] * torch.complex(X, -ym)
    v = _dft(W, t, n, +1).real
    out = torch.empty_like(X)
    out[:, 0::2] = v[:, :h]
    out[:, 1::2] = v[:, h:].flip(1)
    return out


@pytest.mark.parametrize("n", [129, 255, 256, 257, 1000, 2048])
@pytest.mark.parametrize("inverse", [False, True])
def test_wide_tables_give_the_dct(n, inverse):
    g = torch.Generator().manual_seed(n)
    X = torch.rand((8, n), generator=g, dtype=torch.float64) * 2 - 1
    ref = basis_product(X, n, inverse)
    got = fft_dct(X, inverse)
    bound = 2.0 ** -53 * 16 * math.log2(n) * X.norm(dim=1, keepdim=True)
    err = (got - ref).abs()
    print("n=%d inverse=%s max err %.3g (bound %.3g)" % (n, inverse, float(err.max()), float(bound.min())))
    assert bool((err <= bound).all()), float(err.max())


def test_wide_tables_are_linear_in_size():
    from flink_ml_amd.ops.dct import wide_fft_len, wide_tables

    t = wide_tables(1000, False, torch.float32)
    assert t["L"] == wide_fft_len(1000) == 2048
    assert t["roots"].shape == (1024,) and t["mk"].shape == (1000,) and t["w"].shape == (1000,)
    assert t["B"].shape == (2048,)
    t = wide_tables(2048, True, torch.float32)
    assert t["L"] == 2048 and t["w"] is None and t["B"] is None
    assert wide_fft_len(129) == 512 and wide_fft_len(8191) == 16384 and wide_fft_len(4097) == 16384


def test_exact_basis_is_orthonormal_and_matches_dct_matrix():
    from flink_ml_amd.ops.dct import dct_matrix

    M = exact_basis(257)
    assert float((M @ M.t() - torch.eye(257, dtype=torch.float64)).abs().max()) < 1e-14
    assert float((exact_basis(100) - dct_matrix(100)).abs().max()) < 1e-13


LIMITS = [(torch.float32, 128, False), (torch.float32, 129, True), (torch.float32, 8191, True),
          (torch.float32, 8192, True), (torch.float32, 8193, False), (torch.float32, 16384, True),
          (torch.float32, 16385, False), (torch.float64, 128, False), (torch.float64, 129, True),
          (torch.float64, 4095, True), (torch.float64, 4096, True), (torch.float64, 4097, False),
          (torch.float64, 8192, True), (torch.float64, 8193, False)]


@pytest.mark.parametrize("dtype,n,ok", LIMITS)
def test_wide_limits(dtype, n, ok):
    from flink_ml_amd.ops import dct as dk
    from flink_ml_amd.ops import native

    if not os.path.exists(native.kernel_lib_path()):
        pytest.skip("kernel library not built")
    assert dk.dct_wide_supported(n, dtype) is ok
    if ok:
        assert dk._wide_len(n, dtype) == dk.wide_fft_len(n)
    assert not dk.dct_wide_supported(n, torch.bfloat16)
