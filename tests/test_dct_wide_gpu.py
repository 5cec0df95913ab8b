"""The FFT-based DCT kernel for rows wider than 128 (ops/csrc/dct_wide.hip) on the device, against
the product with the exactly reduced fp64 basis of tests/test_dct_wide.py, accumulated in extended
precision (n ≤ 2048), or the complex128 torch.fft form that test validates against it (wider rows:
no 512 MiB basis here).

Per row: max_k |got − ref| ≤ C · eps · log2(L) · ‖x_row‖₂ with L the kernel's FFT length, eps the
row type's unit roundoff, C = 0.5 (f32) / 16 (f64), and C = 1 for inverse(forward(x)) against x —
4× the worst a host prototype of the same algorithm reached on these inputs."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_dct_wide import basis_product, exact_basis, fft_dct

pytestmark = pytest.mark.gpu

EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
C_ONE_WAY = {torch.float32: 0.5, torch.float64: 16.0}
C_ROUND_TRIP = 1.0

F32_SHAPES = [(257, 129), (1000, 256), (3000, 130), (37, 1000), (64, 1023), (5, 2048), (9, 4097), (3, 8191),
              (2, 16384)]
F64_SHAPES = [(257, 129), (500, 256), (37, 1000), (5, 2047), (3, 4095), (2, 8192)]
CASES = [(torch.float32, r, n) for r, n in F32_SHAPES] + [(torch.float64, r, n) for r, n in F64_SHAPES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _basis(n):
    return exact_basis(n)


def _rows(rows, n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed * 1_000_003 + rows * 131 + n)
    X = (torch.rand((rows, n), generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    if rows > 0:
        X[0] = 0
        X[0, n - 1] = 1  # impulse at the last index
    if rows > 1:
        X[1] = 1
    return X


def _reference(X, inverse):
    n = X.shape[1]
    if n <= 2048:
        return basis_product(X, n, inverse)
    return fft_dct(X.double(), inverse)


def _fft_len(n, dtype):
    from flink_ml_amd.ops import native

    L = ctypes.c_int()
    assert native.kernels().fmlx_dct_wide_len(n, int(dtype == torch.float64), ctypes.byref(L)) == 0
    return L.value


def _check(got, ref, X, dtype, C, what):
    L = _fft_len(X.shape[1], dtype)
    bound = C * EPS[dtype] * math.log2(L) * X.double().norm(dim=1)
    err = (got.double().cpu() - ref).abs().max(dim=1).values
    ratio = float((err / bound).max())
    print("%s %s %s L=%d: worst err/bound %.3f (err %.3g)" % (what, tuple(X.shape), dtype, L, ratio, float(err.max())))
    assert bool((err <= bound).all()), (what, ratio)


@pytest.mark.parametrize("dtype,rows,n", CASES)
@pytest.mark.parametrize("inverse", [False, True])
def test_dct_rows_wide_matches_exact_reference(dtype, rows, n, inverse):
    _need_gpu()
    from flink_ml_amd.ops.dct import dct_rows_wide

    X = _rows(rows, n, dtype)
    got = dct_rows_wide(X.cuda(), inverse)
    assert got.dtype == dtype and got.shape == X.shape
    _check(got, _reference(X, inverse), X, dtype, C_ONE_WAY[dtype], "inverse" if inverse else "forward")


@pytest.mark.parametrize("dtype,rows,n", CASES)
def test_dct_rows_wide_round_trip(dtype, rows, n):
    _need_gpu()
    from flink_ml_amd.ops.dct import dct_rows_wide

    X = _rows(rows, n, dtype)
    back = dct_rows_wide(dct_rows_wide(X.cuda(), False), True)
    _check(back, X.double(), X, dtype, C_ROUND_TRIP, "round trip")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_dct_rows_wide_non_contiguous_view(dtype):
    _need_gpu()
    from flink_ml_amd.ops.dct import dct_rows_wide

    X = _rows(33, 600, dtype).cuda()
    view = X[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(dct_rows_wide(view), dct_rows_wide(view.contiguous()))
    assert torch.equal(dct_rows_wide(view, True), dct_rows_wide(view.contiguous(), True))


def test_dct_rows_wide_empty_and_unsupported():
    _need_gpu()
    from flink_ml_amd.ops.dct import dct_rows_wide

    out = dct_rows_wide(torch.empty((0, 300), dtype=torch.float32, device="cuda"))
    assert out.shape == (0, 300) and out.dtype == torch.float32
    for n, dtype in [(128, torch.float32), (8193, torch.float32), (4097, torch.float64)]:
        with pytest.raises(ValueError):
            dct_rows_wide(torch.zeros((2, n), dtype=dtype, device="cuda"))


def _stage(X, inverse=False):
    from flink_ml_amd import Table
    from flink_ml_amd.models import DCT

    return DCT().set_inverse(inverse).set_input_col("i").set_output_col("o").transform(
        Table({"i": X}, num_rows=X.shape[0]))[0].column("o")


class _Spy:
    """Counts the calls of ops.dct.<name> while active (the stage looks the function up there)."""

    def __init__(self, name):
        self.name, self.calls = name, []

    def __enter__(self):
        from flink_ml_amd.ops import dct as dk

        self.real = getattr(dk, self.name)
        setattr(dk, self.name, lambda X, inv=False: self.calls.append((X.dtype, tuple(X.shape))) or self.real(X, inv))
        return self

    def __exit__(self, *exc):
        from flink_ml_amd.ops import dct as dk

        setattr(dk, self.name, self.real)


def test_dct_stage_takes_the_wide_kernel_without_a_basis():
    _need_gpu()
    X = _rows(64, 4096, torch.float32)
    Xd = X.cuda()
    _stage(_rows(4, 4096, torch.float32, seed=1).cuda())  # (tables cached, library loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with _Spy("dct_rows_wide") as spy:
        out = _stage(Xd)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert spy.calls == [(torch.float32, (64, 4096))]
    _check(out, _reference(X, False), X, torch.float32, C_ONE_WAY[torch.float32], "stage")
    assert grown < 8 << 20, grown  # (the 4096 × 4096 f32 basis alone is 64 MiB)


def test_dct_stage_cold_call_allocates_no_basis():
    """The same bound on a first call of a size: building and uploading its tables included."""
    _need_gpu()
    from flink_ml_amd.ops import dct as dk

    Xd = _rows(64, 4096, torch.float32, seed=2).cuda()
    _stage(_rows(4, 1024, torch.float32).cuda())  # (library loaded; another size)
    dk._wide_device_tables.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    _stage(Xd)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 8 << 20


def test_dct_stage_unsupported_size_keeps_the_gemm():
    _need_gpu()
    X = _rows(4, 8193, torch.float32)
    with _Spy("dct_rows_wide") as wide, _Spy("dct_rows") as narrow:
        out = _stage(X.cuda())
    assert wide.calls == [] and narrow.calls == []
    np.testing.assert_allclose(out.double().cpu().numpy(), fft_dct(X.double(), False).numpy(), atol=1e-4)


def test_dct_stage_narrow_rows_keep_the_mfma_kernel():
    _need_gpu()
    X = _rows(100, 128, torch.float32)
    with _Spy("dct_rows_wide") as wide, _Spy("dct_rows") as narrow:
        out = _stage(X.cuda())
    assert wide.calls == [] and narrow.calls == [(torch.float32, (100, 128))]
    np.testing.assert_allclose(out.double().cpu().numpy(), (X.double() @ _basis(128).t()).numpy(), atol=1e-5)
