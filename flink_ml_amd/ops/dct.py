"""Row-wise orthonormal DCT-II / DCT-III on the f32 MFMA (``csrc/dct.hip``): the
even/odd butterfly splits the n × n product into two ⌈n/2⌉-sized ones (rows of n ≤ 128), and on an
LDS-resident FFT for wider rows (``csrc/dct_wide.hip``: ``dct_rows_wide``, O(n log n) per row)."""
from __future__ import annotations

import ctypes
import functools
import math

import torch

from . import native


def set_diag(diag: int = 0, per_cu: int = 0) -> None:
    """Diagnostics of the kernel's pipeline (1: skip the MFMAs, 2: skip the tile loads, 4: skip the
    stores; per_cu: cap on blocks per CU). Results are wrong while diag != 0."""
    native.kernels().fmlx_dct_set_diag(int(diag), int(per_cu))


MAX_N = 128


@functools.lru_cache(maxsize=32)
def dct_matrix(n: int) -> torch.Tensor:
    """Orthonormal DCT-II basis M [n, n] (rows = frequencies), fp64 on the host."""
    k = torch.arange(n, dtype=torch.float64)[:, None]
    i = torch.arange(n, dtype=torch.float64)[None, :]
    m = torch.cos(math.pi * (2 * i + 1) * k / (2 * n))
    m[0] *= math.sqrt(1.0 / n)
    m[1:] *= math.sqrt(2.0 / n)
    return m


@functools.lru_cache(maxsize=64)
def _padded_basis(n: int, inverse: bool, device: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Both half bases of the even/odd butterfly as the kernel reads its MFMA B fragments:
    [2][KP/4][4][16][nt8], element [p][q][hh][r][c] = B_p[4q + hh][16c + r] with B_p[kk][o] =
    M[2o + p][kk] (forward: k' = o, i = kk) or M[2kk + p][o] (inverse: k' = kk, i = o)."""
    kp, nt8 = ctypes.c_int(), ctypes.c_int()
    if native.kernels().fmlx_dct_basis_shape(n, ctypes.byref(kp), ctypes.byref(nt8)) != 0:
        raise ValueError("DCT size %d outside 1..%d" % (n, MAX_N))
    M = dct_matrix(n)
    KP, NT8 = kp.value, nt8.value
    h = (n + 1) // 2
    halves = []
    for p in (0, 1):
        rows = M[p::2, :h]  # M[2k' + p][i], i < h
        B = rows.t() if not inverse else rows  # forward: [i][k'];  inverse: [k'][i]
        P = torch.zeros((KP, 16 * NT8), dtype=dtype)
        P[:B.shape[0], :B.shape[1]] = B.to(dtype)
        halves.append(P.reshape(KP // 4, 4, NT8, 16).permute(0, 1, 3, 2).contiguous())
    return torch.stack(halves).contiguous().to(device)


def dct_rows(X: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """DCT of every row of a CUDA f32 or f64 matrix [rows, n ≤ 128] (exact-f32 / f64 MFMA; one
    read and one write of the rows)."""
    rows, n = X.shape
    X = X.contiguous()
    Y = torch.empty_like(X)
    f64 = X.dtype == torch.float64
    B = _padded_basis(n, bool(inverse), str(X.device), torch.float64 if f64 else torch.float32)
    cus = torch.cuda.get_device_properties(X.device).multi_processor_count
    native.call("fmlx_dct_rows_f64" if f64 else "fmlx_dct_rows", native.ptr(X), rows, n, native.ptr(B), native.ptr(Y),
                int(bool(inverse)), cus, native.stream_ptr(X.device))
    return Y


# ------------------------------------------------------------------------------ rows wider than 128
# ``csrc/dct_wide.hip``: Makhoul's DCT through one complex DFT_n per row, all in LDS. A power-of-two
# n is one FFT of length L = n; any other n is Bluestein's chirp convolution over the power of two
# L ≥ 2n − 1. The kernel computes no sin / cos: every factor comes from the tables below.
def _wide_len(n: int, dtype: torch.dtype):
    """FFT length of the wide kernel for rows of n, or None outside its range (the limits live in
    the kernel library alone: fmlx_dct_wide_len)."""
    if dtype not in (torch.float32, torch.float64):
        return None
    L = ctypes.c_int()
    if native.kernels().fmlx_dct_wide_len(int(n), int(dtype == torch.float64), ctypes.byref(L)) != 0:
        return None
    return L.value


def dct_wide_supported(n: int, dtype: torch.dtype = torch.float32) -> bool:
    """Whether ``dct_rows_wide`` takes rows of n values of ``dtype`` (f32 / f64): 128 < n, and a
    row's FFT fits the LDS — n ≤ 16384 (f32) / 8192 (f64) for a power of two, n ≤ 8191 / 4095 else."""
    return _wide_len(n, dtype) is not None


def wide_fft_len(n: int) -> int:
    """L: n itself for a power of two, else the smallest power of two ≥ 2n − 1 (Bluestein)."""
    return n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()


def _unit(num: torch.Tensor, den: int) -> torch.Tensor:
    """e^{iπ·num/den} for an int64 tensor ``num``, complex128: the angle is reduced in integers
    (mod 2·den) and folded into the first octant, so cos / sin only see arguments in [0, π/4]."""
    q = torch.remainder(num, 2 * den)  # angle πq/den, q in [0, 2·den)
    quad = torch.div(4 * q, 2 * den, rounding_mode="floor")  # quarter turn 0..3
    r = 2 * q - quad * den  # angle within the quarter: π r / (2 den), r in [0, den)
    swap = 2 * r > den  # above π/4: mirror about π/4
    rr = torch.where(swap, den - r, r).to(torch.float64)
    c, s = torch.cos(math.pi * rr / (2 * den)), torch.sin(math.pi * rr / (2 * den))
    c, s = torch.where(swap, s, c), torch.where(swap, c, s)
    re = torch.where(quad == 0, c, torch.where(quad == 1, -s, torch.where(quad == 2, -c, s)))
    im = torch.where(quad == 0, s, torch.where(quad == 1, c, torch.where(quad == 2, -s, -c)))
    return torch.complex(re, im)


@functools.lru_cache(maxsize=16)
def wide_tables(n: int, inverse: bool = False, dtype: torch.dtype = torch.float64) -> dict:
    """The wide kernel's tables for rows of n, on the host in complex128 (``dtype`` is the row
    type they will be rounded to; the fp64 values do not depend on it). With h = ⌈n/2⌉,
    v[i] = x[2i], v[n−1−i] = x[2i+1], V = DFT_n(v), s_0 = √(1/n), s_k = √(2/n):

    * ``L``      FFT length (``wide_fft_len``)
    * ``roots``  [L/2]  e^{−2πij/L}
    * ``mk``     [n]    forward: s_k e^{−iπk/(2n)}, y[k] = Re(mk[k]·V[k]);
                        inverse: mk[0] = s_0, mk[k] = ½ s_k e^{+iπk/(2n)}, W[k] = mk[k]·(y[k] − i·y[n−k])
                        with y[n] = 0, and v[j] = Re Σ_k W[k] e^{+2πijk/n}
    * ``w``      [n]    Bluestein chirp e^{∓iπ(j² mod 2n)/n} (− forward, + inverse); None when L == n
    * ``B``      [L]    FFT_L(b)/L in natural order, b_j = b_{L−j} = conj(w_j) for j < n, else 0:
                        DFT_n(v)_k = w_k · Σ_p FFT_L(v∘w)_p B_p e^{+2πipk/L}; None when L == n
    """
    del dtype
    n = int(n)
    L = wide_fft_len(n)
    sgn = 1 if inverse else -1
    k = torch.arange(n, dtype=torch.int64)
    roots = _unit(-2 * torch.arange(L // 2, dtype=torch.int64), L)
    mk = _unit(sgn * k, 2 * n) * math.sqrt(2.0 / n)
    if inverse:
        mk = mk * 0.5
    mk[0] = math.sqrt(1.0 / n)
    w = B = None
    if L != n:
        w = _unit(sgn * ((k * k) % (2 * n)), n)
        b = torch.zeros(L, dtype=torch.complex128)
        b[:n] = w.conj()
        b[L - n + 1:] = w.conj()[1:].flip(0)
        B = torch.fft.fft(b) / L
    return {"L": L, "roots": roots, "mk": mk, "w": w, "B": B}


def _bit_reverse(L: int) -> torch.Tensor:
    bits = L.bit_length() - 1
    i = torch.arange(L, dtype=torch.int64)
    r = torch.zeros_like(i)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


@functools.lru_cache(maxsize=32)
def _wide_device_tables(n: int, inverse: bool, dtype: torch.dtype, device: str):
    """``wide_tables`` rounded once to the row type and uploaded as interleaved (re, im) pairs; B
    in the bit-reversed order in which the kernel's first FFT leaves the spectrum. O(L) in all."""
    t = wide_tables(n, inverse, dtype)

    def up(z):
        return None if z is None else torch.view_as_real(z).to(dtype).contiguous().to(device)

    B = t["B"]
    return up(t["roots"]), up(t["mk"]), up(t["w"]), up(None if B is None else B[_bit_reverse(t["L"])])


def dct_rows_wide(X: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """DCT-II (DCT-III: ``inverse``) of every row of a CUDA f32 or f64 matrix [rows, n] with
    ``dct_wide_supported(n, X.dtype)``: O(n log n) per row, one read and one write of the rows,
    one kernel, tables of O(n). Raises ValueError for any other n or dtype."""
    rows, n = X.shape
    if not dct_wide_supported(n, X.dtype):
        raise ValueError("DCT size %d (%s) outside the wide kernel's range" % (n, X.dtype))
    X = X.contiguous()
    Y = torch.empty_like(X)
    if rows == 0:
        return Y
    f64 = X.dtype == torch.float64
    roots, mk, w, B = _wide_device_tables(n, bool(inverse), X.dtype, str(X.device))
    cus = torch.cuda.get_device_properties(X.device).multi_processor_count
    native.call("fmlx_dct_wide_rows_f64" if f64 else "fmlx_dct_wide_rows", native.ptr(X), rows, n, native.ptr(roots),
                native.ptr(mk), native.ptr(w), native.ptr(B), native.ptr(Y), int(bool(inverse)), cus,
                native.stream_ptr(X.device))
    return Y
