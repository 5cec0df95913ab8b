// DCT-II / DCT-III of rows wider than 128 in O(n log n) (reference LIB/feature/dct/DCT.java:103-123:
// JTransforms DoubleDCT_1D transforms a row of any length): an FFT-based transform whose whole
// working set is one row in LDS. A row is read from HBM once, transformed in LDS and written
// once; no n × n basis exists anywhere (csrc/dct.hip keeps the n ≤ 128 MFMA product).
//
// Makhoul: with v[i] = x[2i], v[n−1−i] = x[2i+1] and V = DFT_n(v),
//   forward   y[k] = Re(mk[k] · V[k]),                      mk[k] = s_k e^{−iπk/(2n)}
//   inverse   W[k] = mk[k] · (y[k] − i·y[n−k])  (y[n] = 0),  mk[0] = s_0, mk[k] = ½ s_k e^{+iπk/(2n)}
//             v[j] = Re Σ_k W[k] e^{+2πijk/n},  x[2i] = v[i], x[2i+1] = v[n−1−i]
// (s_0 = √(1/n), s_k = √(2/n): the orthonormal scaling of ops/dct.py dct_matrix).
//
// DFT_n, n a power of two: one in-place decimation-in-frequency FFT of length L = n; its result
// is left in bit-reversed order and the read-out looks V[k] up at position rev(k).
// Any other n (Bluestein): L = the power of two ≥ 2n−1, chirp w_j = e^{∓iπ(j² mod 2n)/n},
//   a_j = v_j w_j (zero-padded), c = IFFT_L(FFT_L(a) ∘ B), V_k = c_k w_k, B = FFT_L(conj chirp)/L:
// the forward FFT is the same DIF (bit-reversed result), B is stored bit-reversed, and the inverse
// FFT is a decimation-in-time FFT that takes bit-reversed input, so nothing is ever permuted.
//
// Every pass fuses up to four radix-2 stages (radix 16): a thread holds the 2^r points that those
// stages couple, so a pass reads and writes the same LDS cells and passes need one barrier between
// them and no second buffer. Every twiddle is read from the host-built tables (fp64, rounded once
// to the row type): roots e^{−2πij/L} (j < L/2), mk, w, B — no device sin/cos.
//
// LDS: complex cells, one pad cell after every 32 (f32) / 16 (f64) cells — one pad per 256-byte
// bank row — so the stride-2^k accesses of the late DIF / early DIT passes and the bit-reversed
// read-out spread over the banks. Workgroups of 256 threads transform G rows at a time (G·L ≈ 4096
// cells in f32, 2048 in f64: 32 KiB), one row per workgroup from there up to the 128 KiB limit.
#include "common.h"

namespace {

constexpr int DW_THREADS = 256;

template <typename T> struct DwT;
template <> struct DwT<float> {
  typedef float2 c2;
  typedef float4 vec;                   // 16-byte global access
  static constexpr int VW = 4;          // elements per 16 bytes
  static constexpr int PS = 5;          // one pad cell per 2^PS cells (256 bytes)
  static constexpr int GROUP_CELLS = 4096;
  static constexpr int MAX_LOGL = 14;   // L · 8 bytes ≤ 128 KiB
};
template <> struct DwT<double> {
  typedef double2 c2;
  typedef double2 vec;
  static constexpr int VW = 2;
  static constexpr int PS = 4;
  static constexpr int GROUP_CELLS = 2048;
  static constexpr int MAX_LOGL = 13;   // L · 16 bytes ≤ 128 KiB
};

// rows per workgroup and the padded row stride (cells) for FFT length 2^logl
template <typename T> __host__ __device__ constexpr int dw_group(int logl) {
  return (DwT<T>::GROUP_CELLS >> logl) > 0 ? (DwT<T>::GROUP_CELLS >> logl) : 1;
}
template <typename T> __host__ __device__ constexpr int dw_stride(int logl) {
  return (1 << logl) + ((1 << logl) >> DwT<T>::PS);
}

// pass p of a 2^logl FFT fuses dw_radix(logl, p) radix-2 stages: ⌈logl/4⌉ passes, sizes balanced
__host__ __device__ constexpr int dw_passes(int logl) { return (logl + 3) / 4; }
__host__ __device__ constexpr int dw_radix(int logl, int p) {
  return logl / dw_passes(logl) + (p < logl % dw_passes(logl) ? 1 : 0);
}
__host__ __device__ constexpr int dw_done(int logl, int p) {  // stages before pass p
  int t = 0;
  for (int q = 0; q < p; ++q) t += dw_radix(logl, q);
  return t;
}

template <typename C> __device__ __forceinline__ C cmul(C a, C b) {
  C r;
  r.x = a.x * b.x - a.y * b.y;
  r.y = a.x * b.y + a.y * b.x;
  return r;
}

template <typename T> __device__ __forceinline__ int dw_phys(int i) { return i + (i >> DwT<T>::PS); }

// One decimation-in-frequency pass over the nrows rows of the group: stages T0 … T0+RL−1 of the
// radix-2 network (stage t couples cells L/2^(t+1) apart). csign = −1 conjugates the roots.
template <typename T, int LOGL, int T0, int RL>
__device__ __forceinline__ void dif_pass(typename DwT<T>::c2* sm, int nrows, const typename DwT<T>::c2* __restrict__ roots,
                                         T csign) {
  typedef typename DwT<T>::c2 C;
  constexpr int R = 1 << RL, LM = LOGL - T0 - RL, LP = dw_stride<T>(LOGL);
  for (int i = threadIdx.x; i < (nrows << (LOGL - RL)); i += DW_THREADS) {
    const int g = i >> (LOGL - RL), ii = i & ((1 << (LOGL - RL)) - 1);
    const int j = ii & ((1 << LM) - 1);
    const int base = ((ii >> LM) << (LM + RL)) + j;
    C* row = sm + g * LP;
    C a[R];
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] = row[dw_phys<T>(base + (q << LM))];
#pragma unroll
    for (int e = 0; e < RL; ++e) {
      const int hq = R >> (e + 1);
#pragma unroll
      for (int qp = 0; qp < hq; ++qp) {
        C tw = roots[(j + (qp << LM)) << (T0 + e)];
        tw.y *= csign;
#pragma unroll
        for (int grp = 0; grp < (1 << e); ++grp) {
          const int lo = grp * 2 * hq + qp, hi = lo + hq;
          const C u = a[lo], v = a[hi];
          a[lo].x = u.x + v.x;
          a[lo].y = u.y + v.y;
          C d;
          d.x = u.x - v.x;
          d.y = u.y - v.y;
          a[hi] = cmul(d, tw);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) row[dw_phys<T>(base + (q << LM))] = a[q];
  }
}

// One decimation-in-time pass of the inverse FFT (conjugate roots; bit-reversed input, natural
// result): stages T0 … T0+RL−1, stage t couples cells 2^t apart. MULB: the cells are multiplied
// by B on the way in (the first pass: B is indexed like the bit-reversed spectrum it meets).
template <typename T, int LOGL, int T0, int RL, bool MULB>
__device__ __forceinline__ void dit_pass(typename DwT<T>::c2* sm, int nrows, const typename DwT<T>::c2* __restrict__ roots,
                                         const typename DwT<T>::c2* __restrict__ B) {
  typedef typename DwT<T>::c2 C;
  constexpr int R = 1 << RL, LP = dw_stride<T>(LOGL);
  for (int i = threadIdx.x; i < (nrows << (LOGL - RL)); i += DW_THREADS) {
    const int g = i >> (LOGL - RL), ii = i & ((1 << (LOGL - RL)) - 1);
    const int j = ii & ((1 << T0) - 1);
    const int base = ((ii >> T0) << (T0 + RL)) + j;
    C* row = sm + g * LP;
    C a[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      a[q] = row[dw_phys<T>(base + (q << T0))];
      if (MULB) a[q] = cmul(a[q], B[base + (q << T0)]);
    }
#pragma unroll
    for (int e = 0; e < RL; ++e) {
      const int hq = 1 << e;
#pragma unroll
      for (int qp = 0; qp < hq; ++qp) {
        C tw = roots[(j + (qp << T0)) << (LOGL - T0 - e - 1)];
        tw.y = -tw.y;
#pragma unroll
        for (int grp = 0; grp < (R >> (e + 1)); ++grp) {
          const int lo = grp * 2 * hq + qp, hi = lo + hq;
          const C u = a[lo], t = cmul(a[hi], tw);
          a[lo].x = u.x + t.x;
          a[lo].y = u.y + t.y;
          a[hi].x = u.x - t.x;
          a[hi].y = u.y - t.y;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) row[dw_phys<T>(base + (q << T0))] = a[q];
  }
}

template <typename T, int LOGL, int P>
__device__ __forceinline__ void dif_all(typename DwT<T>::c2* sm, int nrows, const typename DwT<T>::c2* __restrict__ roots,
                                        T csign) {
  if constexpr (P < dw_passes(LOGL)) {
    dif_pass<T, LOGL, dw_done(LOGL, P), dw_radix(LOGL, P)>(sm, nrows, roots, csign);
    __syncthreads();
    dif_all<T, LOGL, P + 1>(sm, nrows, roots, csign);
  }
}

template <typename T, int LOGL, int P>
__device__ __forceinline__ void dit_all(typename DwT<T>::c2* sm, int nrows, const typename DwT<T>::c2* __restrict__ roots,
                                        const typename DwT<T>::c2* __restrict__ B) {
  if constexpr (P < dw_passes(LOGL)) {
    dit_pass<T, LOGL, dw_done(LOGL, P), dw_radix(LOGL, P), P == 0>(sm, nrows, roots, B);
    __syncthreads();
    dit_all<T, LOGL, P + 1>(sm, nrows, roots, B);
  }
}

// BLUE: n is no power of two (L ≥ 2n−1, chirp tables w and B in use); otherwise L = n.
// inverse and vec (16-byte global accesses: n a multiple of VW and 16-byte aligned pointers) are
// uniform run-time branches of the load and store phases only.
template <typename T, int LOGL, bool BLUE>
__global__ __launch_bounds__(DW_THREADS) void dct_wide_kernel(const T* __restrict__ X, long rows, int n,
                                                              const typename DwT<T>::c2* __restrict__ roots,
                                                              const typename DwT<T>::c2* __restrict__ mk,
                                                              const typename DwT<T>::c2* __restrict__ w,
                                                              const typename DwT<T>::c2* __restrict__ B,
                                                              T* __restrict__ Y, int inverse, int vec) {
  typedef typename DwT<T>::c2 C;
  typedef typename DwT<T>::vec V;
  constexpr int L = 1 << LOGL, G = dw_group<T>(LOGL), LP = dw_stride<T>(LOGL), VW = DwT<T>::VW;
  // load / store phases: a wave per row while the group has at least four rows, else the
  // workgroup's threads split evenly over its rows
  constexpr int TPR = G >= 4 ? 64 : DW_THREADS / G;
  extern __shared__ __align__(16) unsigned char dw_smem[];
  C* sm = reinterpret_cast<C*>(dw_smem);
  const int tid = threadIdx.x, rl = tid % TPR;
  const long ngroups = (rows + G - 1) / G;
  auto rev = [](int k) { return (int)(__brev((unsigned)k) >> (32 - LOGL)); };
  auto perm = [n](int e) { return (e & 1) ? n - 1 - (e >> 1) : (e >> 1); };  // x index → v index

  for (long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const long row0 = grp * G;
    const int nrows = rows - row0 < G ? (int)(rows - row0) : G;
    // ---- in: Makhoul permutation (forward) or W (inverse), times the chirp, into LDS
    for (int g = tid / TPR; g < nrows; g += DW_THREADS / TPR) {
      const T* x = X + (row0 + g) * (long)n;
      C* row = sm + g * LP;
      auto put = [&](int e, T xe) {
        C c;
        if (!inverse) {
          const int j = perm(e);
          if (BLUE) {
            const C wj = w[j];
            c.x = xe * wj.x;
            c.y = xe * wj.y;
          } else {
            c.x = xe;
            c.y = (T)0;
          }
          row[dw_phys<T>(j)] = c;
        } else {
          const T ym = e > 0 ? x[n - e] : (T)0;  // the mirrored element: a second, cached read
          const C m = mk[e];
          c.x = m.x * xe + m.y * ym;
          c.y = m.y * xe - m.x * ym;
          if (BLUE) c = cmul(c, w[e]);
          row[dw_phys<T>(e)] = c;
        }
      };
      if (vec) {
        for (int e = rl * VW; e < n; e += TPR * VW) {
          const V v = *reinterpret_cast<const V*>(x + e);
          put(e, v.x);
          put(e + 1, v.y);
          if constexpr (VW == 4) {
            put(e + 2, v.z);
            put(e + 3, v.w);
          }
        }
      } else {
        for (int e = rl; e < n; e += TPR) put(e, x[e]);
      }
      if (BLUE) {
        C z;
        z.x = (T)0;
        z.y = (T)0;
        for (int e = n + rl; e < L; e += TPR) row[dw_phys<T>(e)] = z;
      }
    }
    __syncthreads();
    // ---- DFT_n in LDS
    dif_all<T, LOGL, 0>(sm, nrows, roots, (!BLUE && inverse) ? (T)-1 : (T)1);
    if constexpr (BLUE) dit_all<T, LOGL, 0>(sm, nrows, roots, B);
    // ---- out: post-twiddle and Re (forward) or the inverse permutation
    for (int g = tid / TPR; g < nrows; g += DW_THREADS / TPR) {
      T* y = Y + (row0 + g) * (long)n;
      const C* row = sm + g * LP;
      auto cell = [&](int k) {  // V[k] (forward) / the complex v[k] (inverse)
        if (BLUE) return cmul(row[dw_phys<T>(k)], w[k]);
        return row[dw_phys<T>(rev(k))];
      };
      auto get = [&](int e) {
        if (!inverse) {
          const C v = cell(e), m = mk[e];
          return m.x * v.x - m.y * v.y;
        }
        return cell(perm(e)).x;
      };
      if (vec) {
        for (int e = rl * VW; e < n; e += TPR * VW) {
          V v;
          v.x = get(e);
          v.y = get(e + 1);
          if constexpr (VW == 4) {
            v.z = get(e + 2);
            v.w = get(e + 3);
          }
          *reinterpret_cast<V*>(y + e) = v;
        }
      } else {
        for (int e = rl; e < n; e += TPR) y[e] = get(e);
      }
    }
    __syncthreads();  // the rows are out before the next group lands
  }
}

constexpr size_t DW_LDS_CU = 160 * 1024;

// FFT length of the wide path for rows of n (0: outside its range). Powers of two take L = n.
template <typename T> int dw_len(int n) {
  if (n <= 128) return 0;
  int logl = 0;
  if ((n & (n - 1)) == 0) {
    while ((1 << logl) < n) ++logl;
  } else {
    if (n > (1 << 20)) return 0;
    while ((1L << logl) < 2L * n - 1) ++logl;
  }
  return logl <= DwT<T>::MAX_LOGL ? (1 << logl) : 0;
}

template <typename T, int LOGL, bool BLUE>
int dw_launch(const T* X, long rows, int n, const void* roots, const void* mk, const void* w, const void* B, T* Y,
              int inverse, int num_cu, hipStream_t s) {
  typedef typename DwT<T>::c2 C;
  constexpr int G = dw_group<T>(LOGL);
  constexpr size_t lds = (size_t)G * dw_stride<T>(LOGL) * sizeof(C);
  static_assert(lds <= DW_LDS_CU, "row does not fit the LDS");
  int per_cu = (int)(DW_LDS_CU / lds);
  if (per_cu > 4) per_cu = 4;
  const long ngroups = (rows + G - 1) / G;
  long grid = (long)(num_cu > 0 ? num_cu : 256) * per_cu;
  if (grid > ngroups) grid = ngroups;
  const int vec = (n % DwT<T>::VW) == 0 && ((((uintptr_t)X) | ((uintptr_t)Y)) & 15) == 0;
  hipLaunchKernelGGL((dct_wide_kernel<T, LOGL, BLUE>), dim3((unsigned)grid), dim3(DW_THREADS), lds, s, X, rows, n,
                     (const C*)roots, (const C*)mk, (const C*)w, (const C*)B, Y, inverse, vec);
  return (int)hipGetLastError();
}

template <typename T>
int dw_rows(const T* X, long rows, int n, const void* roots, const void* mk, const void* w, const void* B, T* Y,
            int inverse, int num_cu, void* stream) {
  const int L = dw_len<T>(n);
  if (L == 0) return -1;
  if (rows == 0) return 0;
  if (rows < 0) return -2;
  const bool blue = L != n;
  if (!X || !Y || !roots || !mk || (blue && (!w || !B))) return -3;
  hipStream_t s = (hipStream_t)stream;
  int logl = 0;
  while ((1 << logl) < L) ++logl;
#define FMLX_DW_CASE(LG)                                                                                  \
  case LG:                                                                                                \
    if constexpr (LG <= DwT<T>::MAX_LOGL) {                                                               \
      return blue ? dw_launch<T, LG, true>(X, rows, n, roots, mk, w, B, Y, inverse, num_cu, s)            \
                  : dw_launch<T, LG, false>(X, rows, n, roots, mk, w, B, Y, inverse, num_cu, s);          \
    }                                                                                                     \
    return -4;
  switch (logl) {
    FMLX_DW_CASE(8)
    FMLX_DW_CASE(9)
    FMLX_DW_CASE(10)
    FMLX_DW_CASE(11)
    FMLX_DW_CASE(12)
    FMLX_DW_CASE(13)
    FMLX_DW_CASE(14)
    default:
      return -4;
  }
#undef FMLX_DW_CASE
}

}  // namespace

// The FFT length L of the wide path for rows of n (f64: double rows) → 0, or −1 when n is outside
// its range: 128 < n ≤ 16384 (f32) / 8192 (f64) for a power of two, 2n−1 ≤ that for any other n.
// L == n: the power-of-two path (no w, no B); otherwise Bluestein.
FMLX_API int fmlx_dct_wide_len(int n, int f64, int* L) {
  const int l = f64 ? dw_len<double>(n) : dw_len<float>(n);
  if (l == 0) return -1;
  if (L) *L = l;
  return 0;
}

// Y[rows][n] = DCT-II (inverse = 0) or DCT-III (inverse = 1) of X[rows][n], contiguous rows.
// Tables of interleaved (re, im) pairs in the row type, for this n and direction:
//   roots[L/2] = e^{−2πij/L};  mk[n] as in the header;  and for L != n
//   w[n] = e^{∓iπ(j² mod 2n)/n} (− forward, + inverse);  B[L] = FFT_L(b)/L in bit-reversed order
//   (B[p] = the natural-order value at the LOG2(L)-bit reversal of p), b_j = b_{L−j} = conj(w_j).
FMLX_API int fmlx_dct_wide_rows(const float* X, long rows, int n, const float* roots, const float* mk, const float* w,
                                const float* B, float* Y, int inverse, int num_cu, void* stream) {
  return dw_rows<float>(X, rows, n, roots, mk, w, B, Y, inverse, num_cu, stream);
}

FMLX_API int fmlx_dct_wide_rows_f64(const double* X, long rows, int n, const double* roots, const double* mk,
                                    const double* w, const double* B, double* Y, int inverse, int num_cu,
                                    void* stream) {
  return dw_rows<double>(X, rows, n, roots, mk, w, B, Y, inverse, num_cu, stream);
}

FMLX_DEFINE_PRELOAD()
