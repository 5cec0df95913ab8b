// KMeans on CSR feature columns (fp32 / fp64 values): assign, centroid update and finalize without
// an n x D matrix.
//
// Centroid image: centroid-minor Ct[D][kp], kp = k rounded up to a power of two (<= 64) or to
// 64 * {1, 2, 4, 8, 16}; padding lanes hold 0 and are never argmin candidates. One CSR entry
// (j, v) then reads kp contiguous values, a lane per centroid (NA = kp / 64 accumulators per lane
// above 64 centroids).
//  * kmeans_csr_assign: a wave per row; the row's entries are loaded 64 at a time (coalesced) and
//    broadcast lane by lane; argmin with the semantics of kmeans_assign_generic_kernel.
//  * kmeans_csr_colsum: the update as an inverted-index pass over a column-major copy of the
//    partition (built once per fit: prepare -> seg_sort -> colptr -> gather). A wave owns a column
//    segment, a lane a centroid; a column's entries are in row order and are added one by one, so
//    the sums are bitwise reproducible. No float atomics; the counts are an integer histogram.
//  * kmeans_csr_finalize: Ct = St / count and the per-centroid norms from a fixed-order two-level
//    fold over D.
// An index outside [0, D) is never dereferenced: the entry is skipped and the error word set.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ T kc_bcast(T v, int t);
template <>
__device__ __forceinline__ float kc_bcast<float>(float v, int t) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
}
template <>
__device__ __forceinline__ double kc_bcast<double>(double v, int t) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), t);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <typename T>
__device__ __forceinline__ T kc_abs(T v) {
  return v < (T)0 ? -v : v;
}

// ------------------------------------------------------------------------------------------
// assign
// ------------------------------------------------------------------------------------------
// norms: [0, kp) = ‖c‖, [kp, 2kp) = ‖c‖², [2kp, 3kp) = ‖c‖₁
template <typename T, int NA, bool MANH>
__global__ __launch_bounds__(256) void kmeans_csr_assign_kernel(const long* __restrict__ indptr,
                                                                const int* __restrict__ idx, const T* __restrict__ val,
                                                                long n, int D, const T* __restrict__ Ct, int kp, int k,
                                                                const T* __restrict__ norms, int metric,
                                                                int* __restrict__ labels, int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  const bool live = NA > 1 || lane < kp;  // (kp < 64: the lanes past the image do no loads)
  bool bad = false;
  for (long r = wave; r < n; r += nwaves) {
    const long s = indptr[r], e = indptr[r + 1];
    T acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0;
    T xn2 = 0;
    for (long base = s; base < e; base += 64) {
      const long p = base + lane;
      int j = -1;
      T v = 0;
      if (p < e) {
        j = idx[p];
        v = val[p];
        if ((unsigned)j >= (unsigned)D) {
          j = -1;
          v = 0;
          bad = true;
        }
      }
      xn2 += v * v;
      const int cnt = (int)(e - base < 64 ? e - base : 64);
      for (int t = 0; t < cnt; ++t) {
        const int jj = __builtin_amdgcn_readlane(j, t);
        const T vv = kc_bcast<T>(v, t);
        const T* c = Ct + (long)jj * kp + lane;
        if (jj >= 0 && live) {
#pragma unroll
          for (int a = 0; a < NA; ++a) {
            const T cv = c[a * 64];
            if (MANH)
              acc[a] += kc_abs(vv - cv) - kc_abs(cv);
            else
              acc[a] += vv * cv;
          }
        }
      }
    }
    xn2 = wave_sum(xn2);  // (a symmetric butterfly: every lane holds the same bits)
    const T xn = sqrt(xn2);
    const T init = metric == 0 ? (T)__builtin_huge_val() : (T)1.7976931348623157e308;
    T best = init;
    int bi = 0x7fffffff;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int c = a * 64 + lane;
      if (c < k) {
        T d;
        if (metric == 0) {
          d = xn2 + norms[kp + c] - (T)2 * acc[a];
          d = d > (T)0 ? d : (d == d ? (T)0 : d);
        } else if (metric == 1) {
          d = norms[2 * kp + c] + acc[a];
        } else {
          d = (T)1 - acc[a] / xn / norms[c];
        }
        if (d < best) {  // strict: the lowest index wins ties; a NaN never wins
          best = d;
          bi = c;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T od = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (od < best || (od == best && oi < bi)) {
        best = od;
        bi = oi;
      }
    }
    if (lane == 0) labels[r] = bi == 0x7fffffff ? (metric == 0 ? 0 : -1) : bi;
  }
  if (bad) *err = 1;
}

template <typename T, int NA>
int kc_launch_assign(const long* indptr, const int* idx, const void* val, long n, int D, const void* Ct, int kp, int k,
                     const void* norms, int metric, int* labels, int* err, hipStream_t s) {
  long blocks = (n + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  return with_bool(metric == 1, [&](auto cosine) {
    hipLaunchKernelGGL((kmeans_csr_assign_kernel<T, NA, cosine.value>), dim3((unsigned)blocks), dim3(256), 0, s, indptr,
                       idx, (const T*)val, n, D, (const T*)Ct, kp, k, (const T*)norms, metric, labels, err);
    return (int)hipGetLastError();
  });
}

// accumulators per lane: one up to kp = 64, then kp / 64 (kp a power of two <= 1024: kc_kp_ok)
template <typename F>
int with_na(int kp, F&& f) {
  return with_value<1, 2, 4, 8, 16>(kp <= 64 ? 1 : kp / 64, f);
}

// kp is a power of two <= 64 or 64 * {1, 2, 4, 8, 16}, and holds k
bool kc_kp_ok(int kp, int k) {
  if (k < 1 || kp < k || kp > 1024 || (kp & (kp - 1))) return false;
  return true;
}

// ------------------------------------------------------------------------------------------
// column-major copy
// ------------------------------------------------------------------------------------------
// a wave per row: sort key (the column; 0 for a bad index), entry id, row (-1 for a bad index)
__global__ __launch_bounds__(256) void kmeans_csr_prepare_kernel(const long* __restrict__ indptr,
                                                                 const int* __restrict__ idx, long n, int D,
                                                                 int* __restrict__ keys, int* __restrict__ ids,
                                                                 int* __restrict__ erow, int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  bool bad = false;
  for (long r = wave; r < n; r += nwaves) {
    const long s = indptr[r], e = indptr[r + 1];
    for (long p = s + lane; p < e; p += 64) {
      const int j = idx[p];
      const bool ok = (unsigned)j < (unsigned)D;
      bad |= !ok;
      keys[p] = ok ? j : 0;
      ids[p] = (int)p;
      erow[p] = ok ? (int)r : -1;
    }
  }
  if (bad) *err = 1;
}

// colptr[c] = first sorted position whose key is >= c (keys ascending, in [0, D))
__global__ __launch_bounds__(256) void kmeans_csr_colptr_kernel(const int* __restrict__ keys, long nnz, int D,
                                                                long* __restrict__ colptr) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > nnz) return;
  int cur = p < nnz ? keys[p] : D;
  int prev = p > 0 ? keys[p - 1] : -1;
  if (cur > D) cur = D;
  if (prev < -1) prev = -1;
  for (int c = prev + 1; c <= cur; ++c) colptr[c] = p;
}

template <typename T>
__global__ __launch_bounds__(256) void kmeans_csr_gather_kernel(const int* __restrict__ order,
                                                                const int* __restrict__ erow, const T* __restrict__ val,
                                                                long nnz, int* __restrict__ crow, T* __restrict__ cval) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nnz) return;
  const int e = order[p];
  if (e < 0 || e >= nnz) {  // (cannot happen: the ids are a permutation)
    crow[p] = -1;
    cval[p] = 0;
    return;
  }
  crow[p] = erow[e];
  cval[p] = val[e];
}

// ------------------------------------------------------------------------------------------
// centroid update
// ------------------------------------------------------------------------------------------
// Σ over the column-major entries [p0, p1), in order: the lane whose centroid is the entry's label
// adds the value. Rows with a label outside [0, k) (and skipped entries, row -1) add nothing.
template <typename T, int NA>
__device__ __forceinline__ void kc_sum_range(const int* __restrict__ crow, const T* __restrict__ cval,
                                             const int* __restrict__ labels, long n, long p0, long p1, int k, int lane,
                                             T (&acc)[NA]) {
  for (long base = p0; base < p1; base += 64) {
    const long p = base + lane;
    int lab = -1;
    T v = 0;
    if (p < p1) {
      const int r = crow[p];
      if ((unsigned long)r < (unsigned long)n) lab = labels[r];
      v = cval[p];
    }
    const int cnt = (int)(p1 - base < 64 ? p1 - base : 64);
    for (int t = 0; t < cnt; ++t) {
      const int l = __builtin_amdgcn_readlane(lab, t);
      const T vv = kc_bcast<T>(v, t);
      const int slot = (unsigned)l < (unsigned)k ? l >> 6 : -1, ln = l & 63;
#pragma unroll
      for (int a = 0; a < NA; ++a)
        if (slot == a) acc[a] += lane == ln ? vv : (T)0;
    }
  }
}

template <typename T, int NA>
__device__ __forceinline__ void kc_store(T* __restrict__ dst, int kp, int lane, const T (&acc)[NA]) {
  if (NA > 1 || lane < kp) {
#pragma unroll
    for (int a = 0; a < NA; ++a) dst[a * 64 + lane] = acc[a];
  }
}

// a wave per column (grid-stride): columns of at most seg entries are summed and stored (an empty
// one as zeros); longer ones are left to the segment kernels
template <typename T, int NA>
__global__ __launch_bounds__(256) void kmeans_csr_colsum_kernel(const long* __restrict__ colptr,
                                                                const int* __restrict__ crow, const T* __restrict__ cval,
                                                                const int* __restrict__ labels, long n, int D, int kp,
                                                                int k, long seg, T* __restrict__ St) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  for (long c = wave; c < D; c += nwaves) {
    const long p0 = colptr[c], p1 = colptr[c + 1];
    if (p1 - p0 > seg) continue;
    T acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0;
    kc_sum_range<T, NA>(crow, cval, labels, n, p0, p1, k, lane, acc);
    kc_store<T, NA>(St + c * kp, kp, lane, acc);
  }
}

// a wave per segment of a long column: partial[s][kp]
template <typename T, int NA>
__global__ __launch_bounds__(256) void kmeans_csr_segsum_kernel(const long* __restrict__ colptr,
                                                                const int* __restrict__ crow, const T* __restrict__ cval,
                                                                const int* __restrict__ labels, long n, int D, int kp,
                                                                int k, long seg, long nsegs,
                                                                const int* __restrict__ seg_col,
                                                                const int* __restrict__ seg_k, T* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= nsegs) return;
  const int c = seg_col[s];
  T acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0;
  if ((unsigned)c < (unsigned)D) {
    const long c1 = colptr[c + 1];
    long p0 = colptr[c] + (long)seg_k[s] * seg;
    long p1 = p0 + seg < c1 ? p0 + seg : c1;
    if (p0 < colptr[c]) p0 = p1;  // (a table that does not match colptr sums nothing)
    kc_sum_range<T, NA>(crow, cval, labels, n, p0, p1, k, lane, acc);
  }
  kc_store<T, NA>(partial + s * kp, kp, lane, acc);
}

// a block per long column: its segments' partials added in segment order
template <typename T>
__global__ __launch_bounds__(256) void kmeans_csr_segfold_kernel(const int* __restrict__ long_col,
                                                                 const long* __restrict__ long_seg0, int D, int kp,
                                                                 const T* __restrict__ partial, T* __restrict__ St) {
  const int c = long_col[blockIdx.x];
  if ((unsigned)c >= (unsigned)D) return;
  const long s0 = long_seg0[blockIdx.x], s1 = long_seg0[blockIdx.x + 1];
  for (int t = threadIdx.x; t < kp; t += blockDim.x) {
    T sum = 0;
    for (long s = s0; s < s1; ++s) sum += partial[s * kp + t];
    St[(long)c * kp + t] = sum;
  }
}

// integer histogram of the labels (integer atomics: order-independent)
__global__ __launch_bounds__(256) void kmeans_csr_hist_kernel(const int* __restrict__ labels, long n, int k,
                                                              int* __restrict__ counts) {
  __shared__ int h[1024];
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
    const int l = labels[r];
    if ((unsigned)l < (unsigned)k) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += blockDim.x)
    if (h[i]) atomicAdd(&counts[i], h[i]);
}

// counts into the payload's tail; the integer counts are zeroed for the next round
template <typename T>
__global__ __launch_bounds__(256) void kmeans_csr_counts_kernel(int* __restrict__ counts, int k, T* __restrict__ out) {
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    out[i] = (T)counts[i];
    counts[i] = 0;
  }
}

template <typename T, int NA>
int kc_launch_colsum(const long* colptr, const int* crow, const void* cval, const int* labels, long n, int D, int kp,
                     int k, long seg, int nlong, const int* long_col, const long* long_seg0, long nsegs,
                     const int* seg_col, const int* seg_k, void* partial, int* counts, void* payload, hipStream_t s) {
  T* St = (T*)payload;
  long blocks = ((long)D + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((kmeans_csr_colsum_kernel<T, NA>), dim3((unsigned)blocks), dim3(256), 0, s, colptr, crow,
                     (const T*)cval, labels, n, D, kp, k, seg, St);
  if (nlong > 0 && nsegs > 0) {
    hipLaunchKernelGGL((kmeans_csr_segsum_kernel<T, NA>), dim3((unsigned)((nsegs + 3) / 4)), dim3(256), 0, s, colptr,
                       crow, (const T*)cval, labels, n, D, kp, k, seg, nsegs, seg_col, seg_k, (T*)partial);
    hipLaunchKernelGGL(kmeans_csr_segfold_kernel<T>, dim3((unsigned)nlong), dim3(256), 0, s, long_col, long_seg0, D, kp,
                       (const T*)partial, St);
  }
  long hb = (n + 255) / 256;
  if (hb > 1024) hb = 1024;
  if (hb > 0) hipLaunchKernelGGL(kmeans_csr_hist_kernel, dim3((unsigned)hb), dim3(256), 0, s, labels, n, k, counts);
  hipLaunchKernelGGL(kmeans_csr_counts_kernel<T>, dim3(1), dim3(256), 0, s, counts, k, St + (long)D * kp);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// finalize
// ------------------------------------------------------------------------------------------
// block b owns the rows [b·rpb, (b+1)·rpb) of the image: Ct = St / count, and its partial Σv², Σ|v|
// per centroid in a fixed order (a thread's rows ascending, then the threads of a centroid
// ascending) → part[b][2][kp]
template <typename T>
__global__ __launch_bounds__(256) void kmeans_csr_finalize_kernel(const T* __restrict__ red, int D, int kp, int k,
                                                                  int rpb, T* __restrict__ Ct, T* __restrict__ part) {
  __shared__ T sm[2][256];
  const long r0 = (long)blockIdx.x * rpb;
  const long r1 = r0 + rpb < D ? r0 + rpb : D;
  const T* cnt = red + (long)D * kp;
  T* out = part + (long)blockIdx.x * 2 * kp;
  if (kp <= 256) {
    const int G = 256 / kp, g = threadIdx.x / kp, t = threadIdx.x % kp;
    const T inv = t < k ? (T)1 / cnt[t] : (T)0;
    T s2 = 0, s1 = 0;
    for (long r = r0 + g; r < r1; r += G) {
      const T v = t < k ? red[r * kp + t] * inv : (T)0;
      Ct[r * kp + t] = v;
      s2 += v * v;
      s1 += kc_abs(v);
    }
    sm[0][threadIdx.x] = s2;
    sm[1][threadIdx.x] = s1;
    __syncthreads();
    if (g == 0) {
      T a2 = 0, a1 = 0;
      for (int i = 0; i < G; ++i) {
        a2 += sm[0][i * kp + t];
        a1 += sm[1][i * kp + t];
      }
      out[t] = a2;
      out[kp + t] = a1;
    }
  } else {
    for (int t = threadIdx.x; t < kp; t += blockDim.x) {
      const T inv = t < k ? (T)1 / cnt[t] : (T)0;
      T s2 = 0, s1 = 0;
      for (long r = r0; r < r1; ++r) {
        const T v = t < k ? red[r * kp + t] * inv : (T)0;
        Ct[r * kp + t] = v;
        s2 += v * v;
        s1 += kc_abs(v);
      }
      out[t] = s2;
      out[kp + t] = s1;
    }
  }
}

// one ordered add over the blocks' partials; weights = counts
template <typename T>
__global__ __launch_bounds__(256) void kmeans_csr_norms_kernel(const T* __restrict__ red, int D, int kp, int k, int nb,
                                                               const T* __restrict__ part, T* __restrict__ norms,
                                                               double* __restrict__ weights) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= kp) return;
  T a2 = 0, a1 = 0;
  for (int b = 0; b < nb; ++b) {
    a2 += part[(long)b * 2 * kp + t];
    a1 += part[(long)b * 2 * kp + kp + t];
  }
  norms[t] = sqrt(a2);
  norms[kp + t] = a2;
  norms[2 * kp + t] = a1;
  if (t < k) weights[t] = (double)red[(long)D * kp + t];
}

}  // namespace

FMLX_API int fmlx_kmeans_csr_assign(int f64, const long* indptr, const int* idx, const void* val, long n, int D,
                                    const void* Ct, int kp, int k, const void* norms, int metric, int* labels, int* err,
                                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return 0;
  if (!kc_kp_ok(kp, k) || D < 1 || metric < 0 || metric > 2) return -1;
  return with_acc(f64, [&](auto acc) {
    return with_na(kp, [&](auto na) {
      return kc_launch_assign<decltype(acc), na.value>(indptr, idx, val, n, D, Ct, kp, k, norms, metric, labels, err, s);
    });
  });
}

// sort keys / entry ids / rows of the partition's entries (nnz = indptr[n] < 2^31)
FMLX_API int fmlx_kmeans_csr_prepare(const long* indptr, const int* idx, long n, int D, int* keys, int* ids, int* erow,
                                     int* err, void* stream) {
  if (n <= 0) return 0;
  long blocks = (n + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(kmeans_csr_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, indptr, idx,
                     n, D, keys, ids, erow, err);
  return (int)hipGetLastError();
}

FMLX_API int fmlx_kmeans_csr_colptr(const int* keys_sorted, long nnz, int D, long* colptr, void* stream) {
  if (nnz < 0 || D < 1) return -1;
  hipLaunchKernelGGL(kmeans_csr_colptr_kernel, dim3((unsigned)((nnz + 256) / 256)), dim3(256), 0, (hipStream_t)stream,
                     keys_sorted, nnz, D, colptr);
  return (int)hipGetLastError();
}

FMLX_API int fmlx_kmeans_csr_gather(int f64, const int* order, const int* erow, const void* val, long nnz, int* crow,
                                    void* cval, void* stream) {
  if (nnz <= 0) return 0;
  const dim3 grid((unsigned)((nnz + 255) / 256));
  return with_acc(f64, [&](auto acc) {
    typedef decltype(acc) T;
    hipLaunchKernelGGL(kmeans_csr_gather_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, order, erow, (const T*)val,
                       nnz, crow, (T*)cval);
    return (int)hipGetLastError();
  });
}

// payload = [St[D][kp] | k counts]; columns longer than seg entries go through the segment table
// (nlong columns, long_seg0[nlong + 1] first segments, seg_col / seg_k[nsegs], partial[nsegs][kp])
FMLX_API int fmlx_kmeans_csr_colsum(int f64, const long* colptr, const int* crow, const void* cval, const int* labels,
                                    long n, int D, int kp, int k, long seg, int nlong, const int* long_col,
                                    const long* long_seg0, long nsegs, const int* seg_col, const int* seg_k,
                                    void* partial, int* counts, void* payload, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!kc_kp_ok(kp, k) || D < 1 || seg < 1 || n < 0) return -1;
  return with_acc(f64, [&](auto acc) {
    return with_na(kp, [&](auto na) {
      return kc_launch_colsum<decltype(acc), na.value>(colptr, crow, cval, labels, n, D, kp, k, seg, nlong, long_col,
                                                       long_seg0, nsegs, seg_col, seg_k, partial, counts, payload, s);
    });
  });
}

// part: nb blocks x 2 x kp partial norms, nb = ceil(D / rpb)
FMLX_API int fmlx_kmeans_csr_finalize(int f64, const void* payload, int D, int kp, int k, void* Ct, void* norms,
                                      double* weights, void* part, int rpb, int nb, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!kc_kp_ok(kp, k) || D < 1 || rpb < 1 || (long)nb * rpb < D || (long)(nb - 1) * rpb >= D) return -1;
  return with_acc(f64, [&](auto acc) {
    typedef decltype(acc) T;
    hipLaunchKernelGGL(kmeans_csr_finalize_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)payload, D, kp, k, rpb,
                       (T*)Ct, (T*)part);
    hipLaunchKernelGGL(kmeans_csr_norms_kernel<T>, dim3((kp + 255) / 256), dim3(256), 0, s, (const T*)payload, D, kp, k,
                       nb, (const T*)part, (T*)norms, weights);
    return (int)hipGetLastError();
  });
}

FMLX_DEFINE_PRELOAD()
