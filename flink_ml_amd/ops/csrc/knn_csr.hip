// KNN on CSR feature columns (fp32 / fp64 values): the product block G = Q·Tᵀ of a block of CSR
// query rows with every training row, without an n x D matrix on either side, and the per-row
// squared norms.
//
//  * knn_csr_products: the training set's column-major copy (ops/csr.py ColumnMajor: colptr, crow,
//    cval, a column's entries in row order) is the inverted index. One 256-thread block per (query
//    row, tile of TILE training rows); the tile's accumulators sit in LDS and each of the four waves
//    owns a quarter of them. The wave zeroes its quarter, loads the query row's entries 64 at a
//    time, a lane per entry, and every lane finds the part of its entry's column that falls into
//    the wave's rows with two binary searches over crow (64 searches side by side). The entries
//    are then broadcast one by one, in stored order, and the lanes stride over the column part
//    with a plain LDS load-add-store into slot crow[j] - first_row. Rows are distinct inside a
//    column and the slots are the wave's alone, so lanes never collide; the entries follow each
//    other in program order, so no barrier and no atomic is needed, and every G[r, t] is summed in
//    the query row's stored-entry order whatever the grid, the tile or the query block. The wave
//    finally stores its quarter to G: written once, coalesced, no zero-fill pass.
//  * knn_csr_sqnorm: Σv² per row in stored-entry order, accumulated in fp64 (a thread per row).
//
// An index outside [0, D), a column range outside [0, nnz) or a row outside the wave's quarter is
// never dereferenced: the entry is skipped and the error word set.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ T kx_bcast(T v, int t);
template <>
__device__ __forceinline__ float kx_bcast<float>(float v, int t) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
}
template <>
__device__ __forceinline__ double kx_bcast<double>(double v, int t) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), t);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// first position in [lo, hi) whose row is >= key (rows ascending)
__device__ __forceinline__ int kx_lower_bound(const int* __restrict__ crow, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (crow[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// block b: query row b / ntiles of the block [q0, q0 + nq), training rows [TILE·(b % ntiles), …)
template <typename T, int TILE>
__global__ __launch_bounds__(256) void knn_csr_products_kernel(const long* __restrict__ qptr,
                                                               const int* __restrict__ qidx,
                                                               const T* __restrict__ qval, long q0, int D,
                                                               const long* __restrict__ colptr,
                                                               const int* __restrict__ crow,
                                                               const T* __restrict__ cval, int n, int nnz, int ntiles,
                                                               T* __restrict__ G, long ldg, int* __restrict__ err) {
  constexpr int QUART = TILE / 4;
  __shared__ T acc[TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long qr = blockIdx.x / (unsigned)ntiles;
  const int tile = blockIdx.x % (unsigned)ntiles;
  const long first = (long)tile * TILE + (long)wave * QUART;  // the wave's rows: [first, last)
  if (first >= n) return;
  const int r_lo = (int)first;
  const int r_hi = first + QUART < n ? (int)(first + QUART) : n;
  T* mine = acc + wave * QUART;
  for (int i = lane; i < QUART; i += 64) mine[i] = (T)0;
  __builtin_amdgcn_wave_barrier();
  bool bad = false;
  const long s = qptr[q0 + qr], e = qptr[q0 + qr + 1];
  for (long base = s; base < e; base += 64) {
    const long p = base + lane;
    int pj = 0, pe = 0;  // the lane's entry: its column's positions inside the wave's rows
    T v = (T)0;
    if (p < e) {
      const int c = qidx[p];
      if ((unsigned)c < (unsigned)D) {
        const long c0 = colptr[c], c1 = colptr[c + 1];
        if (c0 >= 0 && c0 <= c1 && c1 <= nnz) {
          v = qval[p];
          pj = kx_lower_bound(crow, (int)c0, (int)c1, r_lo);
          pe = kx_lower_bound(crow, pj, (int)c1, r_hi);
        } else {
          bad = true;
        }
      } else {
        bad = true;
      }
    }
    // the entries that meet the wave's rows, in stored order
    unsigned long long live = __ballot(pe > pj);
    while (live) {
      const int t = __builtin_ctzll(live);
      live &= live - 1;
      const int j0 = __builtin_amdgcn_readlane(pj, t), j1 = __builtin_amdgcn_readlane(pe, t);
      const T vv = kx_bcast<T>(v, t);
      for (int j = j0 + lane; j < j1; j += 64) {
        const unsigned slot = (unsigned)(crow[j] - r_lo);
        if (slot < (unsigned)(r_hi - r_lo))
          mine[slot] += vv * cval[j];
        else
          bad = true;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  T* g = G + qr * ldg + first;
  for (int i = lane; i < r_hi - r_lo; i += 64) g[i] = mine[i];
  if (bad) *err = 1;
}

// a thread per row: Σv² in stored-entry order, in fp64
template <typename T, typename O>
__global__ __launch_bounds__(256) void knn_csr_sqnorm_kernel(const long* __restrict__ indptr,
                                                             const int* __restrict__ idx, const T* __restrict__ val,
                                                             long n, int D, O* __restrict__ out,
                                                             int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool bad = false;
  double sum = 0.0;
  for (long p = indptr[r], e = indptr[r + 1]; p < e; ++p) {
    if ((unsigned)idx[p] < (unsigned)D) {
      const double v = (double)val[p];
      sum += v * v;
    } else {
      bad = true;
    }
  }
  out[r] = (O)sum;
  if (bad) *err = 1;
}

}  // namespace

// G[r - q0][t] for the query rows [q0, q0 + nq) of (qptr, qidx, qval) and the n training rows of
// the column-major copy; tile_rows·sizeof(value) is 32 KiB (8192 fp32 / 4096 fp64 rows) or 8 KiB
FMLX_API int fmlx_knn_csr_products(int f64, const long* qptr, const int* qidx, const void* qval, long q0, long nq,
                                   int D, const long* colptr, const int* crow, const void* cval, long n, long nnz,
                                   int tile_rows, void* G, long ldg, int* err, void* stream) {
  if (nq <= 0 || n <= 0) return 0;
  if (D < 1 || q0 < 0 || n >= (1l << 31) || nnz < 0 || nnz >= (1l << 31) || ldg < n || tile_rows < 4) return -1;
  const long ntiles = (n + tile_rows - 1) / tile_rows;
  if (nq * ntiles >= (1l << 31)) return -1;
  return with_acc(f64, [&](auto acc) {
    typedef decltype(acc) T;
    return with_value<8192, 32768>(tile_rows * (int)sizeof(T), [&](auto bytes) {
      constexpr int TILE = decltype(bytes)::value / (int)sizeof(T);
      hipLaunchKernelGGL((knn_csr_products_kernel<T, TILE>), dim3((unsigned)(nq * ntiles)), dim3(256), 0,
                         (hipStream_t)stream, qptr, qidx, (const T*)qval, q0, D, colptr, crow, (const T*)cval, (int)n,
                         (int)nnz, (int)ntiles, (T*)G, ldg, err);
      return (int)hipGetLastError();
    });
  });
}

// out[r] = Σv² of row r (out_f64: fp64 or fp32 output); an index outside [0, D) adds nothing
FMLX_API int fmlx_knn_csr_sqnorm(int f64, int out_f64, const long* indptr, const int* idx, const void* val, long n,
                                 int D, void* out, int* err, void* stream) {
  if (n <= 0) return 0;
  if (D < 1) return -1;
  const dim3 grid((unsigned)((n + 255) / 256));
  return with_acc(f64, [&](auto acc) {
    typedef decltype(acc) T;
    return with_acc(out_f64, [&](auto o) {
      typedef decltype(o) O;
      hipLaunchKernelGGL((knn_csr_sqnorm_kernel<T, O>), grid, dim3(256), 0, (hipStream_t)stream, indptr, idx,
                         (const T*)val, n, D, (O*)out, err);
      return (int)hipGetLastError();
    });
  });
}

FMLX_DEFINE_PRELOAD()
