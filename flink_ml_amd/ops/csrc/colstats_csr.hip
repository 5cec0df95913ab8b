// Column statistics of a CSR feature column without an n x D matrix: one pass over its column-major
// copy (ops/csr.py: colptr / crow / cval, a column's entries in row order) gives, per column and
// all in fp64, the weighted sums of a window of up to 32 row groups, Σx, Σx², min, max and the
// number of stored entries. What StandardScaler, MinMaxScaler, VarianceThresholdSelector, ANOVATest
// and FValueTest reduce a partition to (colstats.hip and groupstats.hip on a dense matrix).
//
// A wave owns a column (grid-stride), or one segment of a column longer than `seg` entries. Its 64
// entries at a time are loaded coalesced and broadcast lane by lane; lane g < 32 holds group g's
// sum, lanes 32 … 36 hold Σx, Σx², min, max and the stored count. Every slot takes the column's
// entries one by one in entry (= row) order, and a long column's segment partials are folded in
// segment order: no float atomics, bitwise the same from run to run and for every grid.
// min / max compare like colstats.hip (v < mn ? v : mn: a NaN never wins); the rows that store
// nothing in a column are zeros: min = min(min, 0), max = max(max, 0) where stored < n.
// An entry whose row is outside [0, n) (the copy marks a bad feature index with row -1) is skipped.
#include "common.h"

namespace {

constexpr int CS_GROUPS = 32;  // group lanes of a window
constexpr int CS_SUM = 32, CS_SQ = 33, CS_MIN = 34, CS_MAX = 35, CS_CNT = 36;
constexpr int CS_SLOTS = 37;   // a segment's partial record

__device__ __forceinline__ double cs_bcast(double v, int t) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), t);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double cs_init(int lane) {
  return lane == CS_MIN ? __builtin_huge_val() : (lane == CS_MAX ? -__builtin_huge_val() : 0.0);
}

// the entries [p0, p1) into the lane's slot, in order. code: the entry's group within the window,
// -1 for a group outside it, -2 for a skipped entry
template <typename T>
__device__ __forceinline__ double cs_range(const int* __restrict__ crow, const T* __restrict__ cval,
                                           const int* __restrict__ gidx, const double* __restrict__ w, long n, int g0,
                                           int Gw, long p0, long p1, int lane, double acc) {
  for (long base = p0; base < p1; base += 64) {
    const long p = base + lane;
    int code = -2;
    double v = 0.0, wv = 0.0;
    if (p < p1) {
      const int r = crow[p];
      if ((unsigned long)r < (unsigned long)n) {
        v = (double)cval[p];
        const unsigned g = gidx ? (unsigned)gidx[r] - (unsigned)g0 : 0u;
        code = g < (unsigned)Gw ? (int)g : -1;
        wv = w ? w[r] * v : v;
      }
    }
    const int cnt = (int)(p1 - base < 64 ? p1 - base : 64);
    for (int t = 0; t < cnt; ++t) {
      const int c = __builtin_amdgcn_readlane(code, t);
      if (c == -2) continue;  // (wave-uniform)
      const double vv = cs_bcast(v, t), ww = cs_bcast(wv, t);
      const double term = lane < CS_GROUPS ? (c == lane ? ww : 0.0) : (lane == CS_SUM ? vv : (lane == CS_SQ ? vv * vv : 1.0));
      const double s = acc + term;
      const double mn = vv < acc ? vv : acc;
      const double mx = vv > acc ? vv : acc;
      acc = lane == CS_MIN ? mn : (lane == CS_MAX ? mx : s);
    }
  }
  return acc;
}

// a column's finished slots → res[Gw + 4][D] = S | Σx | Σx² | min | max, stored[D]
__device__ __forceinline__ void cs_store(double* __restrict__ res, long* __restrict__ stored, long n, int D, int Gw,
                                         long c, int lane, double acc) {
  const long cnt = (long)cs_bcast(acc, CS_CNT);
  if (cnt < n) {  // the rows without an entry hold zeros
    const double mn = 0.0 < acc ? 0.0 : acc;
    const double mx = 0.0 > acc ? 0.0 : acc;
    acc = lane == CS_MIN ? mn : (lane == CS_MAX ? mx : acc);
  }
  if (lane < Gw)
    res[(long)lane * D + c] = acc;
  else if (lane >= CS_SUM && lane <= CS_MAX)
    res[(long)(Gw + lane - CS_SUM) * D + c] = acc;
  else if (lane == CS_CNT)
    stored[c] = cnt;
}

// a wave per column (grid-stride): columns of at most seg entries; longer ones are left to the
// segment kernels
template <typename T>
__global__ __launch_bounds__(256) void colstats_csr_kernel(const long* __restrict__ colptr, const int* __restrict__ crow,
                                                           const T* __restrict__ cval, const int* __restrict__ gidx,
                                                           const double* __restrict__ w, long n, long nnz, int D, int g0,
                                                           int Gw, long seg, double* __restrict__ res,
                                                           long* __restrict__ stored) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  for (long c = wave; c < D; c += nwaves) {
    long p0 = colptr[c], p1 = colptr[c + 1];
    if (p1 - p0 > seg) continue;
    if (p0 < 0) p0 = 0;  // (cannot happen: colptr is the copy's)
    if (p1 > nnz) p1 = nnz;
    const double acc = cs_range<T>(crow, cval, gidx, w, n, g0, Gw, p0, p1, lane, cs_init(lane));
    cs_store(res, stored, n, D, Gw, c, lane, acc);
  }
}

// a wave per segment of a long column: partial[s][CS_SLOTS]
template <typename T>
__global__ __launch_bounds__(256) void colstats_csr_seg_kernel(const long* __restrict__ colptr,
                                                               const int* __restrict__ crow, const T* __restrict__ cval,
                                                               const int* __restrict__ gidx,
                                                               const double* __restrict__ w, long n, long nnz, int D,
                                                               int g0, int Gw, long seg, long nsegs,
                                                               const int* __restrict__ seg_col,
                                                               const int* __restrict__ seg_k,
                                                               double* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= nsegs) return;
  const int c = seg_col[s];
  double acc = cs_init(lane);
  if ((unsigned)c < (unsigned)D) {
    const long c0 = colptr[c], c1 = colptr[c + 1] < nnz ? colptr[c + 1] : nnz;
    long p0 = c0 + (long)seg_k[s] * seg;
    long p1 = p0 + seg < c1 ? p0 + seg : c1;
    if (p0 < c0 || c0 < 0) p0 = p1;  // (a table that does not match colptr sums nothing)
    acc = cs_range<T>(crow, cval, gidx, w, n, g0, Gw, p0, p1, lane, acc);
  }
  if (lane < CS_SLOTS) partial[s * CS_SLOTS + lane] = acc;
}

// a wave per long column: its segments' partials folded in segment order
__global__ __launch_bounds__(64) void colstats_csr_fold_kernel(const int* __restrict__ long_col,
                                                               const long* __restrict__ long_seg0, long n, int D, int Gw,
                                                               const double* __restrict__ partial,
                                                               double* __restrict__ res, long* __restrict__ stored) {
  const int lane = threadIdx.x & 63;
  const int c = long_col[blockIdx.x];
  if ((unsigned)c >= (unsigned)D) return;
  const long s0 = long_seg0[blockIdx.x], s1 = long_seg0[blockIdx.x + 1];
  double acc = cs_init(lane);
  if (lane < CS_SLOTS) {
    for (long s = s0; s < s1; ++s) {
      const double p = partial[s * CS_SLOTS + lane];
      const double sum = acc + p;
      const double mn = p < acc ? p : acc;
      const double mx = p > acc ? p : acc;
      acc = lane == CS_MIN ? mn : (lane == CS_MAX ? mx : sum);
    }
  }
  cs_store(res, stored, n, D, Gw, c, lane, acc);
}

}  // namespace

// res[Gw + 4][D] = S[g][j] for the groups [g0, g0 + Gw) | Σx | Σx² | min | max, stored[D]; gidx (the
// rows' groups) null: one group; w (the rows' weights) null: 1. Columns longer than seg entries go
// through the segment table of the copy (nlong columns, long_seg0[nlong + 1] first segments,
// seg_col / seg_k[nsegs]) and partial[nsegs][37].
FMLX_API int fmlx_colstats_csr(int f64, const long* colptr, const int* crow, const void* cval, const int* gidx,
                               const double* w, long n, long nnz, int D, int g0, int Gw, long seg, int nlong,
                               const int* long_col, const long* long_seg0, long nsegs, const int* seg_col,
                               const int* seg_k, double* partial, double* res, long* stored, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D < 1 || n < 0 || nnz < 0 || g0 < 0 || Gw < 1 || Gw > CS_GROUPS || seg < 1 || nlong < 0 || nsegs < 0) return -1;
  if (colptr == nullptr || res == nullptr || stored == nullptr) return -1;
  if (nlong > 0 && nsegs > 0 && (long_col == nullptr || long_seg0 == nullptr || seg_col == nullptr || seg_k == nullptr ||
                                 partial == nullptr))
    return -1;
  return with_acc(f64, [&](auto acc) {
    typedef decltype(acc) T;
    long blocks = ((long)D + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(colstats_csr_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, colptr, crow, (const T*)cval,
                       gidx, w, n, nnz, D, g0, Gw, seg, res, stored);
    if (nlong > 0 && nsegs > 0) {
      hipLaunchKernelGGL(colstats_csr_seg_kernel<T>, dim3((unsigned)((nsegs + 3) / 4)), dim3(256), 0, s, colptr, crow,
                         (const T*)cval, gidx, w, n, nnz, D, g0, Gw, seg, nsegs, seg_col, seg_k, partial);
      hipLaunchKernelGGL(colstats_csr_fold_kernel, dim3((unsigned)nlong), dim3(64), 0, s, long_col, long_seg0, n, D, Gw,
                         (const double*)partial, res, stored);
    }
    return (int)hipGetLastError();
  });
}

FMLX_DEFINE_PRELOAD()
