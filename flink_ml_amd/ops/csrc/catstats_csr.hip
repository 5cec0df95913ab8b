// Contingency tables of a CSR feature column, and NaiveBayes prediction on one, without an n x D
// matrix (ChiSqTest K20, NaiveBayes K22 on the sparse columns HashingTF / CountVectorizer emit).
//
// A (column, value, label) count needs only the stored entries: the rows that store nothing in a
// column hold the value 0 there, and their count per label is n_label − Σ stored counts.
//   ccsr_keys     a wave per row: sort key column << 32 | k32 and the payload (the row's label index)
//                 per entry. k32 is the ordered key of an fp32 value (catkeys.h), or the rank of an
//                 fp64 value among the distinct values of the whole column (ccsr_vkeys / ccsr_vids:
//                 one more sort of the 64-bit value keys), so one 64-bit radix sort orders
//                 (column, value) for both dtypes. An index outside [0, D) gets the key ~0 (sorted
//                 last, counted nowhere) and sets the error word.
//   ccsr_heads    per tile of CC_TILE sorted entries: the number of (column, value) run heads;
//   ccsr_scan     one block: exclusive prefix of an int64 array (tile heads → distinct ids; the
//                 columns' value counts → colfirst);
//   ccsr_count    per tile: counts[id][label] with an LDS-privatised integer table when the tile's
//                 id span × L fits (flushed with integer atomics: a run may cross tiles), integer
//                 atomics to the global table otherwise; the heads write their column and value.
//                 Weighted form (the merge of several ranks' tables): the payload names a row of a
//                 [rows, L] weight table that is added instead of 1.
//   ccsr_columns  per column: its range of distinct ids, whether it stores the value 0 and whether
//                 a zero row has to be inserted (no stored zero, but fewer stored entries than rows);
//   ccsr_scatter / ccsr_zero   the final ragged table: stored rows moved past an inserted zero row,
//                 the zero row = n_label − Σ of the column's other rows.
// Integer counts throughout: the result is exact and does not depend on the grid.
//
//   nb_csr_predict  a wave per row, a lane per label: score = base[l] + Σ over the stored entries of
//                 delta[off_j + pos_j(v)][l] (the model's log-probabilities relative to the value 0),
//                 pos by a binary search per entry, added in stored-entry order; first maximum.
#include "catkeys.h"
#include "common.h"
#include "scan.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_PER = 8;
constexpr int CC_TILE = CC_THREADS * CC_PER;
constexpr int CC_LDS_INTS = 8 * 1024;  // 32 KiB: the privatised table of one tile
constexpr uint64_t CC_SKIP = ~0ull;    // no (column < 2^31, k32) pair and no value key (catkeys.h) is all ones

inline unsigned cc_grid(long work, long per_block, long cap) {
  long b = (work + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// {OR, AND} of the thread's keys into orand (one pair of atomics per wave)
__device__ __forceinline__ void cc_orand(unsigned long long o, unsigned long long a,
                                         unsigned long long* __restrict__ orand) {
  for (int off = 32; off > 0; off >>= 1) {
    o |= __shfl_xor(o, off, 64);
    a &= __shfl_xor(a, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicOr(orand, o);
    atomicAnd(orand + 1, a);
  }
}

// 64-bit value keys of fp64 values (entry m: the value 0, so that the ranks always hold it)
__global__ __launch_bounds__(CC_THREADS) void ccsr_vkeys_kernel(const double* __restrict__ val, long m,
                                                                uint64_t* __restrict__ keys,
                                                                uint32_t* __restrict__ pay,
                                                                unsigned long long* __restrict__ orand) {
  unsigned long long o = 0, a = ~0ull;
  for (long e = (long)blockIdx.x * CC_THREADS + threadIdx.x; e <= m; e += (long)gridDim.x * CC_THREADS) {
    const uint64_t k = asc_key(e < m ? val[e] : 0.0);
    keys[e] = k;
    pay[e] = (uint32_t)e;
    o |= k;
    a &= k;
  }
  cc_orand(o, a, orand);
}

__device__ __forceinline__ bool cc_head(const uint64_t* __restrict__ keys, long e) {
  const uint64_t k = keys[e];
  return k != CC_SKIP && (e == 0 || k != keys[e - 1]);
}

__global__ __launch_bounds__(CC_THREADS) void ccsr_heads_kernel(const uint64_t* __restrict__ keys, long total,
                                                                long* __restrict__ tcnt) {
  __shared__ long sh[CC_WAVES];
  const long base = (long)blockIdx.x * CC_TILE;
  long c = 0;
  for (int q = 0; q < CC_PER; ++q) {
    const long e = base + (long)q * CC_THREADS + threadIdx.x;
    if (e < total && cc_head(keys, e)) ++c;
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < CC_WAVES; ++q) c += sh[q];
    tcnt[blockIdx.x] = c;
  }
}

// one block: a ← exclusive prefix of a[0..m); a[m] = total
__global__ __launch_bounds__(1024) void ccsr_scan_kernel(long* __restrict__ a, long m) {
  __shared__ long tmp[16];
  long run = 0;
  for (long base = 0; base < m; base += 1024) {
    const long t = base + threadIdx.x;
    long tot;
    const long ex = run + block_excl_scan<1024>(t < m ? a[t] : 0L, tmp, &tot);
    if (t < m) a[t] = ex;
    run += tot;
  }
  if (threadIdx.x == 0) a[m] = run;
}

// value ranks: vid[entry] = distinct id of its value, gval[id] = the value
__global__ __launch_bounds__(CC_THREADS) void ccsr_vids_kernel(const uint64_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ pay, long total,
                                                               const long* __restrict__ tcnt,
                                                               uint32_t* __restrict__ vid,
                                                               double* __restrict__ gval) {
  __shared__ long sh[CC_WAVES];
  const long e0 = (long)blockIdx.x * CC_TILE + (long)threadIdx.x * CC_PER;
  int hc = 0;
  bool hd[CC_PER];
#pragma unroll
  for (int q = 0; q < CC_PER; ++q) {
    hd[q] = e0 + q < total && cc_head(keys, e0 + q);
    hc += hd[q];
  }
  long g = tcnt[blockIdx.x] + block_excl_scan<CC_THREADS>((long)hc, sh) - 1;
#pragma unroll
  for (int q = 0; q < CC_PER; ++q) {
    const long e = e0 + q;
    if (e < total) {
      if (hd[q]) gval[++g] = key_val(keys[e]);
      const uint32_t p = pay[e];
      if ((long)p < total - 1) vid[p] = (uint32_t)g;  // (entry total − 1 is the added zero)
    }
  }
}

__device__ __forceinline__ uint64_t cc_key(int j, int D, int l, int L, uint32_t k32, bool& bad) {
  if ((unsigned)j >= (unsigned)D) {
    bad = true;
    return CC_SKIP;
  }
  if ((unsigned)l >= (unsigned)L) return CC_SKIP;  // a row without a label index counts nowhere
  return ((uint64_t)(uint32_t)j << 32) | k32;
}

// a wave per row of the CSR column
__global__ __launch_bounds__(CC_THREADS) void ccsr_keys_kernel(const long* __restrict__ indptr,
                                                               const int* __restrict__ idx,
                                                               const float* __restrict__ val,
                                                               const uint32_t* __restrict__ vid,
                                                               const int* __restrict__ li, long n, int D, int L,
                                                               uint64_t* __restrict__ keys,
                                                               uint32_t* __restrict__ pay,
                                                               unsigned long long* __restrict__ orand,
                                                               int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * CC_WAVES;
  unsigned long long o = 0, a = ~0ull;
  bool bad = false;
  for (long r = wave; r < n; r += nwaves) {
    const long s = indptr[r], e = indptr[r + 1];
    const int l = li[r];
    for (long p = s + lane; p < e; p += 64) {
      const uint64_t k = cc_key(idx[p], D, l, L, val ? asc_key32(val[p]) : vid[p], bad);
      keys[p] = k;
      pay[p] = (uint32_t)l;
      o |= k;
      a &= k;
    }
  }
  cc_orand(o, a, orand);
  if (bad) *err = 1;
}

// the rows of gathered tables as entries: payload = the row (ccsr_count's weighted form)
__global__ __launch_bounds__(CC_THREADS) void ccsr_ekeys_kernel(const int* __restrict__ col,
                                                                const uint32_t* __restrict__ vid, long m, int D,
                                                                uint64_t* __restrict__ keys,
                                                                uint32_t* __restrict__ pay,
                                                                unsigned long long* __restrict__ orand,
                                                                int* __restrict__ err) {
  unsigned long long o = 0, a = ~0ull;
  bool bad = false;
  for (long e = (long)blockIdx.x * CC_THREADS + threadIdx.x; e < m; e += (long)gridDim.x * CC_THREADS) {
    const uint64_t k = cc_key(col[e], D, 0, 1, vid[e], bad);
    keys[e] = k;
    pay[e] = (uint32_t)e;
    o |= k;
    a &= k;
  }
  cc_orand(o, a, orand);
  if (bad) *err = 1;
}

// counts[id·L + label] over a tile of sorted entries; heads write ucol / uval at their id.
// paths[0] / paths[1]: tiles counted through LDS / with global atomics.
template <bool WEIGHTED>
__global__ __launch_bounds__(CC_THREADS) void ccsr_count_kernel(const uint64_t* __restrict__ keys,
                                                                const uint32_t* __restrict__ pay, long total,
                                                                const long* __restrict__ tcnt, int L,
                                                                const int* __restrict__ W,
                                                                const double* __restrict__ gval,
                                                                int* __restrict__ cnt, int* __restrict__ ucol,
                                                                double* __restrict__ uval,
                                                                int* __restrict__ paths) {
  __shared__ int h[CC_LDS_INTS];
  __shared__ long sh[CC_WAVES];
  const long t0 = (long)blockIdx.x * CC_TILE;
  if (keys[t0] == CC_SKIP) return;  // (sorted last: the whole tile is skipped entries)
  const long e0 = t0 + (long)threadIdx.x * CC_PER;
  int hc = 0;
  bool hd[CC_PER];
#pragma unroll
  for (int q = 0; q < CC_PER; ++q) {
    hd[q] = e0 + q < total && cc_head(keys, e0 + q);
    hc += hd[q];
  }
  long tot;
  const long pre = block_excl_scan<CC_THREADS>((long)hc, sh, &tot);
  const long tb = tcnt[blockIdx.x];
  const long g_lo = tb - (cc_head(keys, t0) ? 0 : 1);  // id of the tile's first entry
  const long span = tb + tot - g_lo;                    // ids g_lo … tb + tot − 1
  const bool lds = span * L <= CC_LDS_INTS;
  if (lds) {
    for (int i = threadIdx.x; i < (int)(span * L); i += CC_THREADS) h[i] = 0;
    __syncthreads();
  }
  long g = tb + pre - 1;
#pragma unroll
  for (int q = 0; q < CC_PER; ++q) {
    const long e = e0 + q;
    if (e >= total) break;
    const uint64_t k = keys[e];
    if (k == CC_SKIP) break;
    if (hd[q]) {
      ++g;
      ucol[g] = (int)(k >> 32);
      uval[g] = gval ? gval[(uint32_t)k] : (double)key32_val((uint32_t)k);
    }
    const uint32_t p = pay[e];
    if (WEIGHTED) {
      for (int l = 0; l < L; ++l) {
        const int w = W[(long)p * L + l];
        if (w) {
          if (lds)
            atomicAdd(&h[(g - g_lo) * L + l], w);
          else
            atomicAdd(&cnt[g * L + l], w);
        }
      }
    } else {
      if (lds)
        atomicAdd(&h[(g - g_lo) * L + p], 1);
      else
        atomicAdd(&cnt[g * L + p], 1);
    }
  }
  if (lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)(span * L); i += CC_THREADS)
      if (h[i]) atomicAdd(&cnt[g_lo * L + i], h[i]);
  }
  if (threadIdx.x == 0) atomicAdd(&paths[lds ? 0 : 1], 1);
}

// first id in ucol[0..U) whose column is >= j
__device__ __forceinline__ long cc_col_lower(const int* __restrict__ ucol, long U, int j) {
  long lo = 0, hi = U;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (ucol[mid] < j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// per column j: gf[j] = its first distinct id (gf[D] = U); zr[j] = where the value 0 sits / belongs
// among its values; flag[j] = 1 the column stores 0, 2 a zero row is inserted (stored counts < rows),
// 0 no zero row; vcount[j] = values of the final table
__global__ __launch_bounds__(CC_THREADS) void ccsr_columns_kernel(const int* __restrict__ ucol,
                                                                  const double* __restrict__ uval,
                                                                  const int* __restrict__ cnt, long U, int D, int L,
                                                                  long nrows, long* __restrict__ gf,
                                                                  int* __restrict__ flag, int* __restrict__ zr,
                                                                  long* __restrict__ vcount) {
  const long j = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (j > D) return;
  const long a = cc_col_lower(ucol, U, (int)j);
  gf[j] = a;
  if (j == D) return;
  const long b = cc_col_lower(ucol, U, (int)j + 1);
  long lo = a, hi = b;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (uval[mid] < 0.0)  // (NaN last: never below 0)
      lo = mid + 1;
    else
      hi = mid;
  }
  int f = 0;
  if (lo < b && uval[lo] == 0.0) {
    f = 1;
  } else {
    long stored = 0;
    for (long c = a * L; c < b * L; ++c) stored += cnt[c];
    if (stored < nrows) f = 2;
  }
  flag[j] = f;
  zr[j] = (int)(lo - a);
  vcount[j] = (b - a) + (f == 2);
}

// the stored rows at their final places (a stored zero row is written by ccsr_zero_kernel)
__global__ __launch_bounds__(CC_THREADS) void ccsr_scatter_kernel(const int* __restrict__ ucol,
                                                                  const double* __restrict__ uval,
                                                                  const int* __restrict__ cnt, long U, int L,
                                                                  const long* __restrict__ gf,
                                                                  const int* __restrict__ flag,
                                                                  const int* __restrict__ zr,
                                                                  const long* __restrict__ colfirst,
                                                                  double* __restrict__ values,
                                                                  int* __restrict__ out) {
  const long total = U * L;
  for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CC_THREADS) {
    const long g = i / L;
    const int l = (int)(i - g * L);
    const int j = ucol[g];
    const long rel = g - gf[j];
    const int f = flag[j], z = zr[j];
    if (f == 1 && rel == z) continue;
    const long o = colfirst[j] + rel + (f == 2 && rel >= z ? 1 : 0);
    out[o * L + l] = cnt[i];
    if (l == 0) values[o] = uval[g];
  }
}

// zero row of column j, label l: n_label[l] − Σ of the column's other rows
__global__ __launch_bounds__(CC_THREADS) void ccsr_zero_kernel(const int* __restrict__ cnt, int D, int L,
                                                               const long* __restrict__ gf,
                                                               const int* __restrict__ flag,
                                                               const int* __restrict__ zr,
                                                               const long* __restrict__ colfirst,
                                                               const long* __restrict__ n_label,
                                                               double* __restrict__ values, int* __restrict__ out) {
  const long total = (long)D * L;
  for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CC_THREADS) {
    const long j = i / L;
    const int l = (int)(i - j * L);
    const int f = flag[j];
    if (f == 0) continue;
    const long a = gf[j], b = gf[j + 1], skip = f == 1 ? a + zr[j] : -1;
    long s = 0;
    for (long g = a; g < b; ++g)
      if (g != skip) s += cnt[g * L + l];
    const long o = colfirst[j] + zr[j];
    out[o * L + l] = (int)(n_label[l] - s);
    if (l == 0) values[o] = 0.0;
  }
}

// ---- NaiveBayes prediction ------------------------------------------------------------------
// vflat[off[j] … off[j + 1]): the model's sorted values of feature j; delta[(off[j] + pos)·L + l] the
// log-probability of that value relative to the value 0 of the feature (to nothing where the model
// has no value 0). unseen: the lowest feature with a value the model does not hold (atomicMin).
__global__ __launch_bounds__(CC_THREADS) void nb_csr_predict_kernel(const long* __restrict__ indptr,
                                                                    const int* __restrict__ idx,
                                                                    const double* __restrict__ val, long n, int D,
                                                                    const long* __restrict__ off,
                                                                    const double* __restrict__ vflat,
                                                                    const double* __restrict__ delta,
                                                                    const double* __restrict__ base, int L,
                                                                    int* __restrict__ pred,
                                                                    int* __restrict__ unseen,
                                                                    int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * CC_WAVES;
  bool bad = false;
  int miss = 0x7fffffff;
  for (long r = wave; r < n; r += nwaves) {
    const long s = indptr[r], e = indptr[r + 1];
    double best = -__builtin_huge_val();
    int bi = 0x7fffffff;
    for (int l0 = 0; l0 < L; l0 += 64) {
      const int l = l0 + lane;
      double acc = l < L ? base[l] : 0.0;
      for (long b0 = s; b0 < e; b0 += 64) {
        const long p = b0 + lane;
        int pos = -1;
        if (p < e) {
          const int j = idx[p];
          if ((unsigned)j >= (unsigned)D) {
            bad = true;
          } else {
            const double v = val[p];
            long lo = off[j], hi = off[j + 1];
            const long end = hi;
            while (lo < hi) {
              const long mid = (lo + hi) >> 1;
              if (vflat[mid] < v)
                lo = mid + 1;
              else
                hi = mid;
            }
            if (lo < end && vflat[lo] == v)  // (−0 == +0; a NaN is never seen)
              pos = (int)lo;
            else
              miss = j < miss ? j : miss;
          }
        }
        const int cnt = (int)(e - b0 < 64 ? e - b0 : 64);
        for (int t = 0; t < cnt; ++t) {
          const int pt = __builtin_amdgcn_readlane(pos, t);
          if (pt >= 0 && l < L) acc += delta[(long)pt * L + l];
        }
      }
      if (l < L && (bi == 0x7fffffff || acc > best)) {  // (a lane's labels ascend: strict keeps the first)
        best = acc;
        bi = l;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) {
        best = ob;
        bi = oi;
      }
    }
    if (lane == 0) pred[r] = bi == 0x7fffffff ? 0 : bi;
  }
  if (miss != 0x7fffffff) atomicMin(unseen, miss);
  if (bad) *err = 1;
}

}  // namespace

FMLX_API int fmlx_ccsr_tile() { return CC_TILE; }
FMLX_API int fmlx_ccsr_lds_ints() { return CC_LDS_INTS; }

// keys / pay [m + 1]: the ordered 64-bit keys of val[0..m) and of one added 0.0, payload = entry;
// orand: device {OR, AND}, filled {0, ~0} by the caller
FMLX_API int fmlx_ccsr_vkeys(const double* val, long m, uint64_t* keys, uint32_t* pay, unsigned long long* orand,
                             void* stream) {
  if (m < 0 || m + 1 >= (1L << 31)) return -2;
  hipLaunchKernelGGL(ccsr_vkeys_kernel, dim3(cc_grid(m + 1, CC_THREADS * 8L, 4096)), dim3(CC_THREADS), 0,
                     (hipStream_t)stream, val, m, keys, pay, orand);
  return (int)hipGetLastError();
}

// sorted value keys [m + 1] → vid[m] (rank of every entry's value), gval[≤ m + 1] (the values);
// tcnt: int64 [tiles + 1] scratch, tcnt[tiles] = number of distinct values afterwards
FMLX_API int fmlx_ccsr_vids(const uint64_t* keys, const uint32_t* pay, long m, long* tcnt, uint32_t* vid, double* gval,
                            void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long total = m + 1, nt = (total + CC_TILE - 1) / CC_TILE;
  hipLaunchKernelGGL(ccsr_heads_kernel, dim3((unsigned)nt), dim3(CC_THREADS), 0, s, keys, total, tcnt);
  hipLaunchKernelGGL(ccsr_scan_kernel, dim3(1), dim3(1024), 0, s, tcnt, nt);
  hipLaunchKernelGGL(ccsr_vids_kernel, dim3((unsigned)nt), dim3(CC_THREADS), 0, s, keys, pay, total, tcnt, vid, gval);
  return (int)hipGetLastError();
}

// (column << 32 | k32, label index) per entry of the CSR column; k32 from val (fp32) or vid, one of
// them null. err: set for an index outside [0, D)
FMLX_API int fmlx_ccsr_keys(const long* indptr, const int* idx, const float* val, const uint32_t* vid, const int* li,
                            long n, int D, int L, uint64_t* keys, uint32_t* pay, unsigned long long* orand, int* err,
                            void* stream) {
  if (n <= 0) return 0;
  if ((val == nullptr) == (vid == nullptr) || D < 1 || L < 1) return -2;
  hipLaunchKernelGGL(ccsr_keys_kernel, dim3(cc_grid(n, CC_WAVES, 8192)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                     indptr, idx, val, vid, li, n, D, L, keys, pay, orand, err);
  return (int)hipGetLastError();
}

// the same for m table rows (col, vid): payload = the row
FMLX_API int fmlx_ccsr_ekeys(const int* col, const uint32_t* vid, long m, int D, uint64_t* keys, uint32_t* pay,
                             unsigned long long* orand, int* err, void* stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(ccsr_ekeys_kernel, dim3(cc_grid(m, CC_THREADS * 8L, 4096)), dim3(CC_THREADS), 0,
                     (hipStream_t)stream, col, vid, m, D, keys, pay, orand, err);
  return (int)hipGetLastError();
}

// tcnt int64 [tiles + 1] of the sorted keys: exclusive prefix of the tiles' run heads, tcnt[tiles] = U
FMLX_API int fmlx_ccsr_runs(const uint64_t* keys, long total, long* tcnt, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (total <= 0) return -2;
  const long nt = (total + CC_TILE - 1) / CC_TILE;
  hipLaunchKernelGGL(ccsr_heads_kernel, dim3((unsigned)nt), dim3(CC_THREADS), 0, s, keys, total, tcnt);
  hipLaunchKernelGGL(ccsr_scan_kernel, dim3(1), dim3(1024), 0, s, tcnt, nt);
  return (int)hipGetLastError();
}

// cnt int32 [U, L] (zeroed by the caller), ucol [U], uval [U]; W null: payload = label index, else the
// row of the int32 weight table W[rows, L]; gval null: k32 is an fp32 value key; paths int32 [2]
FMLX_API int fmlx_ccsr_count(const uint64_t* keys, const uint32_t* pay, long total, const long* tcnt, int L, const int* W,
                             const double* gval, int* cnt, int* ucol, double* uval, int* paths, void* stream) {
  if (total <= 0 || L < 1) return -2;
  const long nt = (total + CC_TILE - 1) / CC_TILE;
  return with_bool(W != nullptr, [&](auto wt) {
    hipLaunchKernelGGL((ccsr_count_kernel<wt.value>), dim3((unsigned)nt), dim3(CC_THREADS), 0, (hipStream_t)stream, keys,
                       pay, total, tcnt, L, W, gval, cnt, ucol, uval, paths);
    return (int)hipGetLastError();
  });
}

// gf int64 [D + 1], flag / zr int32 [D], colfirst int64 [D + 1] (exclusive prefix of the columns'
// value counts; colfirst[D] = rows of the final table)
FMLX_API int fmlx_ccsr_columns(const int* ucol, const double* uval, const int* cnt, long U, int D, int L, long nrows,
                               long* gf, int* flag, int* zr, long* colfirst, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D < 1 || L < 1) return -2;
  hipLaunchKernelGGL(ccsr_columns_kernel, dim3((unsigned)((D + (long)CC_THREADS) / CC_THREADS)), dim3(CC_THREADS), 0, s,
                     ucol, uval, cnt, U, D, L, nrows, gf, flag, zr, colfirst);
  hipLaunchKernelGGL(ccsr_scan_kernel, dim3(1), dim3(1024), 0, s, colfirst, (long)D);
  return (int)hipGetLastError();
}

// values fp64 [colfirst[D]], out int32 [colfirst[D], L]: every cell is written
FMLX_API int fmlx_ccsr_merge(const int* ucol, const double* uval, const int* cnt, long U, int D, int L, const long* gf,
                             const int* flag, const int* zr, const long* colfirst, const long* n_label, double* values,
                             int* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (U > 0)
    hipLaunchKernelGGL(ccsr_scatter_kernel, dim3(cc_grid(U * L, CC_THREADS * 4L, 8192)), dim3(CC_THREADS), 0, s, ucol,
                       uval, cnt, U, L, gf, flag, zr, colfirst, values, out);
  hipLaunchKernelGGL(ccsr_zero_kernel, dim3(cc_grid((long)D * L, CC_THREADS * 4L, 8192)), dim3(CC_THREADS), 0, s, cnt, D,
                     L, gf, flag, zr, colfirst, n_label, values, out);
  return (int)hipGetLastError();
}

// pred int32 [n] (index of the first maximal score); unseen: int32, filled 0x7fffffff by the caller
FMLX_API int fmlx_nb_csr_predict(const long* indptr, const int* idx, const double* val, long n, int D, const long* off,
                                 const double* vflat, const double* delta, const double* base, int L, int* pred,
                                 int* unseen, int* err, void* stream) {
  if (n <= 0) return 0;
  if (D < 1 || L < 1) return -2;
  hipLaunchKernelGGL(nb_csr_predict_kernel, dim3(cc_grid(n, CC_WAVES, 8192)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                     indptr, idx, val, n, D, off, vflat, delta, base, L, pred, unseen, err);
  return (int)hipGetLastError();
}

FMLX_DEFINE_PRELOAD()
