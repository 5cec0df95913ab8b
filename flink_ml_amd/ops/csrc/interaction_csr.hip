// Interaction (feature crosses) with sparse inputs, from CSR to CSR without the dense [n, Π D_c]
// matrix (the hasSparse branch of InteractionFunction.map, Interaction.java).
//
// Inputs: up to 8 columns, each a CSR column (indptr int64, indices int32 ascending in a row,
// values fp32 / fp64) or dense cells behind (pointer, ld) (a scalar column: d = 1). Row r of the
// result holds one entry per element of S_0 × … × S_{m−1}, S_c = the entries of column c whose
// value is not ±0: index Σ idx_c · Π_{c' > c} D_c' (first input slowest), value the fp64 product
// 1.0 · v_{m−1} · … · v_0 (multiplied from the last column to the first). Every S_c ascends, so
// the row ascends without a sort. The launchers hand the columns to the kernels in REVERSED
// order: kernel column 0 is the last input, the fastest digit and the first factor.
//
//  1. count: one wave per row. Per column the non-zero count is a popcount of ballots over the
//     row's stored entries (cells), 64 at a time; the row's length is the product of the counts.
//     Non-finite values and unsorted / repeated indices (the caller keeps the dense route), an
//     index outside [0, D) (the caller raises) and a row of 2^31 or more entries are OR-ed into one
//     error word. The counts go to an [n, m] table for pass 3.
//  2. prefix: len → indptr with scan.h's block scan (tile sums, one block over the sums, apply).
//  3. emit: split by OUTPUT POSITION, not by row: a block owns `chunk` consecutive entries and
//     walks them in pieces of up to 256 positions, one per thread. A piece's positions belong to
//     row segments; for every (segment, column) the block stages in LDS the window of the
//     compacted non-zero (index, value) list that the segment's positions can reach (the whole
//     list when the segment covers the row), halving the piece until the windows fit. A short
//     list is staged by the segment's first thread, a long one by its wave (ballot ranks). A
//     dense column without a zero in the row is not staged: its cells are read in place. Each
//     thread decodes position − indptr[row] in mixed radix over the row's counts (shift / mask
//     where a count is 1 or a power of two), gathers one entry per column, multiplies and stores
//     index and value coalesced. No atomics: an entry depends on its position alone, so the
//     result does not depend on the grid or the chunk size.
#include "common.h"
#include "scan.h"

namespace {

constexpr int IC_MAX = 8;                  // input columns
constexpr int IC_NT = 256;
constexpr int IC_CAP = 2048;               // staged (index, value) entries of a piece: 24 KiB of LDS
constexpr int IC_SHORT = 8;                // stored entries up to which a segment's first thread stages a list
constexpr int IC_SC_PER = 8;               // scan: values per thread, and per tile
constexpr int IC_SC_TILE = IC_NT * IC_SC_PER;
constexpr long IC_LIMIT = 1L << 31;        // a row (and the whole result) stays below this

// the error word (state[1]); ops/blas.py interaction_csr reads it
enum { IC_ERR_RANGE = 1, IC_ERR_ROUTE = 2, IC_ERR_LONG = 4 };

struct ICol {
  const long* indptr;   // nullptr: a dense column
  const int* indices;
  const void* values;   // the stored values, or a dense column's cells
  long ld;              // dense: elements between rows
  int dim;
  int f64;              // values are fp64 (else fp32)
};
struct ICols {
  ICol c[IC_MAX];       // kernel order: c[0] = the last input
  int m;
};

__device__ __forceinline__ double ic_val(const ICol& c, long i) {
  return c.f64 ? ((const double*)c.values)[i] : (double)((const float*)c.values)[i];
}
// row r's list in column c: the first element's offset, and the number of stored entries / cells
__device__ __forceinline__ void ic_list(const ICol& c, long r, long& s, long& e) {
  if (c.indptr) {
    s = c.indptr[r];
    e = c.indptr[r + 1] - s;
  } else {
    s = r * c.ld;
    e = c.dim;
  }
}
__device__ __forceinline__ int ic_idx(const ICol& c, long s, long i) { return c.indptr ? c.indices[s + i] : (int)i; }

// ---- pass 1: counts, row lengths, the error word ------------------------------------------------
__global__ __launch_bounds__(IC_NT) void ic_count_kernel(ICols a, long n, int* __restrict__ cnt,
                                                         long* __restrict__ len,
                                                         unsigned long long* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (IC_NT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (the whole wave)
  unsigned err = 0;
  long prod = 1;
#pragma unroll
  for (int j = 0; j < IC_MAX; ++j) {
    if (j >= a.m) break;
    const ICol& c = a.c[j];
    long s, e;
    ic_list(c, r, s, e);
    if (e >= IC_LIMIT) {
      err |= IC_ERR_LONG;
      e = 0;
    }
    int k = 0, prev = -1;  // prev: the last index of the 64 entries before
    for (long i0 = 0; i0 < e; i0 += 64) {
      const long i = i0 + lane;
      const bool in = i < e;
      const double v = in ? ic_val(c, s + i) : 0.0;
      const int idx = in ? ic_idx(c, s, i) : 0x7fffffff;
      int before = __shfl_up(idx, 1, 64);
      if (lane == 0) before = prev;
      prev = __shfl(idx, 63, 64);
      if (in) {
        if (!(fabs(v) <= 1.7976931348623157e308)) err |= IC_ERR_ROUTE;  // NaN, ±inf
        if (idx < 0 || idx >= c.dim) err |= IC_ERR_RANGE;
        if (idx <= before) err |= IC_ERR_ROUTE;                         // unsorted, or stored twice
      }
      k += __popcll(__ballot(in && v != 0.0));
    }
    if (lane == 0) cnt[r * a.m + j] = k;
    prod *= k;  // below 2^62: both factors are at most 2^31
    if (prod > IC_LIMIT) prod = IC_LIMIT;
  }
  if (prod >= IC_LIMIT) err |= IC_ERR_LONG;
  if (lane == 0) len[r] = prod;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) err |= __shfl_xor(err, off, 64);
  if (lane == 0 && err) atomicOr(state + 1, (unsigned long long)err);
}

// ---- pass 2: len → indptr (scan.h) ---------------------------------------------------------------
__global__ __launch_bounds__(IC_NT) void ic_tile_sum_kernel(const long* __restrict__ len, long n,
                                                            long* __restrict__ bsum) {
  __shared__ long tmp[IC_NT / 64];
  const long t0 = (long)blockIdx.x * IC_SC_TILE;
  long v = 0;
  for (int j = 0; j < IC_SC_PER; ++j) {
    const long i = t0 + (long)j * IC_NT + threadIdx.x;
    if (i < n) v += len[i];
  }
  long tot;
  block_excl_scan<IC_NT>(v, tmp, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one block: bsum[b] ← the sum of the tiles before b; the total to indptr[n] and state[0]
__global__ __launch_bounds__(1024) void ic_scan_sums_kernel(long* __restrict__ bsum, long nb, long* __restrict__ end,
                                                            long* __restrict__ total) {
  __shared__ long tmp[16];
  long carry = 0;
  for (long b0 = 0; b0 < nb; b0 += 1024) {
    const long b = b0 + threadIdx.x;
    long tot;
    const long ex = carry + block_excl_scan<1024>(b < nb ? bsum[b] : 0L, tmp, &tot);
    if (b < nb) bsum[b] = ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    *end = carry;
    *total = carry;
  }
}

// thread = IC_SC_PER consecutive rows
__global__ __launch_bounds__(IC_NT) void ic_scan_apply_kernel(const long* __restrict__ len, long n,
                                                              const long* __restrict__ bsum,
                                                              long* __restrict__ indptr) {
  __shared__ long tmp[IC_NT / 64];
  const long i0 = (long)blockIdx.x * IC_SC_TILE + (long)threadIdx.x * IC_SC_PER;
  long c[IC_SC_PER];
  long v = 0;
#pragma unroll
  for (int j = 0; j < IC_SC_PER; ++j) {
    c[j] = i0 + j < n ? len[i0 + j] : 0;
    v += c[j];
  }
  long p = bsum[blockIdx.x] + block_excl_scan<IC_NT>(v, tmp);
#pragma unroll
  for (int j = 0; j < IC_SC_PER; ++j) {
    if (i0 + j < n) indptr[i0 + j] = p;
    p += c[j];
  }
}

// ---- pass 3: emit ---------------------------------------------------------------------------------
// x = quot · c + rem (c ≥ 1), off the division path where c is 1 or a power of two
__device__ __forceinline__ void ic_divmod(unsigned x, unsigned c, unsigned& quot, unsigned& rem) {
  if ((c & (c - 1)) == 0) {
    quot = x >> (__ffs((int)c) - 1);
    rem = x & (c - 1);
  } else {
    quot = x / c;
    rem = x - quot * c;
  }
}

// the last row r of [lo, hi] with indptr[r] <= p (indptr[lo] <= p): for p below indptr[hi + 1]
// the row that holds position p, never an empty one
__device__ __forceinline__ long ic_row_of(const long* __restrict__ indptr, long lo, long hi, long p) {
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (indptr[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the slot of the list's k-th non-zero in a window that starts at digit d0 (the window wraps)
__device__ __forceinline__ int ic_slot(int k, int d0, int c) {
  const int s = k - d0;
  return s < 0 ? s + c : s;
}

__global__ __launch_bounds__(IC_NT) void ic_emit_kernel(ICols a, long n, const int* __restrict__ cnt,
                                                        const long* __restrict__ indptr, long total, int chunk,
                                                        int* __restrict__ out_idx, double* __restrict__ out_val) {
  __shared__ int s_idx[IC_CAP];
  __shared__ double s_val[IC_CAP];
  __shared__ int tmp[IC_NT / 64];
  const int t = threadIdx.x, lane = t & 63;
  const long p0 = (long)blockIdx.x * chunk;
  const long p1 = p0 + chunk < total ? p0 + chunk : total;
  const long r0 = ic_row_of(indptr, 0, n - 1, p0), r1 = ic_row_of(indptr, r0, n - 1, p1 - 1);

  for (long pa = p0; pa < p1;) {
    // my position of the piece, its row and the row's counts
    const long p = pa + t;
    long r = r0, ip = 0, ipn = 0;
    int cn[IC_MAX];
#pragma unroll
    for (int j = 0; j < IC_MAX; ++j) cn[j] = 1;
    if (p < p1) {
      r = ic_row_of(indptr, r0, r1, p);
      ip = indptr[r];
      ipn = indptr[r + 1];
#pragma unroll
      for (int j = 0; j < IC_MAX; ++j)
        if (j < a.m) cn[j] = cnt[r * a.m + j];
    }
    // the longest piece [pa, pb) whose windows fit in LDS. My segment = my row's positions inside
    // the piece, lo … hi counted from the row's first; column j's digit of position x is
    // (x / s_j) mod cn[j], s_j = the product of the counts before j, so the segment reaches the
    // w[j] = min(cn[j], hi / s_j − lo / s_j + 1) digits from d0[j] = (lo / s_j) mod cn[j] on,
    // cyclically. One position reaches one digit per column, so a piece of one always fits.
    int d0[IC_MAX], w[IC_MAX];  // w[j] = 0: a dense column without a zero in this row, read in place
    int need, before, pl = IC_NT;
    long pb;
    bool act, head;
    for (;;) {
      pb = pa + pl < p1 ? pa + pl : p1;
      act = p < pb;
      head = act && (t == 0 || p == ip);
      need = 0;
#pragma unroll
      for (int j = 0; j < IC_MAX; ++j) d0[j] = w[j] = 0;
      if (act) {
        unsigned xl = pa > ip ? (unsigned)(pa - ip) : 0u;
        unsigned xh = (unsigned)((ipn < pb ? ipn : pb) - 1 - ip);
#pragma unroll
        for (int j = 0; j < IC_MAX; ++j) {
          if (j >= a.m) break;
          const unsigned c = (unsigned)cn[j];
          unsigned ql, dl, qh, dh;
          ic_divmod(xl, c, ql, dl);
          ic_divmod(xh, c, qh, dh);
          const unsigned span = xh - xl + 1;
          const bool direct = a.c[j].indptr == nullptr && cn[j] == a.c[j].dim;
          d0[j] = (int)dl;
          w[j] = direct ? 0 : (int)(span < c ? span : c);
          need += w[j];
          xl = ql;
          xh = qh;
        }
      }
      int tot;
      before = block_excl_scan<IC_NT>(head ? need : 0, tmp, &tot);
      if (tot <= IC_CAP) break;  // (the whole block)
      pl >>= 1;
    }
    const int base = head ? before : before - need;  // my segment's first LDS entry

    // stage the windows: a short list by the segment's first thread, a long one by its wave
    unsigned longmask = 0;
    if (head) {
      int o = base;
#pragma unroll
      for (int j = 0; j < IC_MAX; ++j) {
        if (j >= a.m) break;
        if (w[j] == 0) continue;
        const ICol& c = a.c[j];
        long s, e;
        ic_list(c, r, s, e);
        if (e <= IC_SHORT) {
          int k = 0;
          for (long i = 0; i < e; ++i) {
            const double v = ic_val(c, s + i);
            if (v != 0.0) {
              const int slot = ic_slot(k, d0[j], cn[j]);
              if (slot < w[j]) {
                s_idx[o + slot] = ic_idx(c, s, i);
                s_val[o + slot] = v;
              }
              ++k;
            }
          }
        } else {
          longmask |= 1u << j;
        }
        o += w[j];
      }
    }
    for (unsigned long long hb = __ballot(longmask != 0); hb; hb &= hb - 1) {
      const int h = __ffsll((long long)hb) - 1;
      const long hr = __shfl(r, h, 64);
      const unsigned hm = __shfl(longmask, h, 64);
      int o = __shfl(base, h, 64);
#pragma unroll
      for (int j = 0; j < IC_MAX; ++j) {
        if (j >= a.m) break;
        const int hw = __shfl(w[j], h, 64), hd0 = __shfl(d0[j], h, 64), hc = __shfl(cn[j], h, 64);
        if ((hm >> j) & 1) {
          const ICol& c = a.c[j];
          long s, e;
          ic_list(c, hr, s, e);
          int kb = 0;  // non-zeros before these 64 entries
          for (long i0 = 0; i0 < e; i0 += 64) {
            const long i = i0 + lane;
            const double v = i < e ? ic_val(c, s + i) : 0.0;
            const unsigned long long bal = __ballot(v != 0.0);
            if (v != 0.0) {
              const int k = kb + __popcll(bal & ((1ull << lane) - 1));
              const int slot = ic_slot(k, hd0, hc);
              if (slot < hw) {
                s_idx[o + slot] = ic_idx(c, s, i);
                s_val[o + slot] = v;
              }
            }
            kb += __popcll(bal);
          }
        }
        o += hw;
      }
    }
    __syncthreads();

    if (act) {
      unsigned x = (unsigned)(p - ip);
      int o = base, index = 0, stride = 1;
      double v = 1.0;
#pragma unroll
      for (int j = 0; j < IC_MAX; ++j) {
        if (j >= a.m) break;
        unsigned q, dg;
        ic_divmod(x, (unsigned)cn[j], q, dg);
        int ix;
        double f;
        if (w[j] == 0) {
          ix = (int)dg;
          f = ic_val(a.c[j], r * a.c[j].ld + dg);
        } else {
          const int slot = ic_slot((int)dg, d0[j], cn[j]);
          ix = s_idx[o + slot];
          f = s_val[o + slot];
          o += w[j];
        }
        v *= f;
        index += ix * stride;
        stride *= a.c[j].dim;
        x = q;
      }
      out_idx[p] = index;
      out_val[p] = v;
    }
    __syncthreads();  // the next piece overwrites the windows
    pa = pb;
  }
}

// the columns in kernel order (reversed); false: not 1 … 8 columns, a width that is not positive,
// or Π D_c ≥ 2^31
bool ic_pack(ICols& a, int m, const void* const* indptr, const void* const* indices, const void* const* values,
             const long* ld, const long* dim, const int* f64) {
  if (m < 1 || m > IC_MAX) return false;
  a = ICols{};
  a.m = m;
  long width = 1;
  for (int j = 0; j < m; ++j) {
    const int q = m - 1 - j;
    if (dim[q] < 1 || dim[q] >= IC_LIMIT) return false;
    if ((indptr[q] == nullptr) != (indices[q] == nullptr)) return false;
    width *= dim[q];
    if (width >= IC_LIMIT) return false;
    a.c[j] = ICol{(const long*)indptr[q], (const int*)indices[q], values[q], ld[q], (int)dim[q], f64[q]};
  }
  return true;
}

}  // namespace

// longs of scratch that fmlx_interaction_csr_count needs for n rows
FMLX_API long fmlx_interaction_csr_scratch(long n) { return n <= 0 ? 1 : (n + IC_SC_TILE - 1) / IC_SC_TILE; }

// Passes 1 and 2. Column q of m: indptr[q] / indices[q] (both null: dense cells behind values[q] with
// row stride ld[q]), dim[q] = D_q, f64[q] = its values are fp64 (else fp32). cnt: int32 [n, m],
// len: int64 [n], out_indptr: int64 [n + 1], state: int64 [2], zeroed by the caller:
// state[0] ← the number of entries, state[1] |= the error word.
FMLX_API int fmlx_interaction_csr_count(int m, const void* const* indptr, const void* const* indices,
                                        const void* const* values, const long* ld, const long* dim, const int* f64,
                                        long n, int* cnt, long* len, long* scratch, long* out_indptr, long* state,
                                        void* stream) {
  ICols a;
  if (!ic_pack(a, m, indptr, indices, values, ld, dim, f64) || n < 1 || n >= IC_LIMIT) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ic_count_kernel, dim3((unsigned)((n + IC_NT / 64 - 1) / (IC_NT / 64))), dim3(IC_NT), 0, st, a, n,
                     cnt, len, (unsigned long long*)state);
  const long nb = (n + IC_SC_TILE - 1) / IC_SC_TILE;
  hipLaunchKernelGGL(ic_tile_sum_kernel, dim3((unsigned)nb), dim3(IC_NT), 0, st, len, n, scratch);
  hipLaunchKernelGGL(ic_scan_sums_kernel, dim3(1), dim3(1024), 0, st, scratch, nb, out_indptr + n, state);
  hipLaunchKernelGGL(ic_scan_apply_kernel, dim3((unsigned)nb), dim3(IC_NT), 0, st, len, n, scratch, out_indptr);
  FMLX_CHECK_LAUNCH();
}

// Pass 3: the `total` entries (0 < total < 2^31, the count pass's state[0]) behind out_indptr into
// out_idx / out_val; a block owns `chunk` consecutive entries (any chunk ≥ 1 gives the same bits).
FMLX_API int fmlx_interaction_csr_emit(int m, const void* const* indptr, const void* const* indices,
                                       const void* const* values, const long* ld, const long* dim, const int* f64,
                                       long n, const int* cnt, const long* out_indptr, long total, int chunk,
                                       int* out_idx, double* out_val, void* stream) {
  ICols a;
  if (!ic_pack(a, m, indptr, indices, values, ld, dim, f64) || n < 1 || chunk < 1) return -1;
  if (total <= 0) return 0;
  if (total >= IC_LIMIT) return -2;
  hipLaunchKernelGGL(ic_emit_kernel, dim3((unsigned)((total + chunk - 1) / chunk)), dim3(IC_NT), 0,
                     (hipStream_t)stream, a, n, cnt, out_indptr, total, chunk, out_idx, out_val);
  FMLX_CHECK_LAUNCH();
}

FMLX_DEFINE_PRELOAD()
