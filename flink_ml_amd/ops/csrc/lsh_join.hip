// MinHashLSH search after the signatures: the similarity join's co-group, its pair de-duplication
// and the Jaccard distances, and the nearest-neighbour bucket filter (reference LSHModel.java:
// 150-252, approxNearestNeighbors / approxSimilarityJoin, and MinHashLSHModelData.keyDistance).
//
// Join, per call (ops/lsh.py similarity_join drives the launches):
//   lsh_keys    every (row, table) entry of A and of B → a 64-bit bucket key (h63 << 1) | side and
//               the row as payload, table-major: table t is the segment [t·L, (t + 1)·L), L = na + nb.
//               h63 is the signature's bit pattern (F = 1) or a 63-bit mix of the F patterns; equal
//               signatures give equal keys, and nothing else is asked of it (emit compares the
//               signatures themselves). The launch also ORs / ANDs the keys (the sort's bit range)
//               and flags NaN, ±inf and −0.0, whose equality the host leaves to the torch path.
//   (radix.hip) a stable segmented sort: inside a table the entries of a bucket are contiguous, A's
//               before B's.
//   lsh_count   per A entry the range [lo, hi) of its bucket's B entries (two binary searches of
//               key | 1 inside the table's segment), cnt = hi − lo.
//   scan        cnt → int64 offsets: block sums, a one-block scan of the sums, apply (three
//               launches; no block ever waits for another).
//   lsh_emit    one launch per chunk of candidates [c0, c1): 16 lanes per candidate, four
//               candidates per wave. The candidate's A entry by binary search over the offsets; the
//               pair is dropped unless the two signatures of table t are equal value by value, and
//               dropped if an earlier table's are too (every pair comes from its first matching
//               table, once: no pair sort, no unique). Then the Jaccard distance; pairs within the
//               threshold are appended through one atomic per wave.
//   lsh_gather  after the host's sort of the survivors by (a, b): rows and distances in that order.
// The distance of two CSR rows: the lanes stride over the shorter row and binary-search the
// longer; 1 − |∩| / |∪| as one fp64 division and one subtraction.
//
// Integer work only apart from that division; ordinary vector stores and global integer atomics.
#include "common.h"
#include "scan.h"

namespace {

constexpr int LJ_THREADS = 256;
constexpr int LJ_GROUP = 16;                       // lanes per candidate pair
constexpr int LJ_PER_BLOCK = LJ_THREADS / LJ_GROUP;
constexpr int LJ_KEY_LDS = 8192;                   // ints of a staged key set (32 KiB)
constexpr int SC_PER_THREAD = 8;
constexpr int SC_TILE = LJ_THREADS * SC_PER_THREAD;

// state words (int64, device): what the host reads back
enum { ST_BADVAL = 0, ST_OR = 1, ST_AND = 2, ST_ERROR = 3, ST_UNSORTED = 4, ST_TOTAL = 5 };
enum { ERR_EMPTY_UNION = 1, ERR_ROW_RANGE = 2 };

__device__ __forceinline__ bool odd_value(unsigned long long bits) {
  // NaN, ±inf (exponent all ones) or −0.0
  return ((bits >> 52) & 0x7ffull) == 0x7ffull || bits == 0x8000000000000000ull;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ long grid_stride() { return (long)gridDim.x * blockDim.x; }
__device__ __forceinline__ long grid_thread() { return (long)blockIdx.x * blockDim.x + threadIdx.x; }

// thread = (table, row), row fastest: a wave's keys and payloads are one contiguous store
__global__ __launch_bounds__(LJ_THREADS) void lsh_keys_kernel(const unsigned long long* __restrict__ H, long n, int T,
                                                              int F, int side, unsigned long long mask, long L,
                                                              long base, unsigned long long* __restrict__ keys,
                                                              unsigned* __restrict__ rows,
                                                              unsigned long long* __restrict__ state) {
  unsigned long long o = 0ull, a = ~0ull;
  bool bad = false;
  const long total = n * (long)T;
  for (long i = grid_thread(); i < total; i += grid_stride()) {
    const long t = i / n, row = i - t * n;
    const unsigned long long* h = H + (row * T + t) * (long)F;
    unsigned long long v = h[0];
    bad |= odd_value(v);
    if (F > 1) {
      v = mix64(v);
      for (int f = 1; f < F; ++f) {
        const unsigned long long x = h[f];
        bad |= odd_value(x);
        v = mix64(v ^ x);
      }
      v >>= 1;
    }
    const unsigned long long key = ((v & mask) << 1) | (unsigned long long)side;
    keys[t * L + base + row] = key;
    rows[t * L + base + row] = (unsigned)row;
    o |= key;
    a &= key;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    o |= __shfl_xor(o, off, 64);
    a &= __shfl_xor(a, off, 64);
  }
  // one OR and one AND per block: every atomic of the launch lands on the same two words
  __shared__ unsigned long long sh_o[LJ_THREADS / 64], sh_a[LJ_THREADS / 64];
  if ((threadIdx.x & 63) == 0) {
    sh_o[threadIdx.x >> 6] = o;
    sh_a[threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < LJ_THREADS / 64; ++w) {
      o |= sh_o[w];
      a &= sh_a[w];
    }
    atomicOr(&state[ST_OR], o);
    atomicAnd(&state[ST_AND], a);
  }
  if (bad) atomicOr(&state[ST_BADVAL], 1ull);
}

// thread = sorted entry p of table p / L; A entries (even keys) look their bucket's B run up
__global__ __launch_bounds__(LJ_THREADS) void lsh_count_kernel(const unsigned long long* __restrict__ skeys, long N,
                                                               long L, int* __restrict__ cnt,
                                                               unsigned* __restrict__ lo_out) {
  for (long p = grid_thread(); p < N; p += grid_stride()) {
    const unsigned long long key = skeys[p];
    int c = 0;
    unsigned l = 0;
    if ((key & 1ull) == 0ull) {
      const long s0 = (p / L) * L;
      const unsigned long long* seg = skeys + s0;
      const unsigned long long want = key | 1ull;
      // B entries of the bucket follow its A entries: search (p, segment end)
      long lo = p - s0 + 1, hi = L;
      while (lo < hi) {
        const long m = (lo + hi) >> 1;
        if (seg[m] < want) lo = m + 1; else hi = m;
      }
      long lo2 = lo, hi2 = L;
      while (lo2 < hi2) {
        const long m = (lo2 + hi2) >> 1;
        if (seg[m] <= want) lo2 = m + 1; else hi2 = m;
      }
      l = (unsigned)lo;
      c = (int)(lo2 - lo);
    }
    cnt[p] = c;
    lo_out[p] = l;
  }
}

// ---- exclusive scan of int32 counts into int64 offsets: sums per tile, scan of the sums, apply
__device__ __forceinline__ long block_sum(long v, long* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long s = 0;
  for (int w = 0; w < LJ_THREADS / 64; ++w) s += sh[w];
  return s;
}

__global__ __launch_bounds__(LJ_THREADS) void scan_reduce_kernel(const int* __restrict__ cnt, long n,
                                                                 long* __restrict__ bsum) {
  __shared__ long sh[LJ_THREADS / 64];
  const long t0 = (long)blockIdx.x * SC_TILE;
  long v = 0;
  for (int j = 0; j < SC_PER_THREAD; ++j) {
    const long i = t0 + (long)j * LJ_THREADS + threadIdx.x;
    if (i < n) v += cnt[i];
  }
  const long s = block_sum(v, sh);
  if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// one block: bsum[b] ← the sum of the tiles before b; the total to off[n] and the state word
__global__ __launch_bounds__(1024) void scan_sums_kernel(long* __restrict__ bsum, long nb, long* __restrict__ off_end,
                                                         long* __restrict__ total) {
  __shared__ long wtot[16];
  long carry = 0;
  for (long b0 = 0; b0 < nb; b0 += 1024) {
    const long b = b0 + threadIdx.x;
    long tot;
    const long ex = carry + block_excl_scan<1024>(b < nb ? bsum[b] : 0L, wtot, &tot);
    if (b < nb) bsum[b] = ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    *off_end = carry;
    *total = carry;
  }
}

// thread = SC_PER_THREAD consecutive counts
__global__ __launch_bounds__(LJ_THREADS) void scan_apply_kernel(const int* __restrict__ cnt, long n,
                                                                const long* __restrict__ bsum,
                                                                long* __restrict__ off) {
  __shared__ long wtot[LJ_THREADS / 64];
  const long i0 = (long)blockIdx.x * SC_TILE + (long)threadIdx.x * SC_PER_THREAD;
  int c[SC_PER_THREAD];
  long v = 0;
#pragma unroll
  for (int j = 0; j < SC_PER_THREAD; ++j) {
    c[j] = i0 + j < n ? cnt[i0 + j] : 0;
    v += c[j];
  }
  long p = bsum[blockIdx.x] + block_excl_scan<LJ_THREADS>(v, wtot);
#pragma unroll
  for (int j = 0; j < SC_PER_THREAD; ++j) {
    if (i0 + j < n) off[i0 + j] = p;
    p += c[j];
  }
}

// ---- Jaccard distance of two CSR rows by a group of LJ_GROUP lanes
// hits of this lane: elements x[sub], x[sub + 16], … of the shorter row found in the longer
__device__ __forceinline__ long lane_hits(const int* x, long lx, const int* y, long ly, int sub) {
  long hits = 0;
  for (long i = sub; i < lx; i += LJ_GROUP) {
    const int v = x[i];
    long lo = 0, hi = ly;
    while (lo < hi) {
      const long m = (lo + hi) >> 1;
      if (y[m] < v) lo = m + 1; else hi = m;
    }
    hits += (lo < ly && y[lo] == v) ? 1 : 0;
  }
  return hits;
}

__device__ __forceinline__ long group_sum(long v) {
#pragma unroll
  for (int off = LJ_GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// every lane of the group returns the distance; `empty`: both rows empty (no distance exists).
// Call it group-uniformly (all lanes of a group or none): the reduction crosses the group's lanes.
__device__ __forceinline__ double group_jaccard(const int* xa, long la, const int* xb, long lb, int sub, bool& empty) {
  const long mine = la <= lb ? lane_hits(xa, la, xb, lb, sub) : lane_hits(xb, lb, xa, la, sub);
  const long inter = group_sum(mine);
  const long uni = la + lb - inter;
  empty = uni <= 0;
  return empty ? 0.0 : 1.0 - (double)inter / (double)uni;
}

__device__ __forceinline__ bool same_signature(const unsigned long long* a, const unsigned long long* b, int F) {
  bool eq = true;
  for (int f = 0; f < F; ++f) eq &= a[f] == b[f];
  return eq;
}

// Appends the kept pairs of a wave (one per group, held by the group's lane 0) behind one atomic.
__device__ __forceinline__ void wave_append(bool keep, unsigned long long key, double dist,
                                            unsigned long long* __restrict__ cursor,
                                            unsigned long long* __restrict__ out_key, double* __restrict__ out_dist,
                                            long cap) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(keep);
  if (m == 0ull) return;
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0ull;
  if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (keep) {
    const long pos = (long)base + __popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap) {
      out_key[pos] = key;
      out_dist[pos] = dist;
    }
  }
}

__global__ __launch_bounds__(LJ_THREADS) void lsh_emit_kernel(
    const unsigned* __restrict__ srows, const long* __restrict__ off, const unsigned* __restrict__ lo, long N, long L,
    long c0, long c1, const unsigned long long* __restrict__ Ha, const unsigned long long* __restrict__ Hb, long na,
    long nb, int T, int F, const long* __restrict__ a_ptr, const int* __restrict__ a_idx,
    const long* __restrict__ b_ptr, const int* __restrict__ b_idx, double threshold,
    unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ out_key, double* __restrict__ out_dist,
    unsigned long long* __restrict__ state) {
  const int sub = threadIdx.x & (LJ_GROUP - 1);
  const long c = c0 + (long)blockIdx.x * LJ_PER_BLOCK + (threadIdx.x / LJ_GROUP);
  bool live = c < c1;
  long a = 0, b = 0;
  int t = 0;
  if (live) {
    // the last entry e with off[e] <= c (entries without candidates share their successor's offset)
    long l = 0, h = N;
    while (l < h) {
      const long m = (l + h) >> 1;
      if (off[m] <= c) l = m + 1; else h = m;
    }
    const long e = l > 0 ? l - 1 : 0;  // (off[0] = 0 <= c: l >= 1)
    const long tt = e / L;
    t = (int)tt;
    const long be = tt * L + lo[e] + (c - off[e]);
    live = c >= off[e] && be < N;
    if (live) {
      a = srows[e];
      b = srows[be];
      live = a < na && b < nb;
    }
  }
  bool keep = false;
  double dist = 0.0;
  if (live) {
    const unsigned long long* ha = Ha + a * (long)T * F;
    const unsigned long long* hb = Hb + b * (long)T * F;
    bool ok = same_signature(ha + (long)t * F, hb + (long)t * F, F);
    // an earlier table with equal signatures has this pair already: the lanes share the tables
    int earlier = 0;
    for (int q = sub; q < t; q += LJ_GROUP) earlier |= same_signature(ha + (long)q * F, hb + (long)q * F, F) ? 1 : 0;
    ok = ok && group_sum(earlier) == 0;
    if (ok) {
      const long sa = a_ptr[a], sb = b_ptr[b];
      bool empty;
      dist = group_jaccard(a_idx + sa, a_ptr[a + 1] - sa, b_idx + sb, b_ptr[b + 1] - sb, sub, empty);
      if (empty && sub == 0) atomicOr(&state[ST_ERROR], (unsigned long long)ERR_EMPTY_UNION);
      keep = !empty && sub == 0 && dist <= threshold;
    }
  }
  wave_append(keep, ((unsigned long long)a << 32) | (unsigned long long)b, dist, cursor, out_key, out_dist, c1 - c0);
}

// STAGE: every pair's A row is row 0 of A (the nearest-neighbour key), staged in LDS when it fits
template <bool STAGE>
__global__ __launch_bounds__(LJ_THREADS) void lsh_pair_kernel(const long* __restrict__ a_ptr,
                                                              const int* __restrict__ a_idx, long na,
                                                              const long* __restrict__ b_ptr,
                                                              const int* __restrict__ b_idx, long nb,
                                                              const long* __restrict__ ia, const long* __restrict__ ib,
                                                              long P, double* __restrict__ dist,
                                                              unsigned long long* __restrict__ state) {
  __shared__ int key_set[STAGE ? LJ_KEY_LDS : 1];
  const int* a0 = a_idx;
  long la0 = 0;
  if (STAGE) {
    const long s = a_ptr[0];
    la0 = a_ptr[1] - s;
    a0 = a_idx + s;
    if (la0 <= LJ_KEY_LDS) {
      for (long i = threadIdx.x; i < la0; i += LJ_THREADS) key_set[i] = a0[i];
      __syncthreads();
      a0 = key_set;
    }
  }
  const int sub = threadIdx.x & (LJ_GROUP - 1);
  const long p = (long)blockIdx.x * LJ_PER_BLOCK + (threadIdx.x / LJ_GROUP);
  if (p >= P) return;  // (whole groups leave together)
  const long a = STAGE ? 0 : ia[p], b = ib[p];
  if (a < 0 || a >= na || b < 0 || b >= nb) {
    if (sub == 0) {
      atomicOr(&state[ST_ERROR], (unsigned long long)ERR_ROW_RANGE);
      dist[p] = 0.0;
    }
    return;
  }
  const long sa = a_ptr[a], sb = b_ptr[b];
  bool empty;
  const double d = group_jaccard(STAGE ? a0 : a_idx + sa, STAGE ? la0 : a_ptr[a + 1] - sa, b_idx + sb,
                                 b_ptr[b + 1] - sb, sub, empty);
  if (sub == 0) {
    if (empty) atomicOr(&state[ST_ERROR], (unsigned long long)ERR_EMPTY_UNION);
    dist[p] = d;
  }
}

// thread = dataset row: 1 where any table's signature equals the key's
__global__ __launch_bounds__(LJ_THREADS) void lsh_match_kernel(const unsigned long long* __restrict__ H, long n, int T,
                                                               int F, const unsigned long long* __restrict__ kh,
                                                               int* __restrict__ flag,
                                                               unsigned long long* __restrict__ state) {
  bool bad = false;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < T * F; i += LJ_THREADS) bad |= odd_value(kh[i]);
  for (long r = grid_thread(); r < n; r += grid_stride()) {
    const unsigned long long* h = H + r * (long)T * F;
    int any = 0;
    for (int t = 0; t < T; ++t) {
      bool eq = true;
      for (int f = 0; f < F; ++f) {
        const unsigned long long v = h[t * F + f];
        bad |= odd_value(v);
        eq &= v == kh[t * F + f];
      }
      any |= eq ? 1 : 0;
    }
    flag[r] = any;
  }
  if (bad) atomicOr(&state[ST_BADVAL], 1ull);
}

// rows with flag 1, in row order (off: the flags' exclusive scan)
__global__ __launch_bounds__(LJ_THREADS) void lsh_compact_kernel(const int* __restrict__ flag,
                                                                 const long* __restrict__ off, long n, long cap,
                                                                 long* __restrict__ idx) {
  for (long r = grid_thread(); r < n; r += grid_stride())
    if (flag[r] && off[r] < cap) idx[off[r]] = r;
}

// a lane group per row: its lanes stride over the row's neighbouring index pairs
__global__ __launch_bounds__(LJ_THREADS) void lsh_sorted_kernel(const long* __restrict__ indptr,
                                                                const int* __restrict__ indices, long n, long nnz,
                                                                unsigned long long* __restrict__ state) {
  const int sub = threadIdx.x & (LJ_GROUP - 1);
  bool bad = false;
  for (long r = grid_thread() / LJ_GROUP; r < n; r += grid_stride() / LJ_GROUP) {
    const long s = indptr[r], e = indptr[r + 1];
    if (s < 0 || e < s || e > nnz) {  // (not a CSR row of these indices: leave it to the torch formulation)
      bad = true;
      continue;
    }
    for (long j = s + 1 + sub; j < e; j += LJ_GROUP) bad |= indices[j] <= indices[j - 1];
  }
  if (bad) atomicOr(&state[ST_UNSORTED], 1ull);
}

// the sorted survivors: rows out of the (a << 32 | b) keys, distances by the payload (position)
__global__ __launch_bounds__(LJ_THREADS) void lsh_gather_kernel(const unsigned long long* __restrict__ skeys,
                                                                const unsigned* __restrict__ pos,
                                                                const double* __restrict__ dist_in, long S,
                                                                long* __restrict__ ia, long* __restrict__ ib,
                                                                double* __restrict__ dist) {
  for (long i = grid_thread(); i < S; i += grid_stride()) {
    const unsigned long long k = skeys[i];
    const unsigned p = pos[i];
    ia[i] = (long)(k >> 32);
    ib[i] = (long)(k & 0xffffffffull);
    dist[i] = p < S ? dist_in[p] : 0.0;
  }
}

unsigned stride_blocks(long work) {
  long blocks = (work + LJ_THREADS - 1) / LJ_THREADS;
  return (unsigned)(blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks));  // (8 blocks per CU; the rest by stride)
}

}  // namespace

// Bucket keys of one side. H: fp64 [n, T, F]; keys / rows: table-major [T, L] with this side's
// entries at [base, base + n) of every table segment; state: int64 [8], words {bad value, OR, AND}
// updated (the caller starts OR at 0 and AND at ~0 once for both sides). n, L < 2^31.
FMLX_API int fmlx_lsh_keys(const double* H, long n, int T, int F, int side, int key_bits, long L, long base,
                           uint64_t* keys, uint32_t* rows, long* state, void* stream) {
  if (T < 1 || F < 1 || key_bits < 1 || key_bits > 63 || side < 0 || side > 1) return -1;
  if (n < 0 || base < 0 || base + n > L || L >= (1L << 31)) return -2;
  if (n == 0) return 0;
  const unsigned long long mask = (1ull << key_bits) - 1ull;
  unsigned blocks = stride_blocks(n * (long)T);
  if (blocks > 512) blocks = 512;  // (two same-address atomics per block)
  hipLaunchKernelGGL(lsh_keys_kernel, dim3(blocks), dim3(LJ_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)H, n, T, F, side, mask, L, base, (unsigned long long*)keys, rows,
                     (unsigned long long*)state);
  return (int)hipGetLastError();
}

// Per sorted entry (N = T·L of them) the candidate count and the first B entry of its bucket
// (relative to the table's segment).
FMLX_API int fmlx_lsh_count(const uint64_t* skeys, long N, long L, int* cnt, uint32_t* lo, void* stream) {
  if (N < 0 || L < 1 || L >= (1L << 31) || N % L) return -1;
  if (N == 0) return 0;
  hipLaunchKernelGGL(lsh_count_kernel, dim3(stride_blocks(N)), dim3(LJ_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)skeys, N, L, cnt, lo);
  return (int)hipGetLastError();
}

// int64 words of scratch fmlx_lsh_scan needs for n counts
FMLX_API long fmlx_lsh_scan_scratch(long n) { return n <= 0 ? 1 : (n + SC_TILE - 1) / SC_TILE; }

// off[i] = cnt[0] + … + cnt[i − 1] for i = 0 … n (off: int64 [n + 1]); the total also to *total.
FMLX_API int fmlx_lsh_scan(const int* cnt, long n, long* off, long* scratch, long* total, void* stream) {
  if (n < 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const long nb = n <= 0 ? 0 : (n + SC_TILE - 1) / SC_TILE;
  if (nb >= (1L << 31)) return -2;
  if (nb > 0)
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(LJ_THREADS), 0, st, cnt, n, scratch);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, scratch, nb, off + (n < 0 ? 0 : n), total);
  if (nb > 0)
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(LJ_THREADS), 0, st, cnt, n, scratch, off);
  return (int)hipGetLastError();
}

// Candidates [c0, c1) of the co-group → the pairs within `threshold`, appended at *cursor (the
// caller zeroes it) to out_key (a << 32 | b) / out_dist, which hold c1 − c0 entries.
// state[3] |= 1 where both sets of a pair are empty.
FMLX_API int fmlx_lsh_emit(const uint32_t* srows, const long* off, const uint32_t* lo, long N, long L, long c0,
                           long c1, const double* Ha, const double* Hb, long na, long nb, int T, int F,
                           const long* a_ptr, const int* a_idx, const long* b_ptr, const int* b_idx,
                           double threshold, long* cursor, uint64_t* out_key, double* out_dist, long* state,
                           void* stream) {
  if (c1 <= c0) return 0;
  if (c0 < 0 || N < 1 || L < 1 || N != (long)T * L || na + nb != L) return -1;
  const long blocks = (c1 - c0 + LJ_PER_BLOCK - 1) / LJ_PER_BLOCK;
  if (blocks >= (1L << 31)) return -2;
  hipLaunchKernelGGL(lsh_emit_kernel, dim3((unsigned)blocks), dim3(LJ_THREADS), 0, (hipStream_t)stream, srows, off, lo,
                     N, L, c0, c1, (const unsigned long long*)Ha, (const unsigned long long*)Hb, na, nb, T, F, a_ptr,
                     a_idx, b_ptr, b_idx, threshold, (unsigned long long*)cursor, (unsigned long long*)out_key,
                     out_dist, (unsigned long long*)state);
  return (int)hipGetLastError();
}

// dist[p] = Jaccard distance of CSR rows A[ia[p]] and B[ib[p]] (ia, ib: int64 [P]). stage_a: every
// pair takes row 0 of A (ia is not read). state[3] |= 1 for an empty union, |= 2 for a row out of range.
FMLX_API int fmlx_lsh_pair_jaccard(const long* a_ptr, const int* a_idx, long na, const long* b_ptr, const int* b_idx,
                                   long nb, const long* ia, const long* ib, long P, double* dist, long* state,
                                   int stage_a, void* stream) {
  if (P <= 0) return 0;
  if (stage_a && na < 1) return -1;
  const long blocks = (P + LJ_PER_BLOCK - 1) / LJ_PER_BLOCK;
  if (blocks >= (1L << 31)) return -2;
  if (stage_a)
    hipLaunchKernelGGL(lsh_pair_kernel<true>, dim3((unsigned)blocks), dim3(LJ_THREADS), 0, (hipStream_t)stream, a_ptr,
                       a_idx, na, b_ptr, b_idx, nb, ia, ib, P, dist, (unsigned long long*)state);
  else
    hipLaunchKernelGGL(lsh_pair_kernel<false>, dim3((unsigned)blocks), dim3(LJ_THREADS), 0, (hipStream_t)stream, a_ptr,
                       a_idx, na, b_ptr, b_idx, nb, ia, ib, P, dist, (unsigned long long*)state);
  return (int)hipGetLastError();
}

// flag[r] = 1 where a table's signature of row r (H: fp64 [n, T, F]) equals the key's (kh: [T, F]);
// state[0] |= 1 for a NaN, ±inf or −0.0 in either.
FMLX_API int fmlx_lsh_match(const double* H, long n, int T, int F, const double* kh, int* flag, long* state,
                            void* stream) {
  if (T < 1 || F < 1 || n < 0) return -1;
  hipLaunchKernelGGL(lsh_match_kernel, dim3(stride_blocks(n)), dim3(LJ_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)H, n, T, F, (const unsigned long long*)kh, flag,
                     (unsigned long long*)state);
  return (int)hipGetLastError();
}

// idx[off[r]] = r for the flagged rows (off: the flags' scan; idx holds cap entries)
FMLX_API int fmlx_lsh_compact(const int* flag, const long* off, long n, long cap, long* idx, void* stream) {
  if (n <= 0 || cap <= 0) return 0;
  hipLaunchKernelGGL(lsh_compact_kernel, dim3(stride_blocks(n)), dim3(LJ_THREADS), 0, (hipStream_t)stream, flag, off,
                     n, cap, idx);
  return (int)hipGetLastError();
}

// state[4] |= 1 if a CSR row's indices are not strictly increasing
FMLX_API int fmlx_lsh_sorted_check(const long* indptr, const int* indices, long n, long nnz, long* state,
                                   void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(lsh_sorted_kernel, dim3(stride_blocks(n * LJ_GROUP)), dim3(LJ_THREADS), 0, (hipStream_t)stream,
                     indptr, indices, n, nnz, (unsigned long long*)state);
  return (int)hipGetLastError();
}

// The S survivors in sorted order: ia / ib from the keys, dist[i] = dist_in[pos[i]].
FMLX_API int fmlx_lsh_gather(const uint64_t* skeys, const uint32_t* pos, const double* dist_in, long S, long* ia,
                             long* ib, double* dist, void* stream) {
  if (S <= 0) return 0;
  hipLaunchKernelGGL(lsh_gather_kernel, dim3(stride_blocks(S)), dim3(LJ_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)skeys, pos, dist_in, S, ia, ib, dist);
  return (int)hipGetLastError();
}

FMLX_DEFINE_PRELOAD()
