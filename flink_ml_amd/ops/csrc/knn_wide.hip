// KNN predict for dense fp32 rows of 128 < D <= 4096, k <= 64: fused MFMA distances + per-query
// top-k (fmlx_knn_fused's contract; the nq×n distance block never reaches HBM). knn.hip's fused
// kernel keeps a wave's whole query rows in registers and stops at D = 128; here nothing row-sized
// stays in registers.
//
// knn_fused_wide_kernel<K, MT>
//  * A block of 256 threads owns 128 queries for the whole kernel: 4 waves × 32 queries, a query
//    per lane column, the two half-waves h splitting the K index (v_mfma_f32_32x32x2_f32, the
//    training tile as A and the queries as B, as in knn_fused_kernel). It walks its training
//    segment in macro-tiles of MT rows and K in chunks of 32 fp32 columns. MT is 128 (64
//    accumulator registers) or 64 per list length K, chosen with the blocks per CU from the
//    compiler's register report (WideTile): two blocks share a CU wherever a rung fits in 256
//    registers, so one block's fill wait and epilogue run under the other's MFMAs.
//  * Both operands of a chunk go as they are stored, from the row-major training matrix and the
//    row-major query block straight into LDS by LDS-DMA (MT × 32 and 128 × 32 floats). No packed
//    image, no copy of T. A tile row is 128 bytes: its 16-byte piece s sits at slot s ^ (r mod 8),
//    applied by the choice of the global piece a lane fetches, so the b128 fragment reads are
//    bank-conflict free without padding. k-step (g, e) of half h is column 8g + 4h + e of the
//    chunk in A and B alike: one b128 read is four consecutive k-steps.
//  * B fragments are read from LDS into registers once per chunk (4 b128 reads, 16 registers) and
//    reused by the MT/32 subtiles; the query block is re-read from L2 once per macro-tile. Holding
//    them across macro-tiles would need D/2 registers per lane, which is what stops knn.hip at 128.
//  * Ring of two slots (A tile, then B tile: 32 KiB at MT = 128): chunk i + 1 fills under chunk
//    i's MFMAs; per chunk one s_waitcnt vmcnt(0) (this wave's share has landed) and one barrier
//    (everyone's has, and everyone is past chunk i − 1, whose slot the next fill takes). The ring
//    starts at LDS offset 0, so every LDS-DMA destination stays below 64 KiB.
//  * ‖t‖² of a macro-tile's rows comes through LDS as well (a plain load issued with the fill of
//    the tile's first chunk, stored to LDS after the next vmcnt(0), published by the same
//    barrier): accumulators start at −‖t‖²/2, so the key |‖q‖² + ‖t‖² − 2·q·t| is one fma per
//    element after the last chunk. ‖q‖² is summed from the B fragments during the block's first
//    macro-tile, in a fixed order.
//  * Tails: queries >= nq and training rows >= n are clamped for the loads (never stored / never
//    admitted); the pieces of the last chunk past D are fetched from the chunk's first piece
//    instead and zeroed in LDS by the lane that fetched them, in both operands: they add exactly 0.
//  * Epilogue per 64-row subtile: knn_fused_kernel's (32 keys per lane, a min against the
//    admission bound, a bit mask of admitted slots, one insertion per trip), on the lists of
//    knn_list.h. grid.y = S training segments of whole macro-tiles; their candidates go through
//    knn_topk_merge_kernel. The K order within a (query, row) is fixed: results do not depend on
//    the grid or on S.
#include "common.h"
#include "knn_list.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int WQ_ROWS = 128;             // queries per block
constexpr int WQ_KC = 32;                // fp32 columns per K-chunk
constexpr int WQ_ROWB = WQ_KC * 4;       // bytes per tile row
constexpr int WQ_TILEQ = WQ_ROWS * WQ_ROWB;

// Rows per macro-tile and blocks per CU for a list of K entries, from the compiler's register
// report (profiles/r21/resources_knn_wide.txt; 256 registers per lane is the most that lets two
// blocks share a CU). K <= 8: 128 rows fit in 162 / 178 registers. K = 16 and K = 64: 128 rows
// spill, 64 rows fit (184 / 254). K = 32 spills at two blocks per CU with either tile, so it runs
// one block per CU on the full register file, with the 128-row tile (more MFMAs per barrier).
template <int K>
struct WideTile {
  static constexpr int MT = (K <= 8 || K == 32) ? 128 : 64;
  static constexpr int BLOCKS = K == 32 ? 1 : 2;
};

// Q / T / tn are not __restrict__: the asm fills read them behind the compiler's back
template <int K, int MT>
__global__ __launch_bounds__(256, WideTile<K>::BLOCKS) void knn_fused_wide_kernel(const float* Q, long ldq, long nq, int D,
                                                                const float* T, long ldt, const float* tn, long n,
                                                                int k, int S, int* __restrict__ out_i,
                                                                float* __restrict__ out_d) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  constexpr int NSUB = MT / 32;            // 32-row MFMA subtiles = 1-KiB fill pieces per wave
  constexpr int TILEA = MT * WQ_ROWB;
  constexpr int SLOTB = TILEA + WQ_TILEQ;  // the training tile, then the query tile
  __shared__ __align__(16) unsigned char lds[2 * SLOTB + MT * 4];  // the ring, then the tile's norms
  float* tnl = reinterpret_cast<float*>(lds + 2 * SLOTB);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r32 = lane & 31;
  const int h = lane >> 5;
  const long row0 = (long)blockIdx.x * WQ_ROWS;
  const long qrow = row0 + wave * 32 + r32;
  const bool qok = qrow < nq;
  const int NC = (D + WQ_KC - 1) / WQ_KC;

  const long ntiles = (n + MT - 1) / MT;
  const long L = (ntiles + S - 1) / S;
  const long t0 = (long)blockIdx.y * L;
  const long t1 = t0 + L < ntiles ? t0 + L : ntiles;
  const long iters = t0 < t1 ? (t1 - t0) * NC : 0;

  // fill geometry: piece q = wave + 4i of a tile covers tile rows 8q … 8q + 7; lane l lands at
  // (row 8q + l/8, slot l%8) and fetches global piece g = slot ^ (row mod 8)
  const int g = (lane & 7) ^ (lane >> 3);
  const bool tail_ok = (NC - 1) * WQ_KC + g * 4 < D;  // this lane's piece of the last chunk is inside the row
  unsigned q_off[4];                                  // byte offset of the lane's query rows from the block's first
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long r = row0 + 8 * (wave + 4 * i) + (lane >> 3);
    r = r < nq ? r : nq - 1;
    q_off[i] = (unsigned)((r - row0) * ldq * 4);
  }
  const unsigned ldtb = (unsigned)(ldt * 4);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* qblk = reinterpret_cast<const char*>(Q) + row0 * ldq * 4;  // uniform

  // chunk (macro-tile P_, chunk KC_) → ring slot S_. Issued by inline asm with the ordering
  // explicit (vmcnt + one barrier per chunk), as in kmeans_wide.hip; every wave issues the same
  // NSUB + 4 loads per chunk. M0: written only by these statements in this kernel.
#define WQ_FILL(P_, KC_, S_)                                                                              \
  {                                                                                                       \
    const unsigned gb_ = ((KC_) == NC - 1 && !tail_ok) ? 0u : (unsigned)(g * 16);                         \
    const char* asrc_ = reinterpret_cast<const char*>(T) + ((long)(P_) * MT * ldt + (long)(KC_) * WQ_KC) * 4; \
    const char* bsrc_ = qblk + (long)(KC_) * WQ_ROWB;                                                     \
    const int rmax_ = (int)(n - 1 - (long)(P_) * MT);                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < NSUB; ++i_) {                                                 \
      const unsigned d_ = dst0 + (unsigned)((S_) * SLOTB + i_ * 4096);                                    \
      int r_ = 8 * (wave + 4 * i_) + (lane >> 3);                                                         \
      r_ = r_ < rmax_ ? r_ : rmax_;                                                                       \
      const unsigned ao_ = (unsigned)r_ * ldtb + gb_;                                                     \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(ao_), "s"(asrc_), "s"(d_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                    \
      const unsigned e_ = dst0 + (unsigned)((S_) * SLOTB + TILEA + i_ * 4096);                            \
      const unsigned bo_ = q_off[i_] + gb_;                                                               \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(bo_), "s"(bsrc_), "s"(e_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
  }
  // ‖t‖² of row threadIdx.x of macro-tile P_ (clamped like the rows)
#define WQ_NORM(P_) tn[((P_) * MT + (long)threadIdx.x) < n ? ((P_) * MT + (long)threadIdx.x) : n - 1]

  float bd[K];
  int bi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { bd[i] = INFINITY; bi[i] = INT32_MAX; }
  float td = INFINITY;
  int ti = INT32_MAX;

  float tv = 0.f;  // the next macro-tile's norm of this thread's row, on its way to LDS
  if (iters > 0) {
    if ((int)threadIdx.x < MT) tv = WQ_NORM(t0);
    WQ_FILL(t0, 0, 0)
  }

  f32x16_t acc[NSUB];
  float qp = 0.f, qn = 0.f;
  // fragment addresses inside a slot: row (32·t + r32), piece (2g + h) ^ (r32 mod 8)
  const int x7 = r32 & 7;
  const int arow = r32 * WQ_ROWB;
  const int brow = TILEA + (32 * wave + r32) * WQ_ROWB;

  long p = t0;             // the chunk being multiplied
  int kc = 0;
  long fp = t0;            // the next chunk to fill (NC >= 5: no wrap here)
  int fkc = 1;
  for (long i = 0; i < iters; ++i) {
    const int slot = (int)(i & 1);
    // this wave's share of chunk i has landed (and tv)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1 && !tail_ok) {
#pragma unroll
      for (int q = 0; q < NSUB; ++q)
        *reinterpret_cast<uint4*>(lds + slot * SLOTB + (wave + 4 * q) * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<uint4*>(lds + slot * SLOTB + TILEA + (wave + 4 * q) * 1024 + lane * 16) =
            make_uint4(0u, 0u, 0u, 0u);
    }
    if (kc == 0 && (int)threadIdx.x < MT) tnl[threadIdx.x] = tv;
    // … and every wave's; every wave is past chunk i − 1, whose slot the next fill takes
    __syncthreads();
    if (i + 1 < iters) {
      WQ_FILL(fp, fkc, slot ^ 1)
      if (fkc == 0 && (int)threadIdx.x < MT) tv = WQ_NORM(fp);
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    if (kc == 0) {
      // accumulator register r of half h is row (r&3) + 8(r>>2) + 4h of its subtile
#pragma unroll
      for (int t = 0; t < NSUB; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(tnl + 32 * t + 8 * g4 + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][4 * g4 + e] = -0.5f * v[e];
        }
    }
    const unsigned char* sb = lds + slot * SLOTB;
    const bool first = p == t0;
#pragma unroll
    for (int g4 = 0; g4 < WQ_KC / 8; ++g4) {
      const int po = ((2 * g4 + h) ^ x7) * 16;
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(sb + brow + po);
      f32x4_t a[NSUB];
#pragma unroll
      for (int t = 0; t < NSUB; ++t) a[t] = *reinterpret_cast<const f32x4_t*>(sb + arow + t * 32 * WQ_ROWB + po);
      if (first) {
#pragma unroll
        for (int e = 0; e < 4; ++e) qp = __builtin_fmaf(b[e], b[e], qp);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][e], b[e], acc[t], 0, 0, 0);
    }
    if (++kc < NC) continue;

    // ---- the macro-tile's keys, 64 rows at a time: 32 keys per lane, admission-bound filter, rare
    // insertions. A NaN key fails every '>' test, so it is admitted only while the list still has
    // room and then ranks as +inf (torch.topk also ranks NaN last).
    if (first) qn = qp + __shfl_xor(qp, 32, 64);
#pragma unroll
    for (int u = 0; u < MT / 64; ++u) {
      float key[32];
      float m = INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        key[r] = fabsf(__builtin_fmaf(-2.0f, acc[2 * u][r], qn));
        key[16 + r] = fabsf(__builtin_fmaf(-2.0f, acc[2 * u + 1][r], qn));
        m = fminf(m, fminf(key[r], key[16 + r]));
      }
      const long jb = p * MT + 64 * u;
      if (jb < n && !(m > td)) {
        // bit r = slot r admitted; built by shifts, highest slot first (a literal 1 << r per slot
        // would sit in a register each for the whole kernel)
        unsigned mask = 0u;
#pragma unroll
        for (int r = 31; r >= 0; --r) mask = (mask << 1) | (key[r] > td ? 0u : 1u);
        if (jb + 64 > n) {  // last tile: drop the clamped rows
          const int lim = (int)(n - jb) - 4 * h;
          unsigned valid = 0u;
#pragma unroll
          for (int r = 31; r >= 0; --r)
            valid = (valid << 1) | ((r >> 4) * 32 + (r & 3) + 8 * ((r & 15) >> 2) < lim ? 1u : 0u);
          mask &= valid;
        }
        while (mask) {
          const int b = __builtin_ctz(mask);
          mask &= mask - 1u;
          float d = select32(key, b);
          d = __builtin_isnan(d) ? INFINITY : d;
          const int j = (int)(jb + (b >> 4) * 32 + (b & 3) + 8 * ((b & 15) >> 2) + 4 * h);
          if (lex_less(d, j, td, ti) && lex_less(d, j, bd[K - 1], bi[K - 1])) topk_insert<K>(bd, bi, d, j);
        }
      }
      // refresh the admission bound: this lane's k-th best vs the partner half-lane's
      kth_entry<K>(bd, bi, k, td, ti);
      const float xd = __shfl_xor(td, 32, 64);
      const int xi = __shfl_xor(ti, 32, 64);
      if (lex_less(xd, xi, td, ti)) { td = xd; ti = xi; }
    }
    kc = 0;
    ++p;
  }
#undef WQ_FILL
#undef WQ_NORM

  // ---- merge the two half-lane lists of each query; lane h == 0 writes
  const long o = (qrow * S + blockIdx.y) * k;
  for (int t = 0; t < k; ++t) {
    const float wd = bd[0];
    const int wi = bi[0];
    const float xd = __shfl_xor(wd, 32, 64);
    const int xi = __shfl_xor(wi, 32, 64);
    const bool mine = lex_less(wd, wi, xd, xi);
    if (h == 0 && qok) {
      const float od = mine ? wd : xd;
      out_i[o + t] = mine ? wi : xi;
      if (out_d) out_d[o + t] = S == 1 ? __builtin_sqrtf(od) : od;
    }
    if (mine) topk_pop<K>(bd, bi);
  }
}

// the list length K of a k: 4 / 8 / 16 / 32 / 64 (the launcher has validated k <= 64; the
// occupancy query answers for any k)
template <typename F>
int with_wide_list(int k, F&& f) {
  return with_ceil<4, 8, 16, 32, 64>(k < 64 ? k : 64, f);
}

}  // namespace

// Resident wide-kernel blocks per CU for k — the host sizes the segment split with it.
FMLX_API int fmlx_knn_fused_wide_blocks_per_cu(int k) {
  return with_wide_list(k, [&](auto K) {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, knn_fused_wide_kernel<K.value, WideTile<K.value>::MT>, 256,
                                                     0) != hipSuccess)
      return 1;
    return b > 0 ? b : 1;
  });
}

// Fused KNN for wide rows: Q [nq, D] and T [n, D] fp32 row-major (leading dims ldq, ldt), tn [n]
// the squared norms of T's rows. k nearest per query (nearest first, ties → lower index) into
// idx [nq, k] and, if non-null, their distances into dist [nq, k]. S training segments (1..256);
// S > 1 needs ws_d/ws_i of nq·S·k. −1 unless 128 < D <= 4096, D % 4 == 0, the pitches are
// multiples of 4 floats below 2^23 (32-bit byte offsets inside a tile), Q and T are 16-byte
// aligned, 1 <= k <= min(64, n) and n < 2^31 − 128.
FMLX_API int fmlx_knn_fused_wide(const float* Q, long ldq, long nq, int D, const float* T, long ldt, const float* tn,
                                 long n, int k, int S, int* idx, float* dist, float* ws_d, int* ws_i, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D <= 128 || D > 4096 || (D % 4) != 0 || ldq < D || ldt < D || (ldq % 4) != 0 || (ldt % 4) != 0 ||
      ldq >= (1L << 23) || ldt >= (1L << 23) || ((uintptr_t)Q % 16) != 0 || ((uintptr_t)T % 16) != 0)
    return -1;
  if (k < 1 || k > 64 || k > n || n >= (long)INT32_MAX - 128 || S < 1 || S > 256 || nq < 0) return -1;
  if (S > 1 && (ws_d == nullptr || ws_i == nullptr)) return -1;
  if (nq == 0) return 0;
  const long bq = (nq + WQ_ROWS - 1) / WQ_ROWS;
  if (bq > 0x7fffffffL) return -1;
  int* si = S > 1 ? ws_i : idx;
  float* sd = S > 1 ? ws_d : dist;
  return with_wide_list(k, [&](auto K) {
    hipLaunchKernelGGL((knn_fused_wide_kernel<K.value, WideTile<K.value>::MT>), dim3((unsigned)bq, S), dim3(256), 0, s,
                       Q, ldq, nq, D, T, ldt, tn, n, k, S, si, sd);
    if (S > 1) launch_topk_merge<K.value>(ws_d, ws_i, nq, S, k, idx, dist, s);
    FMLX_CHECK_LAUNCH();
  });
}

FMLX_DEFINE_PRELOAD()
