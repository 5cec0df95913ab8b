// KNN predict for dense fp64 rows of 16 <= D <= 4096, D even, k <= 32 (FMLX_COMPUTE_DTYPE=fp64, the
// parity mode): fused fp64 MFMA distances + per-query top-k, fmlx_knn_fused_wide's contract for
// doubles (the nq×n product block never reaches HBM). The fp64 route before it is a library GEMM
// per query block and knn_select.hip's radix selection of that block.
//
// knn_fused_f64_kernel<K>: key = |(‖q‖² + ‖t‖²) − 2·q·t|, the expression of knn_select.hip and of
// knn_predict's host path, not seeded into the accumulators; only the summation order of q·t and
// ‖q‖² differs from those paths.
//  * v_mfma_f64_16x16x4_f64 with the training tile as A and the queries as B
//    (kmeans_wide_f64.hip's layout with the operand roles swapped): a lane holds one double of A
//    and of B, row / column lane & 15 and K index lane >> 4; accumulator element q is training row
//    4q + (lane >> 4) of its A tile, query lane & 15.
//  * A block of 256 threads owns 64 queries for the whole kernel, one 16-query B tile per wave. It
//    walks its training segment in macro-tiles of 128 rows (eight A tiles: 8 accumulator tiles of
//    4 doubles, 64 registers) and K in chunks of 16 doubles. A lane then holds, for its query, the
//    32 keys of the rows 4r + (lane >> 4) of the macro-tile, r = 4·tile + q ascending in the row
//    index; the four lane groups of a query hold disjoint rows.
//  * Both operands of a chunk go as they are stored, from the row-major training matrix and the
//    row-major query block straight into LDS by LDS-DMA (128 × 16 and 64 × 16 doubles). No packed
//    image, no copy of T. A tile row is 128 bytes: its 16-byte piece s sits at slot
//    s ^ ((r >> 1) mod 8), applied by the choice of the global piece a lane fetches, so the 16 rows
//    one lane group reads with a ds_read_b128 cover 16 different 16-byte bank groups. A piece is
//    two consecutive K indices; lane group g takes the pieces g and g + 4 of the chunk: K-step
//    (hp, e) of group g is column 8·hp + 2g + e of the chunk in A and B alike. Per chunk and wave
//    18 ds_read_b128 feed 32 MFMAs.
//  * Ring of two 24-KiB slots (training tile, then query tile): chunk i + 1 fills under chunk i's
//    MFMAs; per chunk one s_waitcnt vmcnt(0) (this wave's share has landed) and one barrier
//    (everyone's has, and everyone is past chunk i − 1, whose slot the next fill takes). The
//    fill-ahead cursor wraps to the next macro-tile after every chunk when D = 16 (one chunk).
//  * ‖t‖² of a macro-tile's rows comes through LDS (a plain load issued with the fill of the
//    tile's first chunk, stored after the next vmcnt(0), published by the same barrier). The
//    epilogue reads it after the tile's last chunk, while a faster wave may already publish the
//    next tile's: two buffers, by tile parity. ‖q‖² comes from the B fragments a lane holds during
//    the block's first macro-tile (chunk order, then the four K-steps); the four lane groups'
//    shares meet in a symmetric butterfly, so every lane of a query holds the same sum.
//  * Lists and epilogue: one sorted (double key, int index) list of K entries per lane, on
//    knn_list.h (3K registers); per macro-tile knn.hip's epilogue: the 32 keys against the
//    admission bound, a bit mask of admitted slots, one insertion per trip, every comparison
//    lexicographic on (key, index). The bound of a query is the least of its four lanes' k-th
//    entries: a lane that holds k entries at or below a pair shuts out everything above it,
//    whichever lane meets it; a lane that does not hold k entries yet contributes (inf, INT32_MAX).
//    A NaN key fails the '<=' test against the bound and is never admitted. After the last
//    macro-tile the four lists of a query are merged by cross-lane exchanges; lane group 0 writes.
//  * Tails: queries >= nq and training rows >= n are clamped for the loads (never stored / never
//    admitted); the pieces of the last chunk past D are fetched from the chunk's first piece
//    instead and zeroed in LDS by the lane that fetched them, in both operands: they add exactly 0.
//  * grid.y = S training segments of whole macro-tiles; their candidates [nq, S, k] go through
//    knn_topk_merge_kernel. The K order within a (query, row) and within ‖q‖² is fixed: results do
//    not depend on the grid or on S. No scratch, no workspace when S = 1.
#include "common.h"
#include "knn_list.h"

namespace {

typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int QD_ROWS = 64;              // queries per block
constexpr int QD_MT = 128;               // training rows per macro-tile
constexpr int QD_NA = QD_MT / 16;        // 16-row A tiles per macro-tile
constexpr int QD_NAF = QD_MT / 32;       // 1-KiB fill pieces of the training tile per wave
constexpr int QD_NBF = QD_ROWS / 32;     // … of the query tile
constexpr int QD_KC = 16;                // fp64 columns per K-chunk
constexpr int QD_ROWB = QD_KC * 8;       // bytes per tile row
constexpr int QD_TILEA = QD_MT * QD_ROWB;
constexpr int QD_TILEB = QD_ROWS * QD_ROWB;
constexpr int QD_SLOTB = QD_TILEA + QD_TILEB;  // the training tile, then the query tile

// Blocks per CU for a list of K entries, from the compiler's register report
// (profiles/r24/resources_knn_wide_f64.txt; 256 registers per lane is the most that lets two
// blocks share a CU). K = 4 and 8 fit (196 / 232 registers); K = 16 spills there (328 bytes of
// scratch per lane) and K = 32 carries 96 list registers, so both run one block per CU on the
// full register file (339 / 385 registers, no scratch). Splitting the epilogue into two 16-key
// halves was compiled and rejected: it spills at K = 16 and at K = 32 even with one block per CU.
template <int K>
struct F64Rung {
  static constexpr int BLOCKS = K >= 16 ? 1 : 2;
};

// Q / T / tn are not __restrict__: the asm fills read them behind the compiler's back
template <int K>
__global__ __launch_bounds__(256, F64Rung<K>::BLOCKS) void knn_fused_f64_kernel(const double* Q, long ldq, long nq, int D,
                                                                              const double* T, long ldt,
                                                                              const double* tn, long n, int k, int S,
                                                                              int* __restrict__ out_i,
                                                                              double* __restrict__ out_d) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  __shared__ __align__(16) unsigned char lds[2 * QD_SLOTB + 2 * QD_MT * 8];  // the ring, then two tiles' norms
  double* tnl = reinterpret_cast<double*>(lds + 2 * QD_SLOTB);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int g = lane >> 4;
  const long row0 = (long)blockIdx.x * QD_ROWS;
  const long qrow = row0 + wave * 16 + r16;
  const bool qok = qrow < nq;
  const int NC = (D + QD_KC - 1) / QD_KC;

  const long ntiles = (n + QD_MT - 1) / QD_MT;
  const long L = (ntiles + S - 1) / S;
  const long t0 = (long)blockIdx.y * L;
  const long t1 = t0 + L < ntiles ? t0 + L : ntiles;
  const long iters = t0 < t1 ? (t1 - t0) * NC : 0;

  // fill geometry: piece q = wave + 4i of a tile covers tile rows 8q … 8q + 7; lane l lands at
  // (row 8q + l/8, slot l%8) and fetches global piece slot ^ ((row >> 1) mod 8); (row >> 1) mod 8
  // is 4·(wave mod 2) + l/16 for every i
  const int gp = (lane & 7) ^ (4 * (wave & 1) + (lane >> 4));
  const bool tail_ok = (NC - 1) * QD_KC + gp * 2 < D;  // this lane's piece of the last chunk is inside the row
  unsigned q_off[QD_NBF];                              // byte offset of the lane's query rows from the block's first
#pragma unroll
  for (int i = 0; i < QD_NBF; ++i) {
    long r = row0 + 8 * (wave + 4 * i) + (lane >> 3);
    r = r < nq ? r : nq - 1;
    q_off[i] = (unsigned)((r - row0) * ldq * 8);
  }
  const unsigned ldtb = (unsigned)(ldt * 8);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* qblk = reinterpret_cast<const char*>(Q) + row0 * ldq * 8;  // uniform

  // chunk (macro-tile P_, chunk KC_) → ring slot S_. Issued by inline asm with the ordering
  // explicit (vmcnt + one barrier per chunk), as in kmeans_wide_f64.hip; every wave issues the
  // same QD_NAF + QD_NBF loads per chunk. M0: written only by these statements in this kernel.
#define QD_FILL(P_, KC_, S_)                                                                              \
  {                                                                                                       \
    const unsigned gb_ = ((KC_) == NC - 1 && !tail_ok) ? 0u : (unsigned)(gp * 16);                        \
    const char* asrc_ = reinterpret_cast<const char*>(T) + ((long)(P_) * QD_MT * ldt + (long)(KC_) * QD_KC) * 8; \
    const char* bsrc_ = qblk + (long)(KC_) * QD_ROWB;                                                     \
    const int rmax_ = (int)(n - 1 - (long)(P_) * QD_MT);                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < QD_NAF; ++i_) {                                               \
      const unsigned d_ = dst0 + (unsigned)((S_) * QD_SLOTB + i_ * 4096);                                 \
      int r_ = 8 * (wave + 4 * i_) + (lane >> 3);                                                         \
      r_ = r_ < rmax_ ? r_ : rmax_;                                                                       \
      const unsigned ao_ = (unsigned)r_ * ldtb + gb_;                                                     \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(ao_), "s"(asrc_), "s"(d_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < QD_NBF; ++i_) {                                               \
      const unsigned e_ = dst0 + (unsigned)((S_) * QD_SLOTB + QD_TILEA + i_ * 4096);                      \
      const unsigned bo_ = q_off[i_] + gb_;                                                               \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(bo_), "s"(bsrc_), "s"(e_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
  }
  // ‖t‖² of row threadIdx.x of macro-tile P_ (clamped like the rows)
#define QD_NORM(P_) tn[((P_) * QD_MT + (long)threadIdx.x) < n ? ((P_) * QD_MT + (long)threadIdx.x) : n - 1]

  double bd[K];
  int bi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { bd[i] = INFINITY; bi[i] = INT32_MAX; }
  double td = INFINITY;  // the admission bound of the lane's query
  int ti = INT32_MAX;

  double tv = 0.0;  // the next macro-tile's norm of this thread's row, on its way to LDS
  if (iters > 0) {
    if ((int)threadIdx.x < QD_MT) tv = QD_NORM(t0);
    QD_FILL(t0, 0, 0)
  }

  f64x4_t acc[QD_NA];
  double qs = 0.0, qn = 0.0;  // the lane's share of Σq², and the sum
  // fragment addresses inside a slot: row (16·t + r16), piece (g + 4·hp) ^ ((r16 >> 1) mod 8)
  const int sw = r16 >> 1;
  const int arow = r16 * QD_ROWB;
  const int brow = QD_TILEA + (16 * wave + r16) * QD_ROWB;

  long p = t0;                                       // the chunk being multiplied
  int kc = 0;
  long fp = NC > 1 ? t0 : t0 + 1;                    // the next chunk to fill
  int fkc = NC > 1 ? 1 : 0;
  for (long i = 0; i < iters; ++i) {
    const int slot = (int)(i & 1);
    // this wave's share of chunk i has landed (and tv)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1 && !tail_ok) {
#pragma unroll
      for (int q = 0; q < QD_NAF; ++q)
        *reinterpret_cast<uint4*>(lds + slot * QD_SLOTB + (wave + 4 * q) * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int q = 0; q < QD_NBF; ++q)
        *reinterpret_cast<uint4*>(lds + slot * QD_SLOTB + QD_TILEA + (wave + 4 * q) * 1024 + lane * 16) =
            make_uint4(0u, 0u, 0u, 0u);
    }
    if (kc == 0 && (int)threadIdx.x < QD_MT) tnl[(int)(p & 1) * QD_MT + threadIdx.x] = tv;
    // … and every wave's; every wave is past chunk i − 1, whose slot the next fill takes
    __syncthreads();
    if (i + 1 < iters) {
      QD_FILL(fp, fkc, slot ^ 1)
      if (fkc == 0 && (int)threadIdx.x < QD_MT) tv = QD_NORM(fp);
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    if (kc == 0) {
#pragma unroll
      for (int t = 0; t < QD_NA; ++t) acc[t] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    }
    const unsigned char* sb = lds + slot * QD_SLOTB;
    const bool first = p == t0;
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
      const int po = ((g + 4 * hp) ^ sw) * 16;
      const f64x2_t b = *reinterpret_cast<const f64x2_t*>(sb + brow + po);
      f64x2_t a[QD_NA];
#pragma unroll
      for (int t = 0; t < QD_NA; ++t) a[t] = *reinterpret_cast<const f64x2_t*>(sb + arow + t * 16 * QD_ROWB + po);
      if (first) {
#pragma unroll
        for (int e = 0; e < 2; ++e) qs = __builtin_fma(b[e], b[e], qs);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int t = 0; t < QD_NA; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][e], b[e], acc[t], 0, 0, 0);
    }
    if (++kc < NC) continue;

    if (first) {
      // Σq² of the lane's query: the four lane groups' shares, (g0 + g1) + (g2 + g3) in every lane
      qn = qs + __shfl_xor(qs, 16, 64);
      qn += __shfl_xor(qn, 32, 64);
    }
    // ---- the macro-tile's 32 keys of this lane: slot r is row jb + 4r + g. A NaN key fails '<='
    // and is never admitted.
    const double* tnt = tnl + (int)(p & 1) * QD_MT + g;
    const long jb = p * QD_MT;
    double key[32];
#pragma unroll
    for (int t = 0; t < QD_NA; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) key[4 * t + q] = __builtin_fabs((qn + tnt[16 * t + 4 * q]) - 2.0 * acc[t][q]);
    // bit r = slot r admitted; built by shifts, highest slot first (knn_wide.hip)
    unsigned mask = 0u;
#pragma unroll
    for (int r = 31; r >= 0; --r) mask = (mask << 1) | (key[r] <= td ? 1u : 0u);
    if (jb + QD_MT > n) {  // last tile: drop the clamped rows
      const int lim = (int)(n - jb) - g;
      unsigned valid = 0u;
#pragma unroll
      for (int r = 31; r >= 0; --r) valid = (valid << 1) | (4 * r < lim ? 1u : 0u);
      mask &= valid;
    }
    while (mask) {
      const int b = __builtin_ctz(mask);
      mask &= mask - 1u;
      const double d = select_slot(key, b);
      const int j = (int)(jb + 4 * b + g);
      if (lex_less(d, j, td, ti) && lex_less(d, j, bd[K - 1], bi[K - 1])) topk_insert<K>(bd, bi, d, j);
    }
    // refresh the admission bound: the least k-th entry among the query's four lanes
    kth_entry<K>(bd, bi, k, td, ti);
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double xd = __shfl_xor(td, o, 64);
      const int xi = __shfl_xor(ti, o, 64);
      if (lex_less(xd, xi, td, ti)) { td = xd; ti = xi; }
    }
    kc = 0;
    ++p;
  }
#undef QD_FILL
#undef QD_NORM

  // ---- merge the four lane-group lists of each query under (key, index); lane group 0 writes.
  // The pairs of the four lists are distinct (disjoint rows): one lane pops per winner.
  const long o = (qrow * S + blockIdx.y) * k;
  for (int t = 0; t < k; ++t) {
    double wd = bd[0];
    int wi = bi[0];
#pragma unroll
    for (int x = 16; x <= 32; x <<= 1) {
      const double xd = __shfl_xor(wd, x, 64);
      const int xi = __shfl_xor(wi, x, 64);
      if (lex_less(xd, xi, wd, wi)) { wd = xd; wi = xi; }
    }
    if (g == 0 && qok) {
      out_i[o + t] = wi;
      if (out_d) out_d[o + t] = S == 1 ? __builtin_sqrt(wd) : wd;
    }
    if (bi[0] == wi && wi != INT32_MAX) topk_pop<K>(bd, bi);
  }
}

// the list length K of a k: 4 / 8 / 16 / 32 (the launcher has validated k <= 32; the occupancy
// query answers for any k)
template <typename F>
int with_f64_list(int k, F&& f) {
  return with_ceil<4, 8, 16, 32>(k < 32 ? k : 32, f);
}

}  // namespace

// Resident fp64 fused-kernel blocks per CU for k — the host sizes the segment split with it.
FMLX_API int fmlx_knn_fused_f64_blocks_per_cu(int k) {
  return with_f64_list(k, [&](auto K) {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, knn_fused_f64_kernel<K.value>, 256, 0) != hipSuccess) return 1;
    return b > 0 ? b : 1;
  });
}

// Fused KNN for fp64 rows: Q [nq, D] and T [n, D] fp64 row-major (leading dims ldq, ldt), tn [n]
// the squared norms of T's rows. k nearest per query under |(‖q‖² + tn) − 2·q·t| (nearest first,
// ties → lower index, a NaN key never chosen: with fewer than k keys that are not NaN the last
// slots hold INT32_MAX and +inf) into idx [nq, k] and, if non-null, their distances (sqrt of the
// key) into dist [nq, k]. S training segments (1..256); S > 1 needs ws_d/ws_i of nq·S·k. −1 unless
// 16 <= D <= 4096, D even, the pitches are even and below 2^22 doubles (32-bit byte offsets inside
// a tile), Q and T are 16-byte aligned, 1 <= k <= min(32, n) and n < 2^31 − 128.
FMLX_API int fmlx_knn_fused_f64(const double* Q, long ldq, long nq, int D, const double* T, long ldt, const double* tn,
                                long n, int k, int S, int* idx, double* dist, double* ws_d, int* ws_i, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D < 16 || D > 4096 || (D % 2) != 0 || ldq < D || ldt < D || (ldq % 2) != 0 || (ldt % 2) != 0 ||
      ldq >= (1L << 22) || ldt >= (1L << 22) || ((uintptr_t)Q % 16) != 0 || ((uintptr_t)T % 16) != 0 || tn == nullptr)
    return -1;
  if (k < 1 || k > 32 || k > n || n >= (long)INT32_MAX - 128 || S < 1 || S > 256 || nq < 0) return -1;
  if (S > 1 && (ws_d == nullptr || ws_i == nullptr)) return -1;
  if (nq == 0) return 0;
  const long bq = (nq + QD_ROWS - 1) / QD_ROWS;
  if (bq > 0x7fffffffL) return -1;
  int* si = S > 1 ? ws_i : idx;
  double* sd = S > 1 ? ws_d : dist;
  return with_f64_list(k, [&](auto K) {
    hipLaunchKernelGGL(knn_fused_f64_kernel<K.value>, dim3((unsigned)bq, S), dim3(256), 0, s, Q, ldq, nq, D, T, ldt, tn,
                       n, k, S, si, sd);
    if (S > 1) launch_topk_merge<K.value>(ws_d, ws_i, nq, S, k, idx, dist, s);
    FMLX_CHECK_LAUNCH();
  });
}

FMLX_DEFINE_PRELOAD()
