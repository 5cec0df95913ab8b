// KMeans for dense fp64 rows of 16 <= D <= 4096, D even (euclidean and cosine;
// FMLX_COMPUTE_DTYPE=fp64, the parity mode): the K-tiled fp64 MFMA assign and the update's wide gather-sum. The fp64 routes
// before it are the wave-per-row / thread-per-row kernels of kmeans.hip; kmeans_wide.hip and
// kmeans_wide_f32.hip are the bf16 and fp32 counterparts.
//
// kmeans_assign_f64_kernel: d2 = max(0, pn·pn + cn·cn − 2·x·c) with pn = sqrt(Σx²) and cn = ‖c‖ as
// kmeans_finalize_kernel keeps it, the generic kernels' expression; only the summation order of
// x·c and Σx² differs from kmeans_assign_wave_kernel<double>.
//  * v_mfma_f64_16x16x4_f64 with the centroid tile as A and the rows as B (dct.hip documents the
//    fragments): a lane holds one double of A and of B, row / column lane & 15 and K index
//    lane >> 4; accumulator element q is centroid 4q + (lane >> 4) of the tile, row lane & 15. A
//    lane's accumulators belong to one row of X per B tile.
//  * A block of 256 threads owns 128 rows of X for the whole kernel: 4 waves × 32 rows, two
//    16-row B tiles per wave. It walks the centroids in macro-tiles of 64 (four 16-centroid A
//    tiles: 8 accumulator tiles of 4 doubles, 64 registers) and K in chunks of 16 doubles.
//  * Both operands of a chunk go as they are stored, from the row-major centroid matrix and the
//    row-major X view (pointer, pitch) straight into LDS by LDS-DMA (64 × 16 and 128 × 16
//    doubles). A tile row is 128 bytes: its 16-byte piece s sits at slot s ^ ((r >> 1) mod 8),
//    applied by the choice of the global piece a lane fetches. The 16 rows that the lanes of one
//    lane group read with one ds_read_b128 then cover 16 different 16-byte bank groups of the
//    256-byte bank row (row parity picks the half, r >> 1 the slot): no padding.
//  * A 16-byte piece is two consecutive K indices. Lane group g = lane >> 4 takes the pieces g and
//    g + 4 of the chunk: 4 MFMA K-steps per chunk and tile pair, 12 ds_read_b128 per 32 MFMAs and
//    wave. K-step (hp, e) of group g is column 8·hp + 2g + e of the chunk in A and B alike.
//  * Σx² comes from the B fragments a lane holds during the first macro-tile (chunk order, then
//    the four K-steps); the four lane groups' partial sums of a row meet in a symmetric butterfly
//    before the first epilogue, so every lane of a row holds the same pn. No second pass over X.
//  * Ring of two 24-KiB slots (centroid tile, then X tile): chunk i + 1 fills under chunk i's
//    MFMAs; per chunk one s_waitcnt vmcnt(0) (this wave's share has landed) and one barrier
//    (everyone's has, and everyone is past chunk i − 1, whose slot the next fill takes). The
//    fill-ahead cursor wraps to the next macro-tile after every chunk when D = 16 (one chunk).
//  * ‖c‖ of a macro-tile's centroids comes through LDS (a plain load issued with the fill of the
//    tile's first chunk, stored after the next vmcnt(0), published by the same barrier). The
//    epilogue reads it after the tile's last chunk, while a faster wave may already publish the
//    next tile's: two buffers, by tile parity.
//  * A running (key, centroid) pair per lane and B tile under strict '<': macro-tiles, A tiles and
//    accumulator elements ascend in centroid index, so a lane keeps the lowest index of equal
//    keys. The clamp is written so that a NaN key stays NaN and never wins. After the last
//    macro-tile the four lane groups' candidates of a row meet by two cross-lane exchanges under
//    (key, index) order; a row without a key below +inf gets label 0. Lanes 0–15 of each wave
//    store 2 × 16 consecutive labels. No workspace, one launch.
//  * Tails: rows >= n and centroids >= k are clamped for the loads (never stored / never chosen);
//    the pieces of the last chunk past D are fetched from the chunk's first piece instead and
//    zeroed in LDS by the lane that fetched them, in both operands: they add exactly 0.
//  * The K order within a (row, centroid) and within Σx² is fixed: labels do not depend on the grid.
//  * COSINE (kmeans_assign_f64_kernel<true>): the generic kernels' 1 − x·c / pn / cn on the same
//    accumulators, pn and norm table; NaN (a zero, inf or NaN row or centroid) never wins, and the
//    running index starts at −1, the generic kernels' label for a row without a winner.
//
// kmeans_chunk_sum_f64w_kernel<PPL>: kmeans_chunk_sum_f32w_kernel's contract for fp64 rows of any
// even D up to 4096 — int32 row order, a lane holds the 16-byte pieces lane, lane + 64, … of a row
// (PPL of them, a compile-time rung up to 16; rows wider than 2048 take the columns in two passes
// of 16 pieces), a wave sums its stripe of the chunk's rows in row order with U rows' loads in
// flight, and the four waves' sums are added in wave order.
#include "common.h"

namespace {

typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int KD_ROWS = 128;             // rows per block
constexpr int KD_MT = 64;                // centroids per macro-tile
constexpr int KD_NA = KD_MT / 16;        // 16-centroid A tiles per macro-tile
constexpr int KD_NAF = KD_MT / 32;       // 1-KiB fill pieces of the centroid tile per wave
constexpr int KD_KC = 16;                // fp64 columns per K-chunk
constexpr int KD_ROWB = KD_KC * 8;       // bytes per tile row
constexpr int KD_TILEA = KD_MT * KD_ROWB;
constexpr int KD_TILEB = KD_ROWS * KD_ROWB;
constexpr int KD_SLOTB = KD_TILEA + KD_TILEB;  // the centroid tile, then the X tile
constexpr int KD_CH = 256;               // rows per gather chunk (ops/kmeans.py CHUNK)

// X / C / cnorm are not __restrict__: the asm fills read them behind the compiler's back
template <bool COSINE>
__global__ __launch_bounds__(256, 2) void kmeans_assign_f64_kernel(const double* X, long ld, long n, int D,
                                                                   const double* C, long ldc, const double* cnorm,
                                                                   int k, int* __restrict__ labels) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  __shared__ __align__(16) unsigned char lds[2 * KD_SLOTB + 2 * KD_MT * 8];  // the ring, then two tiles' norms
  double* cnl = reinterpret_cast<double*>(lds + 2 * KD_SLOTB);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int g = lane >> 4;
  const long row0 = (long)blockIdx.x * KD_ROWS;
  const int NC = (D + KD_KC - 1) / KD_KC;
  const int ntiles = (k + KD_MT - 1) / KD_MT;
  const long iters = (long)ntiles * NC;

  // fill geometry: piece q = wave + 4i of a tile covers tile rows 8q … 8q + 7; lane l lands at
  // (row 8q + l/8, slot l%8) and fetches global piece slot ^ ((row >> 1) mod 8); (row >> 1) mod 8
  // is 4·(wave mod 2) + l/16 for every i
  const int gp = (lane & 7) ^ (4 * (wave & 1) + (lane >> 4));
  const bool tail_ok = (NC - 1) * KD_KC + gp * 2 < D;  // this lane's piece of the last chunk is inside the row
  unsigned x_off[4];                                   // byte offset of the lane's X rows from the block's first
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long r = row0 + 8 * (wave + 4 * i) + (lane >> 3);
    r = r < n ? r : n - 1;
    x_off[i] = (unsigned)((r - row0) * ld * 8);
  }
  const unsigned ldcb = (unsigned)(ldc * 8);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* xblk = reinterpret_cast<const char*>(X) + row0 * ld * 8;  // uniform

  // chunk (macro-tile P_, chunk KC_) → ring slot S_. Issued by inline asm with the ordering
  // explicit (vmcnt + one barrier per chunk), as in kmeans_wide_f32.hip; every wave issues the
  // same KD_NAF + 4 loads per chunk. M0: written only by these statements in this kernel.
#define KD_FILL(P_, KC_, S_)                                                                              \
  {                                                                                                       \
    const unsigned gb_ = ((KC_) == NC - 1 && !tail_ok) ? 0u : (unsigned)(gp * 16);                        \
    const char* asrc_ = reinterpret_cast<const char*>(C) + ((long)(P_) * KD_MT * ldc + (long)(KC_) * KD_KC) * 8; \
    const char* bsrc_ = xblk + (long)(KC_) * KD_ROWB;                                                     \
    const int cmax_ = k - 1 - (P_) * KD_MT;                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < KD_NAF; ++i_) {                                               \
      const unsigned d_ = dst0 + (unsigned)((S_) * KD_SLOTB + i_ * 4096);                                 \
      int c_ = 8 * (wave + 4 * i_) + (lane >> 3);                                                         \
      c_ = c_ < cmax_ ? c_ : cmax_;                                                                       \
      const unsigned ao_ = (unsigned)c_ * ldcb + gb_;                                                     \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(ao_), "s"(asrc_), "s"(d_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                    \
      const unsigned e_ = dst0 + (unsigned)((S_) * KD_SLOTB + KD_TILEA + i_ * 4096);                      \
      const unsigned bo_ = x_off[i_] + gb_;                                                               \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(bo_), "s"(bsrc_), "s"(e_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
  }
  // ‖c‖ of centroid threadIdx.x of macro-tile P_ (clamped like the rows)
#define KD_NORM(P_) cnorm[((P_) * KD_MT + (int)threadIdx.x) < k ? ((P_) * KD_MT + (int)threadIdx.x) : k - 1]

  // per B tile: the lane's best key of its row, its share of Σx², pn·pn (cosine: pn)
  double bk[2], xs[2], pp[2];
  int bi[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    bk[j] = __builtin_huge_val();
    bi[j] = COSINE ? -1 : 0;
    xs[j] = 0.0;
    pp[j] = 0.0;
  }

  double cv = 0.0;  // the next macro-tile's norm of this thread's centroid, on its way to LDS
  if ((int)threadIdx.x < KD_MT) cv = KD_NORM(0);
  KD_FILL(0, 0, 0)

  f64x4_t acc[KD_NA][2];
  // fragment addresses inside a slot: row (16·t + r16), piece (g + 4·hp) ^ ((r16 >> 1) mod 8)
  const int sw = r16 >> 1;
  const int arow = r16 * KD_ROWB;
  const int brow = KD_TILEA + (32 * wave + r16) * KD_ROWB;

  int p = 0, kc = 0;                               // the chunk being multiplied
  int fp = NC > 1 ? 0 : 1, fkc = NC > 1 ? 1 : 0;   // the next chunk to fill
  for (long i = 0; i < iters; ++i) {
    const int slot = (int)(i & 1);
    // this wave's share of chunk i has landed (and cv)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1 && !tail_ok) {
#pragma unroll
      for (int q = 0; q < KD_NAF; ++q)
        *reinterpret_cast<uint4*>(lds + slot * KD_SLOTB + (wave + 4 * q) * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<uint4*>(lds + slot * KD_SLOTB + KD_TILEA + (wave + 4 * q) * 1024 + lane * 16) =
            make_uint4(0u, 0u, 0u, 0u);
    }
    if (kc == 0 && (int)threadIdx.x < KD_MT) cnl[(p & 1) * KD_MT + threadIdx.x] = cv;
    // … and every wave's; every wave is past chunk i − 1, whose slot the next fill takes
    __syncthreads();
    if (i + 1 < iters) {
      KD_FILL(fp, fkc, slot ^ 1)
      if (fkc == 0 && (int)threadIdx.x < KD_MT) cv = KD_NORM(fp);
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    if (kc == 0) {
#pragma unroll
      for (int t = 0; t < KD_NA; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[t][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    }
    const unsigned char* sb = lds + slot * KD_SLOTB;
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
      const int po = ((g + 4 * hp) ^ sw) * 16;
      f64x2_t b[2], a[KD_NA];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f64x2_t*>(sb + brow + j * 16 * KD_ROWB + po);
#pragma unroll
      for (int t = 0; t < KD_NA; ++t) a[t] = *reinterpret_cast<const f64x2_t*>(sb + arow + t * 16 * KD_ROWB + po);
      if (p == 0) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int j = 0; j < 2; ++j) xs[j] = __builtin_fma(b[j][e], b[j][e], xs[j]);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int t = 0; t < KD_NA; ++t)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][e], b[j][e], acc[t][j], 0, 0, 0);
    }
    if (++kc < NC) continue;

    if (p == 0) {
      // Σx² of the lane's rows: the four lane groups' shares, (g0 + g1) + (g2 + g3) in every lane
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        double s = xs[j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const double pn = sqrt(s);
        pp[j] = COSINE ? pn : pn * pn;
      }
    }
    // ---- the macro-tile's keys in ascending centroid order under strict '<': the lowest index of
    // equal keys stays, a NaN key and a clamped centroid never win
    const double* cnt = cnl + (p & 1) * KD_MT + g;
    const int cb = p * KD_MT + g;
#pragma unroll
    for (int t = 0; t < KD_NA; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cb + 16 * t + 4 * q;
        const double cn = cnt[16 * t + 4 * q];
        const double cc = cn * cn;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          double d2;
          if constexpr (COSINE) {
            // the generic kernels' expression: NaN (never wins) for a zero, inf or NaN row or centroid
            d2 = 1.0 - acc[t][j][q] / pp[j] / cn;
          } else {
            d2 = pp[j] + cc - 2.0 * acc[t][j][q];
            d2 = d2 < 0.0 ? 0.0 : d2;  // NaN stays NaN
          }
          const bool lt = d2 < bk[j] && c < k;
          bk[j] = lt ? d2 : bk[j];
          bi[j] = lt ? c : bi[j];
        }
      }
    kc = 0;
    ++p;
  }
#undef KD_FILL
#undef KD_NORM

  // ---- the four lane groups of a row meet under (key, index) order; lane group 0 writes
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double ok = __shfl_xor(bk[j], o, 64);
      const int oi = __shfl_xor(bi[j], o, 64);
      if (ok < bk[j] || (ok == bk[j] && oi < bi[j])) {
        bk[j] = ok;
        bi[j] = oi;
      }
    }
    const long xrow = row0 + wave * 32 + 16 * j + r16;
    if (g == 0 && xrow < n) labels[xrow] = bi[j];
  }
}

// ------------------------------------------------------------------------------------------
// the update's gather-sum for wide fp64 rows
// ------------------------------------------------------------------------------------------
template <int PPL>
__global__ __launch_bounds__(256) void kmeans_chunk_sum_f64w_kernel(const double* __restrict__ X, long ld, int D,
                                                                    const int* __restrict__ order,
                                                                    const long* __restrict__ offsets,
                                                                    const long* __restrict__ chunk_off, int k,
                                                                    double* __restrict__ partial) {
  constexpr int U = PPL >= 16 ? 1 : PPL >= 4 ? 2 : 4;  // rows in flight per wave: at least 4 independent loads per lane
  const long b = blockIdx.x;
  if (b >= chunk_off[k]) return;
  int lo = 0, hi = k;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= b) lo = mid; else hi = mid;
  }
  const int j = lo;
  const long p0 = offsets[j] + (b - chunk_off[j]) * KD_CH;
  long p1 = p0 + KD_CH;
  if (p1 > offsets[j + 1]) p1 = offsets[j + 1];
  const int nrow = (int)(p1 - p0);
  __shared__ int rows_s[KD_CH];
  __shared__ __align__(16) double sm[3][PPL * 128];  // the sums of waves 1..3
  if ((int)threadIdx.x < nrow) rows_s[threadIdx.x] = order[p0 + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int np = D / 2;  // 16-byte pieces per row
  // the columns in passes of PPL·64 pieces (one pass up to D = 2048): the same sums whatever the split
  for (int pb = 0; pb < np; pb += PPL * 64) {
    double2 acc[PPL];
#pragma unroll
    for (int v = 0; v < PPL; ++v) acc[v] = make_double2(0.0, 0.0);
    for (int q0 = wave; q0 < nrow; q0 += 4 * U) {
      double2 x[U][PPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = q0 + 4 * u;
        const double* xr = X + (long)rows_s[q < nrow ? q : 0] * ld;  // unconditional (row 0 of the chunk), masked below
#pragma unroll
        for (int v = 0; v < PPL; ++v) {
          const int pc = pb + lane + 64 * v;
          x[u][v] = pc < np ? *reinterpret_cast<const double2*>(xr + pc * 2) : make_double2(0.0, 0.0);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = q0 + 4 * u < nrow;
#pragma unroll
        for (int v = 0; v < PPL; ++v) {
          acc[v].x += ok ? x[u][v].x : 0.0;
          acc[v].y += ok ? x[u][v].y : 0.0;
        }
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < PPL; ++v) *reinterpret_cast<double2*>(&sm[wave - 1][(lane + 64 * v) * 2]) = acc[v];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int v = 0; v < PPL; ++v) {
        const int pl = lane + 64 * v;
        if (pb + pl < np) {
          const double2 s0 = *reinterpret_cast<const double2*>(&sm[0][pl * 2]);
          const double2 s1 = *reinterpret_cast<const double2*>(&sm[1][pl * 2]);
          const double2 s2 = *reinterpret_cast<const double2*>(&sm[2][pl * 2]);
          // D even, partial 16-byte aligned
          *reinterpret_cast<double2*>(partial + b * D + (pb + pl) * 2) =
              make_double2(((acc[v].x + s0.x) + s1.x) + s2.x, ((acc[v].y + s0.y) + s1.y) + s2.y);
        }
      }
    }
    __syncthreads();  // wave 0 has read sm before the next pass writes it
  }
}

template <bool COSINE>
int kd_assign(const double* X, long ld, long n, int D, const double* C, long ldc, const double* cnorm, int k,
              int* labels, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D < 16 || D > 4096 || (D % 2) != 0 || ld < D || ldc < D || (ld % 2) != 0 || (ldc % 2) != 0 ||
      ld >= (1L << 22) || ldc >= (1L << 22) || ((uintptr_t)X % 16) != 0 || ((uintptr_t)C % 16) != 0 || k < 1 ||
      k > INT32_MAX - KD_MT || cnorm == nullptr)
    return -2;
  if (n <= 0) return 0;
  const long blocks = (n + KD_ROWS - 1) / KD_ROWS;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(kmeans_assign_f64_kernel<COSINE>, dim3((unsigned)blocks), dim3(256), 0, s, X, ld, n, D, C, ldc,
                     cnorm, k, labels);
  FMLX_CHECK_LAUNCH();
}

}  // namespace

// The K-tiled fp64 MFMA assign: X [n, D] (pitch ld) and the centroids C [k, D] (pitch ldc) fp64
// row-major; cnorm [k] holds ‖c‖. Label = the lowest index among the minimal
// max(0, ‖x‖² + ‖c‖² − 2·x·c) (NaN counts as +inf; 0 if no key is below +inf). −2 unless
// 16 <= D <= 4096, D even, the pitches are even and below 2^22 doubles (32-bit byte offsets inside
// a tile), X and C are 16-byte aligned and 1 <= k.
FMLX_API int fmlx_kmeans_assign_f64_wide(const double* X, long ld, long n, int D, const double* C, long ldc,
                                         const double* cnorm, int k, int* labels, void* stream) {
  return kd_assign<false>(X, ld, n, D, C, ldc, cnorm, k, labels, stream);
}

// The cosine instantiation, same operands and limits: label = the lowest index among the minimal
// 1 − x·c / ‖x‖ / ‖c‖ (NaN never wins), −1 for a row without a key below +inf.
FMLX_API int fmlx_kmeans_assign_f64_wide_cos(const double* X, long ld, long n, int D, const double* C, long ldc,
                                             const double* cnorm, int k, int* labels, void* stream) {
  return kd_assign<true>(X, ld, n, D, C, ldc, cnorm, k, labels, stream);
}

// fmlx_kmeans_chunk_sum_f32w's contract (int32 row order, partial[max_chunks][D] fp64) for fp64
// rows of any even D up to 4096. −2 for other shapes or rows that are not 16-byte aligned.
FMLX_API int fmlx_kmeans_chunk_sum_f64w(const double* X, long ld, int D, const int* order, const long* offsets,
                                        const long* chunk_off, int k, long max_chunks, double* partial, void* stream) {
  if (max_chunks <= 0) return 0;
  if (D < 2 || D > 4096 || (D % 2) != 0 || (ld % 2) != 0 || ld < D || ((uintptr_t)X % 16) != 0 ||
      ((uintptr_t)partial % 16) != 0)
    return -2;
  return with_ceil<1, 2, 4, 8, 16>(fmlx_ceil_div(D > 2048 ? 2048 : D, 128), [&](auto ppl) {
    hipLaunchKernelGGL(kmeans_chunk_sum_f64w_kernel<ppl.value>, dim3((unsigned)max_chunks), dim3(256), 0,
                       (hipStream_t)stream, X, ld, D, order, offsets, chunk_off, k, partial);
    return (int)hipGetLastError();
  }, -2);
}

FMLX_DEFINE_PRELOAD()
