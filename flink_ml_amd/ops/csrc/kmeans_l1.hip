// KMeans assign under manhattan distance for dense fp32, bf16 and fp64 rows up to D = 4096: a tiled
// VALU kernel (L1 distance is no GEMM: the MFMA assigns of kmeans_wide*.hip cannot be instantiated
// for it). The routes before it are the wave-per-row / thread-per-row kernels of kmeans.hip.
//
// kmeans_assign_l1_kernel<TIn, TAcc>: the tile geometry of kmeans_wide_f32.hip, a register-blocked
// Σ|x − c| in place of the matrix core.
//  * A block of 256 threads owns 128 rows of X for the whole kernel. It walks the centroids in
//    macro-tiles of MT = 128 (fp64: 64) and K in chunks of 128 bytes of a centroid row (32 floats,
//    16 doubles; bf16 rows: 32 columns = 64 bytes of X against 32 fp32 centroid columns). No n × k
//    block exists anywhere; a block reads the whole centroid matrix once and only its own rows.
//  * The threads form a 16 × 16 grid (tr, tc); thread (tr, tc) holds the accumulators of rows
//    tr + 16·i (i < 8) against centroids tc + 16·j (j < MT/16) of the macro-tile: 8 × 8 floats or
//    8 × 4 doubles, 64 VGPRs. A wave is an 8 × 8 patch of that grid (tr = 8·(w & 1) + lane % 8,
//    tc = 8·(w / 2) + lane / 8), so a ds_read_b128 of a row fragment touches 8 consecutive tile
//    rows, one per lane column, and the 8 lanes of a column share an address (broadcast); the
//    centroid fragment likewise with the roles swapped.
//  * Both operands of a chunk go as they are stored from global memory into a two-slot LDS ring
//    (centroid tile, then X tile) by LDS-DMA, 1 KiB per wave instruction. A 128-byte tile row keeps
//    its 16-byte piece s at slot s ^ (row mod 8); a 64-byte bf16 row keeps it at s ^ (row/2 mod 4).
//    Either way 8 consecutive tile rows put one logical piece on 8 different 16-byte bank groups,
//    so the fragment reads above are conflict free. The swizzle is applied by the choice of the
//    global piece a lane fetches. Chunk i + 1 fills under chunk i's arithmetic; per chunk one
//    s_waitcnt vmcnt(0) (this wave's share has landed; nothing else is in flight) and one barrier
//    (everyone's has, and everyone is past chunk i − 1, whose slot the next fill takes).
//  * Inner loop, per 16-byte piece: 8 row fragments and MT/16 centroid fragments, then for every
//    (i, j) a packed difference (v_pk_add_f32 with a negated source: two elements per issue) and
//    one v_add_f32 per element whose source carries |·|: 1.5 VALU issues per pair-element. fp64:
//    v_add_f64 twice, the second with |·|. bf16 row fragments are widened to fp32 once per piece
//    (a shift or a mask per element), amortised over the thread's centroids.
//  * One accumulator per (row, centroid), K ascending: a centroid's key does not depend on the
//    thread, wave or macro-tile it sits in, so duplicate centroids have bitwise equal keys.
//  * Tails: rows >= n and centroids >= k are clamped for the loads (never stored / masked by index
//    in the epilogue); the pieces of the last chunk past D are fetched from the chunk's first piece
//    instead and zeroed in LDS by the lane that fetched them, in both operands: |0 − 0| adds 0.
//  * Epilogue per macro-tile: a running (key, index) per row and thread under strict '<', j
//    ascending; a NaN key never wins and an inf key neither (the running key starts at +inf, the
//    index at −1: DistanceMeasure.findClosest's default rule, the generic kernels' result). After
//    the last macro-tile the 16 threads of a row meet once through LDS (the ring is free then)
//    under (key, index) order and 128 threads store 128 consecutive labels. No workspace.
//  * The X tile is staged again for every macro-tile (k > MT), as in kmeans_wide_f32.hip: the
//    kernel is bound by the VALU (a chunk of one macro-tile is 3 Ki VALU instructions per wave
//    against 32 KiB of fill) and the re-reads are the block's own rows only.
#include "common.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));

constexpr int KL_ROWS = 128;   // rows per block
constexpr int KL_CROWB = 128;  // bytes of a centroid tile row = one K chunk

template <typename TAcc> struct KlFrag;
template <> struct KlFrag<float> { typedef f32x4_t V; };
template <> struct KlFrag<double> { typedef f64x2_t V; };

__device__ __forceinline__ void kl_dma16(unsigned voff, const char* sbase, unsigned dst) {
  // M0: written only by this statement in this file
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(dst)
               : "memory", "m0");
}

// x − c on two elements in one issue. Written as vector arithmetic the compiler splits it into two
// v_sub_f32 (only single elements of the difference are used), 2 issues per pair-element.
__device__ __forceinline__ f32x2_t kl_pk_sub(f32x2_t x, f32x2_t c) {
  f32x2_t d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(x), "v"(c));
  return d;
}

// X / C are not __restrict__: the asm fills read them behind the compiler's back
template <typename TIn, typename TAcc>
__global__ __launch_bounds__(256, 2) void kmeans_assign_l1_kernel(const TIn* X, long ld, long n, int D, const TAcc* C,
                                                                  long ldc, int k, int* __restrict__ labels) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef typename KlFrag<TAcc>::V V;
  constexpr bool BF = sizeof(TIn) == 2;
  constexpr int XES = sizeof(TIn), CES = sizeof(TAcc);
  constexpr int EPP = 16 / CES;                  // accumulator-type elements per 16-byte piece
  constexpr int KC = KL_CROWB / CES;             // columns per K chunk
  constexpr int MT = CES == 8 ? 64 : 128;        // centroids per macro-tile
  constexpr int NJ = MT / 16;                    // centroids per thread
  constexpr int XROWB = KC * XES;                // bytes of an X tile row (128; bf16: 64)
  constexpr int XPR = XROWB / 16;                // 16-byte pieces per X tile row
  constexpr int XRPP = 64 / XPR;                 // X tile rows per 1-KiB fill piece
  constexpr int TILEA = MT * KL_CROWB;
  constexpr int TILEB = KL_ROWS * XROWB;
  constexpr int SLOTB = TILEA + TILEB;           // the centroid tile, then the X tile
  constexpr int NFA = TILEA / 4096, NFB = TILEB / 4096;  // fills per wave and chunk
  static_assert(2 * SLOTB <= 65536 && 2 * SLOTB >= KL_ROWS * 17 * (CES + 4), "ring holds the final candidates");
  __shared__ __align__(16) unsigned char lds[2 * SLOTB];  // at LDS offset 0: every LDS-DMA destination < 64 KiB

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tr = 8 * (wave & 1) + (lane & 7);
  const int tc = 8 * (wave >> 1) + (lane >> 3);
  const long row0 = (long)blockIdx.x * KL_ROWS;
  const int NC = (D + KC - 1) / KC;
  const int ntiles = (k + MT - 1) / MT;
  const long iters = (long)ntiles * NC;

  // fill geometry: 1-KiB piece q = wave + 4i of a tile; lane l lands at byte 16·l of it, that is
  // (tile row 8q + l/8, slot l%8) of a 128-byte row or (16q + l/4, slot l%4) of a 64-byte row, and
  // fetches the global piece that the swizzle keeps at that slot
  const int gc = (lane & 7) ^ (lane >> 3);
  const int gx = XPR == 8 ? gc : ((lane & 3) ^ ((lane >> 3) & 3));
  const bool tail_ok_c = (NC - 1) * KC + gc * (16 / CES) < D;  // the lane's piece of the last chunk is inside the row
  const bool tail_ok_x = (NC - 1) * KC + gx * (16 / XES) < D;
  unsigned x_off[NFB];  // byte offset of the lane's X rows from the block's first
#pragma unroll
  for (int i = 0; i < NFB; ++i) {
    long r = row0 + XRPP * (wave + 4 * i) + lane / XPR;
    r = r < n ? r : n - 1;
    x_off[i] = (unsigned)((r - row0) * ld * XES);
  }
  const unsigned ldcb = (unsigned)(ldc * CES);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* xblk = reinterpret_cast<const char*>(X) + row0 * ld * XES;  // uniform

  // chunk kc_ of macro-tile p_ → ring slot s_; every wave issues the same NFA + NFB loads
  auto fill = [&](int p_, int kc_, int s_) {
    const bool last = kc_ == NC - 1;
    const unsigned ga = (last && !tail_ok_c) ? 0u : (unsigned)(gc * 16);
    const unsigned gb = (last && !tail_ok_x) ? 0u : (unsigned)(gx * 16);
    const char* asrc = reinterpret_cast<const char*>(C) + ((long)p_ * MT * ldc + (long)kc_ * KC) * CES;
    const char* bsrc = xblk + (long)kc_ * XROWB;
    const int cmax = k - 1 - p_ * MT;
#pragma unroll
    for (int i = 0; i < NFA; ++i) {
      int c = 8 * (wave + 4 * i) + (lane >> 3);
      c = c < cmax ? c : cmax;
      kl_dma16((unsigned)c * ldcb + ga, asrc, dst0 + (unsigned)(s_ * SLOTB + i * 4096));
    }
#pragma unroll
    for (int i = 0; i < NFB; ++i) kl_dma16(x_off[i] + gb, bsrc, dst0 + (unsigned)(s_ * SLOTB + TILEA + i * 4096));
  };

  TAcc bk[8];  // this thread's best key of row tr + 16i over its centroids, and that centroid
  int bi[8];
  TAcc acc[8][NJ];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    bk[i] = (TAcc)__builtin_huge_val();
    bi[i] = -1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = 0;
  }

  fill(0, 0, 0);

  // fragment addresses inside a slot: centroid tc + 16j, piece s ^ (tc mod 8); row tr + 16i, piece
  // s ^ (tr mod 8) (bf16: (s/2) ^ (tr/2 mod 4))
  const int c7 = lane >> 3;
  const int x7 = XPR == 8 ? (lane & 7) : ((lane >> 1) & 3);
  const int arow = tc * KL_CROWB;
  const int brow = TILEA + tr * XROWB;

  int p = 0, kc = 0;                // the chunk being accumulated
  int fp = 0, fkc = 1;              // the next chunk to fill
  if (fkc == NC) { fkc = 0; fp = 1; }
  for (long it = 0; it < iters; ++it) {
    const int slot = (int)(it & 1);
    // this wave's share of chunk it has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1) {
      if (!tail_ok_c) {
#pragma unroll
        for (int q = 0; q < NFA; ++q)
          *reinterpret_cast<uint4*>(lds + slot * SLOTB + (wave + 4 * q) * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
      }
      if (!tail_ok_x) {
#pragma unroll
        for (int q = 0; q < NFB; ++q)
          *reinterpret_cast<uint4*>(lds + slot * SLOTB + TILEA + (wave + 4 * q) * 1024 + lane * 16) =
              make_uint4(0u, 0u, 0u, 0u);
      }
    }
    // … and every wave's; every wave is past chunk it − 1, whose slot the next fill takes
    __syncthreads();
    if (it + 1 < iters) {
      fill(fp, fkc, slot ^ 1);
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    const unsigned char* sb = lds + slot * SLOTB;
#pragma unroll 2
    for (int s = 0; s < 8; ++s) {
      V xf[8];
      if constexpr (BF) {
        // 8 bf16 columns per 16-byte piece: the low halves on even s, the high halves on odd s
        const int po = ((s >> 1) ^ x7) * 16 + (s & 1) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const uint2 u = *reinterpret_cast<const uint2*>(sb + brow + i * 16 * XROWB + po);
          xf[i][0] = __builtin_bit_cast(float, u.x << 16);
          xf[i][1] = __builtin_bit_cast(float, u.x & 0xffff0000u);
          xf[i][2] = __builtin_bit_cast(float, u.y << 16);
          xf[i][3] = __builtin_bit_cast(float, u.y & 0xffff0000u);
        }
      } else {
        const int po = (s ^ x7) * 16;
#pragma unroll
        for (int i = 0; i < 8; ++i) xf[i] = *reinterpret_cast<const V*>(sb + brow + i * 16 * XROWB + po);
      }
      const int pc = (s ^ c7) * 16;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const V cf = *reinterpret_cast<const V*>(sb + arow + j * 16 * KL_CROWB + pc);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if constexpr (CES == 4) {
            // two packed differences, then four adds with |·| on the source, K ascending
            const f32x2_t lo = kl_pk_sub(xf[i].lo, cf.lo), hi = kl_pk_sub(xf[i].hi, cf.hi);
            acc[i][j] += __builtin_fabsf(lo.x);
            acc[i][j] += __builtin_fabsf(lo.y);
            acc[i][j] += __builtin_fabsf(hi.x);
            acc[i][j] += __builtin_fabsf(hi.y);
          } else {
            acc[i][j] += __builtin_fabs(xf[i].x - cf.x);
            acc[i][j] += __builtin_fabs(xf[i].y - cf.y);
          }
        }
      }
    }
    if (++kc < NC) continue;

    // ---- the macro-tile's keys, j ascending under strict '<': the lowest index of equal keys
    // stays, a NaN or inf key and a clamped centroid never win
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = p * MT + tc + 16 * j;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool lt = acc[i][j] < bk[i] && c < k;
        bk[i] = lt ? acc[i][j] : bk[i];
        bi[i] = lt ? c : bi[i];
        acc[i][j] = 0;
      }
    }
    kc = 0;
    ++p;
  }

  // ---- the 16 threads of a row meet through LDS under (key, index) order: no fill is in flight,
  // and after the barrier no wave reads the ring any more
  TAcc* ck = reinterpret_cast<TAcc*>(lds);                           // [128][17]
  int* ci = reinterpret_cast<int*>(lds + KL_ROWS * 17 * CES);        // [128][17]
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ck[(tr + 16 * i) * 17 + tc] = bk[i];
    ci[(tr + 16 * i) * 17 + tc] = bi[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < KL_ROWS) {
    const int r = threadIdx.x;
    TAcc key = ck[r * 17];
    int idx = ci[r * 17];
#pragma unroll
    for (int t = 1; t < 16; ++t) {
      const TAcc ok = ck[r * 17 + t];
      const int oi = ci[r * 17 + t];
      // a thread without a winner holds (+inf, −1): never below a real candidate (key < +inf)
      const bool lo = oi >= 0 && (idx < 0 || ok < key || (ok == key && oi < idx));
      key = lo ? ok : key;
      idx = lo ? oi : idx;
    }
    if (row0 + r < n) labels[row0 + r] = idx;
  }
}

template <typename TIn, typename TAcc>
int kl_assign(const TIn* X, long ld, long n, int D, const TAcc* C, long ldc, int k, int* labels, void* stream) {
  constexpr int XPP = 16 / (int)sizeof(TIn), CPP = 16 / (int)sizeof(TAcc);  // elements per 16-byte piece
  constexpr long LDMAX = 1L << (sizeof(TAcc) == 8 ? 22 : 23);               // 32-bit byte offsets inside a tile
  if (D < XPP || D > 4096 || (D % XPP) != 0 || ld < D || ldc < D || (ld % XPP) != 0 || (ldc % CPP) != 0 ||
      ld >= LDMAX || ldc >= LDMAX || ((uintptr_t)X % 16) != 0 || ((uintptr_t)C % 16) != 0 || X == nullptr ||
      C == nullptr || labels == nullptr || k < 1 || k > INT32_MAX - 128)
    return -2;
  if (n <= 0) return 0;
  const long blocks = (n + KL_ROWS - 1) / KL_ROWS;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL((kmeans_assign_l1_kernel<TIn, TAcc>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X,
                     ld, n, D, C, ldc, k, labels);
  FMLX_CHECK_LAUNCH();
}

}  // namespace

// The tiled manhattan assign: X [n, D] (pitch ld) and the centroids C [k, D] (pitch ldc) row-major.
// Label = the lowest index among the minimal keys Σ|x_j − c_j| (fp32 sums, K ascending); a NaN or inf
// key never wins; −1 for a row without a key below +inf. One launch, no workspace. −2 unless
// 4 <= D <= 4096, D % 4 == 0, the pitches are multiples of 4 floats below 2^23 (32-bit byte offsets
// inside a tile), X and C are 16-byte aligned and 1 <= k.
FMLX_API int fmlx_kmeans_assign_l1_f32(const float* X, long ld, long n, int D, const float* C, long ldc, int k,
                                       int* labels, void* stream) {
  return kl_assign<float, float>(X, ld, n, D, C, ldc, k, labels, stream);
}

// bf16 rows read as stored (widened exactly in registers) against the fp32 centroid matrix: D and
// ld multiples of 8, 8 <= D <= 4096; otherwise as fmlx_kmeans_assign_l1_f32.
FMLX_API int fmlx_kmeans_assign_l1_bf16(const void* X, long ld, long n, int D, const float* C, long ldc, int k,
                                        int* labels, void* stream) {
  return kl_assign<bf16_t, float>((const bf16_t*)X, ld, n, D, C, ldc, k, labels, stream);
}

// fp64 rows and centroids, fp64 sums: D and the pitches even, 2 <= D <= 4096, pitches below 2^22.
FMLX_API int fmlx_kmeans_assign_l1_f64(const double* X, long ld, long n, int D, const double* C, long ldc, int k,
                                       int* labels, void* stream) {
  return kl_assign<double, double>(X, ld, n, D, C, ldc, k, labels, stream);
}

FMLX_DEFINE_PRELOAD()
