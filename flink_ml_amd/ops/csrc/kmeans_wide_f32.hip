// KMeans for dense fp32 rows of 128 < D <= 4096 (euclidean and cosine): the K-tiled fp32 MFMA assign
// and the update's wide gather-sum (any metric). The fp32 routes before it are the fused KNN
// kernel with k = 1 (whole rows in registers, D <= 128), a library GEMM + argmin block (k <= 64, many rows) and the
// wave-per-row / thread-per-row kernels of kmeans.hip; kmeans_wide.hip is the bf16 counterpart.
//
// kmeans_assign_f32_wide_kernel: knn_wide.hip's tile geometry with an argmin instead of lists.
//  * A block of 256 threads owns 128 rows of X for the whole kernel: 4 waves × 32 rows, a row per
//    lane column, the two half-waves h splitting the K index (v_mfma_f32_32x32x2_f32, the centroid
//    tile as A and the rows as B). It walks the centroids in macro-tiles of 128 (64 accumulator
//    registers, four 32 × 32 subtiles) and K in chunks of 32 fp32 columns. Without list registers
//    the kernel fits two blocks per CU (profiles/r22/resources_kmeans_wide_f32.txt), so one
//    block's fill wait and epilogue run under the other's MFMAs.
//  * Both operands of a chunk go as they are stored, from the row-major centroid matrix and the
//    row-major X view (pointer, pitch) straight into LDS by LDS-DMA (128 × 32 floats each). A tile
//    row is 128 bytes: its 16-byte piece s sits at slot s ^ (r mod 8), applied by the choice of the
//    global piece a lane fetches, so the b128 fragment reads are bank-conflict free without
//    padding. k-step (g, e) of half h is column 8g + 4h + e of the chunk in A and B alike.
//  * B fragments are read from LDS into registers once per chunk and reused by the four subtiles;
//    the X tile is re-read from L2 once per macro-tile.
//  * Ring of two 32-KiB slots (centroid tile, then X tile): chunk i + 1 fills under chunk i's
//    MFMAs; per chunk one s_waitcnt vmcnt(0) (this wave's share has landed) and one barrier
//    (everyone's has, and everyone is past chunk i − 1, whose slot the next fill takes). The ring
//    starts at LDS offset 0, so every LDS-DMA destination stays below 64 KiB.
//  * ‖c‖² of a macro-tile's centroids comes through LDS as well (a plain load issued with the fill
//    of the tile's first chunk, stored to LDS after the next vmcnt(0), published by the same
//    barrier): accumulators start at −‖c‖²/2, so key = ‖c‖² − 2·x·c is one multiply per element
//    after the last chunk (‖x‖² does not move the argmin and is not computed). The norms are
//    written by kmeans_cnorm2_f32_kernel in front of every assign (a wave per centroid, fixed
//    order), because kmeans_finalize_kernel rewrites the centroids on the device every round.
//  * A running (key, centroid) pair per lane under strict '<': macro-tiles, subtiles and
//    accumulator registers ascend in centroid index, so a lane keeps the lowest index of equal
//    keys; a NaN key never wins. After the last macro-tile the two half-waves' candidates of a row
//    meet by one cross-lane exchange under (key, index) order; a row without a finite key gets
//    label 0. Lanes 0–31 of each wave store 32 consecutive labels. No workspace, one launch.
//  * Tails: rows >= n and centroids >= k are clamped for the loads (never stored / never chosen);
//    the pieces of the last chunk past D are fetched from the chunk's first piece instead and
//    zeroed in LDS by the lane that fetched them, in both operands: they add exactly 0.
//  * The K order within a (row, centroid) is fixed: labels do not depend on the grid.
//  * COSINE (kmeans_assign_f32_wide_kernel<true>): accumulators start at 0 and key = −x·c / ‖c‖.
//    The LDS table holds the scale 1/sqrt(‖c‖²) (NaN for a zero and a NaN centroid: never wins) and
//    is read by the epilogue, so it is published with the tile's second chunk, when every wave has
//    left the previous tile's epilogue. ‖x‖² is summed from the B fragments during the first
//    macro-tile; the two half-waves' shares meet with the candidates. 1/‖x‖ multiplies the winning
//    key at the end (0·inf, inf·0 → NaN): a zero row and a row with an inf or NaN element get −1,
//    the generic kernels' result; the running index starts at −1.
//
// kmeans_chunk_sum_f32w_kernel<PPL>: kmeans_chunk_sum_bf16w_kernel's contract for fp32 rows of any
// D % 4 == 0 up to 4096 — int32 row order, a lane holds the 16-byte pieces lane, lane + 64, … of a
// row (PPL of them, a compile-time rung up to 16), a wave sums its stripe of the chunk's rows in
// row order with U rows' loads in flight, and the four waves' sums are added in wave order.
#include "common.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int KF_ROWS = 128;             // rows per block
constexpr int KF_MT = 128;               // centroids per macro-tile
constexpr int KF_NSUB = KF_MT / 32;      // 32-centroid MFMA subtiles = 1-KiB fill pieces per wave
constexpr int KF_KC = 32;                // fp32 columns per K-chunk
constexpr int KF_ROWB = KF_KC * 4;       // bytes per tile row
constexpr int KF_TILEA = KF_MT * KF_ROWB;
constexpr int KF_TILEB = KF_ROWS * KF_ROWB;
constexpr int KF_SLOTB = KF_TILEA + KF_TILEB;  // the centroid tile, then the X tile
constexpr int KF_CH = 256;               // rows per gather chunk (ops/kmeans.py CHUNK)

// ‖c‖² of every centroid: a wave per centroid, lane l sums the pieces l, l + 64, … in order, then
// a fixed butterfly
__global__ __launch_bounds__(256) void kmeans_cnorm2_f32_kernel(const float* __restrict__ C, long ldc, int D, int k,
                                                                float* __restrict__ cn2) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= k) return;
  const float4* row = reinterpret_cast<const float4*>(C + c * ldc);
  float s = 0.f;
  for (int p = lane; p < D / 4; p += 64) {
    const float4 v = row[p];
    s = __builtin_fmaf(v.x, v.x, s);
    s = __builtin_fmaf(v.y, v.y, s);
    s = __builtin_fmaf(v.z, v.z, s);
    s = __builtin_fmaf(v.w, v.w, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) cn2[c] = s;
}

// X / C / cn2 are not __restrict__: the asm fills read them behind the compiler's back
template <bool COSINE>
__global__ __launch_bounds__(256, 2) void kmeans_assign_f32_wide_kernel(const float* X, long ld, long n, int D,
                                                                        const float* C, long ldc, const float* cn2,
                                                                        int k, int* __restrict__ labels) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  __shared__ __align__(16) unsigned char lds[2 * KF_SLOTB + KF_MT * 4];  // the ring, then the tile's norms
  float* cnl = reinterpret_cast<float*>(lds + 2 * KF_SLOTB);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r32 = lane & 31;
  const int h = lane >> 5;
  const long row0 = (long)blockIdx.x * KF_ROWS;
  const long xrow = row0 + wave * 32 + r32;
  const int NC = (D + KF_KC - 1) / KF_KC;
  const int ntiles = (k + KF_MT - 1) / KF_MT;
  const long iters = (long)ntiles * NC;

  // fill geometry: piece q = wave + 4i of a tile covers tile rows 8q … 8q + 7; lane l lands at
  // (row 8q + l/8, slot l%8) and fetches global piece g = slot ^ (row mod 8)
  const int g = (lane & 7) ^ (lane >> 3);
  const bool tail_ok = (NC - 1) * KF_KC + g * 4 < D;  // this lane's piece of the last chunk is inside the row
  unsigned x_off[4];                                  // byte offset of the lane's X rows from the block's first
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long r = row0 + 8 * (wave + 4 * i) + (lane >> 3);
    r = r < n ? r : n - 1;
    x_off[i] = (unsigned)((r - row0) * ld * 4);
  }
  const unsigned ldcb = (unsigned)(ldc * 4);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* xblk = reinterpret_cast<const char*>(X) + row0 * ld * 4;  // uniform

  // chunk (macro-tile P_, chunk KC_) → ring slot S_. Issued by inline asm with the ordering
  // explicit (vmcnt + one barrier per chunk), as in knn_wide.hip; every wave issues the same
  // KF_NSUB + 4 loads per chunk. M0: written only by these statements in this kernel.
#define KF_FILL(P_, KC_, S_)                                                                              \
  {                                                                                                       \
    const unsigned gb_ = ((KC_) == NC - 1 && !tail_ok) ? 0u : (unsigned)(g * 16);                         \
    const char* asrc_ = reinterpret_cast<const char*>(C) + ((long)(P_) * KF_MT * ldc + (long)(KC_) * KF_KC) * 4; \
    const char* bsrc_ = xblk + (long)(KC_) * KF_ROWB;                                                     \
    const int cmax_ = k - 1 - (P_) * KF_MT;                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < KF_NSUB; ++i_) {                                              \
      const unsigned d_ = dst0 + (unsigned)((S_) * KF_SLOTB + i_ * 4096);                                 \
      int c_ = 8 * (wave + 4 * i_) + (lane >> 3);                                                         \
      c_ = c_ < cmax_ ? c_ : cmax_;                                                                       \
      const unsigned ao_ = (unsigned)c_ * ldcb + gb_;                                                     \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(ao_), "s"(asrc_), "s"(d_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                    \
      const unsigned e_ = dst0 + (unsigned)((S_) * KF_SLOTB + KF_TILEA + i_ * 4096);                      \
      const unsigned bo_ = x_off[i_] + gb_;                                                               \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(bo_), "s"(bsrc_), "s"(e_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
  }
  // ‖c‖² of centroid threadIdx.x of macro-tile P_ (clamped like the rows)
#define KF_NORM(P_) cn2[((P_) * KF_MT + (int)threadIdx.x) < k ? ((P_) * KF_MT + (int)threadIdx.x) : k - 1]

  float bk = __builtin_inff();  // this lane's best key of its row, over the centroids of its half
  int bi = COSINE ? -1 : 0;
  float xs = 0.f;  // cosine: this lane's share (the K indices of half h) of its row's ‖x‖²

  float cv = 0.f;  // the next macro-tile's norm of this thread's centroid, on its way to LDS
  if ((int)threadIdx.x < KF_MT) cv = KF_NORM(0);
  KF_FILL(0, 0, 0)

  f32x16_t acc[KF_NSUB];
  // fragment addresses inside a slot: row (32·t + r32), piece (2g + h) ^ (r32 mod 8)
  const int x7 = r32 & 7;
  const int arow = r32 * KF_ROWB;
  const int brow = KF_TILEA + (32 * wave + r32) * KF_ROWB;

  int p = 0, kc = 0;     // the chunk being multiplied
  int fp = 0, fkc = 1;   // the next chunk to fill (NC >= 5: no wrap here)
  for (long i = 0; i < iters; ++i) {
    const int slot = (int)(i & 1);
    // this wave's share of chunk i has landed (and cv)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1 && !tail_ok) {
#pragma unroll
      for (int q = 0; q < KF_NSUB; ++q)
        *reinterpret_cast<uint4*>(lds + slot * KF_SLOTB + (wave + 4 * q) * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<uint4*>(lds + slot * KF_SLOTB + KF_TILEA + (wave + 4 * q) * 1024 + lane * 16) =
            make_uint4(0u, 0u, 0u, 0u);
    }
    if constexpr (COSINE) {
      // the table holds the scale 1/‖c‖ (NaN for a zero and a NaN centroid) and is read by the
      // epilogue after the tile's last chunk: it is published one barrier later, with chunk 1
      // (NC >= 5), when every wave has left the previous tile's epilogue
      if (kc == 1 && (int)threadIdx.x < KF_MT)
        cnl[threadIdx.x] = (cv > 0.f && cv < __builtin_inff()) ? 1.0f / sqrtf(cv) : __builtin_nanf("");
    } else {
      if (kc == 0 && (int)threadIdx.x < KF_MT) cnl[threadIdx.x] = cv;
    }
    // … and every wave's; every wave is past chunk i − 1, whose slot the next fill takes
    __syncthreads();
    if (i + 1 < iters) {
      KF_FILL(fp, fkc, slot ^ 1)
      if (fkc == 0 && (int)threadIdx.x < KF_MT) cv = KF_NORM(fp);
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    if (kc == 0) {
      // accumulator register r of half h is centroid (r&3) + 8(r>>2) + 4h of its subtile
#pragma unroll
      for (int t = 0; t < KF_NSUB; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          if constexpr (COSINE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][4 * g4 + e] = 0.f;
          } else {
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(cnl + 32 * t + 8 * g4 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][4 * g4 + e] = -0.5f * v[e];
          }
        }
    }
    const unsigned char* sb = lds + slot * KF_SLOTB;
#pragma unroll
    for (int g4 = 0; g4 < KF_KC / 8; ++g4) {
      const int po = ((2 * g4 + h) ^ x7) * 16;
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(sb + brow + po);
      f32x4_t a[KF_NSUB];
#pragma unroll
      for (int t = 0; t < KF_NSUB; ++t) a[t] = *reinterpret_cast<const f32x4_t*>(sb + arow + t * 32 * KF_ROWB + po);
      if constexpr (COSINE) {
        if (p == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) xs = __builtin_fmaf(b[e], b[e], xs);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < KF_NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][e], b[e], acc[t], 0, 0, 0);
    }
    if (++kc < NC) continue;

    // ---- the macro-tile's keys in ascending centroid order under strict '<': the lowest index of
    // equal keys stays, a NaN key and a clamped centroid never win
    const int cb = p * KF_MT + 4 * h;
    if constexpr (COSINE) {
      // key = −x·c / ‖c‖; the positive factor 1/‖x‖ does not move the argmin and waits for the end
#pragma unroll
      for (int t = 0; t < KF_NSUB; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(cnl + 32 * t + 8 * g4 + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = cb + 32 * t + 8 * g4 + e;
            const float key = -acc[t][4 * g4 + e] * v[e];
            const bool lt = key < bk && c < k;
            bk = lt ? key : bk;
            bi = lt ? c : bi;
          }
        }
    } else {
#pragma unroll
      for (int t = 0; t < KF_NSUB; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = cb + 32 * t + (r & 3) + 8 * (r >> 2);
          const float key = -2.0f * acc[t][r];
          const bool lt = key < bk && c < k;
          bk = lt ? key : bk;
          bi = lt ? c : bi;
        }
    }
    kc = 0;
    ++p;
  }
#undef KF_FILL
#undef KF_NORM

  // ---- the two half-lanes of a row meet under (key, index) order; lane h == 0 writes
  const float ok = __shfl_xor(bk, 32, 64);
  const int oi = __shfl_xor(bi, 32, 64);
  if constexpr (COSINE) {
    // 1/‖x‖ makes the key of a zero row (0·inf) and of a row with an inf element (inf·0) NaN, like
    // that of a row with a NaN element: no winner, label −1
    const bool lo = ok < bk || (ok == bk && oi < bi);
    const float x2 = xs + __shfl_xor(xs, 32, 64);
    const float kx = (lo ? ok : bk) * (1.0f / sqrtf(x2));
    bi = kx == kx ? (lo ? oi : bi) : -1;
  } else {
    const bool lo = ok < bk || (ok == bk && oi < bi);
    // ‖x‖² is not in the key: a −inf key (x·c = +inf) means an infinite element in the row, whose
    // distances are all inf or NaN — no winner, label 0
    bi = (lo ? ok : bk) == -__builtin_inff() ? 0 : (lo ? oi : bi);
  }
  if (h == 0 && xrow < n) labels[xrow] = bi;
}

// ------------------------------------------------------------------------------------------
// the update's gather-sum for wide fp32 rows
// ------------------------------------------------------------------------------------------
template <int PPL>
__global__ __launch_bounds__(256) void kmeans_chunk_sum_f32w_kernel(const float* __restrict__ X, long ld, int D,
                                                                    const int* __restrict__ order,
                                                                    const long* __restrict__ offsets,
                                                                    const long* __restrict__ chunk_off, int k,
                                                                    float* __restrict__ partial) {
  constexpr int U = PPL >= 16 ? 1 : PPL >= 4 ? 2 : 4;  // rows in flight per wave: at least 4 independent loads per lane
  const long b = blockIdx.x;
  if (b >= chunk_off[k]) return;
  int lo = 0, hi = k;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= b) lo = mid; else hi = mid;
  }
  const int j = lo;
  const long p0 = offsets[j] + (b - chunk_off[j]) * KF_CH;
  long p1 = p0 + KF_CH;
  if (p1 > offsets[j + 1]) p1 = offsets[j + 1];
  const int nrow = (int)(p1 - p0);
  __shared__ int rows_s[KF_CH];
  __shared__ __align__(16) float sm[3][PPL * 256];  // the sums of waves 1..3
  if ((int)threadIdx.x < nrow) rows_s[threadIdx.x] = order[p0 + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int np = D / 4;  // 16-byte pieces per row
  float4 acc[PPL];
#pragma unroll
  for (int v = 0; v < PPL; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q0 = wave; q0 < nrow; q0 += 4 * U) {
    float4 x[U][PPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 4 * u;
      const float* xr = X + (long)rows_s[q < nrow ? q : 0] * ld;  // unconditional (row 0 of the chunk), masked below
#pragma unroll
      for (int v = 0; v < PPL; ++v) {
        const int pc = lane + 64 * v;
        x[u][v] = pc < np ? *reinterpret_cast<const float4*>(xr + pc * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = q0 + 4 * u < nrow;
#pragma unroll
      for (int v = 0; v < PPL; ++v) {
        acc[v].x += ok ? x[u][v].x : 0.f;
        acc[v].y += ok ? x[u][v].y : 0.f;
        acc[v].z += ok ? x[u][v].z : 0.f;
        acc[v].w += ok ? x[u][v].w : 0.f;
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < PPL; ++v) *reinterpret_cast<float4*>(&sm[wave - 1][(lane + 64 * v) * 4]) = acc[v];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int v = 0; v < PPL; ++v) {
      const int pc = lane + 64 * v;
      if (pc < np) {
        const float4 s0 = *reinterpret_cast<const float4*>(&sm[0][pc * 4]);
        const float4 s1 = *reinterpret_cast<const float4*>(&sm[1][pc * 4]);
        const float4 s2 = *reinterpret_cast<const float4*>(&sm[2][pc * 4]);
        // D % 4 == 0, partial 16-byte aligned
        *reinterpret_cast<float4*>(partial + b * D + pc * 4) =
            make_float4(((acc[v].x + s0.x) + s1.x) + s2.x, ((acc[v].y + s0.y) + s1.y) + s2.y,
                        ((acc[v].z + s0.z) + s1.z) + s2.z, ((acc[v].w + s0.w) + s1.w) + s2.w);
      }
    }
  }
}

template <bool COSINE>
int kf_assign(const float* X, long ld, long n, int D, const float* C, long ldc, float* cn2, int k, int* labels,
              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (D <= 128 || D > 4096 || (D % 4) != 0 || ld < D || ldc < D || (ld % 4) != 0 || (ldc % 4) != 0 ||
      ld >= (1L << 23) || ldc >= (1L << 23) || ((uintptr_t)X % 16) != 0 || ((uintptr_t)C % 16) != 0 || k < 1 ||
      k > INT32_MAX - KF_MT || cn2 == nullptr)
    return -2;
  if (n <= 0) return 0;
  const long blocks = (n + KF_ROWS - 1) / KF_ROWS;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(kmeans_cnorm2_f32_kernel, dim3(fmlx_ceil_div(k, 4)), dim3(256), 0, s, C, ldc, D, k, cn2);
  hipLaunchKernelGGL(kmeans_assign_f32_wide_kernel<COSINE>, dim3((unsigned)blocks), dim3(256), 0, s, X, ld, n, D, C,
                     ldc, (const float*)cn2, k, labels);
  FMLX_CHECK_LAUNCH();
}

}  // namespace

// The K-tiled fp32 MFMA assign: X [n, D] (pitch ld) and the centroids C [k, D] (pitch ldc) fp32
// row-major; cn2 [k] receives ‖c‖² from a kernel launched in front of the assign on the same
// stream. Label = the lowest index among the minimal keys ‖c‖² − 2·x·c (NaN counts as +inf; 0 if no
// key is finite). −2 unless 128 < D <= 4096, D % 4 == 0, the pitches are multiples of 4 floats
// below 2^23 (32-bit byte offsets inside a tile), X and C are 16-byte aligned and 1 <= k.
FMLX_API int fmlx_kmeans_assign_f32_wide(const float* X, long ld, long n, int D, const float* C, long ldc, float* cn2,
                                         int k, int* labels, void* stream) {
  return kf_assign<false>(X, ld, n, D, C, ldc, cn2, k, labels, stream);
}

// The cosine instantiation, same operands and limits: label = the lowest index among the minimal
// −x·c / ‖x‖ / ‖c‖ with ‖c‖² from cn2 (NaN never wins), −1 for a row without a winner (‖x‖ zero, inf
// or NaN; no centroid with a finite non-zero norm).
FMLX_API int fmlx_kmeans_assign_f32_wide_cos(const float* X, long ld, long n, int D, const float* C, long ldc,
                                             float* cn2, int k, int* labels, void* stream) {
  return kf_assign<true>(X, ld, n, D, C, ldc, cn2, k, labels, stream);
}

// fmlx_kmeans_chunk_sum_bf16w's contract (int32 row order, partial[max_chunks][D] fp32) for fp32
// rows of any D % 4 == 0 up to 4096. −2 for other shapes or rows that are not 16-byte aligned.
FMLX_API int fmlx_kmeans_chunk_sum_f32w(const float* X, long ld, int D, const int* order, const long* offsets,
                                        const long* chunk_off, int k, long max_chunks, float* partial, void* stream) {
  if (max_chunks <= 0) return 0;
  if (D < 4 || D > 4096 || (D % 4) != 0 || (ld % 4) != 0 || ld < D || ((uintptr_t)X % 16) != 0 ||
      ((uintptr_t)partial % 16) != 0)
    return -2;
  return with_ceil<1, 2, 4, 8, 16>(fmlx_ceil_div(D, 256), [&](auto ppl) {
    hipLaunchKernelGGL(kmeans_chunk_sum_f32w_kernel<ppl.value>, dim3((unsigned)max_chunks), dim3(256), 0,
                       (hipStream_t)stream, X, ld, D, order, offsets, chunk_off, k, partial);
    return (int)hipGetLastError();
  }, -2);
}

FMLX_DEFINE_PRELOAD()
