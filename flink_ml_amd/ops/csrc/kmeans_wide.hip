// KMeans for dense bf16 rows of 256 < D <= 4096 (euclidean; cosine from D = 64): the K-tiled MFMA
// assign and the update's wide gather-sum. kmeans.hip's MFMA assign keeps a wave's whole rows in
// registers and stops at D = 256; here nothing row-sized stays in registers.
//
// kmeans_assign_bf16_wide_kernel<COSINE> (the euclidean instantiation first)
//  * A block of 256 threads owns 128 rows for the whole kernel, walks the centroids in passes of
//    128 and K in chunks of 64 (4 steps of v_mfma_f32_32x32x16_bf16). The waves sit 2 x 2, each
//    with 64 rows x 64 centroids of the pass as 2 x 2 accumulator tiles (64 fp32 registers); per
//    k-step a lane reads two A and two B fragments (ds_read_b128) for four MFMAs.
//  * Both operands of a chunk — 128 rows x 64 bf16 of X and of the Cb image (−2·c, 16 KiB each) —
//    go from global memory straight into LDS by LDS-DMA. The image is unpadded: the 16-byte piece
//    s of tile row r sits at slot s ^ (r mod 8), applied by the choice of the global piece a lane
//    fetches, so the fragment reads are bank-conflict free.
//  * Ring of TWO 32-KiB slots: chunk i + 1 is filled under chunk i's MFMAs, one barrier per chunk.
//    Two slots (64 KiB) let two blocks share a CU, so one block's fill wait and epilogue run under
//    the other's MFMAs, and they keep every LDS-DMA destination (M0) below 64 KiB; a third slot
//    (96 KiB) would leave one block per CU.
//  * Once per pass: key = acc + ‖c_bf16‖² in plain fp32 (‖x‖² does not move the argmin), a running
//    (key, centroid) per row register under strict '<' (passes and tiles ascend, so a lane keeps
//    the lowest index of equal keys; NaN never wins). After the last pass the 64 candidates of a
//    row (32 lanes x 2 waves) meet in LDS and reduce under (key, index) order: the lowest index of
//    equal keys wins wherever it came from; a row without a finite key gets label 0.
//  * Tails: rows >= n and centroids >= kpad are clamped for the loads (not stored / +inf norm);
//    the pieces of the last chunk past D are fetched from the chunk's first piece instead and
//    zeroed in LDS by the lane that fetched them, in both operands, so they add exactly 0.
//  * The K order within a (row, centroid) is fixed: labels do not depend on the grid.
//  * COSINE: the same walk with key = acc / ‖c_bf16‖, i.e. −2·x·c/‖c‖. The pass's cn registers hold
//    the scale 1/sqrt(‖c_bf16‖²), NaN for the padding (+inf), a zero and a NaN centroid, so none of
//    them wins; the running index starts at −1. ‖x‖² of a row is summed once, during the first
//    pass, from the A fragments (v_dot2_f32_bf16): the wn = 0 / 1 wave of a row pair takes A tile
//    0 / 1, the two K halves meet by one exchange. The positive factor 1/‖x‖ does not move the
//    argmin; it multiplies the winning key after the reduction, where 0·inf (a zero row) and inf·0
//    (an inf element) are NaN like the key of a row with a NaN element: label −1, the generic
//    kernels' result. The chunk walk wraps at one chunk per pass (D = 64).
//
// kmeans_chunk_sum_bf16w_kernel (any metric): kmeans_chunk_sum_bf16v_kernel's contract for any
// D % 8 == 0 up to 4096 — a lane holds the 16-byte pieces lane, lane + 64, … of a row (PPL of them, a compile-time
// rung), a wave sums its stripe of the chunk's rows in row order with U rows' loads in flight, and
// the four waves' sums are added in wave order.
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int KW_ROWS = 128;             // rows per block = centroids per pass
constexpr int KW_KC = 64;                // bf16 values per K-chunk
constexpr int KW_ROWB = KW_KC * 2;       // bytes per tile row
constexpr int KW_TILEB = KW_ROWS * KW_ROWB;
constexpr int KW_SLOTB = 2 * KW_TILEB;   // the X tile, then the Cb tile
constexpr int KW_NS = 2;
constexpr int KW_PW = KW_TILEB / 1024 / 4;  // 1-KiB LDS-DMA pieces per wave and operand
constexpr int KW_CH = 256;               // rows per gather chunk (ops/kmeans.py CHUNK)

// Cb / cnorm are not __restrict__: the asm fills fence the norm loads where they are issued
template <bool COSINE>
__global__ __launch_bounds__(256, 2) void kmeans_assign_bf16_wide_kernel(const bf16_t* X, long ld, long n, int D,
                                                                         const bf16_t* Cb, int DP, const float* cnorm,
                                                                         int kpad, int* __restrict__ labels) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  __shared__ __align__(16) unsigned char lds[KW_NS * KW_SLOTB];
  static_assert(KW_NS * KW_SLOTB >= KW_ROWS * 64 * 8, "the label reduction reuses the ring");

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r32 = lane & 31;
  const int h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const long row0 = (long)blockIdx.x * KW_ROWS;
  const int NC = (D + KW_KC - 1) / KW_KC;
  const int NP = (kpad + KW_ROWS - 1) / KW_ROWS;
  const int T = NC * NP;

  // fill geometry: piece q = wave + 4i of a tile covers tile rows 8q … 8q + 7; lane l lands at
  // (row 8q + l/8, slot l%8) and fetches global piece g = slot ^ (row mod 8)
  const int g = (lane & 7) ^ (lane >> 3);
  const bool tail_ok = (NC - 1) * KW_KC + g * 8 < D;  // this lane's piece of the last chunk is inside the row
  unsigned a_off[KW_PW];                              // byte offset of the lane's row from the block's first row
#pragma unroll
  for (int i = 0; i < KW_PW; ++i) {
    long r = row0 + 8 * (wave + 4 * i) + (lane >> 3);
    r = r < n ? r : n - 1;
    a_off[i] = (unsigned)((r - row0) * ld * 2);
  }
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const char* xblk = reinterpret_cast<const char*>(X) + row0 * ld * 2;  // uniform

  // chunk (P_, KC_) → ring slot S_. Issued by inline asm with the ordering explicit (vmcnt + one
  // barrier per chunk), as in kmeans.hip's pipelined assign; every wave issues the same 2·KW_PW
  // loads per chunk. M0: written only by these statements in this kernel.
#define KW_FILL(P_, KC_, S_)                                                                              \
  {                                                                                                       \
    const unsigned gb_ = ((KC_) == NC - 1 && !tail_ok) ? 0u : (unsigned)(g * 16);                         \
    const char* asrc_ = xblk + (long)(KC_) * KW_ROWB;                                                     \
    const char* bsrc_ = reinterpret_cast<const char*>(Cb) + ((long)(P_) * KW_ROWS * DP + (long)(KC_) * KW_KC) * 2; \
    const int cmax_ = kpad - 1 - (P_) * KW_ROWS;                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < KW_PW; ++i_) {                                                \
      const unsigned d_ = dst0 + (unsigned)((S_) * KW_SLOTB + i_ * 4096);                                 \
      const unsigned ao_ = a_off[i_] + gb_;                                                               \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(ao_), "s"(asrc_), "s"(d_) \
                   : "memory", "m0");                                                                     \
      int c_ = 8 * (wave + 4 * i_) + (lane >> 3);                                                         \
      c_ = c_ < cmax_ ? c_ : cmax_;                                                                       \
      const unsigned bo_ = (unsigned)(c_ * DP * 2) + gb_;                                                 \
      const unsigned e_ = d_ + KW_TILEB;                                                                  \
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(bo_), "s"(bsrc_), "s"(e_) \
                   : "memory", "m0");                                                                     \
    }                                                                                                     \
  }

  KW_FILL(0, 0, 0)

  float best[2][16];
  int bidx[2][16];
  f32x16_t acc[2][2];
  const f32x16_t zero16 = {};
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      best[m][r] = __builtin_inff();
      bidx[m][r] = COSINE ? -1 : 0;
    }
    acc[m][0] = zero16;
    acc[m][1] = zero16;
  }
  // fragment addresses inside a tile: row (64·w + 32·t + r32), piece (2s + h) ^ (r32 mod 8)
  const int x7 = r32 & 7;
  const int arow = (64 * wm + r32) * KW_ROWB;
  const int brow = KW_TILEB + (64 * wn + r32) * KW_ROWB;

  int p = 0, kc = 0;      // the chunk being multiplied
  int fp = 0, fkc = 1;    // the next chunk to fill
  if (fkc == NC) { fkc = 0; fp = 1; }
  float cn[2] = {0.f, 0.f};
  // cosine: this lane's share (K half h) of ‖x‖² of row 64·wm + 32·wn + r32 = 32·wave + r32, from
  // the A fragments of the first pass; the wn = 0 / 1 waves of a row pair take A tile 0 / 1
  float xs = 0.f;
  for (int i = 0; i < T; ++i) {
    const int slot = i & 1;
    // this wave's share of chunk i has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (kc == NC - 1 && !tail_ok) {
#pragma unroll
      for (int q = 0; q < KW_PW; ++q) {
        unsigned char* z = lds + slot * KW_SLOTB + (wave + 4 * q) * 1024 + lane * 16;
        *reinterpret_cast<uint4*>(z) = make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(z + KW_TILEB) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    // … and every wave's; every wave is past chunk i − 1, whose slot the next fill takes
    __syncthreads();
    // the pass's norms, issued before the fill: the compiler's own wait in front of them (the
    // registers' previous loads) then finds nothing in flight
    if (kc == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int c = p * KW_ROWS + 64 * wn + 32 * t + r32;
        cn[t] = c < kpad ? cnorm[c] : __builtin_inff();
        // cosine: the scale 1/‖c_bf16‖; NaN for the padding (+inf), a zero and a NaN centroid
        if constexpr (COSINE) cn[t] = (cn[t] > 0.f && cn[t] < __builtin_inff()) ? 1.0f / sqrtf(cn[t]) : __builtin_nanf("");
      }
    }
    if (i + 1 < T) {
      KW_FILL(fp, fkc, slot ^ 1)
      if (++fkc == NC) { fkc = 0; ++fp; }
    }
    const unsigned char* sb = lds + slot * KW_SLOTB;
#pragma unroll
    for (int s = 0; s < KW_KC / 16; ++s) {
      const int po = ((2 * s + h) ^ x7) * 16;
      bf16x8_t a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = *reinterpret_cast<const bf16x8_t*>(sb + arow + t * 32 * KW_ROWB + po);
        b[t] = *reinterpret_cast<const bf16x8_t*>(sb + brow + t * 32 * KW_ROWB + po);
      }
      if constexpr (COSINE) {
        if (p == 0) {
          const bf16x8_t aw = __builtin_amdgcn_readfirstlane(wn) ? a[1] : a[0];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bf16x2_t a2 = {aw[2 * e], aw[2 * e + 1]};
            xs = __builtin_amdgcn_fdot2_f32_bf16(a2, a2, xs, false);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[t], acc[m][t], 0, 0, 0);
    }
    if (++kc == NC) {
      // the pass's keys: tile 0 before tile 1, passes ascending, strict '<'
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int c = p * KW_ROWS + 64 * wn + 32 * t + r32;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float key = COSINE ? acc[m][t][r] * cn[t] : acc[m][t][r] + cn[t];
            const bool lt = key < best[m][r];
            best[m][r] = lt ? key : best[m][r];
            bidx[m][r] = lt ? c : bidx[m][r];
          }
          acc[m][t] = zero16;
        }
      }
      kc = 0;
      ++p;
    }
  }
#undef KW_FILL

  // candidates of row ρ: word pair (ρ·64 + (32·wn + r32) ^ (ρ mod 32)); accumulator register r of
  // half h is row (r&3) + 8(r>>2) + 4h of its tile. Then two threads per row, 32 candidates each.
  __syncthreads();
  uint2* red = reinterpret_cast<uint2*>(lds);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rho = 64 * wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      red[rho * 64 + ((32 * wn + r32) ^ (rho & 31))] = make_uint2(__float_as_uint(best[m][r]), (unsigned)bidx[m][r]);
    }
  __syncthreads();
  const int rho = threadIdx.x >> 1, half = threadIdx.x & 1;
  float bk = __builtin_inff();
  int bi = 0x7fffffff;
#pragma unroll 8
  for (int j = 0; j < 32; ++j) {
    const uint2 v = red[rho * 64 + ((32 * half + j) ^ (rho & 31))];
    const float k = __uint_as_float(v.x);
    const int c = (int)v.y;
    const bool lt = k < bk || (k == bk && c < bi);
    bk = lt ? k : bk;
    bi = lt ? c : bi;
  }
  const float ok = __shfl_xor(bk, 1, 64);
  const int oi = __shfl_xor(bi, 1, 64);
  if constexpr (COSINE) {
    const bool lo = ok < bk || (ok == bk && oi < bi);
    // row ρ = 32·wave + lane/2 has its ‖x‖² in lanes ρ mod 32 and ρ mod 32 + 32 of this wave. The
    // positive factor 1/‖x‖ was left out of the running keys (it does not move the argmin); here it
    // makes the key of a zero row (0·inf) and of a row with an inf element (inf·0) NaN: label −1
    const float x2 = xs + __shfl_xor(xs, 32, 64);
    const float kx = (lo ? ok : bk) * (1.0f / sqrtf(__shfl(x2, lane >> 1, 64)));
    bi = kx == kx ? (lo ? oi : bi) : -1;
  } else {
    const bool lo = ok < bk || (ok == bk && oi < bi);
    // ‖x‖² is not in the key: a −inf key (x·c = +inf) means an infinite element in the row, whose
    // distances are all inf or NaN — no winner, label 0
    bi = (lo ? ok : bk) == -__builtin_inff() ? 0 : (lo ? oi : bi);
  }
  if (half == 0 && row0 + rho < n) labels[row0 + rho] = bi;
}

// ------------------------------------------------------------------------------------------
// the update's gather-sum for wide bf16 rows
// ------------------------------------------------------------------------------------------
template <int PPL>
__global__ __launch_bounds__(256) void kmeans_chunk_sum_bf16w_kernel(const bf16_t* __restrict__ X, long ld, int D,
                                                                     const int* __restrict__ order,
                                                                     const long* __restrict__ offsets,
                                                                     const long* __restrict__ chunk_off, int k,
                                                                     float* __restrict__ partial) {
  constexpr int U = PPL >= 4 ? 2 : 4;  // rows in flight per wave: at least 4 independent loads per lane
  const long b = blockIdx.x;
  if (b >= chunk_off[k]) return;
  int lo = 0, hi = k;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= b) lo = mid; else hi = mid;
  }
  const int j = lo;
  const long p0 = offsets[j] + (b - chunk_off[j]) * KW_CH;
  long p1 = p0 + KW_CH;
  if (p1 > offsets[j + 1]) p1 = offsets[j + 1];
  const int nrow = (int)(p1 - p0);
  __shared__ int rows_s[KW_CH];
  __shared__ __align__(16) float sm[3][PPL * 512];  // the sums of waves 1..3
  if ((int)threadIdx.x < nrow) rows_s[threadIdx.x] = order[p0 + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int np = D / 8;  // 16-byte pieces per row
  float acc[PPL][8];
#pragma unroll
  for (int v = 0; v < PPL; ++v)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[v][e] = 0.f;
  for (int q0 = wave; q0 < nrow; q0 += 4 * U) {
    uint4 x[U][PPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 4 * u;
      const bf16_t* xr = X + (long)rows_s[q < nrow ? q : 0] * ld;  // unconditional (row 0 of the chunk), masked below
#pragma unroll
      for (int v = 0; v < PPL; ++v) {
        const int pc = lane + 64 * v;
        x[u][v] = pc < np ? *reinterpret_cast<const uint4*>(xr + pc * 8) : make_uint4(0u, 0u, 0u, 0u);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = q0 + 4 * u < nrow;
#pragma unroll
      for (int v = 0; v < PPL; ++v) {
        const unsigned int w4[4] = {x[u][v].x, x[u][v].y, x[u][v].z, x[u][v].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[v][2 * e] += ok ? __uint_as_float(w4[e] << 16) : 0.f;
          acc[v][2 * e + 1] += ok ? __uint_as_float(w4[e] & 0xffff0000u) : 0.f;
        }
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < PPL; ++v) {
      float4* d = reinterpret_cast<float4*>(&sm[wave - 1][(lane + 64 * v) * 8]);
      d[0] = make_float4(acc[v][0], acc[v][1], acc[v][2], acc[v][3]);
      d[1] = make_float4(acc[v][4], acc[v][5], acc[v][6], acc[v][7]);
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int v = 0; v < PPL; ++v) {
      const int pc = lane + 64 * v;
      if (pc < np) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((acc[v][e] + sm[0][pc * 8 + e]) + sm[1][pc * 8 + e]) + sm[2][pc * 8 + e];
        float4* d = reinterpret_cast<float4*>(partial + b * D + pc * 8);  // D % 8 == 0, partial 16-byte aligned
        d[0] = make_float4(o[0], o[1], o[2], o[3]);
        d[1] = make_float4(o[4], o[5], o[6], o[7]);
      }
    }
  }
}

}  // namespace

// The K-tiled MFMA assign: Cb is [kpad][DP] (−2·c, zero from D to DP = 16·ceil(D/16)), cnorm ‖c_bf16‖²
// (+inf on the padding). −2 unless 256 < D <= 4096, D % 8 == 0, ld % 8 == 0, ld < 2^23 (32-bit
// byte offsets inside a block's 128 rows) and X is 16-byte aligned.
FMLX_API int fmlx_kmeans_assign_bf16_wide(const void* X, long ld, long n, int D, const void* Cb, int DP,
                                          const float* cnorm, int kpad, int* labels, void* stream) {
  if (D <= 256 || D > 4096 || (D % 8) != 0 || (ld % 8) != 0 || ld < D || ld >= (1L << 23) ||
      ((uintptr_t)X % 16) != 0 || ((uintptr_t)Cb % 16) != 0 || DP != (D + 15) / 16 * 16 || kpad < 1)
    return -2;
  if (n <= 0) return 0;
  const long blocks = (n + KW_ROWS - 1) / KW_ROWS;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(kmeans_assign_bf16_wide_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)X, ld, n, D, (const bf16_t*)Cb, DP, cnorm, kpad, labels);
  return (int)hipGetLastError();
}

// The cosine instantiation on the same operands: label = the lowest index among the minimal
// −x·c_bf16 / ‖x‖ / ‖c_bf16‖ (NaN never wins), −1 for a row without a winner (‖x‖ zero, inf or NaN; no
// centroid with a finite non-zero norm). Rows from D = 64: cosine has no narrow MFMA kernel, so the
// pitch DP of the image may be any multiple of 16 from D (ops/kmeans.py pads it for D <= 256); the
// image stays below 2^30 elements.
FMLX_API int fmlx_kmeans_assign_bf16_wide_cos(const void* X, long ld, long n, int D, const void* Cb, int DP,
                                              const float* cnorm, int kpad, int* labels, void* stream) {
  if (D < 64 || D > 4096 || (D % 8) != 0 || (ld % 8) != 0 || ld < D || ld >= (1L << 23) ||
      ((uintptr_t)X % 16) != 0 || ((uintptr_t)Cb % 16) != 0 || DP < D || (DP % 16) != 0 || kpad < 1 ||
      (long)kpad * DP >= (1L << 30))
    return -2;
  if (n <= 0) return 0;
  const long blocks = (n + KW_ROWS - 1) / KW_ROWS;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(kmeans_assign_bf16_wide_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)X, ld, n, D, (const bf16_t*)Cb, DP, cnorm, kpad, labels);
  return (int)hipGetLastError();
}

// fmlx_kmeans_chunk_sum_bf16v's contract (int32 row order, partial[max_chunks][D] fp32) for any
// D % 8 == 0 up to 4096. −2 for other shapes or rows that are not 16-byte aligned.
FMLX_API int fmlx_kmeans_chunk_sum_bf16w(const void* X, long ld, int D, const int* order, const long* offsets,
                                         const long* chunk_off, int k, long max_chunks, float* partial,
                                         void* stream) {
  if (max_chunks <= 0) return 0;
  if (D < 8 || D > 4096 || (D % 8) != 0 || (ld % 8) != 0 || ((uintptr_t)X % 16) != 0 || ((uintptr_t)partial % 16) != 0)
    return -2;
  return with_ceil<1, 2, 4, 8>(fmlx_ceil_div(D, 512), [&](auto ppl) {
    hipLaunchKernelGGL(kmeans_chunk_sum_bf16w_kernel<ppl.value>, dim3((unsigned)max_chunks), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)X, ld, D, order, offsets, chunk_off, k, partial);
    return (int)hipGetLastError();
  }, -2);
}

FMLX_DEFINE_PRELOAD()
