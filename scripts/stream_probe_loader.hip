// Does a dedicated loader wave per block (LDS-DMA fills of a ring of slots, counted vmcnt, raw
// s_barrier hand-off to 8 consumer waves) stream the SGD round's rows faster than the round
// kernel's register loop (two steps of 2 rows per wave in flight)? A/B in one process, variants
// interleaved, hipEvent timing: 100k-row × 2000-B bf16 batches (200 MB) rotating through a 4 GB
// buffer; the row → (block, wave, order) mapping is the round kernel's (consumer wave q of block b
// owns rows b·8 + q + j·W, W = 8·grid). Variants:
//   reg     rows_reg<2, 8>: 16-byte non-temporal register loads, trivial consumer
//   ld …    loader/consumer block, trivial consumer (two ds_read_b128 per row, one add)
//   ldm …   the same with the round's math per row (bf16 unpack, packed-fp32 dot against 16
//           register coefficients per lane, DPP wave sum, exp/rcp, packed-fp32 axpy)
// knobs: R rows per slot (8 | 16), S slots, grid, fill form (row = two 1-KiB pieces per row at a
// 2-KiB pitch; grp = 16 contiguous 1-KiB pieces over the 16,000-byte 8-row group).
// One phase per slot: the loader issues slot k + S − 2 (into the slot read two phases ago), waits
// with a counted vmcnt until slot k has landed, then the block's barrier; the consumers read slot
// k after that barrier and retire their ds_reads (lgkmcnt(0)) before the next one. vmcnt counts at
// most 63 loads, so whatever S is, one loader wave keeps at most 63 KiB in flight: the wait is
// min(pieces·(S − 2), 63), and slots beyond that only hold landed rows.
// Prints µs per 200 MB batch and GB/s per variant and repetition, then min / median / max.
//   hipcc --offload-arch=gfx950 -O3 -o stream_probe_loader scripts/stream_probe_loader.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x4 lds_u4_t;

template <int CTRL, int ROW_MASK = 0xF, bool BOUND = true>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, BOUND));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  v += dpp_mov<0x142, 0xA, false>(v);
  v += dpp_mov<0x143, 0xC, false>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// register path: U rows per step, two steps in flight (the round kernel's shape)
template <int U, int WPB>
__global__ __launch_bounds__(WPB * 64) void rows_reg(const u32x4* __restrict__ x, long rows, float* out) {
  const int lane = threadIdx.x & 63;
  const long W = (long)gridDim.x * WPB;
  const long gw = (long)blockIdx.x * WPB + (threadIdx.x >> 6);
  const int c0 = lane, c1 = lane + 64 < 125 ? lane + 64 : 124;
  float s = 0.f;
  u32x4 a[U][2], b[U][2];
  auto load = [&](long r0, u32x4 (&d)[U][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      long r = r0 + u * W;
      r = r < rows ? r : rows - 1;
      d[u][0] = __builtin_nontemporal_load(x + r * 125 + c0);
      d[u][1] = __builtin_nontemporal_load(x + r * 125 + c1);
    }
  };
  auto use = [&](u32x4 (&d)[U][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) s += __uint_as_float(d[u][0].x) + __uint_as_float(d[u][1].w);
  };
  const long step = (long)U * W;
  long r = gw;
  load(r, a);
  while (true) {
    load(r + step, b);
    use(a);
    r += step;
    if (r >= rows) break;
    load(r + step, a);
    use(b);
    r += step;
    if (r >= rows) break;
  }
  if (s == 1234.5f) out[0] = s;
}

template <bool NT>
__device__ __forceinline__ void dma16(const void* g, unsigned lds) {
  unsigned keep;
  if constexpr (NT)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}

// loader/consumer block: waves 0–7 consume, wave 8 loads. R rows per slot (R / 8 steps of the
// block), S slots of R × 2 KiB. GRP: contiguous 8-row group fills (row pitch 2000 B in the slot).
template <int R, int S, bool GRP, bool MATH, bool NT>
__global__ __launch_bounds__(576) void rows_loader(const u32x4* __restrict__ x, long rows, float* out) {
  extern __shared__ __align__(16) unsigned char ring[];
  constexpr int U = R / 8;               // steps per slot = rows per consumer wave per slot
  constexpr int PIECES = 2 * R;          // 1-KiB DMA instructions per slot
  constexpr int SLOT = R * 2048;
  constexpr int NWAIT = PIECES * (S - 2) < 63 ? PIECES * (S - 2) : 63;
  static_assert(S >= 3 && S * SLOT <= 128 * 1024, "ring");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long W = (long)gridDim.x * 8;
  const long b0 = (long)blockIdx.x * 8;
  const long nj = b0 < rows ? (rows - b0 + W - 1) / W : 0;  // steps of this block
  const long nslots = (nj + U - 1) / U;
  const int c1 = lane + 64 < 125 ? lane + 64 : 124;
  const unsigned ring_a = __builtin_amdgcn_readfirstlane((unsigned)(size_t)ring);
  if (wave == 8) {
    auto issue = [&](long k) {
      const unsigned base = ring_a + (unsigned)(k % S) * SLOT;
#pragma unroll
      for (int g = 0; g < U; ++g) {
        long j = k * U + g;
        j = j < nj ? j : nj - 1;  // past the block's steps: a valid step again, masked by the readers
        const long r0 = b0 + j * W;
        if constexpr (GRP) {
          // the whole group lies inside the batch (rows and b0 are multiples of 8 here)
          const u32x4* p = x + r0 * 125;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int c = i * 64 + lane < 1000 ? i * 64 + lane : 999;
            dma16<NT>(p + c, base + g * 16384 + i * 1024);
          }
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            long r = r0 + u;
            r = r < rows ? r : rows - 1;
            dma16<NT>(x + r * 125 + lane, base + g * 16384 + u * 2048);
            dma16<NT>(x + r * 125 + c1, base + g * 16384 + u * 2048 + 1024);
          }
        }
      }
    };
#pragma unroll
    for (int k = 0; k < S - 2; ++k)
      if (k < nslots) issue(k);
    for (long k = 0; k < nslots; ++k) {
      if (k + S - 2 < nslots) {
        issue(k + S - 2);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");  // slot k landed
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
    return;
  }
  float s = 0.f;
  f2_t w2[2][4], acc2[2][4];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w2[k][i] = f2_t{0.001f * (lane + i), 0.002f * (k + 1)};
      acc2[k][i] = f2_t{0.f, 0.f};
    }
  const int pitch = GRP ? 2000 : 2048;
  for (long k = 0; k < nslots; ++k) {
    __builtin_amdgcn_s_barrier();
    const unsigned char* sl = ring + (k % S) * SLOT;
    u32x4 v[U][2];
#pragma unroll
    for (int g = 0; g < U; ++g) {
      const unsigned char* row = sl + g * 16384 + wave * pitch;
      v[g][0] = *(const lds_u4_t*)(row + lane * 16);
      v[g][1] = *(const lds_u4_t*)(row + c1 * 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot may be refilled after the next barrier
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!MATH) {
#pragma unroll
      for (int g = 0; g < U; ++g) s += __uint_as_float(v[g][0].x) + __uint_as_float(v[g][1].w);
    } else {
      f2_t xf[U][2][4];
      float dot[U];
#pragma unroll
      for (int g = 0; g < U; ++g) {
        f2_t s2[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const unsigned q[4] = {v[g][c].x, v[g][c].y, v[g][c].z, v[g][c].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            xf[g][c][i] = f2_t{__uint_as_float(q[i] << 16), __uint_as_float(q[i] & 0xffff0000u)};
            s2[i & 1] = __builtin_elementwise_fma(xf[g][c][i], c == 1 && lane + 64 >= 125 ? f2_t{0.f, 0.f} : w2[c][i], s2[i & 1]);
          }
        }
        const f2_t st = s2[0] + s2[1];
        dot[g] = st.x + st.y;
      }
#pragma unroll
      for (int g = 0; g < U; ++g) dot[g] = wave_sum_dpp(dot[g]);
#pragma unroll
      for (int g = 0; g < U; ++g) {
        const bool ok = k * U + g < nj && b0 + (k * U + g) * W + wave < rows;
        float m = __builtin_amdgcn_rcpf(1.f + __expf(-dot[g])) - 0.5f;
        s += ok ? m * m : 0.f;
        m = ok ? m : 0.f;
        const f2_t m2 = {m, m};
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc2[c][i] = __builtin_elementwise_fma(m2, xf[g][c][i], acc2[c][i]);
      }
    }
  }
  if constexpr (MATH) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) s += acc2[c][i].x + acc2[c][i].y;
  }
  if (s == 1234.5f) out[0] = s;
}

struct Variant {
  std::string name;
  void (*launch)(const u32x4*, long, float*);
  std::vector<double> us;
};

template <int R, int S, bool GRP, bool MATH, int GRID>
static void launch_loader(const u32x4* p, long rows, float* out) {
  rows_loader<R, S, GRP, MATH, true><<<GRID, 576, S * R * 2048>>>(p, rows, out);
}
template <int GRID>
static void launch_reg(const u32x4* p, long rows, float* out) {
  rows_reg<2, 8><<<GRID, 512>>>(p, rows, out);
}

template <int R, int S, bool GRP, bool MATH, int GRID>
static int add_loader(std::vector<Variant>& vs) {
  CK(hipFuncSetAttribute((const void*)rows_loader<R, S, GRP, MATH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, S * R * 2048));
  char nm[64];
  snprintf(nm, sizeof nm, "%s R%d S%d %s g%d", MATH ? "ldm" : "ld ", R, S, GRP ? "grp" : "row", GRID);
  vs.push_back({nm, launch_loader<R, S, GRP, MATH, GRID>, {}});
  return 0;
}
template <int R, int S, int GRID>
static int add_four(std::vector<Variant>& vs) {
  if (add_loader<R, S, false, false, GRID>(vs)) return 1;
  if (add_loader<R, S, true, false, GRID>(vs)) return 1;
  if (add_loader<R, S, false, true, GRID>(vs)) return 1;
  if (add_loader<R, S, true, true, GRID>(vs)) return 1;
  return 0;
}
template <int GRID>
static int add_grid(std::vector<Variant>& vs) {
  char nm[64];
  snprintf(nm, sizeof nm, "reg U2 g%d", GRID);
  vs.push_back({nm, launch_reg<GRID>, {}});
  if (add_four<8, 4, GRID>(vs)) return 1;
  if (add_four<8, 6, GRID>(vs)) return 1;
  if (add_four<8, 8, GRID>(vs)) return 1;
  if (add_four<16, 4, GRID>(vs)) return 1;
  return 0;
}

int main() {
  const long rows_total = 2000000, batch = 100000;
  const size_t bytes = (size_t)rows_total * 2000;
  u32x4* x;
  float* out;
  CK(hipMalloc(&x, bytes));
  CK(hipMalloc(&out, 4));
  CK(hipMemset(x, 0x3c, bytes));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int P = (int)(rows_total / batch);
  const double gb = batch * 2000.0 / 1e9;
  std::vector<Variant> vs;
  if (add_grid<224>(vs)) return 1;
  if (add_grid<256>(vs)) return 1;
  const int reps = 5, iters = 100;
  for (int rep = 0; rep < reps; ++rep) {
    for (auto& v : vs) {
      for (int i = 0; i < 10; ++i) v.launch(x + (size_t)(i % P) * batch * 125, batch, out);
      CK(hipEventRecord(e0));
      for (int i = 0; i < iters; ++i) v.launch(x + (size_t)(i % P) * batch * 125, batch, out);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double us = ms * 1e3 / iters;
      v.us.push_back(us);
      printf("rep %d %-24s %8.2f us/batch %8.0f GB/s\n", rep, v.name.c_str(), us, gb / (us * 1e-6));
      fflush(stdout);
    }
  }
  printf("\n%-24s %8s %8s %8s   (us per 200 MB batch over %d repetitions)\n", "variant", "min", "median", "max", reps);
  for (auto& v : vs) {
    std::sort(v.us.begin(), v.us.end());
    printf("%-24s %8.2f %8.2f %8.2f\n", v.name.c_str(), v.us.front(), v.us[v.us.size() / 2], v.us.back());
  }
  return 0;
}
