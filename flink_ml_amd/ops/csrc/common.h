// Shared device helpers for the flink_ml_amd CDNA4 (gfx950) kernels.
//
// Conventions
//  * wave64 everywhere: lane = threadIdx.x & 63, wave = threadIdx.x >> 6.
//  * bf16 is carried as raw uint16 and widened with a shift (exact); narrowing uses the
//    compiler's cast (v_cvt_pk_bf16_f32 keeps NaN a NaN, see MI355X_MICROARCH correctness).
//  * Every launcher is `extern "C"` taking raw device pointers + a hipStream_t so Python
//    (ctypes) can launch onto torch's current stream, and a stream capture (hipGraph) of a
//    whole training round works unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#define FMLX_API extern "C" __attribute__((visibility("default")))

typedef uint16_t bf16_t;

// dtype codes shared with Python (flink_ml_amd/ops/native.py)
enum FmlxDType { DT_F32 = 0, DT_F64 = 1, DT_BF16 = 2, DT_F16 = 3, DT_I32 = 4, DT_I64 = 5 };
// ... and the C++ type each code stands for in a kernel's template arguments (with_dtype, dispatch.h)
template <typename T> struct DTypeCode;
template <> struct DTypeCode<float> { static constexpr int value = DT_F32; };
template <> struct DTypeCode<double> { static constexpr int value = DT_F64; };
template <> struct DTypeCode<bf16_t> { static constexpr int value = DT_BF16; };
template <> struct DTypeCode<int> { static constexpr int value = DT_I32; };

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}

__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  // round-to-nearest-even; NaN preserved by forcing a quiet-NaN mantissa bit
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return (bf16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}

template <typename T> struct Ld;
template <> struct Ld<float> {
  static __device__ __forceinline__ float f(float v) { return v; }
};
template <> struct Ld<double> {
  static __device__ __forceinline__ double f(double v) { return v; }
};
template <> struct Ld<bf16_t> {
  static __device__ __forceinline__ float f(bf16_t v) { return bf16_to_f32(v); }
};

// Accumulator type per storage type: fp32 for bf16/fp32 inputs, fp64 for fp64 (parity mode).
template <typename T> struct AccOf { typedef float type; };
template <> struct AccOf<double> { typedef double type; };

// --- wave64 reductions (butterfly over __shfl_xor lowers to DPP / ds_swizzle) ------------------
template <typename A>
__device__ __forceinline__ A wave_sum(A v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// Full wave64 sum with DPP row ops (no LDS round trips, unlike ds_bpermute-based shuffles):
// quad xor1/xor2 → half-row mirror → row mirror → row_bcast:15 → row_bcast:31; lane 63 holds the
// total, broadcast with v_readlane into a (wave-uniform) scalar.
template <int CTRL, int ROW_MASK = 0xF, bool BOUND = true>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, BOUND));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);          // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);          // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);         // row_half_mirror
  v += dpp_mov<0x140>(v);         // row_mirror
  v += dpp_mov<0x142, 0xA, false>(v);  // row_bcast:15 → rows 1,3
  v += dpp_mov<0x143, 0xC, false>(v);  // row_bcast:31 → rows 2,3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double wave_sum_dpp(double v) { return wave_sum(v); }

template <typename A>
__device__ __forceinline__ A wave_max(A v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { A o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}
template <typename A>
__device__ __forceinline__ A wave_min(A v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { A o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}

// Vector chunk of EPC elements of T loaded with one instruction (EPC*sizeof(T) in {2,4,8,16}).
template <typename T, int EPC>
struct Chunk {
  T v[EPC];
};

template <typename T, int EPC>
__device__ __forceinline__ void load_chunk(const T* __restrict__ p, Chunk<T, EPC>& c) {
  constexpr int BYTES = EPC * (int)sizeof(T);
  if constexpr (BYTES == 16) {
    *reinterpret_cast<uint4*>(c.v) = *reinterpret_cast<const uint4*>(p);
  } else if constexpr (BYTES == 8) {
    *reinterpret_cast<uint2*>(c.v) = *reinterpret_cast<const uint2*>(p);
  } else if constexpr (BYTES == 4) {
    *reinterpret_cast<uint32_t*>(c.v) = *reinterpret_cast<const uint32_t*>(p);
  } else {
#pragma unroll
    for (int i = 0; i < EPC; ++i) c.v[i] = p[i];
  }
}

// Same, with the non-temporal hint (global_load … nt) for rows streamed exactly once.
template <typename T, int EPC>
__device__ __forceinline__ void load_chunk_nt(const T* __restrict__ p, Chunk<T, EPC>& c) {
  constexpr int BYTES = EPC * (int)sizeof(T);
  if constexpr (BYTES == 16) {
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    __builtin_memcpy(c.v, &v, 16);
  } else {
    load_chunk<T, EPC>(p, c);
  }
}

static inline int fmlx_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

#define FMLX_CHECK_LAUNCH() return (int)hipGetLastError()

#include "dispatch.h"  // host side: run-time dtype / width arguments → template arguments

// --- eager code-object loading ------------------------------------------------------------------
// HIP loads a translation unit's code object lazily, at the first launch of any of its kernels
// (hsa_executable_load_agent_code_object + freeze: ~30 ms for glm.hip's, measured inside a
// sparse SVC fit: profiles/r4/svc_stall_systrace_summary.json). Every .hip file ends with
// FMLX_DEFINE_PRELOAD(): an empty anchor kernel registered at library load; fmlx_preload_all()
// launches each anchor once, so every code object is resident before the first real launch
// (ops/native.py calls it when it loads the library and reports the one-time cost).
namespace fmlx_preload {
inline std::vector<const void*>& registry() {
  static std::vector<const void*> r;
  return r;
}
struct Reg {
  explicit Reg(const void* f) { registry().push_back(f); }
};
}  // namespace fmlx_preload

#define FMLX_DEFINE_PRELOAD()                                                   \
  namespace {                                                                   \
  __global__ void fmlx_tu_anchor_kernel() {}                                    \
  const fmlx_preload::Reg fmlx_tu_anchor_reg((const void*)&fmlx_tu_anchor_kernel); \
  }
