// Integer prefix scans shared by the device kernels: one wave, one block, an array by one block.
// The operators are associative over integers (add, max), so any regrouping gives the same bits.
// A single block scanning more than NT values loops over passes of NT and keeps the running
// total in a register:   ex = carry + block_excl_scan<NT>(v, tmp, &tot);  carry += tot;
#pragma once
#include "common.h"

#include <type_traits>

struct ScanAdd {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct ScanMax {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// inclusive scan over the lanes of a wave; W < 64 (a power of two): log2 W steps, lanes 0 … W − 1
// hold their inclusive prefix (the wave totals of a block)
template <int W = 64, typename T, typename Op>
__device__ __forceinline__ T wave_incl_scan(T v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < W; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, t);
  }
  return v;
}
template <int W = 64, typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  return wave_incl_scan<W>(v, ScanAdd());
}

// exclusive scan of one value per thread over the block. All NT threads call it; tmp: NT / 64
// values of LDS; *total (if asked for) = the block's total. Ends with a barrier: tmp may be
// reused at once. (The wave scan first, lane / w after it: with the other order the register
// allocation of knn_select_kernel changes, profiles/r14/INDEX.md.)
template <int NT, typename T, typename Op>
__device__ __forceinline__ T block_excl_scan(T v, T ident, Op op, T* tmp, T* total = nullptr) {
  const T x = wave_incl_scan(v, op);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 63) tmp[w] = x;
  __syncthreads();
  if (w == 0) {
    const T s = wave_incl_scan<NT / 64>(lane < NT / 64 ? tmp[lane] : ident, op);
    if (lane < NT / 64) tmp[lane] = s;
  }
  __syncthreads();
  const T pre = w ? tmp[w - 1] : ident;
  if (total) *total = tmp[NT / 64 - 1];
  // the lanes before mine in my wave. The shuffle is right for every operator; x − v for the sum is
  // there for code generation only (the instructions the hot integer-add users always had): a new
  // operator needs no branch of its own
  T ex;
  if constexpr (std::is_same<Op, ScanAdd>::value) {
    ex = x - v;
  } else {
    ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = ident;
  }
  __syncthreads();
  return op(pre, ex);
}
template <int NT, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* tmp, T* total = nullptr) {
  return block_excl_scan<NT>(v, (T)0, ScanAdd(), tmp, total);
}

// exclusive scan of v[0..m) into out[0..m) (LDS or global, in place too) by the whole block, each
// thread a run of consecutive values; returns the total
template <int NT, typename T>
__device__ __forceinline__ T block_excl_scan_array(const T* v, T* out, int m, T* tmp, long ostride = 1) {
  const int per = (m + NT - 1) / NT;
  const int q0 = threadIdx.x * per;
  T mine = 0;
  for (int i = 0; i < per; ++i) mine += q0 + i < m ? v[q0 + i] : 0;
  T total;
  T run = block_excl_scan<NT>(mine, tmp, &total);
  for (int i = 0; i < per; ++i)
    if (q0 + i < m) {
      const T c = v[q0 + i];
      out[(long)(q0 + i) * ostride] = run;
      run += c;
    }
  return total;
}
