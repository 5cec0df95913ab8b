// Ordered integer keys of categorical values, shared by the contingency kernels (catstats.hip: dense
// columns; catstats_csr.hip: CSR columns). Value identity: −0 is folded into +0, every NaN is the one
// canonical NaN and sorts last; unsigned key order = value order.
#pragma once
#include "common.h"

__device__ __forceinline__ uint64_t asc_key(double v) {
  if (v == 0.0) v = 0.0;  // −0 → +0
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) b = 0x7ff8000000000000ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_val(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// the same for fp32 values: 32-bit keys (a column index fits above them in one 64-bit sort key)
__device__ __forceinline__ uint32_t asc_key32(float v) {
  if (v == 0.0f) v = 0.0f;
  uint32_t b = __float_as_uint(v);
  if (v != v) b = 0x7fc00000u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key32_val(uint32_t k) {
  return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}
