// The sorted per-lane (dist, index) list of the KNN kernels (knn.hip, knn_wide.hip,
// knn_wide_f64.hip) and the stage that merges the candidates of several training segments. The key
// type KT is float or double, deduced from the arguments.
//
// A list of length K lives in VGPRs (fully unrolled compare-exchange insertion, no scratch). Empty
// slots are (inf, INT32_MAX): every real (dist, index) sorts before them, infinite distances
// included. All comparisons are lexicographic on (dist, index), so ties go to the lower index no
// matter in which order a lane meets them.
#pragma once
#include "common.h"

#include <math.h>

namespace {

__device__ __forceinline__ float key_sqrt(float d) { return __builtin_sqrtf(d); }
__device__ __forceinline__ double key_sqrt(double d) { return __builtin_sqrt(d); }

template <typename KT>
__device__ __forceinline__ bool lex_less(KT da, int ia, KT db, int ib) {
  return da < db || (da == db && ia < ib);
}

template <int K, typename KT>
__device__ __forceinline__ void topk_insert(KT (&bd)[K], int (&bi)[K], KT d, int j) {
  // (d, j) < tail already checked; drop the tail, bubble the new element up in (dist, index)
  // order (an equal distance seen later keeps its place behind the earlier one)
  bd[K - 1] = d;
  bi[K - 1] = j;
#pragma unroll
  for (int i = K - 1; i > 0; --i) {
    if (lex_less(bd[i], bi[i], bd[i - 1], bi[i - 1])) {
      KT td = bd[i]; bd[i] = bd[i - 1]; bd[i - 1] = td;
      int ti = bi[i]; bi[i] = bi[i - 1]; bi[i - 1] = ti;
    }
  }
}

// Merge the 64 lane lists of one wave into the k best (dist, index) pairs, written with
// stride 1 at od/oi (lane 0 writes).
template <int K, bool SQRT, typename KT>
__device__ __forceinline__ void wave_merge_out(KT (&bd)[K], int (&bi)[K], int lane, int k, KT* od, int* oi) {
  for (int t = 0; t < k; ++t) {
    KT wd = bd[0];
    int wi = bi[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const KT xd = __shfl_xor(wd, off, 64);
      const int xi = __shfl_xor(wi, off, 64);
      if (lex_less(xd, xi, wd, wi)) { wd = xd; wi = xi; }
    }
    if (lane == 0) {
      oi[t] = wi;
      if (od) od[t] = SQRT ? key_sqrt(wd) : wd;
    }
    if (bi[0] == wi && wi != INT32_MAX) {  // (dist, index) pairs are unique: one lane pops
#pragma unroll
      for (int i = 0; i < K - 1; ++i) { bd[i] = bd[i + 1]; bi[i] = bi[i + 1]; }
      bd[K - 1] = INFINITY;
      bi[K - 1] = INT32_MAX;
    }
  }
}

// k-th entry (0-based k-1) of a sorted lane list, as a wave-uniform-index select
template <int K, typename KT>
__device__ __forceinline__ void kth_entry(const KT (&bd)[K], const int (&bi)[K], int k, KT& td, int& ti) {
  td = bd[0];
  ti = bi[0];
#pragma unroll
  for (int i = 1; i < K; ++i)
    if (i == k - 1) { td = bd[i]; ti = bi[i]; }
}

// v[b] for a per-lane b in [0, N) as a linear select chain on register values. (A select TREE
// gets folded into an indexed load of the array — select(load a, load b) → load(select) — which
// demotes the whole key array to scratch.)
template <typename KT, int N>
__device__ __forceinline__ KT select_slot(const KT (&v)[N], int b) {
  KT r = INFINITY;
#pragma unroll
  for (int i = 0; i < N; ++i) r = b == i ? v[i] : r;
  return r;
}

// the fp32 kernels' 32 keys per lane
__device__ __forceinline__ float select32(const float (&v)[32], int b) { return select_slot(v, b); }

template <int K, typename KT>
__device__ __forceinline__ void topk_pop(KT (&bd)[K], int (&bi)[K]) {
#pragma unroll
  for (int i = 0; i < K - 1; ++i) { bd[i] = bd[i + 1]; bi[i] = bi[i + 1]; }
  bd[K - 1] = INFINITY;
  bi[K - 1] = INT32_MAX;
}

// Stage 2: wave per row merges the S·k segment candidates (lexicographic (dist, index), so the
// reference's tie rule survives the split).
template <int K, typename KT>
__global__ __launch_bounds__(256) void knn_topk_merge_kernel(const KT* __restrict__ cd, const int* __restrict__ ci,
                                                             long nq, int S, int k, int* __restrict__ out_i,
                                                             KT* __restrict__ out_d) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq) return;
  KT bd[K];
  int bi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { bd[i] = INFINITY; bi[i] = INT32_MAX; }
  const long m = (long)S * k;
  for (long c = lane; c < m; c += 64) {
    const KT d = cd[row * m + c];
    const int j = ci[row * m + c];
    if (lex_less(d, j, bd[K - 1], bi[K - 1])) topk_insert<K>(bd, bi, d, j);
  }
  wave_merge_out<K, true>(bd, bi, lane, k, out_d ? out_d + row * k : (KT*)nullptr, out_i + row * k);
}

// the candidates ws_d / ws_i [nq, S, k] of S segments → idx / dist [nq, k]
template <int K, typename KT>
void launch_topk_merge(const KT* ws_d, const int* ws_i, long nq, int S, int k, int* idx, KT* dist, hipStream_t s) {
  hipLaunchKernelGGL((knn_topk_merge_kernel<K, KT>), dim3(fmlx_ceil_div(nq, 4)), dim3(256), 0, s, ws_d, ws_i, nq, S, k,
                     idx, dist);
}

}  // namespace
