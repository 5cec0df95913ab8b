// Sparse (CSR) SGD rounds (LinearSVC / LR on 1M-wide sparse features).
//
// Reference hot loop: LIB/common/optimizer/SGD.java:263-285 over SparseVector rows with
// LIB/common/lossfunc/HingeLoss.java:39-57 (dot, hinge loss, axpy of the multiplier into the
// gradient), the update of SGD.java:231-243 and RegularizationUtils.java:47-91.
//
// Three round forms, picked per fit by common/optimizer.py (DeviceGlmTrainer):
//  * single-visit bucket round (glm_bkt_*): the reference's regime (each batch visited once or a
//    few times): nothing is precomputed per batch;
//  * transposed rounds (glm_csr_fwd / glm_csr_cell_fwd + glm_csc_bwd / glm_csc_tile_bwd): batches
//    visited many times (or FMLX_DETERMINISTIC=1) amortise a per-batch column-major copy
//    (csc_build.hip) and run atomic-free, deterministic backward passes;
//  * glm_grad_csr_kernel: the scattered-atomic fallback when neither fits.
#include <type_traits>

#include "common.h"
#include "glm_core.h"
#include "scan.h"

namespace {

// Round e visits batch e mod ⌈n / B⌉ (SGD.java:263-268); batch b is the fixed row range
// [b·B, min((b + 1)·B, n)) (SGD.java:192-206 slicing). Two functions: the backward kernels need the
// rows only on their unweighted branch (the end computed ahead of it, or written start + B, costs
// the feedback backwards 8 SGPRs: profiles/r13).
__device__ __forceinline__ long round_batch(int e, long n, long B) {
  const long P = (n + B - 1) / B;
  return (long)(e % P);
}
__device__ __forceinline__ void batch_rows(long b, long n, long B, long& start, long& end) {
  start = b * B;
  end = (b + 1) * B < n ? (b + 1) * B : n;
}

// ------------------------------------------------------------------------------------------
// CSR (sparse features) gradient — a wave per row, gather dot, atomic scatter of mult·x into
// a dense gradient (K5 sparse path, for the 1M-feature LinearSVC config).
// ------------------------------------------------------------------------------------------
template <typename A>
__global__ __launch_bounds__(256) void glm_grad_csr_kernel(const long* __restrict__ indptr, const int* __restrict__ idx,
                                                           const A* __restrict__ val, const A* __restrict__ y,
                                                           const A* __restrict__ wt, const A* __restrict__ coef, long n,
                                                           int d, long B, int loss, const int* __restrict__ state,
                                                           A* __restrict__ grad /* d+2, zeroed */) {
  int e;
  if (!round_running(state, e)) return;
  long start, end;
  batch_rows(round_batch(e, n, B), n, B, start, end);
  const int lane = threadIdx.x & 63;
  const long gw = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long W = ((long)gridDim.x * blockDim.x) >> 6;
  A wsum = 0, lsum = 0;
  for (long r = start + gw; r < end; r += W) {
    const long s0 = indptr[r], s1 = indptr[r + 1];
    A s = 0;
    for (long j = s0 + lane; j < s1; j += 64) s += val[j] * coef[idx[j]];
    s = wave_sum(s);
    const A yy = y[r];
    const A ww = wt ? wt[r] : (A)1;
    A l, m;
    loss_and_mult(loss, s, yy, ww, l, m);
    wsum += ww;
    lsum += l;
    if (m != (A)0)
      for (long j = s0 + lane; j < s1; j += 64) atomicAdd(&grad[idx[j]], m * val[j]);
  }
  if (lane == 0) {
    atomicAdd(&grad[d], wsum);
    atomicAdd(&grad[d + 1], lsum);
  }
}

template <typename A>
__global__ void glm_csr_predict_kernel(const long* __restrict__ indptr, const int* __restrict__ idx,
                                       const A* __restrict__ val, const A* __restrict__ coef, long n,
                                       double* __restrict__ dots) {
  const int lane = threadIdx.x & 63;
  const long gw = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long W = ((long)gridDim.x * blockDim.x) >> 6;
  for (long r = gw; r < n; r += W) {
    A s = 0;
    for (long j = indptr[r] + lane; j < indptr[r + 1]; j += 64) s += val[j] * coef[idx[j]];
    s = wave_sum(s);
    if (lane == 0) dots[r] = (double)s;
  }
}

// ------------------------------------------------------------------------------------------
// Sparse (CSR) SGD round without atomics on the gradient
// ------------------------------------------------------------------------------------------
// Batches are the fixed row ranges [b·B, min((b+1)·B, n)) (SGD.java:192-206 slicing), so the
// transpose of every batch can be built once when the trainer starts (ops/glm.py
// build_batch_csc): per batch, its non-zeros re-sorted by column with the batch-relative row id,
// at the SAME offsets as the CSR (batch b's non-zeros are CSR positions [indptr[bB], indptr[bB+B])),
// plus a dense int32 column pointer [P][d+1]. A round is then two launches:
//   forward  — a G-lane group per row: gathered dot, loss + multiplier m_r (stored, B floats,
//              L2-resident), Σweight/Σloss into a parity slot of `wl`;
//   backward — a thread per column: g_c = Σ m_row·val over the column's batch entries (a
//              segmented gather, no atomics), then either the SGD update + termination check in
//              place (1 GPU) or the feedback row for the all-reduce (N GPUs).
// The 1M-wide scatter of atomicAdds it replaces (glm_grad_csr_kernel) was 472 µs per round on the
// 100k × 64-nnz batch of the sparse LinearSVC config; the reads here are the batch once in each
// layout plus one column-pointer row.
template <int G, typename A>
__device__ __forceinline__ A group_sum(A v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Forward: K independent (index, value) slots per lane are loaded before any coefficient gather,
// so a row costs one dependent step (indptr → entries → coef) instead of a chain per element;
// entries are streamed non-temporally, which keeps the gathered coefficient vector in L2.
constexpr int WL_SLOTS = 256;  // Σweight/Σloss accumulator: [2 parities][WL_SLOTS][WL_STRIDE]
constexpr int WL_STRIDE = 32;  // 128 B apart

// A forward block's Σweight / Σloss into a parity slot of `wl`, in two steps (the bucket forward
// stamps its trace between them). Stage: every wave's sums into `red`, then a barrier; the caller
// passes wave_sum(...) of its threads' sums (made inside the helper, the fp32 forwards scheduled
// their last adds differently: profiles/r13). Add: thread 0 adds the nw waves' sums to slot
// `slot` mod WL_SLOTS of round e's parity — one of WL_SLOTS cache lines per block: same-address
// float atomics from thousands of blocks serialise at the coherence point (measured: the
// single-address version cost more than the row math); the backward sums the slots in a fixed order.
template <int NW, typename A>
__device__ __forceinline__ void fwd_sums_stage(A wave_w, A wave_l, A (&red)[2][NW]) {
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = wave_w;
    red[1][threadIdx.x >> 6] = wave_l;
  }
  __syncthreads();
}
template <int NW, typename A>
__device__ __forceinline__ void fwd_sums_add(const A (&red)[2][NW], int nw, A* __restrict__ wl, int e, int slot) {
  if (threadIdx.x == 0) {
    A a0 = 0, a1 = 0;
    for (int i = 0; i < nw; ++i) {
      a0 += red[0][i];
      a1 += red[1][i];
    }
    A* s = wl + ((long)(e & 1) * WL_SLOTS + (slot & (WL_SLOTS - 1))) * WL_STRIDE;
    if (a0 != (A)0) atomicAdd(&s[0], a0);
    if (a1 != (A)0) atomicAdd(&s[1], a1);
  }
}

template <typename A, int G>
__global__ __launch_bounds__(256) void glm_csr_fwd_kernel(const long* __restrict__ indptr, const int* __restrict__ idx,
                                                          const A* __restrict__ val, const A* __restrict__ y,
                                                          const A* __restrict__ wt, const A* __restrict__ coef, long n,
                                                          long B, int loss, const int* __restrict__ state,
                                                          A* __restrict__ mult, A* __restrict__ wl) {
  constexpr int K = G >= 32 ? 2 : 4;
  int e;
  if (!round_running(state, e)) return;
  long start, end;
  batch_rows(round_batch(e, n, B), n, B, start, end);
  const int lane = threadIdx.x & (G - 1);
  const long grp = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const long NG = ((long)gridDim.x * blockDim.x) / G;
  A wsum = 0, lsum = 0;
  for (long r = start + grp; r < end; r += NG) {
    const long s0 = indptr[r], s1 = indptr[r + 1];
    A s = 0;
    for (long jb = s0; jb < s1; jb += K * G) {
      int ii[K];
      A vv[K];
#pragma unroll
      for (int t = 0; t < K; ++t) {
        const long j = jb + lane + t * G;
        const bool ok = j < s1;
        const long jj = ok ? j : s0;
        ii[t] = __builtin_nontemporal_load(idx + jj);
        const A v = __builtin_nontemporal_load(val + jj);
        vv[t] = ok ? v : (A)0;
      }
#pragma unroll
      for (int t = 0; t < K; ++t) s += vv[t] * coef[ii[t]];
    }
    s = group_sum<G>(s);
    if (lane == 0) {
      const A ww = wt ? wt[r] : (A)1;
      A l, m;
      loss_and_mult(loss, s, y[r], ww, l, m);
      mult[r - start] = m;
      wsum += ww;
      lsum += l;
    }
  }
  __shared__ A red[2][4];
  fwd_sums_stage(wave_sum(wsum), wave_sum(lsum), red);
  fwd_sums_add(red, (int)(blockDim.x >> 6), wl, e, (int)blockIdx.x);
}

// Forward over row-block × column-split cells (BatchCsc cells, csc_build.hip cell_keys … cell_store):
// cell (rb, s) holds the batch's entries of rows [rb·2^CELL_RBB, …) with columns in [s·CS, (s+1)·CS),
// stored column-sorted and packed (column − s·CS) | pos << cb, pos = the entry's rank in the cell's
// row-major order; roff[cell·2^CELL_RBB + r] = first entry of row r of the cell. A block takes a
// cell: its lanes gather coefficients in column order from one slice (consecutive lanes share
// cache lines — the one-row-per-lane-group kernel gathers a random line per lane, ~40 µs per 6.4M,
// profiles/r5/micro_gather_*), write each product into LDS slot pos (plain stores: LDS float
// atomics cost ~27 µs more per round, profiles/r5/svc_cell_forward_ab.jsonl), then every row sums
// its slots in order and the cell stores its row partials. The last of a row block's S cells to
// arrive sums the S partials of every row in split order (deterministic), evaluates loss and
// multiplier, and adds Σweight / Σloss into the slots.
constexpr int CELL_THREADS = 1024;
constexpr int CELL_RBB_MAX = 11;  // rows per row block: 2^rbb ≤ 2^11 (two rows per thread)
constexpr int CELL_U = 8;

template <typename A>
__global__ __launch_bounds__(CELL_THREADS) void glm_csr_cell_fwd_kernel(
    const long* __restrict__ indptr, const uint32_t* __restrict__ cent, const A* __restrict__ cval,
    const int* __restrict__ roff, long rstride, int rbb, int S, int CS, int cb, const A* __restrict__ y,
    const A* __restrict__ wt, const A* __restrict__ coef, long n, long B, int loss, const int* __restrict__ state,
    A* __restrict__ mult, A* __restrict__ wl, A* __restrict__ partial, int* __restrict__ cnt, int xcd) {
  const int RB = 1 << rbb;
  extern __shared__ __align__(16) unsigned char cell_lds[];
  A* prod = reinterpret_cast<A*>(cell_lds);  // [the largest cell's entries]
  __shared__ A red[2][CELL_THREADS / 64];
  __shared__ int sflag;
  int e;
  if (!round_running(state, e)) return;
  const long b = round_batch(e, n, B);
  long start, end;
  batch_rows(b, n, B, start, end);
  const long blen = end - start;
  const int nrb = (int)((blen + RB - 1) >> rbb);
  const int ncell = nrb * S;
  int rb, sp;
  if (xcd) {
    // XCD-aware order: block b runs on XCD b mod 8 (round-robin dispatch); give XCD x the cells
    // of a contiguous split-major range, so its L2 holds the coefficient slices of ≤ 2 splits
    // (a bijection of [0, grid): XCD x holds the n_x = ⌈(grid − x) / 8⌉ blocks b ≡ x mod 8, so it
    // starts at Σ_{y<x} n_y = x·⌊grid/8⌋ + min(x, grid mod 8))
    const int x = (int)(blockIdx.x & 7), q = (int)(gridDim.x >> 3), r = (int)(gridDim.x & 7);
    const int g = x * q + (x < r ? x : r) + (int)(blockIdx.x >> 3);
    if (g >= ncell) return;
    sp = g / nrb;
    rb = g - sp * nrb;
  } else {
    if ((int)blockIdx.x >= ncell) return;  // (the grid covers the largest batch)
    rb = blockIdx.x / S;
    sp = blockIdx.x - rb * S;
  }
  const int c = rb * S + sp;
  const int tid = threadIdx.x;
  const long base = indptr[start];
  const int* __restrict__ ro = roff + b * rstride + ((long)c << rbb);
  const int k0 = ro[0], k1 = ro[RB];
  const uint32_t* __restrict__ en = cent + base;
  const A* __restrict__ ev = cval + base;
  const A* __restrict__ cs = coef + (long)sp * CS;
  const uint32_t cmask = (1u << cb) - 1;
  uint32_t xx[CELL_U];
  A vv[CELL_U];
  if (k0 < k1) {  // (an empty cell may sit at the end of the array: nothing to load)
#pragma unroll
    for (int u = 0; u < CELL_U; ++u) {
      const int k = k0 + tid + u * CELL_THREADS;
      const int kk = k < k1 ? k : k0;
      xx[u] = __builtin_nontemporal_load(en + kk);
      vv[u] = __builtin_nontemporal_load(ev + kk);
    }
  }
  for (int kb = k0 + tid; kb < k1; kb += CELL_U * CELL_THREADS) {
    uint32_t nx[CELL_U];
    A nv[CELL_U];
    const int kn = kb + CELL_U * CELL_THREADS;
    if (kn < k1) {
#pragma unroll
      for (int u = 0; u < CELL_U; ++u) {
        const int k = kn + u * CELL_THREADS;
        const int kk = k < k1 ? k : kn;
        nx[u] = __builtin_nontemporal_load(en + kk);
        nv[u] = __builtin_nontemporal_load(ev + kk);
      }
    }
    // every gather first (lanes past the cell hold its first entry: valid addresses), then the
    // slot stores — a gather per store would serialise CELL_U memory latencies per step
    A pp[CELL_U];
#pragma unroll
    for (int u = 0; u < CELL_U; ++u) pp[u] = vv[u] * cs[xx[u] & cmask];
#pragma unroll
    for (int u = 0; u < CELL_U; ++u)
      if (kb + u * CELL_THREADS < k1) prod[xx[u] >> cb] = pp[u];
#pragma unroll
    for (int u = 0; u < CELL_U; ++u) {
      xx[u] = nx[u];
      vv[u] = nv[u];
    }
  }
  const long rb0 = (long)rb << rbb;
  const int nr = blen - rb0 < RB ? (int)(blen - rb0) : RB;
  constexpr int RQ = (1 << CELL_RBB_MAX) / CELL_THREADS;
  int r0s[RQ], r1s[RQ];
#pragma unroll
  for (int q = 0; q < RQ; ++q) {  // (row offsets loaded before the barrier)
    const int r = tid + q * CELL_THREADS;
    r0s[q] = r < nr ? ro[r] - k0 : 0;
    r1s[q] = r < nr ? ro[r + 1] - k0 : 0;
  }
  __syncthreads();
  A* __restrict__ mine = partial + (long)c * RB;
#pragma unroll
  for (int q = 0; q < RQ; ++q) {
    const int r = tid + q * CELL_THREADS;
    A t = 0;
    for (int j = r0s[q]; j < r1s[q]; ++j) t += prod[j];
    if (r < nr) st_agent(mine + r, t);
  }
  if (!arrive_last(&cnt[rb], S, &sflag)) return;
  if (tid == 0) st_agent(&cnt[rb], 0);  // every arrival of this launch is in: re-arm for the next
  A ws = 0, ls = 0;
  for (int r = tid; r < nr; r += CELL_THREADS) {
    A dot = 0;
    for (int q = 0; q < S; ++q) dot += ld_agent(partial + ((long)rb * S + q) * RB + r);
    const long gr = start + rb0 + r;
    const A ww = wt ? wt[gr] : (A)1;
    A l, m;
    loss_and_mult(loss, dot, y[gr], ww, l, m);
    mult[rb0 + r] = m;
    ws += ww;
    ls += l;
  }
  fwd_sums_stage(wave_sum(ws), wave_sum(ls), red);
  fwd_sums_add(red, CELL_THREADS / 64, wl, e, rb);
}

// Backward: a block owns 256 consecutive columns, whose batch entries are one contiguous CSC
// range. The block walks that range coalesced (every thread loads independent entries: row id →
// multiplier gather → product into LDS), then each thread adds its column's slice of the LDS
// products in entry order — deterministic, no atomics, no per-column dependent load chains.
constexpr int CSC_CAP = 4096;  // entries staged per pass (16 KB fp32 / 32 KB fp64)

// Σweight / Σloss of round e: fixed-order sum of the forward's WL_SLOTS slots (all 256 threads)
template <typename A>
__device__ __forceinline__ void slot_sums(const A* __restrict__ wl, int e, A& W, A& L) {
  __shared__ A red[2][4];
  const bool own = threadIdx.x < WL_SLOTS;  // (blocks of ≥ 256 threads)
  const A* sl = wl + ((long)(e & 1) * WL_SLOTS + (own ? threadIdx.x : 0)) * WL_STRIDE;
  const A w0 = wave_sum(own ? sl[0] : (A)0), l0 = wave_sum(own ? sl[1] : (A)0);
  if ((threadIdx.x & 63) == 0 && own) { red[0][threadIdx.x >> 6] = w0; red[1][threadIdx.x >> 6] = l0; }
  __syncthreads();
  W = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  L = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// The pieces the three backward kernels share (FUSE: the backward applies the update and the
// termination check itself, 1 GPU; else it writes the feedback row fb[d + 2] for the all-reduce).
//
// Begin: block 0 re-arms the other parity's slots (they held the previous round's sums, consumed
// by now); false when the round is not running (a fused backward still arrives: the state advances
// once per launch).
template <bool FUSE, typename A>
__device__ __forceinline__ bool bwd_begin(int* __restrict__ state, A* __restrict__ wl, int& e) {
  const bool run = round_running(state, e);
  if (blockIdx.x == 0 && threadIdx.x < WL_SLOTS) {
    A* o = wl + ((long)((e + 1) & 1) * WL_SLOTS + threadIdx.x) * WL_STRIDE;
    o[0] = 0;
    o[1] = 0;
  }
  if (!run && FUSE) arrive_and_advance(state, e, false, 0);
  return run;
}

// Σweight of the round (batch b): the batch's row count when unweighted, else the fixed-order sum of
// the forward's slots (identical in every block). Σloss only feeds the termination test, which the
// last arriving block makes (bwd_finish), and block 0 of the feedback path, which exports it.
template <bool FUSE, typename A>
__device__ __forceinline__ void bwd_weights(const A* __restrict__ wl, int e, long b, long n, long B, int weighted, A& W,
                                            A& L) {
  L = 0;
  if (weighted || (!FUSE && blockIdx.x == 0)) slot_sums(wl, e, W, L);
  if (!weighted) {
    long start, end;
    batch_rows(b, n, B, start, end);
    W = (A)(end - start);
  }
}

// Column c's gradient sum g: the SGD step on its coefficient (w: its value before the step), or
// its feedback entry.
template <bool FUSE, typename A>
__device__ __forceinline__ void put_col(A* __restrict__ coef, A* __restrict__ fb, long c, A w, A g, A W, A lr, A reg,
                                        A en) {
  if (FUSE)
    coef[c] = sgd_apply<A>(w, g, W, lr, reg, en);
  else
    fb[c] = g;
}
template <bool FUSE, typename A>
__device__ __forceinline__ void put_col(A* __restrict__ coef, A* __restrict__ fb, long c, A g, A W, A lr, A reg, A en) {
  put_col<FUSE>(coef, fb, c, FUSE ? coef[c] : (A)0, g, W, lr, reg, en);
}

// the feedback row's Σweight / Σloss entries (block 0)
template <bool FUSE, typename A>
__device__ __forceinline__ void bwd_export(A* __restrict__ fb, int d, A W, A L) {
  if (!FUSE && blockIdx.x == 0 && threadIdx.x == 0) {
    fb[d] = W;
    fb[d + 1] = L;
  }
}

// The fused backward's last block (each kernel elects it its own way; every other block has
// finished its reads of the state words by then, see arrive_and_advance): Σloss from the slots, the
// termination test and the round state; `rearm`: the election drew ST_ARRIVE tickets.
template <typename A>
__device__ __forceinline__ void bwd_finish(int* __restrict__ state, const A* __restrict__ wl, int e, A W, int max_iter,
                                           A tol, bool rearm) {
  A w2, L;
  slot_sums(wl, e, w2, L);
  if (threadIdx.x == 0) {
    const bool cont = (e + 1 < max_iter) && (L / W > tol);
    state[ST_RUN0 + ((e + 1) & 1)] = cont ? 1 : 0;
    state[ST_EXECUTED] += 1;
    state[ST_ROUND] = e + 1;
    if (rearm) state[ST_ARRIVE] = 0;
  }
}

template <typename A, bool FUSE>
__global__ __launch_bounds__(256) void glm_csc_bwd_kernel(const long* __restrict__ indptr,
                                                          const int* __restrict__ colptr, const int* __restrict__ erow,
                                                          const A* __restrict__ eval, const A* __restrict__ mult,
                                                          long n, int d, long B, int* __restrict__ state,
                                                          A* __restrict__ wl, A* __restrict__ fb, A* __restrict__ coef,
                                                          int max_iter, A tol, A lr, A reg, A en, int weighted) {
  __shared__ A prod[CSC_CAP];
  int e;
  if (!bwd_begin<FUSE>(state, wl, e)) return;
  const long b = round_batch(e, n, B);
  const long base = indptr[b * B];
  const int* __restrict__ cp = colptr + b * (long)(d + 1);
  const int* __restrict__ er = erow + base;
  const A* __restrict__ ev = eval + base;
  A W, L;
  bwd_weights<FUSE>(wl, e, b, n, B, weighted, W, L);
  for (int cb = blockIdx.x * 256; cb < d; cb += gridDim.x * 256) {
    const int c = cb + (int)threadIdx.x;
    const int ce = cb + 256 < d ? cb + 256 : d;
    const int lo = cp[cb], hi = cp[ce];
    const int j0 = c < d ? cp[c] : hi, j1 = c < d ? cp[c + 1] : hi;
    A g = 0;
    for (int pb = lo; pb < hi; pb += CSC_CAP) {
      const int top = pb + CSC_CAP < hi ? pb + CSC_CAP : hi;
      for (int k0 = pb + (int)threadIdx.x; k0 < top; k0 += 4 * 256) {
        int rr[4];
        A vv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = k0 + t * 256;
          const int kk = k < top ? k : k0;
          rr[t] = __builtin_nontemporal_load(er + kk);
          vv[t] = __builtin_nontemporal_load(ev + kk);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = k0 + t * 256;
          const A p = mult[rr[t]] * vv[t];
          if (k < top) prod[k - pb] = p;
        }
      }
      __syncthreads();
      const int a = j0 > pb ? j0 : pb, z = j1 < top ? j1 : top;
      for (int j = a; j < z; ++j) g += prod[j - pb];
      __syncthreads();
    }
    if (c < d) put_col<FUSE>(coef, fb, c, g, W, lr, reg, en);
  }
  bwd_export<FUSE>(fb, d, W, L);
  if (FUSE) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0)
      last = __hip_atomic_fetch_add(&state[ST_ARRIVE], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             (int)gridDim.x - 1;
    __syncthreads();
    if (last) bwd_finish(state, wl, e, W, max_iter, tol, true);
  }
}

// Tiled backward (BatchCsc tiles, csc_build.hip csc_tiles / csc_tile_keys / csc_tile_store): the
// batch's columns are cut into tiles of ≤ ET entries (or one heavy column of > EL), and inside a light
// tile the entries are sorted by ROW, each carrying its slot in the tile's column-ordered range
// (erow = row | slot << rb). A block takes a tile: the multiplier gathers of consecutive lanes
// then fall on the same or nearby cache lines (the one-column-block form gathers a random row per
// lane: measured ~40 µs for 6.4M such 4-byte gathers, the cost scaling with distinct lines per
// wave instruction), each product goes to its column-ordered LDS slot, and a thread per column
// sums its slots in entry order — the same per-column order as the untiled kernel, so results
// are deterministic. A heavy column is a block-strided sum with a fixed-order block reduction.
constexpr int TILE_THREADS = 1024;
constexpr int TILE_U = 8;     // entries per thread per gather step
constexpr int TILE_COLS = 8;  // columns per thread whose pointers are prefetched

template <typename A, bool FUSE>
__global__ __launch_bounds__(TILE_THREADS) void glm_csc_tile_bwd_kernel(
    const long* __restrict__ indptr, const int* __restrict__ colptr, const int2* __restrict__ tiles,
    const int* __restrict__ ntiles, int tstride, const int* __restrict__ erow, const A* __restrict__ eval,
    const A* __restrict__ mult, long n, int d, long B, int rb, int EL, int* __restrict__ state, A* __restrict__ wl,
    A* __restrict__ fb, A* __restrict__ coef, int max_iter, A tol, A lr, A reg, A en, int weighted,
    long long* __restrict__ trace) {
  extern __shared__ unsigned char tile_smem[];
  if (trace && threadIdx.x == 0) trace[(long)blockIdx.x * 4] = (long long)__builtin_amdgcn_s_memrealtime();
  A* prod = reinterpret_cast<A*>(tile_smem);
  __shared__ A hred[TILE_THREADS / 64];
  int e;
  if (!bwd_begin<FUSE>(state, wl, e)) return;
  const long b = round_batch(e, n, B);
  const long base = indptr[b * B];
  const int* __restrict__ cp = colptr + b * (long)(d + 1);
  const int2* __restrict__ tl = tiles + b * (long)tstride;
  const int nt = ntiles[b];
  const int* __restrict__ er = erow + base;
  const A* __restrict__ ev = eval + base;
  const uint32_t rmask = (1u << rb) - 1;
  A W, L;
  bwd_weights<FUSE>(wl, e, b, n, B, weighted, W, L);
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const int2 ta = tl[t], tz = tl[t + 1];  // (start column, first entry) of this and the next tile
    const int c0 = ta.x, c1 = tz.x, k0 = ta.y, k1 = tz.y;
    if (c1 - c0 == 1 && k1 - k0 > EL) {  // heavy column (block-uniform branch)
      A g = 0;
      for (int k = k0 + tid; k < k1; k += TILE_THREADS) {
        const uint32_t x = (uint32_t)__builtin_nontemporal_load(er + k);
        g += mult[x & rmask] * __builtin_nontemporal_load(ev + k);
      }
      g = wave_sum(g);
      if ((tid & 63) == 0) hred[tid >> 6] = g;
      __syncthreads();
      if (tid == 0) {
        A s = 0;
        for (int i = 0; i < TILE_THREADS / 64; ++i) s += hred[i];
        put_col<FUSE>(coef, fb, c0, s, W, lr, reg, en);
      }
      __syncthreads();
      continue;
    }
    // the thread's columns of the tile (c0 + tid + i·TILE_THREADS, i < TILE_COLS): pointers and
    // coefficients loaded before the gathers, so the column pass after the barrier reads only LDS
    const bool few = c1 - c0 <= TILE_COLS * TILE_THREADS;  // (block-uniform)
    int ca[TILE_COLS], cz[TILE_COLS];
    A cw[TILE_COLS];
    if (few) {
#pragma unroll
      for (int i = 0; i < TILE_COLS; ++i) {
        const int c = c0 + tid + i * TILE_THREADS;
        const int cc = c < c1 ? c : c0;
        ca[i] = cp[cc];
        cz[i] = c < c1 ? cp[cc + 1] : ca[i];
        cw[i] = FUSE ? coef[cc] : (A)0;
      }
    }
    constexpr int TU = sizeof(A) == 8 ? TILE_U / 2 : TILE_U;
    // products into their column-ordered slots: TU entries per thread per step (8; 4 for fp64,
    // which spilled at 8 under the 1024-thread register budget), the next
    // step's entries loaded before this step's multiplier gathers (measured against one step of
    // 32 per thread: 71.0 vs 72.3 µs per round; 8 without the overlap: 71.8)
    uint32_t xx[TU];
    A vv[TU];
    if (k0 < k1) {  // (an empty tile may sit at the end of the array: nothing to load)
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int k = k0 + tid + u * TILE_THREADS;
        const int kk = k < k1 ? k : k0;
        xx[u] = (uint32_t)__builtin_nontemporal_load(er + kk);
        vv[u] = __builtin_nontemporal_load(ev + kk);
      }
    }
    for (int kb = k0 + tid; kb < k1; kb += TU * TILE_THREADS) {
      uint32_t nx[TU];
      A nv[TU];
      const int kn = kb + TU * TILE_THREADS;
      if (kn < k1) {
#pragma unroll
        for (int u = 0; u < TU; ++u) {
          const int k = kn + u * TILE_THREADS;
          const int kk = k < k1 ? k : kn;
          nx[u] = (uint32_t)__builtin_nontemporal_load(er + kk);
          nv[u] = __builtin_nontemporal_load(ev + kk);
        }
      }
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const A p = mult[xx[u] & rmask] * vv[u];
        if (kb + u * TILE_THREADS < k1) prod[xx[u] >> rb] = p;
      }
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        xx[u] = nx[u];
        vv[u] = nv[u];
      }
    }
    if (trace && tid == 0) trace[(long)blockIdx.x * 4 + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    __syncthreads();
    if (trace && tid == 0) trace[(long)blockIdx.x * 4 + 2] = (long long)__builtin_amdgcn_s_memrealtime();
    if (few) {
#pragma unroll
      for (int i = 0; i < TILE_COLS; ++i) {
        const int c = c0 + tid + i * TILE_THREADS;
        A g = 0;
        for (int j = ca[i] - k0; j < cz[i] - k0; ++j) g += prod[j];
        if (c < c1) put_col<FUSE>(coef, fb, c, cw[i], g, W, lr, reg, en);
      }
    } else {
      for (int c = c0 + tid; c < c1; c += TILE_THREADS) {
        const int a = cp[c] - k0, z = cp[c + 1] - k0;
        A g = 0;
        for (int j = a; j < z; ++j) g += prod[j];
        put_col<FUSE>(coef, fb, c, g, W, lr, reg, en);
      }
    }
    __syncthreads();
  }
  bwd_export<FUSE>(fb, d, W, L);
  if (trace && tid == 0) trace[(long)blockIdx.x * 4 + 3] = (long long)__builtin_amdgcn_s_memrealtime();
  if (FUSE) {
    __shared__ int last;
    __syncthreads();
    if (tid == 0)
      last = __hip_atomic_fetch_add(&state[ST_ARRIVE], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             (int)gridDim.x - 1;
    __syncthreads();
    if (last) bwd_finish(state, wl, e, W, max_iter, tol, true);
  }
}

// ------------------------------------------------------------------------------------------
// Single-visit sparse round: column-slice buckets built inside the round (no per-batch transpose)
// ------------------------------------------------------------------------------------------
// The reference's LinearSVC benchmark visits every 100k-row batch once (maxIter 20 over 10M rows:
// SGD.java:263-268), so a column-major copy built per batch (radix passes, ~0.25 ms per 6.4M-entry
// batch) never pays back. Here the fit counts its batches once and a round is two launches over
// the CSR batch as it stands:
//   count    — (once per fit, every batch it visits: grid.y = batch) a block per CG forward blocks
//              of rb rows: their entries per column slice of 2^csb columns (a "bucket"), an LDS
//              histogram written into the bucket-major [bucket][forward block] count matrix;
//   scan     — (likewise) a block per bucket: each forward block's first position inside the
//              bucket and the bucket's total;
//   forward  — a block takes its rb rows: their entries and gathered coefficients in registers,
//              the products summed per row in LDS, loss + multiplier per row; then the entries,
//              sorted by bucket in LDS, are stored as (column in slice, m_row·x) records at their
//              exact bucket positions (no device atomics, deterministic placement);
//   backward — a block takes a chunk of one bucket (contiguous reads), counting-sorts it by column
//              in LDS (integer atomics only) and sums each column's run, then applies the SGD
//              update + regularisation to the slice (1 GPU) or writes its feedback slice (N GPUs);
//              a bucket of several chunks sums them through an accumulator row and its last chunk
//              finishes it.
// A device atomic per ENTRY would run at the scattered-atomic rate (~0.08 TB/s: the 472 µs of
// glm_grad_csr_kernel). The multi-chunk accumulator's float atomics make the last bits depend on
// arrival order: FMLX_DETERMINISTIC=1 keeps the transposed path.
constexpr int BK_NT = 1024;     // threads of the kernels
// scatter: 512-thread blocks, entries staged per piece (LDS: a column, a value and a row id each;
// ≤ 36 KiB, so four blocks share a CU — more independent blocks to overlap each one's chain of
// bookkeeping loads, scans and stores than two 1024-thread ones)
constexpr int SC_NT = 512;
template <typename A>
constexpr int bk_ecap() {
  return sizeof(A) == 8 ? 2048 : 3584;
}
constexpr int BK_NB_MAX = 1024; // buckets

// a bucket entry: one 8-byte store in the scatter, one 8-byte load in the backward (fp64: 16 B)
template <typename A>
struct BkRec {
  uint32_t key;
  A val;
};


struct BktArgs {
  int csb, nb;     // slice bits, buckets = ceil(d / 2^csb)
  int rb;          // forward rows per block
  int chunk;       // backward entries per work item
  int* cntm;       // [slots][nb][fwd blocks] entries per (bucket, forward block)
  int* offm;       // [slots][fwd blocks][nb] each forward block's first record position in each bucket
  int* lofs;       // [slots][fwd blocks][nb] exclusive prefix over buckets of the block's own counts
  int* tot;        // [slots][nb] entries per bucket
  int* bst;        // [slots][nb + 1] bucket starts (exclusive prefix of tot; [nb] = the batch's entries)
  int slots;       // > 0: the counts of batches 0 … slots − 1 were made once for the fit (slot = batch);
                   // 0: count + scan + base run in every round, for its batch (slot 0)
  long mstride;    // elements of one slot of cntm / offm / lofs
  int* done;       // [nb] chunk arrivals of multi-chunk buckets (zero between rounds)
  void* rec;       // [largest batch nnz] BkRec<A>: (column within the slice, m_row · x)
  void* acc;       // [d] zero between rounds: partial slices of multi-chunk buckets
};

__device__ __forceinline__ bool bk_batch(const int* state, long n, long B, long& start, long& end, int& e) {
  if (!round_running(state, e)) return false;
  batch_rows(round_batch(e, n, B), n, B, start, end);
  return true;
}

// the count / offset slot of round e's batch
__device__ __forceinline__ long bk_slot(int e, long n, long B, const BktArgs& k) {
  const long s = k.slots ? (long)(e % ((n + B - 1) / B)) : 0;
  return s < k.slots ? s : (k.slots ? k.slots - 1 : 0);  // (host-guarded; never an out-of-range slot)
}

// count / scan: round e's batch (per-round mode), or batch blockIdx.y (the fit's one-time counts)
__device__ __forceinline__ bool bk_count_batch(const int* state, long n, long B, const BktArgs& k, long& start,
                                               long& end, long& slot) {
  if (k.slots) {
    slot = blockIdx.y;
    start = slot * B;
    end = start + B < n ? start + B : n;
    return start < n;
  }
  int e;
  slot = 0;
  return bk_batch(state, n, B, start, end, e);
}

// count: a block takes CG consecutive forward blocks (their entries are one contiguous range) and
// writes their per-bucket counts into the bucket-major count matrix [slot][bucket][forward block]
// and each one's exclusive prefix over the buckets (its LDS staging offsets) block-major into lofs
constexpr int CG = 8;
__global__ __launch_bounds__(BK_NT) void glm_bkt_count_kernel(const long* __restrict__ indptr,
                                                              const int* __restrict__ idx, long n, long B,
                                                              const int* __restrict__ state, BktArgs k) {
  extern __shared__ int bk_hist[];  // [CG][nb]
  __shared__ long jsub[CG + 1];
  long start, end, slot;
  if (!bk_count_batch(state, n, B, k, start, end, slot)) return;
  const int nfb = (int)((end - start + k.rb - 1) / k.rb);
  const int f0 = blockIdx.x * CG;
  if (f0 >= nfb) return;
  const int ns = nfb - f0 < CG ? nfb - f0 : CG;
  if (threadIdx.x <= ns) {
    const long r = start + (long)(f0 + threadIdx.x) * k.rb;
    jsub[threadIdx.x] = indptr[r < end ? r : end];
  }
  for (int i = threadIdx.x; i < ns * k.nb; i += BK_NT) bk_hist[i] = 0;
  __syncthreads();
  const long j0 = jsub[0], j1 = jsub[ns];
  // sub-block of an entry from its offset in the range (32-bit: a count block's range is short)
  int bnd[CG];
#pragma unroll
  for (int i = 1; i < CG; ++i) bnd[i] = i < ns ? (int)(jsub[i] - j0) : 0x7fffffff;
  auto count = [&](long jj, int c) {
    const int r = (int)(jj - j0);
    int q = 0;
#pragma unroll
    for (int i = 1; i < CG; ++i) q += bnd[i] <= r ? 1 : 0;
    atomicAdd(&bk_hist[q * k.nb + (c >> k.csb)], 1);
  };
  // the column indices as 16-byte vectors over the 4-aligned middle of the range (two vectors in
  // flight per thread: 4× the bytes outstanding of scalar loads), scalar head and tail
  const long a = (j0 + 3) & ~3L, b = j1 & ~3L;
  if (a >= b) {
    for (long j = j0 + threadIdx.x; j < j1; j += BK_NT) count(j, __builtin_nontemporal_load(idx + j));
  } else {
    if (j0 + (long)threadIdx.x < a) count(j0 + threadIdx.x, __builtin_nontemporal_load(idx + j0 + threadIdx.x));
    if (b + (long)threadIdx.x < j1) count(b + threadIdx.x, __builtin_nontemporal_load(idx + b + threadIdx.x));
    typedef int i4_t __attribute__((ext_vector_type(4)));
    const i4_t* v = reinterpret_cast<const i4_t*>(idx + a);
    const long nv = (b - a) >> 2;
    long q = threadIdx.x;
    for (; q + 1 * BK_NT < nv; q += 2 * BK_NT) {
      i4_t c[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) c[t] = __builtin_nontemporal_load(v + q + t * BK_NT);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const long jj = a + 4 * (q + t * BK_NT);
        count(jj, c[t].x);
        count(jj + 1, c[t].y);
        count(jj + 2, c[t].z);
        count(jj + 3, c[t].w);
      }
    }
    for (; q < nv; q += BK_NT) {
      const i4_t c = __builtin_nontemporal_load(v + q);
      const long jj = a + 4 * q;
      count(jj, c.x);
      count(jj + 1, c.y);
      count(jj + 2, c.z);
      count(jj + 3, c.w);
    }
  }
  __syncthreads();
  // (bucket-major: consecutive threads take one bucket's ns consecutive blocks, 32-byte runs)
  int* cm = k.cntm + slot * k.mstride;
  for (int i = threadIdx.x; i < ns * k.nb; i += BK_NT) {
    const int b = i / ns, q = i - b * ns;
    cm[(long)b * nfb + f0 + q] = bk_hist[q * k.nb + b];
  }
  // a wave per forward block: the exclusive prefix of its counts over the buckets (CG ≤ waves)
  const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (w < ns) {
    const int* h = bk_hist + w * k.nb;
    int* out = k.lofs + slot * k.mstride + (long)(f0 + w) * k.nb;
    const int per = (k.nb + 63) >> 6;
    const int q0 = ln * per;
    int sum = 0;
    for (int i = 0; i < per; ++i) sum += q0 + i < k.nb ? h[q0 + i] : 0;
    int run = wave_incl_scan(sum) - sum;
    for (int i = 0; i < per; ++i)
      if (q0 + i < k.nb) {
        const int c = h[q0 + i];
        out[q0 + i] = run;
        run += c;
      }
  }
}
static_assert(CG <= BK_NT / 64, "a wave per forward block of a count block");

// one block per bucket: row b of the (bucket-major) count matrix → each forward block's offset
// inside the bucket (in place) and the bucket's total
__global__ __launch_bounds__(BK_NT) void glm_bkt_scan_kernel(long n, long B, const int* __restrict__ state,
                                                             BktArgs k) {
  __shared__ int tmp[BK_NT / 64];
  long start, end, slot;
  if (!bk_count_batch(state, n, B, k, start, end, slot)) return;
  const int nfb = (int)((end - start + k.rb - 1) / k.rb);
  const int b = blockIdx.x;
  const long row = slot * k.mstride + (long)b * nfb;
  const int total = block_excl_scan_array<BK_NT>(k.cntm + row, k.cntm + row, nfb, tmp);
  if (threadIdx.x == 0) k.tot[slot * k.nb + b] = total;
}

// bucket starts (exclusive prefix of the totals) into bst; every forward block's offsets plus its
// bucket's start, transposed through LDS tiles of TBK buckets × TFB blocks into the block-major
// record positions offm[f][b]: the forward then reads one contiguous row per block
constexpr int TBK = 32, TFB = 64;
__global__ __launch_bounds__(BK_NT) void glm_bkt_base_kernel(long n, long B, const int* __restrict__ state,
                                                             BktArgs k) {
  extern __shared__ int sb[];  // [nb + 1]
  __shared__ int tile[TBK][TFB + 1];
  __shared__ int tmp[BK_NT / 64];
  long start, end, slot;
  if (!bk_count_batch(state, n, B, k, start, end, slot)) return;
  const int nfb = (int)((end - start + k.rb - 1) / k.rb);
  sb[k.nb] = block_excl_scan_array<BK_NT>(k.tot + slot * k.nb, sb, k.nb, tmp);
  __syncthreads();
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i <= k.nb; i += BK_NT) k.bst[slot * (k.nb + 1) + i] = sb[i];
  const int ntf = (nfb + TFB - 1) / TFB;
  const int b0 = (int)(blockIdx.x / ntf) * TBK, f0 = (int)(blockIdx.x % ntf) * TFB;
  const int* cm = k.cntm + slot * k.mstride;
  for (int i = threadIdx.x; i < TBK * TFB; i += BK_NT) {
    const int bb = i / TFB, ff = i - bb * TFB;
    if (b0 + bb < k.nb && f0 + ff < nfb) tile[bb][ff] = cm[(long)(b0 + bb) * nfb + f0 + ff] + sb[b0 + bb];
  }
  __syncthreads();
  int* om = k.offm + slot * k.mstride;
  for (int i = threadIdx.x; i < TBK * TFB; i += BK_NT) {
    const int ff = i / TBK, bb = i - ff * TBK;
    if (b0 + bb < k.nb && f0 + ff < nfb) om[(long)(f0 + ff) * k.nb + b0 + bb] = tile[bb][ff];
  }
}

// forward + bucket writes: a block takes its rb rows (one piece of ≤ ECAP entries in the common
// case, held in registers): the entries and their coefficients are gathered at once, the products
// staged in LDS and summed per row by G-lane groups, a thread per row turns its dot into the loss and
// multiplier, then the entries are sorted by bucket in LDS and stored as (column in slice, m·x)
// records at their exact positions. One read of the batch per round (the separate forward read it
// a second time: 43 + 38 µs of forward + scatter per 100k × 64 batch, profiles/r6/INDEX.md).
// (≤ 64 VGPRs: eight waves per SIMD, so four 512-thread blocks share a CU — the LDS allows four;
// at 70 VGPRs only three fit and the 100k-row batch's 1786 blocks ran in 2.3 waves instead of 1.7)
template <typename A, int G>
__global__ __launch_bounds__(SC_NT) void glm_bkt_fwd_scatter_kernel(
    const long* __restrict__ indptr, const int* __restrict__ idx, const A* __restrict__ val, const A* __restrict__ y,
    const A* __restrict__ wt, const A* __restrict__ coef, long n, long B, int loss, const int* __restrict__ state,
    A* __restrict__ wl, BktArgs k, long long* __restrict__ trace, long trace_blocks) {
  constexpr int BK_ECAP = bk_ecap<A>();
  constexpr int BK_EPT = BK_ECAP / SC_NT;
  constexpr int NGRP = SC_NT / G;
  extern __shared__ __align__(16) unsigned char bk_smem[];
  // [nb] base | ph | pofs, then rp[rb + 1], mrow[rb], scol[ECAP], sval[ECAP], srow[ECAP]
  int* base = reinterpret_cast<int*>(bk_smem);
  int* ph = base + k.nb;
  int* pofs = ph + k.nb;
  int* rp = pofs + k.nb;
  A* mrow = reinterpret_cast<A*>(bk_smem + (((3 * (long)k.nb + k.rb + 1) * 4 + 15) & ~15L));
  int* scol = reinterpret_cast<int*>(mrow + k.rb);
  A* sval = reinterpret_cast<A*>(scol + BK_ECAP);
  uint16_t* srow = reinterpret_cast<uint16_t*>(sval + BK_ECAP);
  __shared__ int tmp[SC_NT / 64];
  __shared__ A red[2][SC_NT / 64];
  long start, end;
  int e;
  if (!bk_batch(state, n, B, start, end, e)) return;
  const long r0 = start + (long)blockIdx.x * k.rb;
  if (r0 >= end) return;  // (the grid covers the largest batch)
  // diagnostics (fmlx_glm_bkt_set_trace): phase stamps of each block, 100 MHz
  long long* tb = trace && blockIdx.x < trace_blocks ? trace + (long)blockIdx.x * 8 : nullptr;
#define BK_STAMP(p) \
  if (tb && threadIdx.x == 0) tb[p] = (long long)__builtin_amdgcn_s_memrealtime();
  BK_STAMP(0)
  const int nr = end - r0 < k.rb ? (int)(end - r0) : k.rb;
  const long jb = indptr[r0];
  const long je = indptr[r0 + nr];
  const int tid = threadIdx.x;
  const int csb = k.csb;
  const uint32_t mask = (1u << csb) - 1;
  BkRec<A>* brec = reinterpret_cast<BkRec<A>*>(k.rec);
  const int E = (int)(je - jb);
  const bool one = E <= BK_ECAP;
  // one piece (the common case): the block's entries are requested first, with the bookkeeping
  // loads behind them; their coefficients (an L2-resident gather) follow as soon as they land
  int col[BK_EPT];
  A pv[BK_EPT];
  if (one) {
#pragma unroll
    for (int u = 0; u < BK_EPT; ++u) {
      const int t = tid + u * SC_NT;
      col[u] = t < E ? __builtin_nontemporal_load(idx + jb + t) : 0;
      pv[u] = t < E ? __builtin_nontemporal_load(val + jb + t) : (A)0;
    }
  }
  // this thread's row (its loss below): label and weight
  A yv = 0, wv = 1;
  if (tid < nr) {
    yv = y[r0 + tid];
    if (wt) wv = wt[r0 + tid];
  }
  // this block's first record position in every bucket and its LDS staging offsets (one
  // contiguous row each, made once per fit: count / scan / base kernels)
  const long mo = bk_slot(e, n, B, k) * k.mstride + (long)blockIdx.x * k.nb;
  for (int i = tid; i < k.nb; i += SC_NT) {
    base[i] = k.offm[mo + i];
    const int lo = k.lofs[mo + i];
    pofs[i] = lo;
    ph[i] = lo;
  }
  for (int i = tid; i <= nr; i += SC_NT) rp[i] = (int)(indptr[r0 + i] - jb);
  BK_STAMP(6)  // (wave 0's entries and bookkeeping rows have landed)
  if (one) {
    // the products into the staging values (free until the records are staged)
#pragma unroll
    for (int u = 0; u < BK_EPT; ++u) {
      const int t = tid + u * SC_NT;
      if (t < E) sval[t] = pv[u] * coef[col[u]];
    }
  }
  __syncthreads();
  BK_STAMP(1)
  const int lane = tid & (G - 1), grp = tid / G;
  if (one) {
    // every entry's row id into LDS (a thread per row; read by the staging after two barriers)
    for (int q = tid; q < nr; q += SC_NT)
      for (int j = rp[q]; j < rp[q + 1]; ++j) srow[j] = (uint16_t)q;
    BK_STAMP(2)
    // row dots: a G-lane group per row over its staged products
    for (int q = grp; q < nr; q += NGRP) {
      A s = 0;
      for (int j = rp[q] + lane; j < rp[q + 1]; j += G) s += sval[j];
      s = group_sum<G>(s);
      if (lane == 0) mrow[q] = s;
    }
  } else {
    // (rows of more than ECAP entries per block) row dots straight from the batch
    for (int q = grp; q < nr; q += NGRP) {
      A s = 0;
      for (int j = rp[q] + lane; j < rp[q + 1]; j += G) s += val[jb + j] * coef[idx[jb + j]];
      s = group_sum<G>(s);
      if (lane == 0) mrow[q] = s;
    }
  }
  __syncthreads();
  // loss + multiplier, a thread per row; Σweight / Σloss of the block into a parity slot of `wl`
  A wsum = 0, lsum = 0;
  for (int q = tid; q < nr; q += SC_NT) {
    const A yy = q == tid ? yv : y[r0 + q];
    const A ww = q == tid ? wv : (wt ? wt[r0 + q] : (A)1);
    A l, m;
    loss_and_mult(loss, mrow[q], yy, ww, l, m);
    mrow[q] = m;
    wsum += ww;
    lsum += l;
  }
  fwd_sums_stage(wave_sum(wsum), wave_sum(lsum), red);
  BK_STAMP(3)
  fwd_sums_add(red, SC_NT / 64, wl, e, (int)blockIdx.x);
  if (one) {
    // a returning integer atomic on its bucket's cursor gives each entry its staging slot (the
    // products' staging values were consumed by the row dots before the last barrier)
#pragma unroll
    for (int u = 0; u < BK_EPT; ++u) {
      const int t = tid + u * SC_NT;
      if (t < E) {
        const int sl = atomicAdd(&ph[col[u] >> csb], 1);
        scol[sl] = col[u];
        sval[sl] = pv[u] * mrow[srow[t]];
      }
    }
    __syncthreads();
    BK_STAMP(4)
    for (int t = tid; t < E; t += SC_NT) {
      const int c = scol[t];
      const int bk = c >> csb;
      const long dst = (long)base[bk] + (t - pofs[bk]);
      brec[dst] = BkRec<A>{(uint32_t)c & mask, sval[t]};
    }
    BK_STAMP(5)
    return;
  }
#undef BK_STAMP
  // several pieces (rows of more than ECAP entries per block): per piece, pass 1 draws each entry's
  // rank in its bucket (kept in srow), pass 2 re-reads the entry (L2) and stages it at its slot —
  // no per-thread arrays across the barriers, so this rare path does not set the kernel's registers
  for (int p0 = 0; p0 < E; p0 += BK_ECAP) {
    const int pe = E - p0 < BK_ECAP ? E - p0 : BK_ECAP;
    for (int i = tid; i < k.nb; i += SC_NT) ph[i] = 0;
    __syncthreads();
    for (int t = tid; t < pe; t += SC_NT) srow[t] = (uint16_t)atomicAdd(&ph[idx[jb + p0 + t] >> csb], 1);
    __syncthreads();
    block_excl_scan_array<SC_NT>(ph, pofs, k.nb, tmp);
    __syncthreads();
    for (int t = tid; t < pe; t += SC_NT) {
      const int j = p0 + t;
      int lo = 0, hi = nr;  // the entry's row: rp[lo] <= j < rp[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp[mid] <= j) lo = mid; else hi = mid;
      }
      const int c = idx[jb + j];
      const int sl = pofs[c >> csb] + srow[t];
      scol[sl] = c;
      sval[sl] = val[jb + j] * mrow[lo];
    }
    __syncthreads();
    for (int t = tid; t < pe; t += SC_NT) {
      const int c = scol[t];
      const int bk = c >> csb;
      const long dst = (long)base[bk] + (t - pofs[bk]);
      brec[dst] = BkRec<A>{(uint32_t)c & mask, sval[t]};
    }
    __syncthreads();
    for (int i = tid; i < k.nb; i += SC_NT) base[i] += ph[i];
    // (the next piece's first barrier orders these updates before their reads)
  }
}

// backward LDS budget: the chunk's values in column order + one counter per slice column
template <typename A>
constexpr int bk_chunk() {
  return sizeof(A) == 8 ? 16384 : 32768;
}

template <typename A, bool FUSE>
__global__ __launch_bounds__(BK_NT) void glm_bkt_bwd_kernel(const long* __restrict__ indptr, long n, int d, long B,
                                                            int* __restrict__ state, A* __restrict__ wl,
                                                            A* __restrict__ fb, A* __restrict__ coef, int max_iter,
                                                            A tol, A lr, A reg, A en, int weighted, BktArgs k) {
  // LDS float atomics run ~7x slower than integer ones on gfx950 (scripts/micro_lds_atomic.hip:
  // 6.4M ds_add_f32 35 µs, ds_add_u32 5 µs), so a chunk is not summed by float atomics into a
  // slab: it is counting-sorted by column in LDS (integer histogram, scan, returning integer
  // atomics for the slots), and each column then sums its slots — no float atomics at all.
  extern __shared__ __align__(16) unsigned char bk_smem[];
  A* sv = reinterpret_cast<A*>(bk_smem);                        // [chunk] values, column-sorted
  int* cc = reinterpret_cast<int*>(sv + k.chunk);               // [2^csb + 1] column counts → starts
  int* bst = cc + (1 << k.csb) + 1;                              // [nb + 1] bucket starts
  int* iofs = bst + k.nb + 1;                                    // [nb + 1] first item of each bucket
  int* nch = iofs + k.nb + 1;                                    // [nb] items of each bucket
  __shared__ int tmp[BK_NT / 64];
  __shared__ int sflag;
  int e;
  if (!bwd_begin<FUSE>(state, wl, e)) return;
  const long b = round_batch(e, n, B);
  A W, L;
  bwd_weights<FUSE>(wl, e, b, n, B, weighted, W, L);
  // bucket starts, then the work items: chunks of `chunk` entries of each bucket (at least one per
  // bucket: every column is updated, regularisation included)
  const long sl = bk_slot(e, n, B, k);
  const int* tot = k.tot + sl * k.nb;
  for (int i = threadIdx.x; i <= k.nb; i += BK_NT) bst[i] = k.bst[sl * (k.nb + 1) + i];
  for (int i = threadIdx.x; i < k.nb; i += BK_NT) {
    const int len = tot[i];
    nch[i] = len > k.chunk ? (len + k.chunk - 1) / k.chunk : 1;
  }
  __syncthreads();
  iofs[k.nb] = block_excl_scan_array<BK_NT>(nch, iofs, k.nb, tmp);
  __syncthreads();
  const int T = iofs[k.nb];
  const int CS = 1 << k.csb;  // ≤ 4 · BK_NT (host-checked csb ≤ 12)
  const BkRec<A>* __restrict__ brec = reinterpret_cast<const BkRec<A>*>(k.rec);
  A* acc = reinterpret_cast<A*>(k.acc);
  constexpr int RPT = bk_chunk<A>() / BK_NT;  // records of a chunk per thread, held in registers
  for (int it = blockIdx.x; it < T; it += gridDim.x) {
    int lo = 0, hi = k.nb;  // iofs[lo] <= it < iofs[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (iofs[mid] <= it) lo = mid; else hi = mid;
    }
    const int bk = lo, nc = nch[bk], ch = it - iofs[bk];
    for (int c = threadIdx.x; c <= CS; c += BK_NT) cc[c] = 0;
    // the slice's coefficients this thread updates, requested now (their latency runs under the
    // chunk's loads and the LDS sort); CS / BK_NT ≤ 4 columns per thread
    const long c0 = (long)bk << k.csb;
    const int cols = d - c0 < CS ? (int)(d - c0) : CS;
    A wold[4];
    if (FUSE && nc == 1) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = (int)threadIdx.x + u * BK_NT;
        wold[u] = c < cols ? coef[c0 + c] : (A)0;
      }
    }
    const int k0 = bst[bk] + ch * k.chunk;
    const int be = bst[bk + 1];
    const int k1 = k0 + k.chunk < be ? k0 + k.chunk : be;
    // the whole chunk into registers (one 8-byte record load per entry, all in flight at once)
    uint32_t kk[RPT];
    A vv[RPT];
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int q = k0 + (int)threadIdx.x + u * BK_NT;
      const BkRec<A> r = brec[q < k1 ? q : k0];
      kk[u] = r.key;
      vv[u] = r.val;
    }
    __syncthreads();  // (the counters are zeroed)
    // pass 1: column histogram of the chunk
#pragma unroll
    for (int u = 0; u < RPT; ++u)
      if (k0 + (int)threadIdx.x + u * BK_NT < k1) atomicAdd(&cc[kk[u]], 1);
    __syncthreads();
    // column starts (exclusive scan of the counts; cc[c] becomes the column's slot cursor and the
    // counts are recovered from the next column's start after the scatter)
    cc[CS] = block_excl_scan_array<BK_NT>(cc, cc, CS, tmp);
    __syncthreads();
    // pass 2: values into their column's slots
#pragma unroll
    for (int u = 0; u < RPT; ++u)
      if (k0 + (int)threadIdx.x + u * BK_NT < k1) sv[atomicAdd(&cc[kk[u]], 1)] = vv[u];
    __syncthreads();
    // column c's slots: [end of c − 1, end of c) (cc[c] is now the end of column c)
    if (nc == 1) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = (int)threadIdx.x + u * BK_NT;
        if (c >= cols) break;
        const int j0 = c ? cc[c - 1] : 0, j1 = cc[c];
        A g = 0;
        for (int j = j0; j < j1; ++j) g += sv[j];
        put_col<FUSE>(coef, fb, c0 + c, wold[u], g, W, lr, reg, en);
      }
    } else {
      for (int c = threadIdx.x; c < cols; c += BK_NT) {
        const int j0 = c ? cc[c - 1] : 0, j1 = cc[c];
        A g = 0;
        for (int j = j0; j < j1; ++j) g += sv[j];
        atomicAdd(&acc[c0 + c], g);
      }
      if (arrive_last(&k.done[bk], nc, &sflag)) {
        for (int c = threadIdx.x; c < cols; c += BK_NT) {
          const A g = __hip_atomic_exchange(&acc[c0 + c], (A)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          put_col<FUSE>(coef, fb, c0 + c, g, W, lr, reg, en);
        }
        if (threadIdx.x == 0) st_agent(&k.done[bk], 0);
      }
    }
    __syncthreads();
  }
  bwd_export<FUSE>(fb, d, W, L);
  if (FUSE) {
    // two-level arrival (a single counter serialises every block's ticket, ~11 ns each): the last
    // block of each group of blocks ≡ g (mod 8) draws a top ticket; the last top one finishes
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
      int* grp = k.done + k.nb;  // [8] group tickets, [8] the top ticket (zero between rounds)
      const int g = blockIdx.x & 7;
      const int gs = ((int)gridDim.x - g + 7) >> 3;  // blocks of group g
      const int ng = gridDim.x < 8 ? (int)gridDim.x : 8;
      bool top = __hip_atomic_fetch_add(&grp[g], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gs - 1;
      if (top) {
        st_agent(&grp[g], 0);  // (every block of the group has drawn; re-armed for the next round)
        top = __hip_atomic_fetch_add(&grp[8], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ng - 1;
        if (top) st_agent(&grp[8], 0);
      }
      last = top;
    }
    __syncthreads();
    if (last) bwd_finish(state, wl, e, W, max_iter, tol, false);
  }
}

// the launch variants' visitors (the accumulator type and the flags: with_acc / with_bool,
// dispatch.h): f is called with the lane-group size as a compile-time constant; −1 for a group
// size no kernel has
template <typename F>
int with_group(int G, F&& f) {
  return with_value<4, 8, 16, 32, 64>(G, f);
}

}  // namespace

static long long* g_sparse_trace = nullptr;  // per-block timestamps of the tiled backward (diagnostics)
FMLX_API void fmlx_glm_sparse_set_trace(void* trace) { g_sparse_trace = (long long*)trace; }
// per-block phase stamps of the bucket forward (8 int64 per block, blocks < `blocks`), or off
static long long* g_bkt_trace = nullptr;
static long g_bkt_trace_blocks = 0;
FMLX_API void fmlx_glm_bkt_set_trace(void* trace, long blocks) {
  g_bkt_trace = blocks > 0 ? (long long*)trace : nullptr;
  g_bkt_trace_blocks = blocks > 0 ? blocks : 0;
}

FMLX_API int fmlx_glm_grad_csr(int acc_f64, const long* indptr, const int* idx, const void* val, const void* y,
                               const void* wt, const void* coef, long n, int d, long B, int loss, const int* state,
                               void* grad, void* stream) {
  long waves = B < n ? B : n;
  int blocks = (int)((waves + 3) / 4);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return with_acc(acc_f64, [&](auto acc) {
    typedef decltype(acc) A;
    hipLaunchKernelGGL(glm_grad_csr_kernel<A>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, indptr, idx,
                       (const A*)val, (const A*)y, (const A*)wt, (const A*)coef, n, d, B, loss, state, (A*)grad);
    return (int)hipGetLastError();
  });
}

static int g_csc_fwd_cap = 65535, g_csc_bwd_cap = 1024, g_csc_tile_cap = 0;  // 0: CUs × tile blocks per CU

FMLX_API void fmlx_glm_set_csc_tuning(int fwd_cap, int bwd_cap) {
  g_csc_fwd_cap = fwd_cap > 0 ? fwd_cap : 65535;
  g_csc_bwd_cap = bwd_cap > 0 ? bwd_cap : 1024;
  g_csc_tile_cap = bwd_cap > 0 ? bwd_cap : 0;
}

// what both round entry points take: the CSR partition, the model and the round's parameters
struct SparseRound {
  const long* indptr;
  const int* idx;
  const void *val, *y, *wt;
  void* coef;
  long n;
  int d;
  long B;
  int loss;
  int* state;
  void *wl, *fb;
  int fuse, max_iter;
  double tol, lr, reg, en;
};

// tiled backward: the column tiles of the batches (BatchCsc.tiles) and the packing of erow
// forward cells in XCD-aware order (default; fmlx_glm_set_cell_xcd(0): launch order) — 63.5 → 61.4 µs
// per SVC round, profiles/r5/svc_cell_forward_ab.jsonl
static int g_cell_xcd = 1;
struct CscTiles {
  const int2* tiles;  // [P][tstride] (start column, first entry) per tile (nullptr: untiled layout)
  const int* ntiles;  // int32 [P]
  int tstride, rb, EL, ET;  // EL: heavy-column threshold (entries)
  // row-block × column-split cells of the forward (cent == nullptr: the one-row-per-group forward)
  const uint32_t* cent;
  const void* cval;
  const int* roff;  // [P][rstride] first entry of every (cell, row): cell·2^CELL_RBB + row
  int rstride, rbb, S, CS, cb, cells;  // cells: grid (cells of the largest batch); rows per block 2^rbb
  int cmax;         // entries of the largest cell (its LDS slots)
  void* partial;    // [cells][2^CELL_RBB] row partials
  int* cnt;         // [row blocks] arrival tickets (zeroed once, re-armed by the finishers)
};
FMLX_API int fmlx_glm_wl_elems() { return 2 * WL_SLOTS * WL_STRIDE; }

// the transposed round's two launches: forward (cells, or a G-lane group per row), backward (tiled or not)
template <typename A, int G>
static int launch_csc_round(const SparseRound& r, void* mult, const int* colptr, const int* erow, const void* eval,
                            const CscTiles& ti, hipStream_t s) {
  if (ti.cent != nullptr) {
    hipLaunchKernelGGL(glm_csr_cell_fwd_kernel<A>, dim3(ti.cells), dim3(CELL_THREADS), (size_t)ti.cmax * sizeof(A),
                       s, r.indptr, ti.cent, (const A*)ti.cval, ti.roff, (long)ti.rstride, ti.rbb, ti.S, ti.CS, ti.cb,
                       (const A*)r.y, (const A*)r.wt, (const A*)r.coef, r.n, r.B, r.loss, r.state, (A*)mult, (A*)r.wl,
                       (A*)ti.partial, ti.cnt, g_cell_xcd);
  } else {
    const long groups = r.B < r.n ? r.B : r.n;
    long fb_blocks = (groups * G + 255) / 256;  // one row per lane group: the batch in one pass
    if (fb_blocks > g_csc_fwd_cap) fb_blocks = g_csc_fwd_cap;
    if (fb_blocks < 1) fb_blocks = 1;
    hipLaunchKernelGGL((glm_csr_fwd_kernel<A, G>), dim3((int)fb_blocks), dim3(256), 0, s, r.indptr, r.idx,
                       (const A*)r.val, (const A*)r.y, (const A*)r.wt, (const A*)r.coef, r.n, r.B, r.loss, r.state,
                       (A*)mult, (A*)r.wl);
  }
  const int weighted = r.wt != nullptr;
  return with_bool(r.fuse, [&](auto fuse) {
    constexpr bool F = decltype(fuse)::value;
    if (ti.tiles != nullptr) {
      const size_t lds = (size_t)ti.ET * sizeof(A);
      int per_cu = (int)(LDS_PER_CU / (lds + 2048));
      per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);  // ≤ 32 waves per CU at 1024 threads
      int tb = g_csc_tile_cap > 0 ? g_csc_tile_cap : NUM_CU * per_cu;
      if (tb > ti.tstride) tb = ti.tstride;
      hipLaunchKernelGGL((glm_csc_tile_bwd_kernel<A, F>), dim3(tb), dim3(TILE_THREADS), lds, s, r.indptr, colptr,
                         ti.tiles, ti.ntiles, ti.tstride, erow, (const A*)eval, (const A*)mult, r.n, r.d, r.B, ti.rb,
                         ti.EL, r.state, (A*)r.wl, (A*)r.fb, (A*)r.coef, r.max_iter, (A)r.tol, (A)r.lr, (A)r.reg,
                         (A)r.en, weighted, g_sparse_trace);
    } else {
      int bb = (r.d + 255) / 256;  // grid-strided: each block takes the arrival ticket once
      if (bb > g_csc_bwd_cap) bb = g_csc_bwd_cap;
      hipLaunchKernelGGL((glm_csc_bwd_kernel<A, F>), dim3(bb), dim3(256), 0, s, r.indptr, colptr, erow,
                         (const A*)eval, (const A*)mult, r.n, r.d, r.B, r.state, (A*)r.wl, (A*)r.fb, (A*)r.coef,
                         r.max_iter, (A)r.tol, (A)r.lr, (A)r.reg, (A)r.en, weighted);
    }
    return (int)hipGetLastError();
  });
}

FMLX_API void fmlx_glm_set_cell_xcd(int on) { g_cell_xcd = on != 0; }

// One sparse SGD round through the per-batch transpose (see glm_csc_bwd_kernel). fuse=1: the
// backward applies the update + termination (1 GPU); fuse=0: it writes fb[d+2] for the
// all-reduce and fmlx_glm_update follows.
FMLX_API int fmlx_glm_csc_round(int acc_f64, int G, const long* indptr, const int* idx, const void* val,
                                const void* y, const void* wt, void* coef, long n, int d, long B, int loss, int* state,
                                void* mult, void* wl, const int* colptr, const int* erow, const void* eval, void* fb,
                                int fuse, int max_iter, double tol, double lr, double reg, double en,
                                const int* tiles, const int* ntiles, int tstride, int rb, int EL, int ET,
                                const uint32_t* cent, const void* cval, const int* roff, int rstride, int rbb, int S,
                                int CS, int cb, int cells, int cmax, void* partial, int* ccnt, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0 || B <= 0) return -2;
  const CscTiles ti{reinterpret_cast<const int2*>(tiles), ntiles, tstride, rb, EL, ET, cent, cval, roff, rstride,
                    rbb, S, CS, cb, cells, cmax, partial, ccnt};
  if (cent != nullptr) {
    // (cell ids, packed entries and the row blocks of the largest batch: host-checked sizes)
    const long lds = (long)cmax * (acc_f64 ? 8 : 4);
    if (cval == nullptr || roff == nullptr || partial == nullptr || ccnt == nullptr || S < 1 || CS < 1 || cb < 1 ||
        cb >= 32 || rbb < 1 || rbb > CELL_RBB_MAX || cells < 1 || (long)rstride < ((long)cells << rbb) + 1 ||
        (long)CS * S < d || cmax < 0 ||
        (long)cmax > (1L << (32 - cb)) || lds > 150 * 1024)  // (64-bit: cb = 1 allows 2^31 ranks)
      return -5;
  }
  if (tiles != nullptr) {
    const size_t esz = acc_f64 ? 8 : 4;
    // the packed erow (row | slot << rb) and the LDS slot array of a light tile (< ET entries)
    if (rb < 1 || ET < 2 || EL < 1 || EL >= ET || tstride < 2 || (size_t)ET * esz > (size_t)LDS_PER_CU - 1024) return -3;
    if (((long)ET - 1) >> (32 - rb) != 0 || (B - 1) >> rb != 0) return -4;
  }
  const SparseRound r{indptr, idx, val, y, wt, coef, n, d, B, loss, state, wl, fb, fuse, max_iter, tol, lr, reg, en};
  return with_acc(acc_f64, [&](auto acc) {
    return with_group(G, [&](auto g) {
      return launch_csc_round<decltype(acc), decltype(g)::value>(r, mult, colptr, erow, eval, ti, s);
    });
  });
}

FMLX_API int fmlx_glm_csr_predict(int acc_f64, const long* indptr, const int* idx, const void* val, const void* coef,
                                  long n, double* dots, void* stream) {
  if (n == 0) return 0;
  int blocks = (int)((n + 3) / 4);
  if (blocks > 4096) blocks = 4096;
  return with_acc(acc_f64, [&](auto acc) {
    typedef decltype(acc) A;
    hipLaunchKernelGGL(glm_csr_predict_kernel<A>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, indptr, idx,
                       (const A*)val, (const A*)coef, n, dots);
    return (int)hipGetLastError();
  });
}

// ---- single-visit bucket round (glm_bkt_*) ----
FMLX_API int fmlx_glm_bkt_limits(int* out) {
  out[0] = BK_NT;
  out[1] = bk_ecap<float>();
  out[2] = BK_NB_MAX;
  out[3] = bk_ecap<double>();
  out[4] = bk_chunk<float>();
  out[5] = bk_chunk<double>();
  out[6] = (int)sizeof(BkRec<float>);
  out[7] = (int)sizeof(BkRec<double>);
  return 0;
}

static int bkt_base_blocks(long fblocks, int nb) {
  return (int)(((fblocks + TFB - 1) / TFB) * ((nb + TBK - 1) / TBK));
}

static size_t bkt_fwd_lds(const BktArgs& k, size_t es) {
  return (((3 * (size_t)k.nb + k.rb + 1) * 4 + 15) & ~(size_t)15) + (size_t)k.rb * es +
         (size_t)(es == 8 ? bk_ecap<double>() : bk_ecap<float>()) * (4 + es + 2);
}

// the backward's LDS: the chunk's values, a counter per slice column (+ 1), bst / iofs [nb + 1], nch [nb]
static size_t bkt_bwd_lds(const BktArgs& k, size_t es) {
  return (size_t)k.chunk * es + (((size_t)1 << k.csb) + 1 + 3 * (size_t)k.nb + 2) * 4;
}

// the bucket round's launches: count + scan + base of the round's batch unless the fit counted its
// batches once (k.slots), forward + scatter, backward
template <typename A, int G>
static int launch_bkt_round(const SparseRound& r, const BktArgs& k, int bwd_blocks, hipStream_t s) {
  const long rows = r.B < r.n ? r.B : r.n;
  const int fblocks = (int)((rows + k.rb - 1) / k.rb);
  if (!k.slots) {
    hipLaunchKernelGGL(glm_bkt_count_kernel, dim3((fblocks + CG - 1) / CG), dim3(BK_NT), (size_t)CG * k.nb * 4, s,
                       r.indptr, r.idx, r.n, r.B, r.state, k);
    hipLaunchKernelGGL(glm_bkt_scan_kernel, dim3(k.nb), dim3(BK_NT), 0, s, r.n, r.B, r.state, k);
    hipLaunchKernelGGL(glm_bkt_base_kernel, dim3(bkt_base_blocks(fblocks, k.nb)), dim3(BK_NT),
                       (size_t)(k.nb + 1) * 4, s, r.n, r.B, r.state, k);
  }
  hipLaunchKernelGGL((glm_bkt_fwd_scatter_kernel<A, G>), dim3(fblocks), dim3(SC_NT), bkt_fwd_lds(k, sizeof(A)), s,
                     r.indptr, r.idx, (const A*)r.val, (const A*)r.y, (const A*)r.wt, (const A*)r.coef, r.n, r.B,
                     r.loss, r.state, (A*)r.wl, k, g_bkt_trace, g_bkt_trace_blocks);
  const int weighted = r.wt != nullptr;
  return with_bool(r.fuse, [&](auto fuse) {
    hipLaunchKernelGGL((glm_bkt_bwd_kernel<A, decltype(fuse)::value>), dim3(bwd_blocks), dim3(BK_NT),
                       bkt_bwd_lds(k, sizeof(A)), s, r.indptr, r.n, r.d, r.B, r.state, (A*)r.wl, (A*)r.fb, (A*)r.coef,
                       r.max_iter, (A)r.tol, (A)r.lr, (A)r.reg, (A)r.en, weighted, k);
    return (int)hipGetLastError();
  });
}

// The fit's one-time counts: count + scan of batches 0 … slots − 1 of the partition in two launches
// (grid.y = batch), before its first round; the rounds then run forward + scatter + backward only.
FMLX_API int fmlx_glm_bkt_count_all(const long* indptr, const int* idx, long n, long B, int csb, int nb, int rb,
                                    int* cntm, int* offm, int* lofs, int* tot, int* bst, int slots, long mstride,
                                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0 || B <= 0 || slots < 1 || nb < 1 || nb > BK_NB_MAX || rb < 1) return -2;
  const long rows = B < n ? B : n;
  const long fblocks = (rows + rb - 1) / rb;
  if (mstride < fblocks * nb || (long)slots * B >= n + B) return -3;
  const BktArgs k{csb, nb, rb, 0, cntm, offm, lofs, tot, bst, slots, mstride, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(glm_bkt_count_kernel, dim3((int)((fblocks + CG - 1) / CG), slots), dim3(BK_NT),
                     (size_t)CG * nb * 4, s, indptr, idx, n, B, (const int*)nullptr, k);
  hipLaunchKernelGGL(glm_bkt_scan_kernel, dim3(nb, slots), dim3(BK_NT), 0, s, n, B, (const int*)nullptr, k);
  hipLaunchKernelGGL(glm_bkt_base_kernel, dim3(bkt_base_blocks(fblocks, nb), slots), dim3(BK_NT),
                     (size_t)(nb + 1) * 4, s, n, B, (const int*)nullptr, k);
  return (int)hipGetLastError();
}

// One sparse SGD round through column-slice buckets (see glm_bkt_count_kernel …). fuse=1: the
// backward applies the update + termination (1 GPU); fuse=0: it writes fb[d+2] for the
// all-reduce and fmlx_glm_update follows. Host-checked: key/val hold the largest batch's entries,
// cntm/offm hold [ceil(B / rb)][nb], acc[d] and done[nb] are zero, tot[nb] exists.
FMLX_API int fmlx_glm_bkt_round(int acc_f64, int G, const long* indptr, const int* idx, const void* val,
                                const void* y, const void* wt, void* coef, long n, int d, long B, int loss, int* state,
                                void* wl, void* fb, int fuse, int max_iter, double tol, double lr, double reg,
                                double en, int csb, int rb, int chunk, int* cntm, int* offm, int* lofs, int* tot,
                                int* bst, int slots, long mstride, int* done, void* rec, void* acc, int bwd_blocks,
                                void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0 || B <= 0 || d <= 0) return -2;
  const size_t es = acc_f64 ? 8 : 4;
  if (csb < 1 || csb > 16 || ((size_t)es << csb) > 64 * 1024) return -3;
  const long nb = ((long)d + (1L << csb) - 1) >> csb;
  const long rows = B < n ? B : n;
  const long fblocks = (rows + rb - 1) / rb;
  if (nb > BK_NB_MAX || rb < 1 || rb > 4096 || chunk < BK_NT || bwd_blocks < 1)
    return -4;
  if (chunk > (acc_f64 ? bk_chunk<double>() : bk_chunk<float>()) || csb > 12) return -6;
  const BktArgs k{csb, (int)nb, rb, chunk, cntm, offm, lofs, tot, bst, slots, mstride, done, rec, acc};
  if (bkt_bwd_lds(k, es) > (size_t)LDS_PER_CU) return -7;
  if (slots < 0 || mstride < fblocks * nb) return -8;
  if (bkt_fwd_lds(k, es) > (size_t)LDS_PER_CU / 2) return -5;
  const SparseRound r{indptr, idx, val, y, wt, coef, n, d, B, loss, state, wl, fb, fuse, max_iter, tol, lr, reg, en};
  return with_acc(acc_f64, [&](auto a) {
    return with_group(G, [&](auto g) {
      return launch_bkt_round<decltype(a), decltype(g)::value>(r, k, bwd_blocks, s);
    });
  });
}

// One dry launch of every bucket-round and row-group forward kernel (all variants) on a round state
// whose running flags are 0, so each exits at its first check: the first launch of a kernel symbol
// pays a one-time runtime cost (argument layout, dispatch set-up), which then falls at library load
// instead of inside the first fit (the reference's totalTimeMs is a cold job).
FMLX_API int fmlx_glm_sparse_warm(void* stream) {
  hipStream_t s = (hipStream_t)stream;
  // [state | 4 KiB scratch | the Σw/Σloss slots the backward re-arms before its running check]
  constexpr size_t WARM_BYTES = 8192 + 2 * WL_SLOTS * WL_STRIDE * sizeof(double);
  static void* dstate = nullptr;
  if (dstate == nullptr) {
    if (hipMalloc(&dstate, WARM_BYTES) != hipSuccess) return -1;
  }
  if (hipMemsetAsync(dstate, 0, WARM_BYTES, s) != hipSuccess) return -2;
  int* st = (int*)dstate;
  void* scratch = (char*)dstate + 4096;
  void* wls = (char*)dstate + 8192;
  const long* ip = (const long*)scratch;
  const int* ix = (const int*)scratch;
  int* si = (int*)scratch;
  BktArgs k{12, 1, 1, BK_NT, si, si, si, si, si, 0, 1, si, scratch, scratch};
  hipLaunchKernelGGL(glm_bkt_count_kernel, dim3(1), dim3(BK_NT), (size_t)CG * 4, s, ip, ix, 1L, 1L, (const int*)st, k);
  hipLaunchKernelGGL(glm_bkt_scan_kernel, dim3(1), dim3(BK_NT), 0, s, 1L, 1L, (const int*)st, k);
  hipLaunchKernelGGL(glm_bkt_base_kernel, dim3(1), dim3(BK_NT), 8, s, 1L, 1L, (const int*)st, k);
  for (int f64 = 0; f64 < 2; ++f64)
    with_acc(f64, [&](auto acc) {
      typedef decltype(acc) A;
      for (int G = 4; G <= 64; G *= 2)
        with_group(G, [&](auto g) {
          hipLaunchKernelGGL((glm_csr_fwd_kernel<A, decltype(g)::value>), dim3(1), dim3(256), 0, s, ip, ix,
                             (const A*)scratch, (const A*)scratch, (const A*)nullptr, (const A*)scratch, 1L, 1L, 1,
                             (const int*)st, (A*)scratch, (A*)scratch);
          hipLaunchKernelGGL((glm_bkt_fwd_scatter_kernel<A, decltype(g)::value>), dim3(1), dim3(SC_NT), 4096, s, ip,
                             ix, (const A*)scratch, (const A*)scratch, (const A*)nullptr, (const A*)scratch, 1L, 1L, 1,
                             (const int*)st, (A*)wls, k, (long long*)nullptr, 0L);
          return 0;
        });
      for (int fuse = 0; fuse < 2; ++fuse)
        with_bool(fuse, [&](auto f) {
          hipLaunchKernelGGL((glm_bkt_bwd_kernel<A, decltype(f)::value>), dim3(1), dim3(BK_NT), 1024, s, ip, 1L, 1, 1L,
                             st, (A*)wls, (A*)scratch, (A*)scratch, 1, (A)0, (A)0, (A)0, (A)0, 0, k);
          return 0;
        });
      return 0;
    });
  return (int)hipGetLastError();
}

FMLX_DEFINE_PRELOAD()
