// Top-k retrieval over a gallery.  Queries q and candidates g with scores S[q, g]; a candidate is
// excluded for a query when ids are given and id_q == id_g.  The result of a query is the first k candidates in the
// total order (score descending, candidate index ascending; -0.0 counts as +0.0): idx int32 [n_q][k], val float32
// [n_q][k] (the kernel's own fp32 score of idx), tail idx = -1, val = -inf where fewer than k candidates remain.
//
// A query keeps a list of k 64-bit keys in global memory, key = ordered(score) << 32 | (0xFFFFFFFF - index): the
// unsigned order of the keys IS the total order above, keys of different candidates differ, and no key is 0 (index <
// 2^31 leaves the low word >= 0x80000000), so 0 means "empty".  Building blocks:
//   topk_zero_kernel:    empties the lists before the sweep
//   topk_insert:         the bounded cascade -- slot s takes max(slot, v) in ONE atomicMax and v goes on as the smaller
//                        of the two.  No lock, no flag, nothing waits: a value carried past a slot leaves a larger one
//                        there and slots only grow, so under any interleaving the k slots end as the k largest keys
//                        ever inserted (in some order), and at any moment the last slot holds a key that k - 1 larger
//                        ones sit above: a key at or below it, however stale the read, is not in the top k
//   topk_tile_insert:    one 64 x 64 wave tile (MFMA accumulator layout) -> inserts; the score GEMM's epilogue in both
//                        call forms.  The lane-owned side (columns, the GEMM's B operand) is the query side
//   topk_matrix_kernel:  the same lists from a caller's fp32 [n_rows][n_cols] matrix
//   topk_finish_kernel:  sorts each list descending, decodes idx / val, fills the tail
#pragma once
#include "mi_common.h"
#include "mi_gemm.h"
#include "mi_gemm_bf16.h"

namespace mi {

constexpr int kTopkMaxK = 32;  // MI_TOPK_MAX_K (include/mi_critic.h)
typedef unsigned long long topk_key_t;

// float -> unsigned with the same order (-0.0 first folded into +0.0), and back
__device__ __forceinline__ unsigned topk_ordered(float v) {
  unsigned u = __float_as_uint(v);
  u = u == 0x80000000u ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float topk_score(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ topk_key_t topk_key(float v, int64_t cand) {
  return ((topk_key_t)topk_ordered(v) << 32) | (topk_key_t)(0xFFFFFFFFu - (unsigned)cand);
}

// the query's last slot, as fresh as a relaxed load gives it (a stale value is only a lower threshold)
__device__ __forceinline__ topk_key_t topk_threshold(const topk_key_t* list, int k) {
  return __hip_atomic_load(list + k - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// at most k atomics, never a retry
__device__ __forceinline__ void topk_insert(topk_key_t* list, int k, topk_key_t v) {
  for (int s = 0; s < k && v != 0; ++s) {
    const topk_key_t old = atomicMax(list + s, v);
    v = old < v ? old : v;
  }
}

struct TopkOut {
  const int64_t* sid_q;  // [N] ids of the queries (the tile's columns), or null: nothing excluded
  const int64_t* sid_c;  // [M] ids of the candidates (the tile's rows); null with sid_q
  topk_key_t* keys;      // [N][k], emptied before the sweep
  int k;
};

// acc element (tm, tn, r) of this lane is S[mb + tm 32 + (r & 3) + 8 (r >> 2) + 4 half, nb + tn 32 + (lane & 31)]
// (mi_rank.h): a lane owns one query column per sub-tile and walks 32 of its candidates.  Out-of-range rows and columns
// of partial tiles and excluded pairs are dropped; a key goes to the cascade only above the query's threshold, which
// is read again after every insertion of the lane's own.  One shuffle between the halves, no barrier: any wave may call
// it, with all its 64 lanes.
__device__ __forceinline__ void topk_tile_insert(const f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                 const TopkOut& o) {
  if (mb >= M || nb >= N) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const bool ids = o.sid_q != nullptr;  // (uniform)
  topk_key_t* list[2];
  topk_key_t thr[2];
  int64_t sq[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    list[tn] = o.keys + (cok[tn] ? col : 0) * o.k;
    sq[tn] = cok[tn] && ids ? o.sid_q[col] : 0;
    thr[tn] = cok[tn] ? topk_threshold(list[tn], o.k) : ~0ull;
  }
  // Pre-selection.  Every tile of a query's column runs at the same time (B = 4096: one round of 256 x 256 workgroup
  // tiles), so at first each lane sees an empty list and would cascade most of its 32 keys.  Pass 0 therefore inserts
  // only the best key of the tile's 64 candidates per query (the two halves meet in one shuffle); the threshold read
  // after it is close to the final one, and pass 1 sends what is still above it -- on random scores about one key per
  // query and sweep.  Which keys reach the cascade changes, the final lists do not.
  topk_key_t best[2] = {0ull, 0ull};
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sc = rok && ids ? o.sid_c[row] : 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const topk_key_t key = topk_key(acc[tm][tn][r], row);
        const bool take = rok && cok[tn] && !(ids && sc == sq[tn]);
        best[tn] = take && key > best[tn] ? key : best[tn];
      }
    }
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const topk_key_t other = __shfl_xor(best[tn], 32);
    best[tn] = other > best[tn] ? other : best[tn];
    if (half == 0 && best[tn] > thr[tn]) topk_insert(list[tn], o.k, best[tn]);
    thr[tn] = cok[tn] ? topk_threshold(list[tn], o.k) : ~0ull;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (row >= M) continue;
      const int64_t sc = ids ? o.sid_c[row] : 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        if (!cok[tn] || (ids && sc == sq[tn])) continue;
        const topk_key_t key = topk_key(acc[tm][tn][r], row);
        if (key > thr[tn] && key != best[tn]) {
          topk_insert(list[tn], o.k, key);
          thr[tn] = topk_threshold(list[tn], o.k);
        }
      }
    }
}

// score GEMM epilogue, both call forms (as EpiRankCounts: not a reducing epilogue, every wave inserts its own tile)
struct EpiTopkInsert {
  static constexpr bool kReducesPartial = false;
  TopkOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    topk_tile_insert(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    topk_tile_insert(acc, mb, nb, M, N, o);
  }
};

// ------------------------------------------------------------------------------------------------ lists
static __global__ __launch_bounds__(256) void topk_zero_kernel(topk_key_t* keys, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) keys[e] = 0ull;
}

// One wave per query: lane s < k holds slot s; its place is the number of keys above it (empty slots, all 0, keep their
// slot order among themselves behind every key).
static __global__ __launch_bounds__(256) void topk_finish_kernel(const topk_key_t* __restrict__ keys, int64_t n_q, int k,
                                                                 int32_t* __restrict__ idx, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_q) return;  // (wave-uniform)
  const topk_key_t mine = lane < k ? keys[q * k + lane] : 0ull;
  int pos = 0;
  for (int t = 0; t < k; ++t) {
    const topk_key_t other = __shfl(mine, t);
    pos += (other > mine || (other == mine && t < lane)) ? 1 : 0;
  }
  if (lane < k) {
    idx[q * k + pos] = mine ? (int32_t)(0xFFFFFFFFu - (unsigned)mine) : -1;
    val[q * k + pos] = mine ? topk_score((unsigned)(mine >> 32)) : MI_NEG_INF;
  }
}

// ------------------------------------------------------------------------------------------------ materialised scores
// A caller's fp32 [n_rows][n_cols] matrix, walked as rank_matrix_kernel walks it.  axis 0 (each row's top-k columns): wave
// w of workgroup g runs along row 4 g + w.  axis 1 (each column's top-k rows): lane l of workgroup g owns column
// 64 g + l (loads coalesced along the row), wave w runs down the rows w, w + 4, ...  Same lists, same finish.
static __global__ __launch_bounds__(256) void topk_matrix_kernel(const float* __restrict__ s,
                                                                 const int64_t* __restrict__ sid_rows,
                                                                 const int64_t* __restrict__ sid_cols, int64_t n_rows,
                                                                 int64_t n_cols, int axis, topk_key_t* keys, int k) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ids = sid_rows != nullptr;
  if (axis == 0) {
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= n_rows) return;  // (wave-uniform; no barrier in this kernel)
    topk_key_t* list = keys + i * k;
    const int64_t si = ids ? sid_rows[i] : 0;
    topk_key_t thr = topk_threshold(list, k);
    for (int64_t j = lane; j < n_cols; j += 64) {
      if (ids && sid_cols[j] == si) continue;
      const topk_key_t key = topk_key(s[i * n_cols + j], j);
      if (key > thr) {
        topk_insert(list, k, key);
        thr = topk_threshold(list, k);
      }
    }
    return;
  }
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;
  if (j >= n_cols) return;
  topk_key_t* list = keys + j * k;
  const int64_t sj = ids ? sid_cols[j] : 0;
  topk_key_t thr = topk_threshold(list, k);
  for (int64_t i = wave; i < n_rows; i += 4) {
    if (ids && sid_rows[i] == sj) continue;
    const topk_key_t key = topk_key(s[i * n_cols + j], i);
    if (key > thr) {
      topk_insert(list, k, key);
      thr = topk_threshold(list, k);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int topk_zero(topk_key_t* keys, int64_t n, hipStream_t st) {
  int64_t blocks = (n + 255) / 256;
  blocks = blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks;
  {
    ProfScope prof_("topk_zero_kernel", st);
    hipLaunchKernelGGL(topk_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, st, keys, n);
  }
  MI_LAUNCH_CHECK("topk_zero_kernel");
  return MI_OK;
}

static inline int topk_finish(const topk_key_t* keys, int64_t n_q, int k, int32_t* idx, float* val, hipStream_t st) {
  {
    ProfScope prof_("topk_finish_kernel", st);
    hipLaunchKernelGGL(topk_finish_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, st, keys, n_q, k, idx, val);
  }
  MI_LAUNCH_CHECK("topk_finish_kernel");
  return MI_OK;
}

static inline int topk_matrix(const float* scores, const int64_t* sid_rows, const int64_t* sid_cols, int64_t n_rows,
                              int64_t n_cols, int axis, topk_key_t* keys, int k, hipStream_t st) {
  const int64_t blocks = axis == 0 ? (n_rows + 3) / 4 : (n_cols + 63) / 64;
  {
    ProfScope prof_("topk_matrix_kernel", st);
    hipLaunchKernelGGL(topk_matrix_kernel, dim3((unsigned)blocks), dim3(256), 0, st, scores, sid_rows, sid_cols, n_rows,
                       n_cols, axis, keys, k);
  }
  MI_LAUNCH_CHECK("topk_matrix_kernel");
  return MI_OK;
}

}  // namespace mi
