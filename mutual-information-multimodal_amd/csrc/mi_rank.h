// Image-report retrieval ranks.  With S[i, j] = critic(img_i, txt_j) over b pairs and the
// package's masking (a pair i != j with sid_i == sid_j is dropped: neither a hit nor a miss):
//   rank_i2t[i] = #{ j : sid_j != sid_i and S[i, j] > S[i, i] }     (image -> report)
//   rank_t2i[j] = #{ i : sid_i != sid_j and S[i, j] > S[j, j] }     (report -> image)
// 0-based int32, strictly greater (a tie counts for the true pair).  Counts are integers: every result is exact and
// identical from call to call (integer atomics commute).  Building blocks:
//   rank_diag_*_kernel:  diag[i] = S[i, i] from the score GEMM's own operands, before the sweep; zeroes the ranks
//   rank_tile_counts:    one 64 x 64 wave tile (MFMA accumulator layout) -> one count per row and per column of the tile,
//                        added to the ranks (no b x b / 64 buffer of tile counts, no merge launch)
//   rank_matrix_kernel:  both ranks of a caller's fp32 [b][b] score matrix, no workspace
#pragma once
#include "mi_common.h"
#include "mi_gemm.h"
#include "mi_gemm_bf16.h"

namespace mi {

struct RankOut {
  const int64_t* sid;  // [b]
  float* diag;         // [b]: S[i, i], written by the diagonal kernel before the sweep
  int* rank_i2t;       // [b] or null, zeroed before the sweep: row counts are added here
  int* rank_t2i;       // [b] or null: column counts
};

// acc element (tm, tn, r) of this lane is S[mb + tm 32 + (r & 3) + 8 (r >> 2) + 4 half, nb + tn 32 + (lane & 31)]
// (MFMA 32x32 C/D layout, mi_gemm.h foreach_acc).  A lane owns one column per sub-tile: the column counts are per-lane
// sums plus one exchange between the halves.  A row's 64 values sit in the 32 lanes of one half, so the two 32-bit
// halves of a ballot are the counts of rows r and r + 4: no shuffle butterfly.  Lane l keeps the count of tile row l and
// adds it once (int atomics, nothing to add: no atomic).  Out-of-range rows and columns of partial tiles contribute
// nothing.  No block-level barrier: any wave may call it alone.  M == N == b (square problems only).
__device__ __forceinline__ void rank_tile_counts(const f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                 const RankOut& o) {
  if (mb >= M || nb >= N) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const bool rows = o.rank_i2t != nullptr, cols = o.rank_t2i != nullptr;  // (uniform)
  int64_t sc[2];
  float dc[2];
  bool cok[2];
  int cc[2] = {0, 0};
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? o.sid[col] : 0;
    dc[tn] = cok[tn] && cols ? o.diag[col] : 0.0f;
  }
  int mine = 0;  // count of tile row `lane`
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row_l = tm * 32 + (r & 3) + 8 * (r >> 2);  // half 0's row; half 1 holds row_l + 4
      const int64_t row = mb + row_l + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? o.sid[row] : 0;
      const float dr = rok && rows ? o.diag[row] : 0.0f;
      int lo = 0, hi = 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const float v = acc[tm][tn][r];
        const bool neg = rok && cok[tn] && pair_kind(row, nb + tn * 32 + col_l, sr, sc[tn]) == 2;
        cc[tn] += (neg && v > dc[tn]) ? 1 : 0;
        if (rows) {
          const unsigned long long bal = __ballot(neg && v > dr);
          lo += __popc((unsigned)bal);
          hi += __popc((unsigned)(bal >> 32));
        }
      }
      mine = lane == row_l ? lo : lane == row_l + 4 ? hi : mine;
    }
  if (rows && mine != 0 && mb + lane < M) atomicAdd(o.rank_i2t + mb + lane, mine);
  if (cols) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int c = cc[tn] + __shfl_xor(cc[tn], 32);
      const int64_t col = nb + tn * 32 + col_l;
      if (half == 0 && c != 0 && col < N) atomicAdd(o.rank_t2i + col, c);
    }
  }
}

// score GEMM epilogue, both call forms: the generic kernels' (mi_gemm.h) and the 16-bit chain's (mi_gemm_bf16.h; not a
// reducing epilogue there: every wave adds its own counts)
struct EpiRankCounts {
  static constexpr bool kReducesPartial = false;
  RankOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    rank_tile_counts(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    rank_tile_counts(acc, mb, nb, M, N, o);
  }
};

// ------------------------------------------------------------------------------------------------ diagonal
// diag[i] = sum_k A[i, k] B[i, k] in fp32, one wave per row, which also zeroes the row's two ranks for the sweep's
// atomics.  The 16-bit chain's operands as they lie in the workspace (bf16x3: the split parts along the tripled K, so the
// sum is hi hi + hi lo + lo hi as in the sweep); K % 8 == 0.
static __global__ __launch_bounds__(256) void rank_diag_bf16_kernel(const bf16_t* __restrict__ a,
                                                                    const bf16_t* __restrict__ bm, int64_t b, int64_t K,
                                                                    float* __restrict__ diag, float* diag_out,
                                                                    int* rank_i2t, int* rank_t2i) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= b) return;  // (wave-uniform)
  float s = 0.0f;
  for (int64_t k = (int64_t)lane * 8; k < K; k += 512) {
    const bf16x8 va = *reinterpret_cast<const bf16x8*>(a + i * K + k);
    const bf16x8 vb = *reinterpret_cast<const bf16x8*>(bm + i * K + k);
#pragma unroll
    for (int q = 0; q < 8; ++q) s = fmaf((float)va[q], (float)vb[q], s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    diag[i] = s;
    if (diag_out) diag_out[i] = s;
    if (rank_i2t) rank_i2t[i] = 0;
    if (rank_t2i) rank_t2i[i] = 0;
  }
}

// The generic kernels' operands: fp32 rows, rounded to OpT as the GEMM rounds them when it stages a tile
template <typename OpT>
static __global__ __launch_bounds__(256) void rank_diag_kernel(const float* __restrict__ a, const float* __restrict__ bm,
                                                               int64_t b, int64_t K, float* __restrict__ diag,
                                                               float* diag_out, int* rank_i2t, int* rank_t2i) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= b) return;  // (wave-uniform)
  float s = 0.0f;
  for (int64_t k = lane; k < K; k += 64) s = fmaf((float)(OpT)a[i * K + k], (float)(OpT)bm[i * K + k], s);
  s = wave_sum(s);
  if (lane == 0) {
    diag[i] = s;
    if (diag_out) diag_out[i] = s;
    if (rank_i2t) rank_i2t[i] = 0;
    if (rank_t2i) rank_t2i[i] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ materialised scores
// A caller's fp32 [b][b] matrix.  Workgroup g < n_rb walks rows: wave w counts row 4 g + w over all columns.  Workgroup
// n_rb + g walks 64 columns transposed: lane l owns column 64 g + l (loads coalesced along the row), wave w runs down the
// rows w, w + 4, ...; the four partial counts meet in LDS.
static __global__ __launch_bounds__(256) void rank_matrix_kernel(const float* __restrict__ s, const int64_t* __restrict__ sid,
                                                                 int64_t b, int64_t n_rb, int* rank_i2t, int* rank_t2i) {
  __shared__ int red[4][64];
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (g < n_rb) {
    const int64_t i = g * 4 + wave;
    if (i >= b || !rank_i2t) return;  // (wave-uniform; no barrier on this branch)
    const float d = s[i * b + i];
    const int64_t si = sid[i];
    unsigned n = 0;
    for (int64_t j = lane; j < b; j += 64) n += (pair_kind(i, j, si, sid[j]) == 2 && s[i * b + j] > d) ? 1u : 0u;
    n = wave_sum_u(n);
    if (lane == 0) rank_i2t[i] = (int)n;
    return;
  }
  if (!rank_t2i) return;  // (uniform)
  const int64_t j = (g - n_rb) * 64 + lane;
  int n = 0;
  if (j < b) {
    const float d = s[j * b + j];
    const int64_t sj = sid[j];
    for (int64_t i = wave; i < b; i += 4) n += (pair_kind(i, j, sid[i], sj) == 2 && s[i * b + j] > d) ? 1 : 0;
  }
  red[wave][lane] = n;
  __syncthreads();
  if (wave == 0 && j < b) rank_t2i[j] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
}

// ------------------------------------------------------------------------------------------------ host side
static inline RankOut rank_out(const int64_t* sid, float* diag, int* rank_i2t, int* rank_t2i) {
  return RankOut{sid, diag, rank_i2t, rank_t2i};
}

static inline int rank_diag_bf16(const bf16_t* a, const bf16_t* bm, int64_t b, int64_t K, const RankOut& o, float* diag_out,
                                 hipStream_t st) {
  {
    ProfScope prof_("rank_diag_bf16_kernel", st);
    hipLaunchKernelGGL(rank_diag_bf16_kernel, dim3((unsigned)((b + 3) / 4)), dim3(256), 0, st, a, bm, b, K, o.diag,
                       diag_out, o.rank_i2t, o.rank_t2i);
  }
  MI_LAUNCH_CHECK("rank_diag_bf16_kernel");
  return MI_OK;
}

template <typename OpT>
static inline int rank_diag(const float* a, const float* bm, int64_t b, int64_t K, const RankOut& o, float* diag_out,
                            hipStream_t st) {
  {
    ProfScope prof_("rank_diag_kernel", st);
    hipLaunchKernelGGL(rank_diag_kernel<OpT>, dim3((unsigned)((b + 3) / 4)), dim3(256), 0, st, a, bm, b, K, o.diag,
                       diag_out, o.rank_i2t, o.rank_t2i);
  }
  MI_LAUNCH_CHECK("rank_diag_kernel");
  return MI_OK;
}

static inline int rank_matrix(const float* scores, const int64_t* sid, int64_t b, int* rank_i2t, int* rank_t2i,
                              hipStream_t st) {
  const int64_t n_rb = (b + 3) / 4, n_cb = (b + 63) / 64;
  {
    ProfScope prof_("rank_matrix_kernel", st);
    hipLaunchKernelGGL(rank_matrix_kernel, dim3((unsigned)(n_rb + n_cb)), dim3(256), 0, st, scores, sid, b, n_rb, rank_i2t,
                       rank_t2i);
  }
  MI_LAUNCH_CHECK("rank_matrix_kernel");
  return MI_OK;
}

}  // namespace mi
