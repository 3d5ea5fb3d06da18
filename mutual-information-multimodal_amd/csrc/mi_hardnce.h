// Hard-negative InfoNCE: the per-sample InfoNCE of mi_nce.h restricted to each query's top-k
// negatives.  With H_i the image -> report list of mi_topk.h for query i (ids on both sides, so equal-id candidates and
// the true pair are left out) and H'_j the report -> image list of column j:
//   r_i = log(exp S[i, i] + sum_{j in H_i} exp S[i, j]),  c_j = log(exp S[j, j] + sum_{i in H'_j} exp S[i, j])
//   rowwise: L = (1/B) sum_i (r_i - S[i, i]);  symmetric: half of that plus half of (1/B) sum_j (c_j - S[j, j])
// The selection is a constant of the gradient:
//   dL/dS[i, j] = wr (1[j in H_i u {i}] exp(S[i, j] - r_i) - delta_ij) + wc (1[i in H'_j u {j}] exp(S[i, j] - c_j) - delta_ij)
// A row (column) without negatives contributes exactly 0 to the loss and to G.  A training loss, not an MI bound.
// Building blocks:
//   EpiHardNceInsert:    the top-k sweep's epilogue (topk_tile_insert) that also writes the diagonal S[i, i] of its tile
//   hardnce_rows_kernel: list values + diagonal -> r, c, the per-sample terms (max, then sum of exponentials, list order)
//                        -> nce_loss_kernel
//   hardnce_tile_grad:   one 64 x 64 wave tile of recomputed scores -> G.  Support by INDEX MEMBERSHIP: an element is in
//                        the row part iff its column is one of the row's <= k listed indices (or the diagonal), in the
//                        column part iff its row is listed for the column -- independent of the score bits of this sweep
//   EpiHardNceGrad<TG> / EpiHardNceGrad2: the G GEMM's epilogues of the generic kernels and of the 16-bit chain
#pragma once
#include "mi_nce.h"
#include "mi_topk.h"

namespace mi {

// ------------------------------------------------------------------------------------------------ selection sweep
// rows and columns of the tile index the same B samples (square problem): the element row == col is S[i, i] in either
// operand order
__device__ __forceinline__ void hardnce_tile_diag(const f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                  float* diag) {
  if (!(mb < nb + 64 && nb < mb + 64) || mb >= M || nb >= N) return;  // (wave-uniform) the diagonal does not cross
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        if (row == col && row < M && col < N) diag[row] = acc[tm][tn][r];
      }
    }
}

// EpiTopkInsert plus the diagonal (diag == nullptr: the inserts alone).  Both call forms, not a reducing epilogue.
struct EpiHardNceInsert {
  static constexpr bool kReducesPartial = false;
  TopkOut o;
  float* diag;  // [B] or null
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    if (diag) hardnce_tile_diag(acc, mb, nb, M, N, diag);
    topk_tile_insert(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    if (diag) hardnce_tile_diag(acc, mb, nb, M, N, diag);
    topk_tile_insert(acc, mb, nb, M, N, o);
  }
};

// ------------------------------------------------------------------------------------------------ rows
// thread q < b: row q, b <= q < 2b: column q - b (symmetric mode; its term is 0 otherwise).  val: the finished lists'
// scores ([.][k], -inf tails), diag[i * diag_stride] = S[i, i].  A query without negatives: m = S_ii, s = 1, lse = S_ii
// and a term of exactly 0.
static __global__ __launch_bounds__(256) void hardnce_rows_kernel(const float* __restrict__ val_rows,
                                                                  const float* __restrict__ val_cols,
                                                                  const float* __restrict__ diag, int64_t diag_stride,
                                                                  int64_t b, int k, int symmetric, float* r_ws, float* c_ws,
                                                                  float* r_out, float* c_out, float* __restrict__ terms) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= 2 * b) return;
  const bool is_row = q < b;
  if (!is_row && !symmetric) {
    terms[q] = 0.0f;
    return;
  }
  const int64_t i = is_row ? q : q - b;
  const float* v = (is_row ? val_rows : val_cols) + i * k;
  const float d = diag[i * diag_stride];
  float m = d;
  for (int t = 0; t < k; ++t) m = fmaxf(m, v[t]);
  float s = expf(d - m);
  for (int t = 0; t < k; ++t) s += expf(v[t] - m);  // expf(-inf) == 0: the tail adds nothing
  const float lse = m + logf(s);
  if (is_row) {
    r_ws[i] = lse;
    if (r_out) r_out[i] = lse;
  } else {
    c_ws[i] = lse;
    if (c_out) c_out[i] = lse;
  }
  terms[q] = lse - d;
}

// ------------------------------------------------------------------------------------------------ gradient
struct HardNceGradIn {
  const int32_t* idx_rows;  // [M][k] H_i: column indices, -1 tails (first entry -1: the row has no negatives)
  const int32_t* idx_cols;  // [N][k] H'_j: row indices; read in the symmetric mode only
  int k;
  const float* r;         // [M]
  const float* c;         // [N]; symmetric mode only
  const float* grad_out;  // [1] or null (1)
  float wr, wc;           // 1/B, 0 (rowwise) or 1/(2B), 1/(2B) (symmetric)
};

// bit d of the result: index base + d is one of the query's listed indices, or `self` (its positive); 0 for an empty list
__device__ __forceinline__ unsigned long long hardnce_members(const int32_t* list, int k, int64_t base, int64_t self) {
  if (list[0] < 0) return 0ull;
  unsigned long long mask = 0ull;
  for (int t = 0; t < k; ++t) {
    const int64_t d = (int64_t)list[t] - base;  // (a -1 tail is below every base)
    if (d >= 0 && d < 64) mask |= 1ull << d;
  }
  const int64_t d = self - base;
  if (d >= 0 && d < 64) mask |= 1ull << d;
  return mask;
}

// acc (scores) -> G = grad_out * dL/dS, 0 outside M x N and outside the support.  Lane l holds the membership mask of
// row mb + l over the tile's 64 columns (handed to the lanes that own the row's elements by one shuffle per accumulator
// row); each lane holds the masks of its two columns over the tile's 64 rows.  All 64 lanes call it.
template <bool FAST>
__device__ __forceinline__ void hardnce_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                  const HardNceGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const float go = g.grad_out ? g.grad_out[0] : 1.0f;
  const float wr = go * g.wr, wc = go * g.wc;
  const bool cols = g.wc != 0.0f;  // uniform: the symmetric mode
  unsigned long long rmask_l = 0ull;
  float rr_l = 0.0f;
  {
    const int64_t row = mb + lane;
    if (row < M) {
      rmask_l = hardnce_members(g.idx_rows + row * g.k, g.k, nb, row);
      rr_l = g.r[row];
    }
  }
  unsigned long long cmask[2] = {0ull, 0ull};
  float cc[2] = {0.0f, 0.0f};
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    if (cols && col < N) {
      cmask[tn] = hardnce_members(g.idx_cols + col * g.k, g.k, mb, col);
      cc[tn] = g.c[col];
    }
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const unsigned long long rm = __shfl(rmask_l, rl);
      const float rr = __shfl(rr_l, rl);
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int cl = tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        const bool pos = mb + rl == nb + cl;
        float gv = 0.0f;
        if ((rm >> cl) & 1ull) {
          gv = wr * nce_exp<FAST>(v - rr);
          if (pos) gv -= wr;
        }
        if ((cmask[tn] >> rl) & 1ull) {
          gv += wc * nce_exp<FAST>(v - cc[tn]);
          if (pos) gv -= wc;
        }
        acc[tm][tn][r] = gv;
      }
    }
}

// recompute GEMM epilogue of the generic kernels, as EpiNceGrad<TG>
template <typename TG>
struct EpiHardNceGrad {
  HardNceGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    hardnce_tile_grad<false>(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute GEMM epilogue of the 16-bit chain, as EpiNceGrad2: the same forms of G / G^T, the same stores
struct EpiHardNceGrad2 {
  static constexpr bool kReducesPartial = false;
  HardNceGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    hardnce_tile_grad<true>(acc, mb, nb, M, N, in);
    const bool staged = (M % 8 == 0) && (N % 8 == 0);
    if (staged && split) {
      wave_tile_store_split(acc, lds, g, 1, gt, 1, mb, nb, M, N);
    } else if (staged) {
      wave_tile_store_bf16(acc, lds, g, N, gt, M, mb, nb, M, N);
    } else {
      foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
        if (row < M && col < N) g[row * N + col] = (bf16_t)v;
      });
      foreach_acc4(acc, mb, nb, [&](int64_t row0, int64_t col, float v0, float v1, float v2, float v3) {
        if (col < N) store4_transposed(gt, M, row0, col, M, v0, v1, v2, v3);
      });
    }
  }
};

// a caller's fp32 [b][b] scores: one wave per 64 x 64 tile, as nce_matrix_grad_kernel (exact expf)
static __global__ __launch_bounds__(64) void hardnce_matrix_grad_kernel(const float* __restrict__ s, int64_t b,
                                                                        HardNceGradIn in, float* __restrict__ grad) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  hardnce_tile_grad<false>(acc, mb, nb, b, b, in);
  foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
    if (row < b && col < b) grad[row * b + col] = v;
  });
}

// ------------------------------------------------------------------------------------------------ host side
// the lists of both sides ([2b][k]: the rows' H_i, then the columns' H'_j) and the O(b) floats of the loss
struct HardNceLists {
  topk_key_t* keys;
  int32_t* idx;
  float* val;
  float *r, *c, *terms;
};

static inline HardNceLists plan_hardnce_lists(Workspace& ws, int64_t b, int k) {
  HardNceLists q{};
  q.keys = ws.take<topk_key_t>(2 * b * k);
  q.idx = ws.take<int32_t>(2 * b * k);
  q.val = ws.take<float>(2 * b * k);
  q.r = ws.take<float>(b);
  q.c = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  return q;
}

static inline HardNceGradIn hardnce_grad_in(const int32_t* idx_rows, const int32_t* idx_cols, int k, const float* r,
                                            const float* c, const float* grad_out, int64_t b, int mode) {
  const float fb = (float)b;
  if (mode == MI_NCE_SYMMETRIC) return HardNceGradIn{idx_rows, idx_cols, k, r, c, grad_out, 0.5f / fb, 0.5f / fb};
  return HardNceGradIn{idx_rows, nullptr, k, r, nullptr, grad_out, 1.0f / fb, 0.0f};
}

// finished lists + diagonal -> r, c (workspace and the caller's optional copies), the terms, the loss
static inline int hardnce_finish(const float* val_rows, const float* val_cols, const float* diag, int64_t diag_stride,
                                 int64_t b, int k, int mode, const HardNceLists& q, float* loss_out, float* lse_rows,
                                 float* lse_cols, hipStream_t st) {
  const int sym = mode == MI_NCE_SYMMETRIC ? 1 : 0;
  {
    ProfScope prof_("hardnce_rows_kernel", st);
    hipLaunchKernelGGL(hardnce_rows_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, val_rows, val_cols,
                       diag, diag_stride, b, k, sym, q.r, q.c, lse_rows, sym ? lse_cols : nullptr, q.terms);
  }
  MI_LAUNCH_CHECK("hardnce_rows_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, q.terms, b, sym, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

}  // namespace mi
