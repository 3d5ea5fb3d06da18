// Per-sample InfoNCE against a memory bank of past embeddings, DESIGN.md section 13.
// Batch x [B], y [B], ids sid [B]; bank bank_x [M], bank_y [M], ids bank_sid [M] (constants: no gradient).  Index B + m is
// bank entry m on either side; S[i, j] = critic(img_i, txt_j).
//   r_i = log sum_{j in C_i} exp S[i, j],  C_i = {i} u {j < B : sid_j != sid_i} u {B + m : bank_sid_m != sid_i}
//   c_j = log sum_{i in R_j} exp S[i, j],  R_j = {j} u {i < B : sid_i != sid_j} u {B + m : bank_sid_m != sid_j}
//   rowwise: L = (1/B) sum_i (r_i - S[i, i]);  symmetric: L = 1/2 (1/B) sum_i (r_i - S[i, i]) + 1/2 (1/B) sum_j (c_j - S[j, j])
// The score matrix is L-shaped: a top block [B] x [B + M] (batch images against batch and bank reports) and, in the
// symmetric mode, a left block [M] x [B] (bank images against batch reports); there is no bank x bank block.  Both blocks
// are GEMMs of the existing kernels (mi_gemm.h, mi_gemm_bf16.h) with the epilogues of this header:
//   bank_tile_stats: one 64 x 64 wave tile -> the records of mi_nce.h (NceRec), column ids from two arrays (sid for columns
//                    < B, bank_sid beyond), positives only where row == col in the top block; row records for the top
//                    block only, column records for columns < B only (top block: its row tiles; left block: its row tiles
//                    behind them) -- nobody reads a bank row's or a bank column's records
//   bank_tile_grad:  one wave tile -> G = grad_out * dL/dS of its block
// nce_merge_kernel / nce_loss_kernel (mi_nce.h) merge the records in tile order: fixed order, no float atomics.
// bank_cvt_kernel converts the fp32 batch and bank rows straight into the chain's operand buffers at their row offsets.
#pragma once
#include "mi_nce.h"

namespace mi {

struct BankStatsOut {
  const int64_t* sid_rows;   // ids of the block's rows (top block: sid, left block: bank_sid)
  const int64_t* sid_cols0;  // ids of columns < nb0
  const int64_t* sid_cols1;  // ids of columns >= nb0 (column nb0 + m: sid_cols1[m]); unused when N == nb0
  int64_t nb0;               // B
  NceRec* rowp;              // [M][n_ct]: row i over the columns of tile t, or null (left block)
  int64_t n_ct;
  NceRec* colp;              // [nb0][n_rt]: column j < nb0 over the rows of tile rt_off + t, or null (row-wise mode)
  int64_t n_rt, rt_off;
  float* diag;               // [M]: S[i, i], or null: the block holds no positives (left block)
};

struct BankGradIn {
  const int64_t* sid_rows;
  const int64_t* sid_cols0;
  const int64_t* sid_cols1;
  int64_t nb0;
  const float* r;         // row LSE of the block's rows, or null: no row term (left block)
  const float* c;         // column LSE of columns < nb0, or null: no column term (row-wise mode)
  const float* grad_out;  // [1] or null (1)
  float wr, wc;           // 1/B, 0 (row-wise) or 1/(2B), 1/(2B) (symmetric)
  int has_diag;           // top block: positives at row == col
};

__device__ __forceinline__ int64_t bank_col_id(const int64_t* s0, const int64_t* s1, int64_t nb0, int64_t col) {
  return col < nb0 ? s0[col] : s1[col - nb0];
}

// acc layout as nce_tile_stats (mi_nce.h).  Consumes acc.
template <bool FAST>
__device__ __forceinline__ void bank_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                const BankStatsOut& o) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const bool dtile = o.diag != nullptr && mb < nb + 64 && nb < mb + 64;
  int64_t sc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? bank_col_id(o.sid_cols0, o.sid_cols1, o.nb0, col) : 0;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? o.sid_rows[row] : 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        const bool ok = rok && cok[tn];
        const bool pos = o.diag != nullptr && row == col;
        if (dtile && ok && pos) o.diag[row] = v;
        acc[tm][tn][r] = (ok && (sr != sc[tn] || pos)) ? v : MI_NEG_INF;
      }
    }
  if (o.rowp && nb < N) {
    const int64_t t = nb >> 6;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a0 = acc[tm][0][r], a1 = acc[tm][1][r];
        float m = fmaxf(a0, a1);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float s = m == MI_NEG_INF ? 0.0f : nce_exp<FAST>(a0 - m) + nce_exp<FAST>(a1 - m);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);
        const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (col_l == 0 && row < M) o.rowp[row * o.n_ct + t] = NceRec{m, s};
      }
  }
  // column records: only the batch's columns have a column term (wave-uniform test: tiles beyond nb0 skip the reduction)
  if (o.colp && mb < M && nb < o.nb0) {
    const int64_t t = o.rt_off + (mb >> 6);
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      float m = MI_NEG_INF;
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[tm][tn][r]);
      m = fmaxf(m, __shfl_xor(m, 32));
      float s = 0.0f;
      if (m != MI_NEG_INF) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) s += nce_exp<FAST>(acc[tm][tn][r] - m);
      }
      s += __shfl_xor(s, 32);
      const int64_t col = nb + tn * 32 + col_l;
      if (half == 0 && col < N && col < o.nb0) o.colp[col * o.n_rt + t] = NceRec{m, s};
    }
  }
}

// acc (scores) -> G of the block: 1[candidate] (wr exp(S - r_i) + [col < nb0] wc exp(S - c_j)) - (wr + wc) delta_ij; 0
// outside M x N.  A row whose only candidate is its positive has r_i == S[i, i] exactly: wr + wc - (wr + wc) == 0.
template <bool FAST>
__device__ __forceinline__ void bank_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                               const BankGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const float go = g.grad_out ? g.grad_out[0] : 1.0f;
  const float wr = go * g.wr, wc = go * g.wc;
  const bool rows = g.r != nullptr, cols = g.c != nullptr;  // uniform
  int64_t sc[2];
  float cc[2];
  bool cok[2], ccol[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    ccol[tn] = cok[tn] && cols && col < g.nb0;
    sc[tn] = cok[tn] ? bank_col_id(g.sid_cols0, g.sid_cols1, g.nb0, col) : 0;
    cc[tn] = ccol[tn] ? g.c[col] : 0.0f;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? g.sid_rows[row] : 0;
      const float rr = rok && rows ? g.r[row] : 0.0f;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        const bool pos = g.has_diag && row == col;
        float gv = 0.0f;
        if (rok && cok[tn] && (sr != sc[tn] || pos)) {
          if (rows) gv = wr * nce_exp<FAST>(v - rr);
          if (ccol[tn]) gv += wc * nce_exp<FAST>(v - cc[tn]);
          if (pos) gv -= wr + wc;
        }
        acc[tm][tn][r] = gv;
      }
    }
}

// score GEMM epilogue, both call forms (the generic kernels' and the 16-bit chain's), as EpiNceStats
template <bool FAST>
struct EpiBankStats {
  static constexpr bool kReducesPartial = false;
  BankStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    bank_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    bank_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
};

// recompute GEMM epilogue of the generic kernels: G as TG [M][N]
template <typename TG>
struct EpiBankGrad {
  BankGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    bank_tile_grad<false>(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute GEMM epilogue of the 16-bit chain: G [M][N] and G^T [N][M] as bf16 (bf16x3: split parts in the A-side role).
// G^T is written for the tiles that start below column n_gt only: the top block's backward reads the batch's rows of G^T
// (dY of the batch) and, for the separable critic, the bank's (n_gt == N); the tiles beyond are nobody's operand.
struct EpiBankGrad2 {
  static constexpr bool kReducesPartial = false;
  BankGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int64_t n_gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    bank_tile_grad<true>(acc, mb, nb, M, N, in);
    bf16_t* t = nb < n_gt ? gt : nullptr;  // wave-uniform
    const bool staged = (M % 8 == 0) && (N % 8 == 0);
    if (staged && split) {
      wave_tile_store_split(acc, lds, g, 1, t, t ? 1 : 0, mb, nb, M, N);
    } else if (staged) {
      wave_tile_store_bf16(acc, lds, g, N, t, M, mb, nb, M, N);
    } else {
      foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
        if (row < M && col < N) g[row * N + col] = (bf16_t)v;
      });
      if (t)
        foreach_acc4(acc, mb, nb, [&](int64_t row0, int64_t col, float v0, float v1, float v2, float v3) {
          if (col < N) store4_transposed(t, M, row0, col, M, v0, v1, v2, v3);
        });
    }
  }
};

// ------------------------------------------------------------------------------------------------ operand prep
// One matrix of R0 + R1 rows whose rows come from two fp32 sources (in0 [R0][C], then in1 [R1][C]; R1 == 0: one source)
// -> bf16 row-major [R][C] and / or transposed [C][R] (bf16x3: [R][3 C] / [C][3 R] with the parts of split3_offsets), and
// / or an fp32 copy [R][C] (the generic kernels' report operand).  32 x 32 tiles through LDS, any shape.
struct BankCvtJob {
  const float* in0;
  int64_t R0;
  const float* in1;
  int64_t R1;
  int64_t C;
  bf16_t* out_rm;
  bf16_t* out_t;
  int split_rm, split_t;
  float* out_f32;
};
constexpr int kBankCvtJobs = 6;
struct BankCvtJobs {
  BankCvtJob j[kBankCvtJobs];  // blockIdx.z; unused jobs have R0 == 0
};

static __global__ __launch_bounds__(256) void bank_cvt_kernel(BankCvtJobs jobs) {
  __shared__ float tile[32][33];
  const BankCvtJob& J = jobs.j[blockIdx.z];
  const int64_t R = J.R0 + J.R1;
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  if (r0 >= R || c0 >= J.C) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int64_t h0, h1, lo;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t r = r0 + ty + 8 * q, c = c0 + tx;
    const bool in = r < R && c < J.C;
    const float v = !in ? 0.0f : (r < J.R0 ? J.in0[r * J.C + c] : J.in1[(r - J.R0) * J.C + c]);
    tile[ty + 8 * q][tx] = v;
    if (!in) continue;
    if (J.out_f32) J.out_f32[r * J.C + c] = v;
    if (J.out_rm && !J.split_rm) J.out_rm[r * J.C + c] = (bf16_t)v;
    if (J.out_rm && J.split_rm) {
      split3_offsets(J.split_rm, J.C, h0, h1, lo);
      bf16_t* row = J.out_rm + r * 3 * J.C + c;
      row[h0] = (bf16_t)v;
      row[h1] = (bf16_t)v;
      row[lo] = (bf16_t)bf16_residual(v);
    }
  }
  if (!J.out_t) return;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t c = c0 + ty + 8 * q, r = r0 + tx;
    if (c >= J.C || r >= R) continue;
    const float v = tile[tx][ty + 8 * q];
    if (!J.split_t) {
      J.out_t[c * R + r] = (bf16_t)v;
    } else {
      split3_offsets(J.split_t, R, h0, h1, lo);
      bf16_t* row = J.out_t + c * 3 * R + r;
      row[h0] = (bf16_t)v;
      row[h1] = (bf16_t)v;
      row[lo] = (bf16_t)bf16_residual(v);
    }
  }
}

static inline int launch_bank_cvt(const BankCvtJobs& jobs, hipStream_t st, const char* what) {
  int64_t rmax = 0, cmax = 0;
  for (int q = 0; q < kBankCvtJobs; ++q) {
    const BankCvtJob& J = jobs.j[q];
    if (J.R0 <= 0) continue;
    if (J.R0 + J.R1 > rmax) rmax = J.R0 + J.R1;
    if (J.C > cmax) cmax = J.C;
  }
  if (rmax <= 0 || cmax <= 0) return MI_OK;
  {
    ProfScope prof_(what, st);
    dim3 grid((unsigned)((cmax + 31) / 32), (unsigned)((rmax + 31) / 32), kBankCvtJobs);
    hipLaunchKernelGGL(bank_cvt_kernel, grid, dim3(256), 0, st, jobs);
  }
  MI_LAUNCH_CHECK(what);
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ host side
// The records of the L: rows of the top block over its n_ct column tiles; columns < B over the top block's row tiles and
// then the left block's (n_rt == 0 in the row-wise mode: no column records, c is not formed)
struct BankNceRecords {
  NceRec* rowp;  // [b][n_ct]
  NceRec* colp;  // [b][n_rt]
  float *diag, *r, *c, *terms;
  int64_t n_ct, n_rt_top, n_rt;
};

static inline BankNceRecords plan_banknce_records(Workspace& ws, int64_t b, int64_t m, bool sym) {
  BankNceRecords q{};
  q.n_ct = (b + m + 63) / 64;
  q.n_rt_top = (b + 63) / 64;
  q.n_rt = sym ? q.n_rt_top + (m + 63) / 64 : 0;
  q.rowp = ws.take<NceRec>(b * q.n_ct);
  q.colp = ws.take<NceRec>(b * (q.n_rt > 0 ? q.n_rt : 1));
  q.diag = ws.take<float>(b);
  q.r = ws.take<float>(b);
  q.c = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  return q;
}

static inline BankStatsOut banknce_stats_top(const BankNceRecords& q, const int64_t* sid, const int64_t* bank_sid,
                                             int64_t b) {
  return BankStatsOut{sid, sid, bank_sid, b, q.rowp, q.n_ct, q.n_rt > 0 ? q.colp : nullptr, q.n_rt, 0, q.diag};
}
static inline BankStatsOut banknce_stats_left(const BankNceRecords& q, const int64_t* sid, const int64_t* bank_sid,
                                              int64_t b) {
  return BankStatsOut{bank_sid, sid, nullptr, b, nullptr, 0, q.colp, q.n_rt, q.n_rt_top, nullptr};
}
static inline BankGradIn banknce_grad_top(const BankNceRecords& q, const int64_t* sid, const int64_t* bank_sid, int64_t b,
                                          const float* grad_out, int mode) {
  const float fb = (float)b;
  if (mode == MI_NCE_SYMMETRIC) return BankGradIn{sid, sid, bank_sid, b, q.r, q.c, grad_out, 0.5f / fb, 0.5f / fb, 1};
  return BankGradIn{sid, sid, bank_sid, b, q.r, nullptr, grad_out, 1.0f / fb, 0.0f, 1};
}
static inline BankGradIn banknce_grad_left(const BankNceRecords& q, const int64_t* sid, const int64_t* bank_sid, int64_t b,
                                           const float* grad_out) {
  return BankGradIn{bank_sid, sid, nullptr, b, nullptr, q.c, grad_out, 0.0f, 0.5f / (float)b, 0};
}

// records -> r, c (workspace and the caller's optional copies), loss: the kernels of mi_nce.h on the L's record counts
static inline int banknce_finish(const BankNceRecords& q, int64_t b, int mode, float* loss_out, float* lse_rows,
                                 float* lse_cols, hipStream_t st) {
  const bool sym = mode == MI_NCE_SYMMETRIC;
  {
    ProfScope prof_("banknce merge records", st);
    hipLaunchKernelGGL(nce_merge_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp, q.diag, b,
                       q.n_ct, q.n_rt, q.r, q.c, lse_rows, sym ? lse_cols : nullptr, q.terms);
  }
  MI_LAUNCH_CHECK("banknce merge records");
  {
    ProfScope prof_("banknce loss", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, q.terms, b, sym ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("banknce loss");
  return MI_OK;
}

}  // namespace mi
