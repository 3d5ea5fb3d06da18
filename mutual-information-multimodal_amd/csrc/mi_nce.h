// Per-sample InfoNCE (row-wise and symmetric image-report contrastive loss), DESIGN.md section 8.
//   r_i = log sum_{j in C_i} exp S[i, j],  C_i = {i} u {j : sid_j != sid_i}   (row LSE)
//   c_j = log sum_{i in R_j} exp S[i, j],  R_j = {j} u {i : sid_i != sid_j}   (column LSE)
//   rowwise: L = (1/B) sum_i (r_i - S[i, i]);  symmetric: L = 1/2 (1/B) sum_i (r_i - S[i, i]) + 1/2 (1/B) sum_j (c_j - S[j, j])
// Building blocks, shared by the bf16 / bf16x3 GEMM chain (mi_gemm_bf16.h), the generic kernels (mi_gemm.h) and the
// kernels on a caller's materialised score matrix:
//   nce_tile_stats: one 64 x 64 wave tile (MFMA accumulator layout) -> per-row (max, sum exp) over the tile's 64 columns,
//                   per-column records over its 64 rows, the diagonal scores
//   nce_merge_kernel + nce_loss_kernel: the records of every tile merged in tile order -> r, c, the per-sample terms, the
//                   loss (fixed order everywhere, no float atomics: bit-reproducible)
//   nce_tile_grad:  one wave tile -> G = grad_out * dL/dS from r, c, the mask and the diagonal term
// Row blocks (the sharded step): the tiles of rows [row_offset, row_offset + M) of the global B x B
// matrix; local row i is global sample row_offset + i, so its positive is column row_offset + i.  The whole batch is
// row_offset == 0, sid_rows == sid_cols.
//   nce_rank_part_kernel:   a rank's records -> r (kept), one flat part (column partials, row terms, diagonal)
//   nce_merge_parts_kernel: the parts of every rank, in rank order -> c, the per-sample terms -> nce_loss_kernel
#pragma once
#include "mi_common.h"
#include "mi_gemm.h"
#include "mi_gemm_bf16.h"

namespace mi {

// (max, sum exp(v - max)) of one row (column) over one 64-wide tile; m == -inf, s == 0: no candidate in the tile
struct NceRec {
  float m, s;
};

struct NceStatsOut {
  const int64_t* sid_rows;  // [M]
  const int64_t* sid_cols;  // [N]
  int64_t row_offset;       // global index of local row 0
  NceRec* rowp;             // [M][n_ct]: row i over the columns of tile t
  NceRec* colp;             // [N][n_rt]: column j over the rows of tile t
  float* diag;              // [M]: S[i, row_offset + i]
  int64_t n_ct, n_rt;
};

struct NceGradIn {
  const int64_t* sid_rows;  // [M]
  const int64_t* sid_cols;  // [N]
  int64_t row_offset;
  const float* r;         // [M] row LSE
  const float* c;         // [N] column LSE
  const float* grad_out;  // [1] or null (1)
  float wr, wc;           // weights of the row and column terms: 1/B, 0 (rowwise) or 1/(2B), 1/(2B) (symmetric); B is
                          // the global batch
};

template <bool FAST>
__device__ __forceinline__ float nce_exp(float x) {
  // FAST: hardware exponential (v_exp_f32), as the DV epilogues of the 16-bit chain; exp(-inf) = 0 either way
  if (FAST) return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
  return expf(x);
}

// acc element (tm, tn, r) of this lane is S[mb + tm 32 + (r & 3) + 8 (r >> 2) + 4 half, nb + tn 32 + (lane & 31)]
// (MFMA 32x32 C/D layout, mi_gemm.h foreach_acc).  Consumes acc.  No block-level barrier: any wave may call it alone.
template <bool FAST>
__device__ __forceinline__ void nce_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                               const NceStatsOut& o) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const int64_t off = o.row_offset;
  // only tiles that the diagonal crosses hold positive pairs (row_offset == 0: mb == nb; other offsets may straddle two)
  const bool dtile = mb + off < nb + 64 && nb < mb + off + 64;
  int64_t sc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? o.sid_cols[col] : 0;
  }
  // mask: non-candidates and elements outside M x N become -inf; the diagonal is kept (and recorded)
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
        const bool pos = row + off == col;
        if (dtile && ok && pos) o.diag[row] = v;
        acc[tm][tn][r] = (ok && (sr != sc[tn] || pos)) ? v : MI_NEG_INF;
      }
    }
  // rows: each row's 64 values sit in the 32 lanes of one half (two per lane): butterfly max, then butterfly sum
  if (nb < N) {
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
  // columns: 32 of a column's 64 values in one lane, the other 32 in the lane of the other half
  if (mb < M) {
    const int64_t t = mb >> 6;
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
      if (half == 0 && col < N) o.colp[col * o.n_rt + t] = NceRec{m, s};
    }
  }
}

// acc (scores) -> G = grad_out * dL/dS:  wr 1[j in C_i] exp(S - r_i) + wc 1[j in C_i] exp(S - c_j) - (wr + wc) delta_ij
// (j in C_i <=> i in R_j; delta_ij: row_offset + i == j).  0 outside M x N.
template <bool FAST>
__device__ __forceinline__ void nce_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                              const NceGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const float go = g.grad_out ? g.grad_out[0] : 1.0f;
  const float wr = go * g.wr, wc = go * g.wc;
  const bool cols = g.wc != 0.0f;  // uniform: the symmetric mode
  int64_t sc[2];
  float cc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? g.sid_cols[col] : 0;
    cc[tn] = cok[tn] && cols ? g.c[col] : 0.0f;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? g.sid_rows[row] : 0;
      const float rr = rok ? g.r[row] : 0.0f;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        const bool pos = row + g.row_offset == col;
        float gv = 0.0f;
        if (rok && cok[tn] && (sr != sc[tn] || pos)) {
          gv = wr * nce_exp<FAST>(v - rr);
          if (cols) gv += wc * nce_exp<FAST>(v - cc[tn]);
          if (pos) gv -= wr + wc;
        }
        acc[tm][tn][r] = gv;
      }
    }
}

// score GEMM epilogue: row / column records and the diagonal.  Both call forms: the generic kernels' (mi_gemm.h) and the
// 16-bit chain's (mi_gemm_bf16.h; not a reducing epilogue there: every wave writes its own records)
template <bool FAST>
struct EpiNceStats {
  static constexpr bool kReducesPartial = false;
  NceStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    nce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    nce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
};

// recompute GEMM epilogue of the generic kernels: G as TG [M][N] (the generic backward reads G^T through strides)
template <typename TG>
struct EpiNceGrad {
  NceGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    nce_tile_grad<false>(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute GEMM epilogue of the 16-bit chain: G and G^T as bf16 (bf16x3: split parts in the A-side role), as
// EpiGradScore2 does for DV
struct EpiNceGrad2 {
  static constexpr bool kReducesPartial = false;
  NceGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    nce_tile_grad<true>(acc, mb, nb, M, N, in);
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

// ------------------------------------------------------------------------------------------------ materialised scores
// One wave per 64 x 64 tile of a caller's fp32 [b][b] score matrix, loaded into the accumulator layout so that the
// GEMM epilogues' code runs unchanged (exact expf: these kernels serve fp32 scores of any critic).
__device__ __forceinline__ void nce_load_tile(const float* __restrict__ s, int64_t b, int64_t mb, int64_t nb,
                                              f32x16 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int64_t col = nb + tn * 32 + col_l;
        acc[tm][tn][r] = (row < b && col < b) ? s[row * b + col] : 0.0f;
      }
}

static __global__ __launch_bounds__(64) void nce_matrix_stats_kernel(const float* __restrict__ s, int64_t b,
                                                                     NceStatsOut o) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  nce_tile_stats<false>(acc, mb, nb, b, b, o);
}

static __global__ __launch_bounds__(64) void nce_matrix_grad_kernel(const float* __restrict__ s, int64_t b, NceGradIn in,
                                                                    float* __restrict__ grad) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  nce_tile_grad<false>(acc, mb, nb, b, b, in);
  foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
    if (row < b && col < b) grad[row * b + col] = v;
  });
}

// ------------------------------------------------------------------------------------------------ merge
// thread k < b: row k, b <= k < 2b: column k - b.  Records merged in tile order (exact expf / logf).
static __global__ __launch_bounds__(256) void nce_merge_kernel(const NceRec* __restrict__ rowp,
                                                               const NceRec* __restrict__ colp,
                                                               const float* __restrict__ diag, int64_t b, int64_t n_ct,
                                                               int64_t n_rt, float* r_ws, float* c_ws, float* r_out,
                                                               float* c_out, float* terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const bool is_row = k < b;
  const int64_t i = is_row ? k : k - b;
  const NceRec* p = is_row ? rowp + i * n_ct : colp + i * n_rt;
  const int64_t n = is_row ? n_ct : n_rt;
  float m = MI_NEG_INF, s = 0.0f;
  for (int64_t t = 0; t < n; ++t) lse_merge(m, s, p[t].m, p[t].s);
  // the diagonal is always a candidate, so s >= exp(S_ii - m) > 0 for finite scores; a row whose only candidate is its
  // own positive gets m = S_ii, s = 1: lse - S_ii == 0 exactly
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  if (is_row) {
    r_ws[i] = lse;
    if (r_out) r_out[i] = lse;
  } else {
    c_ws[i] = lse;
    if (c_out) c_out[i] = lse;
  }
  terms[k] = lse - diag[i];
}

// one workgroup: L = wr sum_i row_term_i + wc sum_j col_term_j, every sum in a fixed order
static __global__ __launch_bounds__(256) void nce_loss_kernel(const float* __restrict__ terms, int64_t b, int symmetric,
                                                              float* loss_out) {
  __shared__ float red[2][256];
  const int tid = threadIdx.x;
  float sr = 0.0f, sc = 0.0f;
  for (int64_t i = tid; i < b; i += 256) {
    sr += terms[i];
    sc += terms[b + i];
  }
  red[0][tid] = sr;
  red[1][tid] = sc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float fb = (float)b;
    loss_out[0] = symmetric ? 0.5f * (red[0][0] / fb) + 0.5f * (red[1][0] / fb) : red[0][0] / fb;
  }
}

// ------------------------------------------------------------------------------------------------ row blocks
// The part of one rank (nce_part_floats(br, b) floats, gathered in rank order by the caller):
//   [0, 2b)              column j: (m, s) of its candidates in this rank's rows, merged in row-tile order (NceRec)
//   [2b, 2b + br)        row term r_i - S[i, row_offset + i] of local row i
//   [2b + br, 2b + 2 br) S[i, row_offset + i]
__host__ __device__ inline int64_t nce_part_floats(int64_t br, int64_t b) { return 2 * b + 2 * br; }

// thread k < br: local row k (records merged in tile order exactly as nce_merge_kernel: the same r bits), br <= k < br + b:
// column k - br over this rank's row tiles
static __global__ __launch_bounds__(256) void nce_rank_part_kernel(const NceRec* __restrict__ rowp,
                                                                   const NceRec* __restrict__ colp,
                                                                   const float* __restrict__ diag, int64_t br, int64_t b,
                                                                   int64_t n_ct, int64_t n_rt, float* r_ws, float* r_out,
                                                                   float* __restrict__ part) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= br + b) return;
  const bool is_row = k < br;
  const int64_t i = is_row ? k : k - br;
  const NceRec* p = is_row ? rowp + i * n_ct : colp + i * n_rt;
  const int64_t n = is_row ? n_ct : n_rt;
  float m = MI_NEG_INF, s = 0.0f;
  for (int64_t t = 0; t < n; ++t) lse_merge(m, s, p[t].m, p[t].s);
  if (!is_row) {
    part[2 * i] = m;
    part[2 * i + 1] = s;
    return;
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  r_ws[i] = lse;
  if (r_out) r_out[i] = lse;
  part[2 * b + i] = lse - diag[i];
  part[2 * b + br + i] = diag[i];
}

// parts [n_ranks][nce_part_floats(br, b)] in rank order (rank g holds rows [g br, (g + 1) br)).  Thread k < b: the row term
// of sample k, copied; b <= k < 2b: column j = k - b, its partials merged in rank order from an empty (-inf, 0) start --
// exact for one rank, so one rank gives the bits of nce_merge_kernel -- then c_j and its term c_j - S[j, j] (the diagonal
// from the part of the rank that owns row j).  Every rank runs this on the same gathered buffer: identical bits.
static __global__ __launch_bounds__(256) void nce_merge_parts_kernel(const float* __restrict__ parts, int64_t n_ranks,
                                                                     int64_t br, int64_t b, float* c_out,
                                                                     float* __restrict__ terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const int64_t pf = nce_part_floats(br, b);
  if (k < b) {
    terms[k] = parts[(k / br) * pf + 2 * b + k % br];
    return;
  }
  const int64_t j = k - b;
  float m = MI_NEG_INF, s = 0.0f;
  for (int64_t g = 0; g < n_ranks; ++g) lse_merge(m, s, parts[g * pf + 2 * j], parts[g * pf + 2 * j + 1]);
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  c_out[j] = lse;
  terms[k] = lse - parts[(j / br) * pf + 2 * b + br + j % br];
}

// ------------------------------------------------------------------------------------------------ host side
struct NcePlan {
  NceRec* rowp;
  NceRec* colp;
  float *diag, *r, *c, *terms;
  int64_t n_t;  // 64-wide tiles per row and per column
};

static inline NcePlan plan_nce(Workspace& ws, int64_t b) {
  NcePlan q{};
  q.n_t = (b + 63) / 64;
  q.rowp = ws.take<NceRec>(b * q.n_t);
  q.colp = ws.take<NceRec>(b * q.n_t);
  q.diag = ws.take<float>(b);
  q.r = ws.take<float>(b);
  q.c = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  return q;
}

static inline NceStatsOut nce_stats_out(const NcePlan& q, const int64_t* sid) {
  return NceStatsOut{sid, sid, 0, q.rowp, q.colp, q.diag, q.n_t, q.n_t};
}

// b: the GLOBAL batch (the loss weights); a row block passes its own ids, the global ids and its offset
static inline NceGradIn nce_grad_in(const int64_t* sid_rows, const int64_t* sid_cols, int64_t row_offset, const float* r,
                                    const float* c, const float* grad_out, int64_t b, int mode) {
  const float fb = (float)b;
  if (mode == MI_NCE_SYMMETRIC) return NceGradIn{sid_rows, sid_cols, row_offset, r, c, grad_out, 0.5f / fb, 0.5f / fb};
  return NceGradIn{sid_rows, sid_cols, row_offset, r, c, grad_out, 1.0f / fb, 0.0f};
}
static inline NceGradIn nce_grad_in(const int64_t* sid, const float* r, const float* c, const float* grad_out, int64_t b,
                                    int mode) {
  return nce_grad_in(sid, sid, 0, r, c, grad_out, b, mode);
}

// records -> r, c (workspace and the caller's optional copies), loss
static inline int nce_finish(const NcePlan& q, int64_t b, int mode, float* loss_out, float* lse_rows, float* lse_cols,
                             hipStream_t st) {
  {
    ProfScope prof_("nce_merge_kernel", st);
    hipLaunchKernelGGL(nce_merge_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp, q.diag, b,
                       q.n_t, q.n_t, q.r, q.c, lse_rows, lse_cols, q.terms);
  }
  MI_LAUNCH_CHECK("nce_merge_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, q.terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ row blocks, host side
// The records of one rank's row block [br] x [b] and the row LSE r: the forward writes r, the backward reads it from the
// same workspace (the same plan gives the same offsets).
struct NceShardPlan {
  NceRec* rowp;  // [br][n_ct]
  NceRec* colp;  // [b][n_rt]
  float *diag, *r;
  int64_t n_ct, n_rt;
};

static inline NceShardPlan plan_nce_shard(Workspace& ws, int64_t br, int64_t b) {
  NceShardPlan q{};
  q.n_ct = (b + 63) / 64;
  q.n_rt = (br + 63) / 64;
  q.rowp = ws.take<NceRec>(br * q.n_ct);
  q.colp = ws.take<NceRec>(b * q.n_rt);
  q.diag = ws.take<float>(br);
  q.r = ws.take<float>(br);
  return q;
}

static inline NceStatsOut nce_stats_out(const NceShardPlan& q, const int64_t* sid_rows, const int64_t* sid_cols,
                                        int64_t row_offset) {
  return NceStatsOut{sid_rows, sid_cols, row_offset, q.rowp, q.colp, q.diag, q.n_ct, q.n_rt};
}

static inline int nce_rank_part(const NceShardPlan& q, int64_t br, int64_t b, float* part_out, float* lse_rows,
                                hipStream_t st) {
  {
    ProfScope prof_("nce_rank_part_kernel", st);
    hipLaunchKernelGGL(nce_rank_part_kernel, dim3((unsigned)((br + b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp,
                       q.diag, br, b, q.n_ct, q.n_rt, q.r, lse_rows, part_out);
  }
  MI_LAUNCH_CHECK("nce_rank_part_kernel");
  return MI_OK;
}

// terms: [2b] scratch
static inline int nce_merge_parts(const float* parts, int64_t n_ranks, int64_t br, int64_t b, int mode, float* loss_out,
                                  float* lse_cols, float* terms, hipStream_t st) {
  {
    ProfScope prof_("nce_merge_parts_kernel", st);
    hipLaunchKernelGGL(nce_merge_parts_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, parts, n_ranks, br,
                       b, lse_cols, terms);
  }
  MI_LAUNCH_CHECK("nce_merge_parts_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

}  // namespace mi
