// Jensen-Shannon and NWJ mutual-information bounds, on the reference's pairs: n_pos positives
// (i, i), n_neg negatives (i, j), i != j, sid_i != sid_j; equal-id off-diagonal pairs are dropped.
//   MI_FDIV_JSD: L = mean_pos sp(-s) + mean_neg sp(s)                     dL/ds = -sigma(-s) / n_pos  |  sigma(s) / n_neg
//   MI_FDIV_NWJ: L = exp(LSE_neg - log n_neg - 1) - mean_pos s            dL/ds = -1 / n_pos  |  exp(s - 1 - log n_neg)
// sp(x) = log(1 + e^x) = max(x, 0) + log1p(e^-|x|) and sigma(x) are evaluated in forms that cannot overflow, so "jsd" is
// finite for any finite scores.  NWJ's gradient is DV's with lse replaced by 1 + log n_neg: its statistics block carries
// that constant in the lse field, and every DV gradient kernel (pair_grad) serves it unchanged.
// Building blocks:
//   FdivRec / fdiv_push / fdiv_merge: partial sums over masked scores (JSD: sums of sp; NWJ: DV's (max, sum exp))
//   fdiv_{bound,matrix}_partials_kernel: the reference's logits layout, a [b_rows, b] row block of a score matrix
//   fdiv_tile_stats / fdiv_tile_grad: one 64 x 64 wave tile of a score GEMM (records; G = grad_out dL/dS)
//   fdiv_finalize_kernel: every record in a fixed order -> loss, the two expectation terms, the statistics block
// No float atomics anywhere: repeated calls give identical bits.
#pragma once
#include "mi_common.h"
#include "mi_gemm.h"
#include "mi_gemm_bf16.h"

namespace mi {

// ---- pair functions ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fdiv_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
// one exponential and one reciprocal (v_rcp_f32, 1 ulp); e = exp(-|x|) never overflows
__device__ __forceinline__ float fdiv_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.0f + e);
  return x >= 0.0f ? r : e * r;
}

// gradient rules of the bound kernels (template argument of the concat-MLP backward kernels)
constexpr int kGradDV = 0;   // DV, the reference's "infonce" and NWJ (normaliser from the statistics block)
constexpr int kGradJSD = 1;  // Jensen-Shannon: sigma(-s) / n_pos, sigma(s) / n_neg
// g is given: the kernels' score-matrix argument holds the caller's dL/dS [b_rows, b]; no pair kinds, no study ids, no
// exponential (mi_concat_mlp_bwd_from_g)
constexpr int kGradGiven = 2;

// d loss / d score of one pair of kind 1 (positive) / 2 (negative) / 0 (dropped), given the mode's constants
struct FdivGrad {
  int mode;
  float gpos;  // -go / n_pos
  float gneg;  // JSD: go / n_neg
  float go, lse;
};
__device__ __forceinline__ FdivGrad fdiv_grad_params(int mode, const mi_stats* st, float go) {
  FdivGrad p;
  p.mode = mode;
  p.go = go;
  p.lse = st->lse;
  p.gpos = -go / (float)st->n_pos;
  p.gneg = go / (float)st->n_neg;
  return p;
}
__device__ __forceinline__ float fdiv_pair_grad(const FdivGrad& p, int kind, float s) {
  if (kind == 1) return p.mode == MI_FDIV_JSD ? p.gpos * fdiv_sigmoid(-s) : p.gpos;
  if (kind == 2) return p.mode == MI_FDIV_JSD ? p.gneg * fdiv_sigmoid(s) : p.go * expf(s - p.lse);
  return 0.0f;
}

// ---- partial records -----------------------------------------------------------------------------------------------
// JSD: a = sum_neg sp(s), b unused (0);  NWJ: (a, b) = (max, sum exp(s - max)) of the negatives.  pos: JSD sum_pos sp(-s),
// NWJ sum_pos s.  cnt: number of negatives.
struct FdivRec {
  float a, b, pos;
  unsigned cnt;
};
__device__ __forceinline__ FdivRec fdiv_empty(int mode) {
  return FdivRec{mode == MI_FDIV_NWJ ? MI_NEG_INF : 0.0f, 0.0f, 0.0f, 0u};
}
__device__ __forceinline__ void fdiv_push(int mode, FdivRec& r, int kind, float s) {
  if (kind == 1) {
    r.pos += mode == MI_FDIV_JSD ? fdiv_softplus(-s) : s;
  } else if (kind == 2) {
    if (mode == MI_FDIV_JSD) r.a += fdiv_softplus(s);
    else lse_push(r.a, r.b, s);
    r.cnt += 1;
  }
}
__device__ __forceinline__ void fdiv_merge(int mode, FdivRec& r, const FdivRec& q) {
  if (mode == MI_FDIV_JSD) r.a += q.a;
  else lse_merge(r.a, r.b, q.a, q.b);
  r.pos += q.pos;
  r.cnt += q.cnt;
}
// butterfly over one wave (fixed order); the result is in every lane
__device__ __forceinline__ void fdiv_wave_merge(int mode, FdivRec& r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    FdivRec q;
    q.a = __shfl_xor(r.a, o);
    q.b = __shfl_xor(r.b, o);
    q.pos = __shfl_xor(r.pos, o);
    q.cnt = (unsigned)__shfl_xor((int)r.cnt, o);
    fdiv_merge(mode, r, q);
  }
}
// workgroup of NWAVES waves; valid in thread 0.  All threads must call.
template <int NWAVES>
__device__ __forceinline__ FdivRec fdiv_block_merge(int mode, FdivRec r, FdivRec* scratch) {
  fdiv_wave_merge(mode, r);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NWAVES; ++w) fdiv_merge(mode, r, scratch[w]);
  __syncthreads();
  return r;
}

// ---- materialised scores -------------------------------------------------------------------------------------------
constexpr int kFdivBlock = 256;
constexpr int kFdivMaxBlocks = 2048;

// logits [n], rows [0, pos) positive, the rest negative (the reference's mi_output layout)
static __global__ __launch_bounds__(kFdivBlock) void fdiv_bound_partials_kernel(const float* __restrict__ logits, int64_t n,
                                                                                int64_t pos, int mode,
                                                                                FdivRec* __restrict__ out) {
  __shared__ FdivRec scratch[kFdivBlock / 64];
  FdivRec r = fdiv_empty(mode);
  const int64_t stride = (int64_t)gridDim.x * kFdivBlock;
  for (int64_t k = (int64_t)blockIdx.x * kFdivBlock + threadIdx.x; k < n; k += stride)
    fdiv_push(mode, r, k < pos ? 1 : 2, logits[k]);
  r = fdiv_block_merge<kFdivBlock / 64>(mode, r, scratch);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// scores [b_rows, b]; local row i is global row row_offset + i.  One workgroup walks whole rows.
static __global__ __launch_bounds__(kFdivBlock) void fdiv_matrix_partials_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ sid_rows, const int64_t* __restrict__ sid_cols,
    int64_t b_rows, int64_t b, int64_t row_offset, int mode, FdivRec* __restrict__ out) {
  __shared__ FdivRec scratch[kFdivBlock / 64];
  FdivRec r = fdiv_empty(mode);
  for (int64_t i = blockIdx.x; i < b_rows; i += gridDim.x) {
    const int64_t si = sid_rows[i], gi = row_offset + i;
    for (int64_t j = threadIdx.x; j < b; j += kFdivBlock)
      fdiv_push(mode, r, pair_kind(gi, j, si, sid_cols[j]), scores[i * b + j]);
  }
  r = fdiv_block_merge<kFdivBlock / 64>(mode, r, scratch);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

static __global__ __launch_bounds__(kFdivBlock) void fdiv_bound_bwd_kernel(const float* __restrict__ logits, int64_t n,
                                                                           int64_t pos, int mode,
                                                                           const mi_stats* __restrict__ stats,
                                                                           const float* __restrict__ grad_out,
                                                                           float* __restrict__ grad) {
  const FdivGrad p = fdiv_grad_params(mode, stats, grad_out ? grad_out[0] : 1.0f);
  const int64_t stride = (int64_t)gridDim.x * kFdivBlock;
  for (int64_t k = (int64_t)blockIdx.x * kFdivBlock + threadIdx.x; k < n; k += stride)
    grad[k] = fdiv_pair_grad(p, k < pos ? 1 : 2, logits[k]);
}

static __global__ __launch_bounds__(kFdivBlock) void fdiv_matrix_bwd_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ sid_rows, const int64_t* __restrict__ sid_cols,
    int64_t b_rows, int64_t b, int64_t row_offset, int mode, const mi_stats* __restrict__ stats,
    const float* __restrict__ grad_out, float* __restrict__ grad) {
  const FdivGrad p = fdiv_grad_params(mode, stats, grad_out ? grad_out[0] : 1.0f);
  for (int64_t i = blockIdx.x; i < b_rows; i += gridDim.x) {
    const int64_t si = sid_rows[i], gi = row_offset + i;
    for (int64_t j = threadIdx.x; j < b; j += kFdivBlock)
      grad[i * b + j] = fdiv_pair_grad(p, pair_kind(gi, j, si, sid_cols[j]), scores[i * b + j]);
  }
}

// One workgroup: records [n_rec] merged in a fixed order -> loss_out[0], terms_out[0..1] (positive-pair and negative-pair
// terms, optional) and the statistics block (include/mi_critic.h, fdiv family).  The float32 constants follow the DV
// finalisation (logf((float)n_neg)).
static __global__ __launch_bounds__(kFdivBlock) void fdiv_finalize_kernel(const FdivRec* __restrict__ recs, int64_t n_rec,
                                                                          int64_t n_pos, int mode, float* loss_out,
                                                                          float* terms_out, mi_stats* stats) {
  __shared__ FdivRec scratch[kFdivBlock / 64];
  __shared__ unsigned long long cnt_scratch[kFdivBlock / 64];
  FdivRec r = fdiv_empty(mode);
  unsigned long long cnt = 0;
  for (int64_t k = threadIdx.x; k < n_rec; k += kFdivBlock) {
    FdivRec q = recs[k];
    cnt += q.cnt;
    q.cnt = 0;
    fdiv_merge(mode, r, q);
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) cnt_scratch[threadIdx.x >> 6] = cnt;
  r = fdiv_block_merge<kFdivBlock / 64>(mode, r, scratch);
  if (threadIdx.x != 0) return;
  unsigned long long total = 0;
  for (int w = 0; w < kFdivBlock / 64; ++w) total += cnt_scratch[w];
  const float log_n = logf((float)total);
  float pos_term, neg_term;
  if (mode == MI_FDIV_JSD) {
    pos_term = r.pos / (float)n_pos;
    neg_term = r.a / (float)total;  // no negatives: 0 / 0 = NaN, as the definition
  } else {
    const float lse = (r.b > 0.0f) ? r.a + logf(r.b) : MI_NEG_INF;
    pos_term = -(r.pos / (float)n_pos);
    neg_term = expf((lse - log_n) - 1.0f);  // no negatives: -inf - (-inf) = NaN
  }
  const float loss = pos_term + neg_term;
  if (loss_out) loss_out[0] = loss;
  if (terms_out) {
    terms_out[0] = pos_term;
    terms_out[1] = neg_term;
  }
  stats->lse = mode == MI_FDIV_NWJ ? 1.0f + log_n : 0.0f;
  stats->pos_mean = pos_term;
  stats->loss_dv = stats->loss_infonce = loss;
  stats->log_n_neg = log_n;
  stats->neg_max = mode == MI_FDIV_NWJ ? r.a : 0.0f;
  stats->reserved0 = neg_term;
  stats->reserved1 = 0.0f;
  stats->n_neg = (int64_t)total;
  stats->n_pos = n_pos;
  stats->reserved2 = stats->reserved3 = 0;
}

// ---- score-GEMM epilogues ------------------------------------------------------------------------------------------
// acc element (tm, tn, r) of this lane is S[mb + tm 32 + (r & 3) + 8 (r >> 2) + 4 half, nb + tn 32 + (lane & 31)]
// (MFMA 32x32 C/D layout).  Local row i is global sample row_offset + i.
struct FdivStatsOut {
  const int64_t* sid_rows;
  const int64_t* sid_cols;
  int64_t row_offset;
  int mode;
  FdivRec* rec;  // [n_rt][n_ct]: one record per 64 x 64 tile
  int64_t n_ct;
};

__device__ __forceinline__ void fdiv_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                const FdivStatsOut& o) {
  if (mb >= M || nb >= N) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  int64_t sc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? o.sid_cols[col] : 0;
  }
  FdivRec r = fdiv_empty(o.mode);
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t row = mb + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
      if (row >= M) continue;
      const int64_t sr = o.sid_rows[row];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        if (!cok[tn]) continue;
        fdiv_push(o.mode, r, pair_kind(row + o.row_offset, nb + tn * 32 + col_l, sr, sc[tn]), acc[tm][tn][q]);
      }
    }
  fdiv_wave_merge(o.mode, r);
  if (lane == 0) o.rec[(mb >> 6) * o.n_ct + (nb >> 6)] = r;
}

struct FdivGradIn {
  const int64_t* sid_rows;
  const int64_t* sid_cols;
  int64_t row_offset;
  int mode;
  const mi_stats* stats;  // the forward's (device)
  const float* grad_out;  // [1] or null (1)
};

__device__ __forceinline__ void fdiv_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                               const FdivGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const FdivGrad p = fdiv_grad_params(g.mode, g.stats, g.grad_out ? g.grad_out[0] : 1.0f);
  int64_t sc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    sc[tn] = cok[tn] ? g.sid_cols[col] : 0;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t row = mb + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? g.sid_rows[row] : 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int kind = (rok && cok[tn]) ? pair_kind(row + g.row_offset, nb + tn * 32 + col_l, sr, sc[tn]) : 0;
        acc[tm][tn][q] = fdiv_pair_grad(p, kind, acc[tm][tn][q]);
      }
    }
}

// score GEMM epilogue (both call forms: the generic kernels' and the 16-bit chain's)
struct EpiFdivStats {
  static constexpr bool kReducesPartial = false;
  FdivStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    fdiv_tile_stats(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    fdiv_tile_stats(acc, mb, nb, M, N, o);
  }
};

// recompute epilogue of the generic kernels: G as TG [M][N]
template <typename TG>
struct EpiFdivGrad {
  FdivGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    fdiv_tile_grad(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute epilogue of the 16-bit chain: G and G^T as bf16 (bf16x3: split parts), as EpiNceGrad2
struct EpiFdivGrad2 {
  static constexpr bool kReducesPartial = false;
  FdivGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    fdiv_tile_grad(acc, mb, nb, M, N, in);
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

// ---- host side -----------------------------------------------------------------------------------------------------
static inline int fdiv_check_mode(const char* fn, int mode) {
  MI_CHECK_ARG(mode == MI_FDIV_JSD || mode == MI_FDIV_NWJ, "%s: unknown mode %d (MI_FDIV_JSD, MI_FDIV_NWJ)", fn, mode);
  return MI_OK;
}

static inline int launch_fdiv_finalize(const FdivRec* recs, int64_t n_rec, int64_t n_pos, int mode, float* loss_out,
                                       float* terms_out, mi_stats* stats, hipStream_t st) {
  {
    ProfScope prof_("fdiv_finalize_kernel", st);
    hipLaunchKernelGGL(fdiv_finalize_kernel, dim3(1), dim3(kFdivBlock), 0, st, recs, n_rec, n_pos, mode, loss_out,
                       terms_out, stats);
  }
  MI_LAUNCH_CHECK("fdiv_finalize_kernel");
  return MI_OK;
}

// the row block [b_rows] x [b] of a materialised score matrix -> records [grid] -> finalize
static inline int fdiv_matrix_forward(const float* scores, const int64_t* sid_rows, const int64_t* sid_cols,
                                      int64_t b_rows, int64_t b, int64_t row_offset, int64_t n_pos, int mode,
                                      FdivRec* recs, float* loss_out, float* terms_out, mi_stats* stats, hipStream_t st) {
  const int grid = (int)(b_rows < kFdivMaxBlocks ? (b_rows < 1 ? 1 : b_rows) : kFdivMaxBlocks);
  {
    ProfScope prof_("fdiv_matrix_partials_kernel", st);
    hipLaunchKernelGGL(fdiv_matrix_partials_kernel, dim3(grid), dim3(kFdivBlock), 0, st, scores, sid_rows, sid_cols, b_rows,
                       b, row_offset, mode, recs);
  }
  MI_LAUNCH_CHECK("fdiv_matrix_partials_kernel");
  return launch_fdiv_finalize(recs, grid, n_pos, mode, loss_out, terms_out, stats, st);
}

}  // namespace mi
