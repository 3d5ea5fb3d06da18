// MI estimates of a trained critic from one forward sweep: DV, NWJ, JSD, the two per-sample
// InfoNCE bounds and SMILE (clipped DV) at up to MI_EST_MAX_TAUS clips, on the reference's pairs: n_pos = b positives
// (i, i), n_neg negatives (i, j), i != j, sid_i != sid_j; equal-id off-diagonal pairs are dropped.  Estimates, not losses:
// higher means more MI, in nats.  Forward only, nothing here is differentiated.
//   dv      = mean_pos s - (LSE_neg s - log n_neg)              nwj = mean_pos s - exp(LSE_neg s - log n_neg - 1)
//   jsd     = -(mean_pos sp(-s) + mean_neg sp(s))               smile[k] = mean_pos s - (log sum_neg exp(clip(s, +-tau_k)) - log n_neg)
//   nce_i2t = (1/b) sum_i (S_ii - r_i + log |C_i|)              nce_t2i = (1/b) sum_j (S_jj - c_j + log |R_j|)
// r_i, c_j, C_i, R_j are the per-sample InfoNCE's (mi_nce.h); |C_i| = |R_i| = b + 1 - #{j : sid_j == sid_i}.
// SMILE sums exp(clip(s, -tau, tau)) as it stands: tau <= 40 keeps every term in [e^-40, e^40] = [4.2e-18, 2.4e17],
// normal fp32 numbers, and fewer than 2^62 of them sum to less than 1.1e36 < FLT_MAX, so a plain sum needs no running
// maximum and no shift (a shift by tau was measured: s - 40 rounds to ulp(40) = 3.8e-6 and the log lands near -30, which
// cost 2.6e-6 on an O(1) estimate).
// Building blocks:
//   est_tile_stats:      one 64 x 64 wave tile (MFMA accumulator layout) -> one EstRec of the tile (fdiv_push in both of
//                        its modes, the negatives' sum and the clipped sums), then nce_tile_stats' row / column records
//   est_matrix_kernel:   the same device function on a tile of a caller's fp32 [b][b] matrix
//   est_merge_kernel:    sample i: its row and its column records in tile order -> r_i, c_i, |C_i| -> the two terms
//   est_finalize_kernel: one workgroup: the tile records and the 2b terms in a fixed order -> the MI_EST_FLOATS outputs
// No float atomics, 64-bit negative count: two calls give identical bits.
#pragma once
#include <type_traits>

#include "mi_common.h"
#include "mi_fdiv.h"
#include "mi_nce.h"

namespace mi {

// the clips, by value in the kernel arguments
struct EstTaus {
  int n;
  float t[MI_EST_MAX_TAUS];
};

// partial sums of one 64 x 64 tile
struct EstRec {
  float m, s;                   // negatives: (max, sum exp(v - max))
  float sp_neg, sum_neg;        // sum_neg sp(v), sum_neg v
  float sum_pos, sp_pos;        // sum_pos v, sum_pos sp(-v)
  unsigned cnt;                 // negatives
  float clip[MI_EST_MAX_TAUS];  // sum_neg exp(clip(v, -tau_k, tau_k))
  unsigned pad;
};

struct EstStatsOut {
  NceStatsOut nce;  // the whole batch: row_offset == 0, sid_rows == sid_cols
  EstRec* rec;      // [n_rt][n_ct]
  EstTaus taus;
};

// acc element (tm, tn, r) of this lane is S[mb + tm 32 + (r & 3) + 8 (r >> 2) + 4 half, nb + tn 32 + (lane & 31)]
// (MFMA 32x32 C/D layout).  Consumes acc.  No block-level barrier: any wave may call it alone.  FAST selects the
// exponential of the row / column records only (nce_tile_stats); the tile record takes the exact one, as fdiv_tile_stats.
template <bool FAST>
__device__ __forceinline__ void est_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                               const EstStatsOut& o) {
  if (mb < M && nb < N) {  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int col_l = lane & 31, half = lane >> 5;
    int64_t sc[2];
    bool cok[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = nb + tn * 32 + col_l;
      cok[tn] = col < N;
      sc[tn] = cok[tn] ? o.nce.sid_cols[col] : 0;
    }
    // f(kind, score) for every element of the tile inside M x N.  The loop over the two 32-row halves is written out (tm
    // is a template constant) and the record takes two passes: with the exact exponentials and log1p of all 64 elements
    // in one loop nest the compiler gives up unrolling it, and acc, indexed at run time, goes to scratch.
    auto half_pass = [&](auto tm_c, auto f) {
      constexpr int tm = decltype(tm_c)::value;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = mb + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
        if (row >= M) continue;
        const int64_t sr = o.nce.sid_rows[row];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          if (!cok[tn]) continue;
          f(pair_kind(row, nb + tn * 32 + col_l, sr, sc[tn]), acc[tm][tn][q]);
        }
      }
    };
    auto each_pair = [&](auto f) {
      half_pass(std::integral_constant<int, 0>{}, f);
      half_pass(std::integral_constant<int, 1>{}, f);
    };
    FdivRec rj = fdiv_empty(MI_FDIV_JSD), rn = fdiv_empty(MI_FDIV_NWJ);
    float sum_neg = 0.0f;
    float clip[MI_EST_MAX_TAUS] = {};
    each_pair([&](int kind, float v) {
      fdiv_push(MI_FDIV_NWJ, rn, kind, v);
      if (kind == 2) {
        sum_neg += v;
#pragma unroll
        for (int k = 0; k < MI_EST_MAX_TAUS; ++k)
          if (k < o.taus.n) clip[k] += expf(fminf(fmaxf(v, -o.taus.t[k]), o.taus.t[k]));
      }
    });
    each_pair([&](int kind, float v) { fdiv_push(MI_FDIV_JSD, rj, kind, v); });
    fdiv_wave_merge(MI_FDIV_JSD, rj);
    fdiv_wave_merge(MI_FDIV_NWJ, rn);
    sum_neg = wave_sum(sum_neg);
#pragma unroll
    for (int k = 0; k < MI_EST_MAX_TAUS; ++k) clip[k] = wave_sum(clip[k]);
    if (lane == 0) {
      EstRec r;
      r.m = rn.a;
      r.s = rn.b;
      r.sp_neg = rj.a;
      r.sum_neg = sum_neg;
      r.sum_pos = rn.pos;
      r.sp_pos = rj.pos;
      r.cnt = rn.cnt;
#pragma unroll
      for (int k = 0; k < MI_EST_MAX_TAUS; ++k) r.clip[k] = clip[k];
      r.pad = 0u;
      o.rec[(mb >> 6) * o.nce.n_ct + (nb >> 6)] = r;
    }
  }
  nce_tile_stats<FAST>(acc, mb, nb, M, N, o.nce);
}

// score GEMM epilogue (both call forms: the generic kernels' and the 16-bit chain's; not a reducing epilogue there: every
// wave writes its own records)
template <bool FAST>
struct EpiEstStats {
  static constexpr bool kReducesPartial = false;
  EstStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    est_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    est_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
};

// ------------------------------------------------------------------------------------------------ materialised scores
// one wave per 64 x 64 tile of a caller's fp32 [b][b] matrix, in the accumulator layout (exact expf)
static __global__ __launch_bounds__(64) void est_matrix_kernel(const float* __restrict__ s, int64_t b, EstStatsOut o) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  est_tile_stats<false>(acc, mb, nb, b, b, o);
}

// ------------------------------------------------------------------------------------------------ merge, finalize
// A workgroup serves kEstMergeSamples samples.  First the candidate count from the ids: the workgroup walks all b ids in
// chunks of 256 through LDS and thread (slice, sample) compares the sample's id with 16 ids of every chunk; the 16 slices
// of a sample meet in LDS (integer counts, any order).  Then one thread per sample merges row i's and column i's records
// in tile order, as nce_merge_kernel.  terms[i] = S_ii - r_i + log |C_i|, terms[b + i] = S_ii - c_i + log |R_i|.  A
// sample whose only candidate is its own positive gets r_i == S_ii and log 1: exactly 0.
constexpr int kEstMergeSamples = 16;
static __global__ __launch_bounds__(256) void est_merge_kernel(const NceRec* __restrict__ rowp,
                                                               const NceRec* __restrict__ colp,
                                                               const float* __restrict__ diag,
                                                               const int64_t* __restrict__ sid, int64_t b, int64_t n_t,
                                                               float* __restrict__ terms) {
  __shared__ int64_t ids[256];
  __shared__ int cnt[256 / kEstMergeSamples][kEstMergeSamples];
  const int tid = threadIdx.x, sample = tid % kEstMergeSamples, slice = tid / kEstMergeSamples;
  const int64_t i = (int64_t)blockIdx.x * kEstMergeSamples + sample;
  const bool ok = i < b;
  const int64_t si = ok ? sid[i] : 0;
  int same = 0;  // (at most b / 16 < 2^27)
  for (int64_t j0 = 0; j0 < b; j0 += 256) {  // (uniform trip count: every thread reaches the barriers)
    __syncthreads();
    ids[tid] = j0 + tid < b ? sid[j0 + tid] : 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = slice * 16 + q;
      same += (j0 + e < b && ids[e] == si) ? 1 : 0;
    }
  }
  cnt[slice][sample] = same;
  __syncthreads();
  if (slice != 0 || !ok) return;
  int64_t total = 0;
  for (int q = 0; q < 256 / kEstMergeSamples; ++q) total += cnt[q][sample];
  float lse[2];
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const NceRec* p = (side == 0 ? rowp : colp) + i * n_t;
    float m = MI_NEG_INF, s = 0.0f;
    for (int64_t t = 0; t < n_t; ++t) lse_merge(m, s, p[t].m, p[t].s);
    lse[side] = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  }
  const float log_c = logf((float)(b + 1 - total));
  const float d = diag[i];
  terms[i] = (d - lse[0]) + log_c;
  terms[b + i] = (d - lse[1]) + log_c;
}

constexpr int kEstBlock = 256;

// what the finalize step carries per thread: an EstRec with a 64-bit count
struct EstAcc {
  float m, s;
  float f[4 + MI_EST_MAX_TAUS];  // sp_neg, sum_neg, sum_pos, sp_pos, clip[]
  unsigned long long cnt;
};
__device__ __forceinline__ void est_acc_merge(EstAcc& r, const EstAcc& q) {
  lse_merge(r.m, r.s, q.m, q.s);
#pragma unroll
  for (int k = 0; k < 4 + MI_EST_MAX_TAUS; ++k) r.f[k] += q.f[k];
  r.cnt += q.cnt;
}

// One workgroup.  Tile records [n_rec]: thread t takes records t, t + 256, ... in order, then a butterfly over the wave,
// then the four waves in order (fixed everywhere).  The 2b per-sample terms: the order of nce_loss_kernel.  Writes all
// MI_EST_FLOATS outputs; the float constants follow the DV and fdiv finalisations (logf of a float count).
static __global__ __launch_bounds__(kEstBlock) void est_finalize_kernel(const EstRec* __restrict__ recs, int64_t n_rec,
                                                                        const float* __restrict__ terms, int64_t b,
                                                                        EstTaus taus, float* __restrict__ est_out) {
  __shared__ EstAcc scratch[kEstBlock / 64];
  __shared__ float red[2][kEstBlock];
  const int tid = threadIdx.x;
  EstAcc r;
  r.m = MI_NEG_INF;
  r.s = 0.0f;
#pragma unroll
  for (int k = 0; k < 4 + MI_EST_MAX_TAUS; ++k) r.f[k] = 0.0f;
  r.cnt = 0;
  for (int64_t k = tid; k < n_rec; k += kEstBlock) {
    const EstRec e = recs[k];
    EstAcc q;
    q.m = e.m;
    q.s = e.s;
    q.f[0] = e.sp_neg;
    q.f[1] = e.sum_neg;
    q.f[2] = e.sum_pos;
    q.f[3] = e.sp_pos;
#pragma unroll
    for (int t = 0; t < MI_EST_MAX_TAUS; ++t) q.f[4 + t] = e.clip[t];
    q.cnt = e.cnt;
    est_acc_merge(r, q);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    EstAcc q;
    q.m = __shfl_xor(r.m, o);
    q.s = __shfl_xor(r.s, o);
#pragma unroll
    for (int k = 0; k < 4 + MI_EST_MAX_TAUS; ++k) q.f[k] = __shfl_xor(r.f[k], o);
    q.cnt = __shfl_xor(r.cnt, o);
    est_acc_merge(r, q);
  }
  if ((tid & 63) == 0) scratch[tid >> 6] = r;
  float sr = 0.0f, sc = 0.0f;
  for (int64_t i = tid; i < b; i += kEstBlock) {
    sr += terms[i];
    sc += terms[b + i];
  }
  red[0][tid] = sr;
  red[1][tid] = sc;
  __syncthreads();
  for (int off = kEstBlock / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  for (int w = 1; w < kEstBlock / 64; ++w) est_acc_merge(r, scratch[w]);
  const float fb = (float)b, fn = (float)r.cnt;
  const float log_n = logf(fn);  // no negatives: -inf
  const float lse = r.s > 0.0f ? r.m + logf(r.s) : MI_NEG_INF;
  const float pos_mean = r.f[2] / fb;
  est_out[MI_EST_DV] = pos_mean - (lse - log_n);               // no negatives: -inf - (-inf) = NaN
  est_out[MI_EST_NWJ] = pos_mean - expf((lse - log_n) - 1.0f);
  est_out[MI_EST_JSD] = -(r.f[3] / fb + r.f[0] / fn);          // 0 / 0 = NaN
  est_out[MI_EST_NCE_I2T] = red[0][0] / fb;
  est_out[MI_EST_NCE_T2I] = red[1][0] / fb;
  est_out[MI_EST_POS_MEAN] = pos_mean;
  est_out[MI_EST_NEG_MEAN] = r.f[1] / fn;
  est_out[MI_EST_LOG_N_NEG] = log_n;
  for (int k = 0; k < MI_EST_MAX_TAUS; ++k) {
    const float v = pos_mean - (logf(r.f[4 + k]) - log_n);  // no negatives: log 0 = -inf, and -inf - (-inf) = NaN
    est_out[MI_EST_SMILE + k] = k < taus.n ? v : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct EstPlan {
  NceRec* rowp;  // [b][n_t]
  NceRec* colp;  // [b][n_t]
  float *diag, *terms;
  EstRec* rec;  // [n_t][n_t]
  int64_t n_t;
};

static inline EstPlan plan_est(Workspace& ws, int64_t b) {
  EstPlan q{};
  q.n_t = (b + 63) / 64;
  q.rowp = ws.take<NceRec>(b * q.n_t);
  q.colp = ws.take<NceRec>(b * q.n_t);
  q.diag = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  q.rec = ws.take<EstRec>(q.n_t * q.n_t);
  return q;
}

static inline EstStatsOut est_stats_out(const EstPlan& q, const int64_t* sid, const EstTaus& taus) {
  return EstStatsOut{NceStatsOut{sid, sid, 0, q.rowp, q.colp, q.diag, q.n_t, q.n_t}, q.rec, taus};
}

// the clips of a call: a host array, read now.  n_tau in [0, MI_EST_MAX_TAUS], every tau finite in (0, 40].
static inline int est_read_taus(const char* fn, const float* taus_host, int n_tau, EstTaus& out) {
  MI_CHECK_ARG(n_tau >= 0 && n_tau <= MI_EST_MAX_TAUS, "%s: n_tau must be in [0, %d] (got %d)", fn, MI_EST_MAX_TAUS, n_tau);
  MI_CHECK_ARG(n_tau == 0 || taus_host, "%s: null pointer (taus_host with n_tau %d)", fn, n_tau);
  out.n = n_tau;
  for (int k = 0; k < MI_EST_MAX_TAUS; ++k) out.t[k] = 1.0f;
  for (int k = 0; k < n_tau; ++k) {
    const float t = taus_host[k];
    MI_CHECK_ARG(t > 0.0f && t <= 40.0f, "%s: tau[%d] = %g is outside (0, 40]", fn, k, (double)t);  // (NaN fails both)
    out.t[k] = t;
  }
  return MI_OK;
}

// records -> the per-sample terms -> the outputs
static inline int est_finish(const EstPlan& q, const int64_t* sid, int64_t b, const EstTaus& taus, float* est_out,
                             hipStream_t st) {
  {
    ProfScope prof_("est_merge_kernel", st);
    const unsigned grid = (unsigned)((b + kEstMergeSamples - 1) / kEstMergeSamples);
    hipLaunchKernelGGL(est_merge_kernel, dim3(grid), dim3(256), 0, st, q.rowp, q.colp, q.diag, sid, b, q.n_t, q.terms);
  }
  MI_LAUNCH_CHECK("est_merge_kernel");
  {
    ProfScope prof_("est_finalize_kernel", st);
    hipLaunchKernelGGL(est_finalize_kernel, dim3(1), dim3(kEstBlock), 0, st, q.rec, q.n_t * q.n_t, q.terms, b, taus,
                       est_out);
  }
  MI_LAUNCH_CHECK("est_finalize_kernel");
  return MI_OK;
}

static inline int est_matrix(const float* scores, const int64_t* sid, int64_t b, const EstTaus& taus, float* est_out,
                             const EstPlan& q, hipStream_t st) {
  {
    ProfScope prof_("est_matrix_kernel", st);
    hipLaunchKernelGGL(est_matrix_kernel, dim3((unsigned)q.n_t, (unsigned)q.n_t), dim3(64), 0, st, scores, b,
                       est_stats_out(q, sid, taus));
  }
  MI_LAUNCH_CHECK("est_matrix_kernel");
  return est_finish(q, sid, b, taus, est_out, st);
}

}  // namespace mi
