// Soft-target InfoNCE from finding-label bit masks: the row-wise / symmetric InfoNCE whose target
// distribution of row i puts weight on every report in proportion to how similar its finding set is to that of image i.
//   lab_i: int64 whose low 63 bits are a multi-hot set of findings (bit 63 is masked off),  n_i = popcount(lab_i)
//   a_ij  = popcount(lab_i & lab_j) / sqrt(n_i n_j)   (0 where n_i n_j = 0);  a_ii := 1 always
//   k_ij  = exp((a_ij - 1) / tau)                      (<= 1, k_ii = 1, k_ij == k_ji bit for bit)
//   z_i   = sum_j k_ij                                 (>= 1; serves rows and, k being symmetric, columns)
//   qr_ij = (1 - mix) delta_ij + mix k_ij / z_i        qc_ij = (1 - mix) delta_ij + mix k_ij / z_j
//   r_i = log sum_{j < B} exp S[i, j],  c_j = log sum_{i < B} exp S[i, j]                        (nothing is masked)
//   row term t_i = r_i - sum_j qr_ij S[i, j],  column term t'_j = c_j - sum_i qc_ij S[i, j]
//   rowwise: L = (1/B) sum_i t_i;  symmetric: L = 1/2 (1/B) sum_i t_i + 1/2 (1/B) sum_j t'_j
//   dL/dS[i, j] = wr (exp(S[i, j] - r_i) - qr_ij) + wc (exp(S[i, j] - c_j) - qc_ij)
//   (wr, wc) = (1/B, 0) or (1/(2B), 1/(2B))
// mix = 0 IS the per-sample InfoNCE on unique ids (mi_nce.h).  Every mask equal and mix = 1: the study-positive loss
// (mi_posnce.h) with all ids equal.  All masks zero: uniform smoothing of weight exp(-1/tau) off the diagonal.  B == 1:
// loss exactly 0 and exact-zero gradients.  Each row's share of dL/dS sums to zero.  A training loss, not an MI bound.
// fp32 arithmetic of the weights: a_ij = popcount * (rs_i * rs_j) with rs = 1 / sqrt(n) per sample (0 where n = 0), the
// product of the two per-sample factors first: commutative, so k_ij == k_ji exactly and one z serves both sides.  The
// diagonal weight is formed as 1 - mix (1 - 1/z_i), which is exactly 1 where z_i = 1 (B == 1, mix = 0).
// Building blocks (written for the MFMA 32x32 accumulator layout that nce_tile_stats documents):
//   softnce_label_norm_kernel: masks -> z, 1/z, rs (one wave per sample, fixed order, no atomics); runs before the score
//                        GEMM, so both epilogues form the final q directly
//   softnce_tile_stats:  one 64 x 64 wave tile -> per-row (max, sum exp) over ALL in-range columns of the tile and the
//                        tile's share of sum_j qr_ij S[i, j]; the same per column with qc
//   softnce_merge_kernel: the records of every tile, in tile order -> r, c, the per-sample terms -> nce_loss_kernel
//                        (fixed order everywhere, no float atomics: bit-reproducible)
//   softnce_tile_grad:   one wave tile of recomputed scores -> G = grad_out * dL/dS
//   EpiSoftNceStats<FAST> / EpiSoftNceGrad<TG> / EpiSoftNceGrad2: the epilogues of the score GEMM and of the G GEMM on the
//                        generic kernels and on the 16-bit chain
// FAST takes the k exponentials through nce_exp<true> in the label-norm kernel and in both epilogues alike, so
// sum_j q_ij = 1 holds to rounding on either path.
// Row blocks (the sharded step): the tiles of rows [row_offset, row_offset + M) of the global B x B
// matrix; local row i is global sample row_offset + i, so its diagonal (a_ii := 1) is column row_offset + i and its z, rs
// are entries row_offset + i of the per-sample arrays, which every rank computes for ALL B samples from the gathered
// masks (same inputs, same order: same bits everywhere).  The whole batch is row_offset == 0, lab_rows == lab_cols.
//   softnce_rank_part_kernel:   a rank's records -> r (kept), one flat part (column partials, row terms)
//   softnce_merge_parts_kernel: the parts of every rank, in rank order -> c, the per-sample terms -> nce_loss_kernel
#pragma once
#include "mi_nce.h"

namespace mi {

struct SoftNceStatsOut {
  const int64_t* lab_rows;  // [M]
  const int64_t* lab_cols;  // [N] (the whole batch: the same array)
  int64_t row_offset;       // global index of local row 0
  const float* rs;          // [N] 1 / sqrt(n_i) of every global sample, 0 where n_i = 0
  const float* inv_z;       // [N] 1 / z_i of every global sample
  NceRec* rowp;             // [M][n_ct]: row i over the columns of tile t
  NceRec* colp;             // [N][n_rt]: column j over the rows of tile t
  float* rowq;              // [M][n_ct]: sum of qr_ij S[i, j] over the columns of tile t
  float* colq;              // [N][n_rt]: sum of qc_ij S[i, j] over the rows of tile t
  int64_t n_ct, n_rt;
  float inv_tau, mix;
};

struct SoftNceGradIn {
  const int64_t* lab_rows;  // [M]
  const int64_t* lab_cols;  // [N]
  int64_t row_offset;
  const float* rs;          // [N] of every global sample, or null: then from the masks
  const float* inv_z;       // [N] 1 / z_i of every global sample, or null: then from z
  const float* z;           // [N] z_i (read where inv_z is null)
  const float* r;           // [M] row LSE
  const float* c;           // [N] column LSE (symmetric mode)
  const float* grad_out;    // [1] or null (1)
  float wr, wc;             // 1/B, 0 (rowwise) or 1/(2B), 1/(2B) (symmetric); B is the global batch
  float inv_tau, mix;
};

// the finding set of a sample: bit 63 is ignored
__device__ __forceinline__ uint64_t softnce_mask(int64_t lab) { return (uint64_t)lab & 0x7fffffffffffffffull; }

// 1 / sqrt(n) of a set of n findings, 0 for the empty set.  The only place this value is formed.
__device__ __forceinline__ float softnce_rs_of_count(int n) { return n > 0 ? 1.0f / sqrtf((float)n) : 0.0f; }

// k_ij off the diagonal.  rr = rs_i * rs_j (commutative); the minimum stops contraction and keeps k <= 1.
template <bool FAST>
__device__ __forceinline__ float softnce_k(uint64_t li, uint64_t lj, float rr, float inv_tau) {
  const float a = fminf((float)__popcll(li & lj) * rr, 1.0f);
  return nce_exp<FAST>(fmaf(a, inv_tau, -inv_tau));
}

// ------------------------------------------------------------------------------------------------ label norm
// One wave per sample i: lane l adds k_ij over j = l, l + 64, ... in that order, then a butterfly over the 64 lanes.
// rs of every count 0 .. 63 once per block in LDS.
template <bool FAST>
static __global__ __launch_bounds__(256) void softnce_label_norm_kernel(const int64_t* __restrict__ lab, int64_t b,
                                                                        float inv_tau, float* __restrict__ z_ws,
                                                                        float* __restrict__ inv_z, float* __restrict__ rs,
                                                                        float* __restrict__ z_out, int64_t out_lo,
                                                                        int64_t out_n) {
  __shared__ float rs_of[64];
  if (threadIdx.x < 64) rs_of[threadIdx.x] = softnce_rs_of_count((int)threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= b) return;  // wave-uniform, behind the only barrier
  const uint64_t li = softnce_mask(lab[i]);
  const float rsi = rs_of[__popcll(li)];
  float s = 0.0f;
  for (int64_t j = lane; j < b; j += 64) {
    const uint64_t lj = softnce_mask(lab[j]);
    s += j == i ? 1.0f : softnce_k<FAST>(li, lj, rsi * rs_of[__popcll(lj)], inv_tau);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) {
    z_ws[i] = s;
    inv_z[i] = 1.0f / s;
    rs[i] = rsi;
    if (z_out && i >= out_lo && i < out_lo + out_n) z_out[i - out_lo] = s;  // the caller's rows [out_lo, out_lo + out_n)
  }
}

// ------------------------------------------------------------------------------------------------ tiles
// acc element (tm, tn, r) of this lane: as nce_tile_stats.  Consumes acc.  No block-level barrier.
template <bool FAST>
__device__ __forceinline__ void softnce_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                   const SoftNceStatsOut& o) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  uint64_t lc[2];
  float rsc[2], mc[2], dc[2], qcs[2] = {0.0f, 0.0f};
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    lc[tn] = cok[tn] ? softnce_mask(o.lab_cols[col]) : 0ull;
    rsc[tn] = cok[tn] ? o.rs[col] : 0.0f;
    const float iz = cok[tn] ? o.inv_z[col] : 0.0f;
    mc[tn] = o.mix * iz;
    dc[tn] = 1.0f - o.mix * (1.0f - iz);
  }
  // one pass over the rows: the only mask (elements outside M x N become -inf), the row records and the row share of
  // sum q S by butterflies over the 32 lanes of a half (two values per lane), the column share in qcs
  const bool rows = nb < N;
  const int64_t t = nb >> 6;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const uint64_t lr = rok ? softnce_mask(o.lab_rows[row]) : 0ull;
      const float rsr = rok ? o.rs[row + o.row_offset] : 0.0f;
      const float izr = rok ? o.inv_z[row + o.row_offset] : 0.0f;
      const float mr = o.mix * izr, dr = 1.0f - o.mix * (1.0f - izr);
      float qrs = 0.0f;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        if (rok && cok[tn]) {
          const bool dg = row + o.row_offset == col;
          const float k = softnce_k<FAST>(lr, lc[tn], rsr * rsc[tn], o.inv_tau);
          qrs += (dg ? dr : mr * k) * v;
          qcs[tn] += (dg ? dc[tn] : mc[tn] * k) * v;
        } else {
          acc[tm][tn][r] = MI_NEG_INF;
        }
      }
      if (rows) {
        const float a0 = acc[tm][0][r], a1 = acc[tm][1][r];
        float m = fmaxf(a0, a1);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float s = m == MI_NEG_INF ? 0.0f : nce_exp<FAST>(a0 - m) + nce_exp<FAST>(a1 - m);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
          s += __shfl_xor(s, off);
          qrs += __shfl_xor(qrs, off);
        }
        if (col_l == 0 && rok) {
          o.rowp[row * o.n_ct + t] = NceRec{m, s};
          o.rowq[row * o.n_ct + t] = qrs;
        }
      }
    }
  // columns: 32 of a column's 64 values in one lane, the other 32 in the lane of the other half
  if (mb < M) {
    const int64_t tr = mb >> 6;
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
      const float q = qcs[tn] + __shfl_xor(qcs[tn], 32);
      const int64_t col = nb + tn * 32 + col_l;
      if (half == 0 && col < N) {
        o.colp[col * o.n_rt + tr] = NceRec{m, s};
        o.colq[col * o.n_rt + tr] = q;
      }
    }
  }
}

// exp(S - lse) - q of one element, q = (diagonal ? d : m k).  The rounding is written out, not left to the compiler's
// contraction: with the diagonal test of the whole batch (row == col) the compiler knew that the quadrants tm != tn of a
// wave tile hold no diagonal element and fused m k into the subtraction there, and only there.  A row block's diagonal
// crosses any quadrant, so the same choice is spelled out per quadrant: the whole-batch step keeps its bits and a row
// block that is the whole batch gives them too.
__device__ __forceinline__ float softnce_excess(bool off_quadrant, bool dg, float e, float d, float m, float k) {
  if (off_quadrant) return dg ? e - d : __fmaf_rn(-m, k, e);
  return e - (dg ? d : __fmul_rn(m, k));
}

// acc (scores) -> G = grad_out * dL/dS.  0 outside M x N.
template <bool FAST>
__device__ __forceinline__ void softnce_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                  const SoftNceGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const float go = g.grad_out ? g.grad_out[0] : 1.0f;
  const float wr = go * g.wr, wc = go * g.wc;
  const bool cols = g.wc != 0.0f;  // uniform: the symmetric mode
  uint64_t lc[2];
  float rsc[2], mc[2], dc[2], cc[2];
  bool cok[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t col = nb + tn * 32 + col_l;
    cok[tn] = col < N;
    lc[tn] = cok[tn] ? softnce_mask(g.lab_cols[col]) : 0ull;
    rsc[tn] = !cok[tn] ? 0.0f : g.rs ? g.rs[col] : softnce_rs_of_count(__popcll(lc[tn]));
    const float iz = !(cok[tn] && cols) ? 0.0f : g.inv_z ? g.inv_z[col] : 1.0f / g.z[col];
    mc[tn] = g.mix * iz;
    dc[tn] = 1.0f - g.mix * (1.0f - iz);
    cc[tn] = cok[tn] && cols ? g.c[col] : 0.0f;
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const uint64_t lr = rok ? softnce_mask(g.lab_rows[row]) : 0ull;
      const float rsr = !rok ? 0.0f : g.rs ? g.rs[row + g.row_offset] : softnce_rs_of_count(__popcll(lr));
      const float izr = !rok ? 0.0f : g.inv_z ? g.inv_z[row + g.row_offset] : 1.0f / g.z[row + g.row_offset];
      const float mr = g.mix * izr, dr = 1.0f - g.mix * (1.0f - izr);
      const float rr = rok ? g.r[row] : 0.0f;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int64_t col = nb + tn * 32 + col_l;
        const float v = acc[tm][tn][r];
        float gv = 0.0f;
        if (rok && cok[tn]) {
          const bool dg = row + g.row_offset == col;
          const float k = softnce_k<FAST>(lr, lc[tn], rsr * rsc[tn], g.inv_tau);
          gv = __fmul_rn(wr, softnce_excess(tm != tn, dg, nce_exp<FAST>(v - rr), dr, mr, k));
          if (cols) gv = __fmaf_rn(wc, softnce_excess(tm != tn, dg, nce_exp<FAST>(v - cc[tn]), dc[tn], mc[tn], k), gv);
        }
        acc[tm][tn][r] = gv;
      }
    }
}

// score GEMM epilogue: both call forms, as EpiNceStats
template <bool FAST>
struct EpiSoftNceStats {
  static constexpr bool kReducesPartial = false;
  SoftNceStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    softnce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    softnce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
};

// recompute GEMM epilogue of the generic kernels: G as TG [M][N]
template <typename TG>
struct EpiSoftNceGrad {
  SoftNceGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    softnce_tile_grad<false>(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute GEMM epilogue of the 16-bit chain: G and G^T as bf16 (bf16x3: split parts), stores as EpiPosNceGrad2
struct EpiSoftNceGrad2 {
  static constexpr bool kReducesPartial = false;
  SoftNceGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    softnce_tile_grad<true>(acc, mb, nb, M, N, in);
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
// One wave per 64 x 64 tile of a caller's fp32 [b][b] score matrix through nce_load_tile (exact expf): the route for a
// critic without a GEMM form.
static __global__ __launch_bounds__(64) void softnce_matrix_stats_kernel(const float* __restrict__ s, int64_t b,
                                                                         SoftNceStatsOut o) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  softnce_tile_stats<false>(acc, mb, nb, b, b, o);
}

static __global__ __launch_bounds__(64) void softnce_matrix_grad_kernel(const float* __restrict__ s, int64_t b,
                                                                        SoftNceGradIn in, float* __restrict__ grad) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  softnce_tile_grad<false>(acc, mb, nb, b, b, in);
  foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
    if (row < b && col < b) grad[row * b + col] = v;
  });
}

// ------------------------------------------------------------------------------------------------ merge
// thread k < b: row k, b <= k < 2b: column k - b.  NceRecs merged and the q S shares added in tile order (exact expf /
// logf).
static __global__ __launch_bounds__(256) void softnce_merge_kernel(const NceRec* __restrict__ rowp,
                                                                   const NceRec* __restrict__ colp,
                                                                   const float* __restrict__ rowq,
                                                                   const float* __restrict__ colq, int64_t b, int64_t n_t,
                                                                   float* r_ws, float* c_ws, float* r_out, float* c_out,
                                                                   float* terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const bool is_row = k < b;
  const int64_t i = is_row ? k : k - b;
  const NceRec* p = (is_row ? rowp : colp) + i * n_t;
  const float* q = (is_row ? rowq : colq) + i * n_t;
  float m = MI_NEG_INF, s = 0.0f, qs = 0.0f;
  for (int64_t t = 0; t < n_t; ++t) {
    lse_merge(m, s, p[t].m, p[t].s);
    qs += q[t];
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  if (is_row) {
    r_ws[i] = lse;
    if (r_out) r_out[i] = lse;
  } else {
    c_ws[i] = lse;
    if (c_out) c_out[i] = lse;
  }
  terms[k] = lse - qs;
}

// ------------------------------------------------------------------------------------------------ row blocks
// The part of one rank (softnce_part_floats(br, b) floats, gathered in rank order by the caller):
//   [0, 2b)          column j: (m, s) over this rank's rows, merged in row-tile order (NceRec)
//   [2b, 3b)         column j: sum of qc_ij S[i, j] over this rank's rows i, in row-tile order
//   [3b, 3b + br)    row term t_i = r_i - sum_j qr_ij S[i, j] of local row i (complete on this rank)
__host__ __device__ inline int64_t softnce_part_floats(int64_t br, int64_t b) { return 3 * b + br; }

// thread k < br: local row k (records merged and q S shares added in tile order exactly as softnce_merge_kernel: the same
// r and term bits), br <= k < br + b: column k - br over this rank's row tiles
static __global__ __launch_bounds__(256) void softnce_rank_part_kernel(const NceRec* __restrict__ rowp,
                                                                       const NceRec* __restrict__ colp,
                                                                       const float* __restrict__ rowq,
                                                                       const float* __restrict__ colq, int64_t br,
                                                                       int64_t b, int64_t n_ct, int64_t n_rt, float* r_ws,
                                                                       float* r_out, float* __restrict__ part) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= br + b) return;
  const bool is_row = k < br;
  const int64_t i = is_row ? k : k - br;
  const int64_t n = is_row ? n_ct : n_rt;
  const NceRec* p = (is_row ? rowp : colp) + i * n;
  const float* q = (is_row ? rowq : colq) + i * n;
  float m = MI_NEG_INF, s = 0.0f, qs = 0.0f;
  for (int64_t t = 0; t < n; ++t) {
    lse_merge(m, s, p[t].m, p[t].s);
    qs += q[t];
  }
  if (!is_row) {
    part[2 * i] = m;
    part[2 * i + 1] = s;
    part[2 * b + i] = qs;
    return;
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  r_ws[i] = lse;
  if (r_out) r_out[i] = lse;
  part[3 * b + i] = lse - qs;
}

// parts [n_ranks][softnce_part_floats(br, b)] in rank order (rank g holds rows [g br, (g + 1) br)).  Thread k < b: the row
// term of sample k, copied; b <= k < 2b: column j = k - b, its (m, s) merged and its q S shares added in rank order from
// an empty (-inf, 0), 0 start -- exact for one rank, so one rank gives the bits of softnce_merge_kernel -- then c_j and
// its term.  Every rank runs this on the same gathered buffer: identical bits.
static __global__ __launch_bounds__(256) void softnce_merge_parts_kernel(const float* __restrict__ parts, int64_t n_ranks,
                                                                         int64_t br, int64_t b, float* c_out,
                                                                         float* __restrict__ terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const int64_t pf = softnce_part_floats(br, b);
  if (k < b) {
    terms[k] = parts[(k / br) * pf + 3 * b + k % br];
    return;
  }
  const int64_t j = k - b;
  float m = MI_NEG_INF, s = 0.0f, qs = 0.0f;
  for (int64_t g = 0; g < n_ranks; ++g) {
    lse_merge(m, s, parts[g * pf + 2 * j], parts[g * pf + 2 * j + 1]);
    qs += parts[g * pf + 2 * b + j];
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  c_out[j] = lse;
  terms[k] = lse - qs;
}

// ------------------------------------------------------------------------------------------------ host side
struct SoftNcePlan {
  NceRec* rowp;
  NceRec* colp;
  float* rowq;
  float* colq;
  float *r, *c, *z, *inv_z, *rs, *terms;
  int64_t n_t;  // 64-wide tiles per row and per column
};

static inline SoftNcePlan plan_softnce(Workspace& ws, int64_t b) {
  SoftNcePlan q{};
  q.n_t = (b + 63) / 64;
  q.rowp = ws.take<NceRec>(b * q.n_t);
  q.colp = ws.take<NceRec>(b * q.n_t);
  q.rowq = ws.take<float>(b * q.n_t);
  q.colq = ws.take<float>(b * q.n_t);
  q.r = ws.take<float>(b);
  q.c = ws.take<float>(b);
  q.z = ws.take<float>(b);
  q.inv_z = ws.take<float>(b);
  q.rs = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  return q;
}

static inline SoftNceStatsOut softnce_stats_out(const SoftNcePlan& q, const int64_t* lab, float tau, float mix) {
  return SoftNceStatsOut{lab, lab, 0, q.rs, q.inv_z, q.rowp, q.colp, q.rowq, q.colq, q.n_t, q.n_t, 1.0f / tau, mix};
}

// b: the GLOBAL batch (the loss weights); a row block passes its own masks, the global masks and its offset; rs, inv_z
// and z are indexed by global sample
static inline SoftNceGradIn softnce_grad_in(const int64_t* lab_rows, const int64_t* lab_cols, int64_t row_offset,
                                            const float* rs, const float* inv_z, const float* z, const float* r,
                                            const float* c, const float* grad_out, int64_t b, int mode, float tau,
                                            float mix) {
  const float fb = (float)b;
  const bool sym = mode == MI_NCE_SYMMETRIC;
  return SoftNceGradIn{lab_rows, lab_cols, row_offset, rs, inv_z, z, r, c, grad_out, sym ? 0.5f / fb : 1.0f / fb,
                       sym ? 0.5f / fb : 0.0f, 1.0f / tau, mix};
}
static inline SoftNceGradIn softnce_grad_in(const int64_t* lab, const float* rs, const float* inv_z, const float* z,
                                            const float* r, const float* c, const float* grad_out, int64_t b, int mode,
                                            float tau, float mix) {
  return softnce_grad_in(lab, lab, 0, rs, inv_z, z, r, c, grad_out, b, mode, tau, mix);
}

// masks of all b samples -> z, 1 / z, rs [b]; z of samples [out_lo, out_lo + out_n) also to the caller's optional
// target_norm [out_n].  fast: the k exponentials of the 16-bit chain's epilogues
static inline int softnce_label_norm(const int64_t* lab, int64_t b, float tau, bool fast, float* z, float* inv_z,
                                     float* rs, float* target_norm, int64_t out_lo, int64_t out_n, hipStream_t st) {
  const dim3 grid((unsigned)((b + 3) / 4)), block(256);
  {
    ProfScope prof_("softnce_label_norm_kernel", st);
    if (fast)
      hipLaunchKernelGGL(softnce_label_norm_kernel<true>, grid, block, 0, st, lab, b, 1.0f / tau, z, inv_z, rs,
                         target_norm, out_lo, out_n);
    else
      hipLaunchKernelGGL(softnce_label_norm_kernel<false>, grid, block, 0, st, lab, b, 1.0f / tau, z, inv_z, rs,
                         target_norm, out_lo, out_n);
  }
  MI_LAUNCH_CHECK("softnce_label_norm_kernel");
  return MI_OK;
}
static inline int softnce_label_norm(const int64_t* lab, int64_t b, float tau, bool fast, const SoftNcePlan& q,
                                     float* target_norm, hipStream_t st) {
  return softnce_label_norm(lab, b, tau, fast, q.z, q.inv_z, q.rs, target_norm, 0, b, st);
}

// records -> r, c (workspace and the caller's optional copies), loss
static inline int softnce_finish(const SoftNcePlan& q, int64_t b, int mode, float* loss_out, float* lse_rows,
                                 float* lse_cols, hipStream_t st) {
  {
    ProfScope prof_("softnce_merge_kernel", st);
    hipLaunchKernelGGL(softnce_merge_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp,
                       q.rowq, q.colq, b, q.n_t, q.r, q.c, lse_rows, lse_cols, q.terms);
  }
  MI_LAUNCH_CHECK("softnce_merge_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, q.terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ row blocks, host side
// The records of one rank's row block [br] x [b], the row LSE r and the label norms of ALL b samples: the forward writes
// them, the backward reads r, 1 / z and rs from the same workspace (the same plan gives the same offsets).
struct SoftNceShardPlan {
  NceRec* rowp;  // [br][n_ct]
  NceRec* colp;  // [b][n_rt]
  float* rowq;   // [br][n_ct]
  float* colq;   // [b][n_rt]
  float *r, *z, *inv_z, *rs;  // [br], [b], [b], [b]
  int64_t n_ct, n_rt;
};

static inline SoftNceShardPlan plan_softnce_shard(Workspace& ws, int64_t br, int64_t b) {
  SoftNceShardPlan q{};
  q.n_ct = (b + 63) / 64;
  q.n_rt = (br + 63) / 64;
  q.rowp = ws.take<NceRec>(br * q.n_ct);
  q.colp = ws.take<NceRec>(b * q.n_rt);
  q.rowq = ws.take<float>(br * q.n_ct);
  q.colq = ws.take<float>(b * q.n_rt);
  q.r = ws.take<float>(br);
  q.z = ws.take<float>(b);
  q.inv_z = ws.take<float>(b);
  q.rs = ws.take<float>(b);
  return q;
}

static inline SoftNceStatsOut softnce_stats_out(const SoftNceShardPlan& q, const int64_t* lab_rows, const int64_t* lab_cols,
                                                int64_t row_offset, float tau, float mix) {
  return SoftNceStatsOut{lab_rows, lab_cols, row_offset, q.rs,   q.inv_z, q.rowp, q.colp,
                         q.rowq,   q.colq,   q.n_ct,     q.n_rt, 1.0f / tau, mix};
}

static inline int softnce_rank_part(const SoftNceShardPlan& q, int64_t br, int64_t b, float* part_out, float* lse_rows,
                                    hipStream_t st) {
  {
    ProfScope prof_("softnce_rank_part_kernel", st);
    hipLaunchKernelGGL(softnce_rank_part_kernel, dim3((unsigned)((br + b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp,
                       q.rowq, q.colq, br, b, q.n_ct, q.n_rt, q.r, lse_rows, part_out);
  }
  MI_LAUNCH_CHECK("softnce_rank_part_kernel");
  return MI_OK;
}

// terms: [2b] scratch
static inline int softnce_merge_parts(const float* parts, int64_t n_ranks, int64_t br, int64_t b, int mode,
                                      float* loss_out, float* lse_cols, float* terms, hipStream_t st) {
  {
    ProfScope prof_("softnce_merge_parts_kernel", st);
    hipLaunchKernelGGL(softnce_merge_parts_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, parts, n_ranks,
                       br, b, lse_cols, terms);
  }
  MI_LAUNCH_CHECK("softnce_merge_parts_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

}  // namespace mi
