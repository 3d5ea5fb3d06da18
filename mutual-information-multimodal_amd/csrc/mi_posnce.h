// Study-positive InfoNCE: the per-sample InfoNCE of mi_nce.h with every same-study pair as a
// positive (the multi-positive loss of SupCon, "L_out": the average over the positives stands outside the logarithm).
//   P_i = {j : sid_j == sid_i} (contains i),  n_i = |P_i| >= 1
//   r_i = log sum_{j < B} exp S[i, j],  c_j = log sum_{i < B} exp S[i, j]                       (nothing is masked)
//   row term t_i = r_i - (1/n_i) sum_{p in P_i} S[i, p],  column term t'_j = c_j - (1/n_j) sum_{p in P_j} S[p, j]
//   rowwise: L = (1/B) sum_i t_i;  symmetric: L = 1/2 (1/B) sum_i t_i + 1/2 (1/B) sum_j t'_j
//   dL/dS[i, j] = wr exp(S[i, j] - r_i) + wc exp(S[i, j] - c_j) - (wr + wc) 1[sid_i == sid_j] / n_i
//   (wr, wc) = (1/B, 0) or (1/(2B), 1/(2B));  n_i == n_j wherever the indicator is 1
// With unique ids this IS the loss of mi_nce.h (same r, c, loss, gradients).  With duplicates it differs twice: same-study
// pairs enter the denominators, and they share the positive weight.  All ids equal: t_i = r_i - mean_j S[i, j] >= log B,
// not zero.  B == 1: loss exactly 0 and exact-zero gradients (m = S_00, s = 1, logf(1) = 0, exp2(0) - 1 = 0).  Each row's
// share of dL/dS sums to zero.  A training loss, not an MI bound: log B - L bounds nothing once some n_i > 1.
// Building blocks (written for the MFMA 32x32 accumulator layout that nce_tile_stats documents):
//   posnce_tile_stats:   one 64 x 64 wave tile -> per-row (max, sum exp) over ALL in-range columns of the tile and a
//                        positive record (sum S, count) over its same-id columns; the same per column over its rows.
//                        Positives may sit in any tile; a tile without one (a wave-uniform vote) stores zero records
//   posnce_merge_kernel: the records of every tile, in tile order -> r, c, n_pos, 1/n, the per-sample terms
//                        -> nce_loss_kernel (fixed order everywhere, no float atomics: bit-reproducible)
//   posnce_tile_grad:    one wave tile of recomputed scores -> G = grad_out * dL/dS from r, c and 1/n of the row
// Row blocks (the sharded step): the tiles of rows [row_offset, row_offset + M) of the global B x B
// matrix, with the ids of the block's rows and of every column.  Positives are found by id, so no offset enters a tile: a
// row sees all of its columns (r_i, n_i and t_i are complete on the owning rank), a column only this rank's rows.  The
// whole batch is sid_rows == sid_cols.
//   posnce_rank_part_kernel:   a rank's records -> r and 1/n (kept), one flat part (column partials, row terms, counts)
//   posnce_merge_parts_kernel: the parts of every rank, in rank order -> c, the per-sample terms -> nce_loss_kernel
//   EpiPosNceStats<FAST> / EpiPosNceGrad<TG> / EpiPosNceGrad2: the epilogues of the score GEMM and of the G GEMM on the
//                        generic kernels and on the 16-bit chain
#pragma once
#include "mi_nce.h"

namespace mi {

// (sum of scores, count) of one row's (column's) positives inside one 64-wide tile; {0, 0}: none in the tile
struct PosRec {
  float sum;
  int32_t count;
};

struct PosNceStatsOut {
  const int64_t* sid_rows;  // [M]
  const int64_t* sid_cols;  // [N] (the whole batch: the same array)
  NceRec* rowp;             // [M][n_ct]: row i over the columns of tile t
  NceRec* colp;             // [N][n_rt]: column j over the rows of tile t
  PosRec* rowq;             // [M][n_ct]: the positives of row i among the columns of tile t
  PosRec* colq;             // [N][n_rt]: the positives of column j among the rows of tile t
  int64_t n_ct, n_rt;
};

struct PosNceGradIn {
  const int64_t* sid_rows;  // [M]
  const int64_t* sid_cols;  // [N]
  const float* r;           // [M] row LSE
  const float* c;           // [N] column LSE (symmetric mode)
  const float* inv_n;       // [M] 1 / n_i of the rows, or null: then from n_pos
  const int32_t* n_pos;     // [M] n_i (read where inv_n is null)
  const float* grad_out;    // [1] or null (1)
  float wr, wc;             // 1/B, 0 (rowwise) or 1/(2B), 1/(2B) (symmetric); B is the global batch
};

// acc element (tm, tn, r) of this lane: as nce_tile_stats.  Consumes acc.  No block-level barrier.
template <bool FAST>
__device__ __forceinline__ void posnce_tile_stats(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                  const PosNceStatsOut& o) {
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
  // the only mask: elements outside M x N become -inf.  pm[tn] bit (tm 16 + r): that element is a same-id pair
  uint32_t pm[2] = {0u, 0u};
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool rok = row < M;
      const int64_t sr = rok ? o.sid_rows[row] : 0;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const bool ok = rok && cok[tn];
        if (ok && sr == sc[tn]) pm[tn] |= 1u << (tm * 16 + r);
        if (!ok) acc[tm][tn][r] = MI_NEG_INF;
      }
    }
  // positives are sparse: one vote per wave, tiles without one skip the positive butterflies (and store zero records:
  // the merge reads every slot)
  const bool any_pos = __any((pm[0] | pm[1]) != 0u);
  // rows: each row's 64 values sit in the 32 lanes of one half (two per lane)
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
        PosRec q{0.0f, 0};
        if (any_pos) {
          const uint32_t bit = 1u << (tm * 16 + r);
          const bool p0 = (pm[0] & bit) != 0u, p1 = (pm[1] & bit) != 0u;
          float ps = (p0 ? a0 : 0.0f) + (p1 ? a1 : 0.0f);
          int pc = (int)p0 + (int)p1;
#pragma unroll
          for (int off = 16; off > 0; off >>= 1) {
            ps += __shfl_xor(ps, off);
            pc += __shfl_xor(pc, off);
          }
          q = PosRec{ps, pc};
        }
        const int64_t row = mb + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (col_l == 0 && row < M) {
          o.rowp[row * o.n_ct + t] = NceRec{m, s};
          o.rowq[row * o.n_ct + t] = q;
        }
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
      PosRec q{0.0f, 0};
      if (any_pos) {
        float ps = 0.0f;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (pm[tn] & (1u << (tm * 16 + r))) ps += acc[tm][tn][r];
        int pc = __popc(pm[tn]);
        ps += __shfl_xor(ps, 32);
        pc += __shfl_xor(pc, 32);
        q = PosRec{ps, pc};
      }
      const int64_t col = nb + tn * 32 + col_l;
      if (half == 0 && col < N) {
        o.colp[col * o.n_rt + t] = NceRec{m, s};
        o.colq[col * o.n_rt + t] = q;
      }
    }
  }
}

// acc (scores) -> G = grad_out * dL/dS.  0 outside M x N.
template <bool FAST>
__device__ __forceinline__ void posnce_tile_grad(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N,
                                                 const PosNceGradIn& g) {
  const int lane = threadIdx.x & 63;
  const int col_l = lane & 31, half = lane >> 5;
  const float go = g.grad_out ? g.grad_out[0] : 1.0f;
  const float wr = go * g.wr, wc = go * g.wc;
  const float wp = wr + wc;
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
      const float inv = !rok ? 0.0f : g.inv_n ? g.inv_n[row] : 1.0f / (float)g.n_pos[row];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const float v = acc[tm][tn][r];
        float gv = 0.0f;
        if (rok && cok[tn]) {
          gv = wr * nce_exp<FAST>(v - rr);
          if (cols) gv += wc * nce_exp<FAST>(v - cc[tn]);
          if (sr == sc[tn]) gv -= wp * inv;
        }
        acc[tm][tn][r] = gv;
      }
    }
}

// score GEMM epilogue: both call forms, as EpiNceStats
template <bool FAST>
struct EpiPosNceStats {
  static constexpr bool kReducesPartial = false;
  PosNceStatsOut o;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    posnce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char*) const {
    posnce_tile_stats<FAST>(acc, mb, nb, M, N, o);
  }
};

// recompute GEMM epilogue of the generic kernels: G as TG [M][N]
template <typename TG>
struct EpiPosNceGrad {
  PosNceGradIn in;
  TG* g;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N) const {
    posnce_tile_grad<false>(acc, mb, nb, M, N, in);
    foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
      if (row < M && col < N) g[row * N + col] = (TG)v;
    });
  }
};

// recompute GEMM epilogue of the 16-bit chain: G and G^T as bf16 (bf16x3: split parts), stores as EpiNceGrad2
struct EpiPosNceGrad2 {
  static constexpr bool kReducesPartial = false;
  PosNceGradIn in;
  bf16_t* g;
  bf16_t* gt;
  int split;
  __device__ __forceinline__ void operator()(f32x16 (&acc)[2][2], int64_t mb, int64_t nb, int64_t M, int64_t N, int, int,
                                             char* lds) const {
    posnce_tile_grad<true>(acc, mb, nb, M, N, in);
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
static __global__ __launch_bounds__(64) void posnce_matrix_stats_kernel(const float* __restrict__ s, int64_t b,
                                                                        PosNceStatsOut o) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  posnce_tile_stats<false>(acc, mb, nb, b, b, o);
}

static __global__ __launch_bounds__(64) void posnce_matrix_grad_kernel(const float* __restrict__ s, int64_t b,
                                                                       PosNceGradIn in, float* __restrict__ grad) {
  f32x16 acc[2][2];
  const int64_t mb = (int64_t)blockIdx.y * 64, nb = (int64_t)blockIdx.x * 64;
  nce_load_tile(s, b, mb, nb, acc);
  posnce_tile_grad<false>(acc, mb, nb, b, b, in);
  foreach_acc(acc, mb, nb, [&](int64_t row, int64_t col, float v) {
    if (row < b && col < b) grad[row * b + col] = v;
  });
}

// ------------------------------------------------------------------------------------------------ merge
// thread k < b: row k, b <= k < 2b: column k - b.  NceRecs merged and PosRecs added in tile order (exact expf / logf).
// Every sample is its own positive, so count >= 1.  The row side also writes n_pos and 1 / n.
static __global__ __launch_bounds__(256) void posnce_merge_kernel(const NceRec* __restrict__ rowp,
                                                                  const NceRec* __restrict__ colp,
                                                                  const PosRec* __restrict__ rowq,
                                                                  const PosRec* __restrict__ colq, int64_t b, int64_t n_t,
                                                                  float* r_ws, float* c_ws, float* inv_n, float* r_out,
                                                                  float* c_out, int32_t* n_pos_out, float* terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const bool is_row = k < b;
  const int64_t i = is_row ? k : k - b;
  const NceRec* p = (is_row ? rowp : colp) + i * n_t;
  const PosRec* q = (is_row ? rowq : colq) + i * n_t;
  float m = MI_NEG_INF, s = 0.0f, ps = 0.0f;
  int32_t pc = 0;
  for (int64_t t = 0; t < n_t; ++t) {
    lse_merge(m, s, p[t].m, p[t].s);
    ps += q[t].sum;
    pc += q[t].count;
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  if (is_row) {
    r_ws[i] = lse;
    if (r_out) r_out[i] = lse;
    inv_n[i] = 1.0f / (float)pc;
    if (n_pos_out) n_pos_out[i] = pc;
  } else {
    c_ws[i] = lse;
    if (c_out) c_out[i] = lse;
  }
  terms[k] = lse - ps / (float)pc;
}

// ------------------------------------------------------------------------------------------------ row blocks
// The part of one rank (posnce_part_floats(br, b) floats, gathered in rank order by the caller):
//   [0, 2b)                  column j: (m, s) over this rank's rows, merged in row-tile order (NceRec)
//   [2b, 3b)                 column j: sum of S[p, j] over this rank's rows p with sid_p == sid_j, in row-tile order
//   [3b, 3b + br)            row term t_i = r_i - (1/n_i) sum_{p in P_i} S[i, p] of local row i (complete on this rank)
//   [3b + br, 3b + 2 br)     n_i of local row i as a float (exact below 2^24: the entry points refuse larger b); it is
//                            also the count of column row_offset + i, the same sample
__host__ __device__ inline int64_t posnce_part_floats(int64_t br, int64_t b) { return 3 * b + 2 * br; }

// thread k < br: local row k (records merged and positives added in tile order exactly as posnce_merge_kernel: the same
// r, n and term bits), br <= k < br + b: column k - br over this rank's row tiles
static __global__ __launch_bounds__(256) void posnce_rank_part_kernel(const NceRec* __restrict__ rowp,
                                                                      const NceRec* __restrict__ colp,
                                                                      const PosRec* __restrict__ rowq,
                                                                      const PosRec* __restrict__ colq, int64_t br,
                                                                      int64_t b, int64_t n_ct, int64_t n_rt, float* r_ws,
                                                                      float* inv_n, float* r_out, int32_t* n_pos_out,
                                                                      float* __restrict__ part) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= br + b) return;
  const bool is_row = k < br;
  const int64_t i = is_row ? k : k - br;
  const int64_t n = is_row ? n_ct : n_rt;
  const NceRec* p = (is_row ? rowp : colp) + i * n;
  const PosRec* q = (is_row ? rowq : colq) + i * n;
  float m = MI_NEG_INF, s = 0.0f, ps = 0.0f;
  int32_t pc = 0;
  for (int64_t t = 0; t < n; ++t) {
    lse_merge(m, s, p[t].m, p[t].s);
    ps += q[t].sum;
    pc += q[t].count;
  }
  if (!is_row) {
    part[2 * i] = m;
    part[2 * i + 1] = s;
    part[2 * b + i] = ps;
    return;
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  r_ws[i] = lse;
  if (r_out) r_out[i] = lse;
  inv_n[i] = 1.0f / (float)pc;
  if (n_pos_out) n_pos_out[i] = pc;
  part[3 * b + i] = lse - ps / (float)pc;
  part[3 * b + br + i] = (float)pc;
}

// parts [n_ranks][posnce_part_floats(br, b)] in rank order (rank g holds rows [g br, (g + 1) br)).  Thread k < b: the row
// term of sample k, copied; b <= k < 2b: column j = k - b, its (m, s) merged and its positive scores added in rank order
// from an empty (-inf, 0), 0 start -- exact for one rank, so one rank gives the bits of posnce_merge_kernel -- then c_j
// and its term c_j - sum / n_j (n_j from the part of the rank that owns sample j).  Every rank runs this on the same
// gathered buffer: identical bits.
static __global__ __launch_bounds__(256) void posnce_merge_parts_kernel(const float* __restrict__ parts, int64_t n_ranks,
                                                                        int64_t br, int64_t b, float* c_out,
                                                                        float* __restrict__ terms) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * b) return;
  const int64_t pf = posnce_part_floats(br, b);
  if (k < b) {
    terms[k] = parts[(k / br) * pf + 3 * b + k % br];
    return;
  }
  const int64_t j = k - b;
  float m = MI_NEG_INF, s = 0.0f, ps = 0.0f;
  for (int64_t g = 0; g < n_ranks; ++g) {
    lse_merge(m, s, parts[g * pf + 2 * j], parts[g * pf + 2 * j + 1]);
    ps += parts[g * pf + 2 * b + j];
  }
  const float lse = s > 0.0f ? m + logf(s) : MI_NEG_INF;
  c_out[j] = lse;
  terms[k] = lse - ps / parts[(j / br) * pf + 3 * b + br + j % br];
}

// ------------------------------------------------------------------------------------------------ host side
struct PosNcePlan {
  NceRec* rowp;
  NceRec* colp;
  PosRec* rowq;
  PosRec* colq;
  float *r, *c, *inv_n, *terms;
  int64_t n_t;  // 64-wide tiles per row and per column
};

static inline PosNcePlan plan_posnce(Workspace& ws, int64_t b) {
  PosNcePlan q{};
  q.n_t = (b + 63) / 64;
  q.rowp = ws.take<NceRec>(b * q.n_t);
  q.colp = ws.take<NceRec>(b * q.n_t);
  q.rowq = ws.take<PosRec>(b * q.n_t);
  q.colq = ws.take<PosRec>(b * q.n_t);
  q.r = ws.take<float>(b);
  q.c = ws.take<float>(b);
  q.inv_n = ws.take<float>(b);
  q.terms = ws.take<float>(2 * b);
  return q;
}

static inline PosNceStatsOut posnce_stats_out(const PosNcePlan& q, const int64_t* sid) {
  return PosNceStatsOut{sid, sid, q.rowp, q.colp, q.rowq, q.colq, q.n_t, q.n_t};
}

// b: the GLOBAL batch (the loss weights); a row block passes its own ids and the global ids
static inline PosNceGradIn posnce_grad_in(const int64_t* sid_rows, const int64_t* sid_cols, const float* r, const float* c,
                                          const float* inv_n, const int32_t* n_pos, const float* grad_out, int64_t b,
                                          int mode) {
  const float fb = (float)b;
  if (mode == MI_NCE_SYMMETRIC)
    return PosNceGradIn{sid_rows, sid_cols, r, c, inv_n, n_pos, grad_out, 0.5f / fb, 0.5f / fb};
  return PosNceGradIn{sid_rows, sid_cols, r, c, inv_n, n_pos, grad_out, 1.0f / fb, 0.0f};
}
static inline PosNceGradIn posnce_grad_in(const int64_t* sid, const float* r, const float* c, const float* inv_n,
                                          const int32_t* n_pos, const float* grad_out, int64_t b, int mode) {
  return posnce_grad_in(sid, sid, r, c, inv_n, n_pos, grad_out, b, mode);
}

// records -> r, c, n_pos (workspace and the caller's optional copies), loss
static inline int posnce_finish(const PosNcePlan& q, int64_t b, int mode, float* loss_out, float* lse_rows, float* lse_cols,
                                int32_t* n_pos_out, hipStream_t st) {
  {
    ProfScope prof_("posnce_merge_kernel", st);
    hipLaunchKernelGGL(posnce_merge_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp, q.rowq,
                       q.colq, b, q.n_t, q.r, q.c, q.inv_n, lse_rows, lse_cols, n_pos_out, q.terms);
  }
  MI_LAUNCH_CHECK("posnce_merge_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, q.terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ row blocks, host side
// The records of one rank's row block [br] x [b], the row LSE r and 1 / n of its rows: the forward writes r and 1 / n,
// the backward reads them from the same workspace (the same plan gives the same offsets).
struct PosNceShardPlan {
  NceRec* rowp;  // [br][n_ct]
  NceRec* colp;  // [b][n_rt]
  PosRec* rowq;  // [br][n_ct]
  PosRec* colq;  // [b][n_rt]
  float *r, *inv_n;
  int64_t n_ct, n_rt;
};

static inline PosNceShardPlan plan_posnce_shard(Workspace& ws, int64_t br, int64_t b) {
  PosNceShardPlan q{};
  q.n_ct = (b + 63) / 64;
  q.n_rt = (br + 63) / 64;
  q.rowp = ws.take<NceRec>(br * q.n_ct);
  q.colp = ws.take<NceRec>(b * q.n_rt);
  q.rowq = ws.take<PosRec>(br * q.n_ct);
  q.colq = ws.take<PosRec>(b * q.n_rt);
  q.r = ws.take<float>(br);
  q.inv_n = ws.take<float>(br);
  return q;
}

static inline PosNceStatsOut posnce_stats_out(const PosNceShardPlan& q, const int64_t* sid_rows, const int64_t* sid_cols) {
  return PosNceStatsOut{sid_rows, sid_cols, q.rowp, q.colp, q.rowq, q.colq, q.n_ct, q.n_rt};
}

static inline int posnce_rank_part(const PosNceShardPlan& q, int64_t br, int64_t b, float* part_out, float* lse_rows,
                                   int32_t* n_pos_out, hipStream_t st) {
  {
    ProfScope prof_("posnce_rank_part_kernel", st);
    hipLaunchKernelGGL(posnce_rank_part_kernel, dim3((unsigned)((br + b + 255) / 256)), dim3(256), 0, st, q.rowp, q.colp,
                       q.rowq, q.colq, br, b, q.n_ct, q.n_rt, q.r, q.inv_n, lse_rows, n_pos_out, part_out);
  }
  MI_LAUNCH_CHECK("posnce_rank_part_kernel");
  return MI_OK;
}

// terms: [2b] scratch
static inline int posnce_merge_parts(const float* parts, int64_t n_ranks, int64_t br, int64_t b, int mode, float* loss_out,
                                     float* lse_cols, float* terms, hipStream_t st) {
  {
    ProfScope prof_("posnce_merge_parts_kernel", st);
    hipLaunchKernelGGL(posnce_merge_parts_kernel, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, parts, n_ranks,
                       br, b, lse_cols, terms);
  }
  MI_LAUNCH_CHECK("posnce_merge_parts_kernel");
  {
    ProfScope prof_("nce_loss_kernel", st);
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, terms, b, mode == MI_NCE_SYMMETRIC ? 1 : 0, loss_out);
  }
  MI_LAUNCH_CHECK("nce_loss_kernel");
  return MI_OK;
}

}  // namespace mi
