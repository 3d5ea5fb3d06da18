// Fused bilinear critic  S = (X W) Y^T  + bound + all gradients (BASELINE.json headline configuration).
// Replaces the call site mutual_info_img_txt/main_utils.py:220-226 for a bilinear critic: the B x B score matrix
// is never written to HBM in the forward (the log-sum-exp is an epilogue of the score GEMM) and the pair rows of
// create_mi_pairs (main_utils.py:80-110) are index arithmetic plus a study-id compare in that epilogue.
// The reference has no bilinear critic: scorer parity is pinned by the oracle only; bound, masking and pair
// semantics are the reference's (mi_critics.py:3-23, main_utils.py:99-108).
//
// bf16 fast path (all widths and batch sizes multiples of 8): every operand is converted once to bf16 in both
// orientations so that every GEMM reads K-contiguous rows (mi_gemm_bf16.h):
//   forward : prep X, Y, W -> T = X W (bf16, both orientations) -> S tiles = T Y^T with masked online-LSE epilogue
//             -> fixed-order merge -> stats, loss
//   backward: G = dL/dS from recomputed S tiles (bf16, both orientations, 2 x 33 MB at B = 4096: cache resident)
//             -> {dT = G Y, dY = G^T T} as ONE two-problem launch (2 x 128 tiles fill the chip) -> dW = X^T dT (split-K
//             slabs + ordered reduce) -> dX = dT W^T.  The backward reuses the forward's workspace (X, Y, W, T copies).
// generic path (fp32 parity mode, odd shapes): mi_gemm.h kernels with strided operands, T recomputed in the backward.
#include "mi_gemm.h"
#include "mi_gemm_bf16.h"
#include "mi_bilinear_flash.h"
#include "mi_bilinear_tail.h"
#include "mi_fp8.h"
#include "mi_nce.h"
#include "mi_fdiv.h"
#include "mi_rank.h"
#include "mi_topk.h"
#include "mi_hardnce.h"
#include "mi_banknce.h"
#include "mi_posnce.h"
#include "mi_softnce.h"
#include "mi_estimates.h"

namespace mi {

// The fused B x B stage (mi_bilinear_flash.h) of a critic with scores S = Q K^T -- T Y^T for the bilinear critic, A C^T
// for the separable one: scores, masked log-sum-exp records and (grad) the unnormalised sums of both gradient
// contractions.  Problem 0 sweeps the b rows of K for every local row of Q; problem 1 is problem 0 with operands, ids and
// the sign of row_offset swapped.  That convention is written here and nowhere else.
struct ReduceOut {
  float* f32;      // [m][d] or null
  bf16_t* bf;      // [m][d] or null
  bf16_t* bf_t;    // [d][m] or null
};
struct FusedStage {
  FlashPlan fl;
  int64_t br, b, d;                  // local rows of Q, rows of K, score width
  const bf16_t* frag[2];             // stationary operand per problem, fragment-major: Q [br][d], K [b][d]
  const bf16_t* rows[2];             // streamed operand per problem, row-major: K [b][d], Q [br][d]
  Partial* rec[2];                   // per-wave records
  float* slab[2];                    // partial sums
  unsigned char* dup[2];             // equal-id flags per 32 x 32 block: [br / 32][b / 32] and its transpose
  const char *what_grad, *what_fwd;  // launch labels with and without the gradient sums

  int64_t m(int q) const { return q ? b : br; }
  // records, slabs and flags of both problems (nothing where the shape does not take the fused kernel)
  void take(Workspace& ws) {
    for (int q = 0; q < 2 && fl.ok; ++q) {
      rec[q] = ws.take<Partial>(fl.n_rec[q]);
      slab[q] = ws.take<float>((fl.slab_bytes[q] + 3) / 4);
      dup[q] = ws.take<unsigned char>((br / 32) * (b / 32));
    }
  }
  // the flags ride along with a conversion launch
  DupFlagJob dup_job(const int64_t* sid_rows, const int64_t* sid_cols, int64_t row_offset) const {
    return DupFlagJob{sid_rows, sid_cols, (int)(br / 32), (int)(b / 32), dup[0], dup[1], row_offset};
  }
  int launch(const int64_t* sid_rows, const int64_t* sid_cols, int64_t row_offset, bool grad, hipStream_t st) const {
    const int64_t* sid[2] = {sid_rows, sid_cols};
    FlashArgs a{};
    for (int q = 0; q < 2; ++q)
      a.p[q] = FlashProblem{frag[q], rows[q], sid[q], sid[1 - q], m(q), m(1 - q), q ? -row_offset : row_offset, fl.n_rb[q],
                            fl.n_split[q], fl.tiles_per_split[q], dup[q], slab[q], rec[q]};
    a.n_problems = grad ? 2 : 1;
    a.slab_f16 = fl.slab_f16 ? 1 : 0;
    return launch_flash(a, d, grad, st, grad ? what_grad : what_fwd);
  }
  // the two jobs that turn the launch's sums into gradient rows: job q scales the slabs of problem q, subtracts the
  // diagonal term (a row of the problem's streamed operand) and writes to out[q]
  void reduce_jobs(FlashReduceJob* j, int64_t row_offset, const ReduceOut& out0, const ReduceOut& out1) const {
    const ReduceOut* out[2] = {&out0, &out1};
    for (int q = 0; q < 2; ++q)
      j[q] = FlashReduceJob{slab[q], rec[q], fl.n_split[q], fl.n_rb[q], m(q), rows[q], m(1 - q),
                            q ? -row_offset : row_offset, out[q]->f32, out[q]->bf, out[q]->bf_t};
  }
};

struct BilinearPlan {
  // generic path
  float* t;
  float* dt;
  void* g;
  Partial* partials;
  int64_t n_partials;
  // bf16 fast path
  bf16_t *xb, *xtb, *yb, *ytb, *wb, *wtb, *tb, *ttb, *gb, *gtb, *dtb, *dttb;
  float* dw_slab;
  int dw_splits;
  int64_t dw_kchunk;
  // row blocks of a sharded batch (b_rows < b): dT = G Y has few output tiles and a long K; split K into slabs
  float* dt_slab;
  int dt_splits;
  int64_t dt_kchunk;
  // fused B x B stage on S = T Y^T
  FusedStage stage;
  bf16_t *tfb, *yfb;         // fragment-major copies of T and Y: the stationary operands of the fused kernel
  // the backward's tail (mi_bilinear_tail.h): fragment-major W (B operand of dX = dT W^T), X^T and dT^T (operands of dW)
  bool tail;
  bf16_t *wfb, *xtfb, *dttfb;
  // bf16x3 (MI_PREC_BF16X3): every bf16 operand copy holds hi and lo parts along a tripled K (mi_gemm_bf16.h,
  // split3_offsets); A-side role: xb, xtb, tb, gb, gtb, dtb; B-side role: yb, ytb, wb, wtb, ttb, dttb
  int x3;  // 3 in that mode, else 1
  // fp8 mode (MI_PREC_FP8, mi_fp8.h): e4m3 copies of the operands of the two forward products and the scale block; the
  // bf16 copies of the quantised values for the backward live in xtb, ytb, wb, ttb
  fp8_t *qx8, *qy8, *qwt8, *qt8;
  Fp8Scales* f8sc;
  // exact-fp32 path (MI_PREC_F32): split-K slabs of the products whose output has too few 128 x 128 tiles to fill the chip
  float* gen_slab;
  int64_t gen_slab_floats;
  // which kernels the shape takes (MI_PATH_*), or MI_ESHAPE for an fp8 call outside the fp8 kernels' shapes
  int path;
  size_t bytes;
};

// Split-K of a generic-path product: with fewer than 192 output tiles the launch leaves CUs idle (dW = X^T dT at d = 512 is
// 16 tiles with K = B: 567 us for 2 GFLOP at B = 4096).  Splits fill ~256 workgroups, K chunks are multiples of 64.
static void generic_splitk(int64_t m, int64_t n, int64_t k, int& splits, int64_t& kchunk) {
  const int64_t tiles = ((m + kTile - 1) / kTile) * ((n + kTile - 1) / kTile);
  int64_t sp = tiles >= 192 ? 1 : (256 + tiles - 1) / tiles;
  if (sp > 16) sp = 16;
  kchunk = (k + sp - 1) / sp;
  kchunk = (kchunk + 63) / 64 * 64;
  sp = kchunk > 0 ? (k + kchunk - 1) / kchunk : 1;
  splits = (int)(sp < 1 ? 1 : sp);
}
static int64_t generic_slab_floats(int64_t m, int64_t n, int64_t k) {
  int sp;
  int64_t kc;
  generic_splitk(m, n, k, sp, kc);
  return sp > 1 ? (int64_t)sp * m * n : 0;
}

static bool fp8_ok(int64_t br, int64_t b, int64_t dx, int64_t dy, int precision, bool has_w) {
  return precision == MI_PREC_FP8 && has_w && br % 8 == 0 && b % 8 == 0 && dx % 16 == 0 && dy % 16 == 0;
}
static bool fast_ok(int64_t br, int64_t b, int64_t dx, int64_t dy, int precision, bool has_w) {
  return (precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3) && has_w && br % 8 == 0 && b % 8 == 0 &&
         dx % 8 == 0 && dy % 8 == 0;
}

// has_w: the call has a weight matrix (w == NULL, S = X Y^T, runs the generic kernels); it decides the path only, never
// the layout.  gemms_only: no fused B x B stage (the per-sample InfoNCE runs the G-materialising chain, mi_nce.h)
static BilinearPlan plan_bilinear(Workspace& ws, int64_t br, int64_t b, int64_t dx, int64_t dy, int precision, bool has_w,
                                  bool gemms_only = false) {
  BilinearPlan p{};
  p.n_partials = ((b + kTile - 1) / kTile) * ((br + kTile - 1) / kTile);
  p.partials = ws.take<Partial>(p.n_partials);
  // forward buffers of the fast path come first so that forward-only callers can pass a smaller workspace
  const int64_t x3 = precision == MI_PREC_BF16X3 ? 3 : 1;
  p.x3 = (int)x3;
  p.xb = ws.take<bf16_t>(x3 * br * dx);
  p.xtb = ws.take<bf16_t>(x3 * br * dx);
  p.yb = ws.take<bf16_t>(x3 * b * dy);
  p.ytb = ws.take<bf16_t>(x3 * b * dy);
  p.wb = ws.take<bf16_t>(x3 * dx * dy);
  p.wtb = ws.take<bf16_t>(x3 * dx * dy);
  p.tb = ws.take<bf16_t>(x3 * br * dy);
  p.ttb = ws.take<bf16_t>(x3 * br * dy);
  p.t = ws.take<float>(br * dy);
  if (precision == MI_PREC_FP8) {
    p.qx8 = ws.take<fp8_t>(br * dx);
    p.qy8 = ws.take<fp8_t>(b * dy);
    p.qwt8 = ws.take<fp8_t>(dx * dy);
    p.qt8 = ws.take<fp8_t>(br * dy);
    p.f8sc = ws.take<Fp8Scales>(1);
  }
  FusedStage& s = p.stage;
  if (precision == MI_PREC_BF16 && br % 8 == 0 && b % 8 == 0 && dx % 8 == 0 && !gemms_only) s.fl = flash_plan(br, b, dy);
  s.br = br, s.b = b, s.d = dy;
  s.what_grad = "bilinear fused S | P Y | P^T T", s.what_fwd = "bilinear fused S + LSE";
  s.take(ws);
  p.tfb = s.fl.ok ? ws.take<bf16_t>(br * dy) : nullptr;
  p.yfb = s.fl.ok ? ws.take<bf16_t>(b * dy) : nullptr;
  s.frag[0] = p.tfb, s.rows[0] = p.yb;  // problem 0: the rows of Y for every row of T
  s.frag[1] = p.yfb, s.rows[1] = p.tb;
  static const bool no_tail = getenv("MI_NO_TAIL") != nullptr;  // A/B switch: the round-2 backward tail (three launches)
  p.tail = s.fl.ok && !no_tail && flash_tail_ok(br, dx, dy);
  if (precision == MI_PREC_FP8) p.path = fp8_ok(br, b, dx, dy, precision, has_w) ? MI_PATH_FP8_GEMMS : MI_ESHAPE;
  else if (!fast_ok(br, b, dx, dy, precision, has_w)) p.path = MI_PATH_GENERIC;
  else if (!s.fl.ok) p.path = MI_PATH_GEMMS;
  else p.path = p.tail ? MI_PATH_FUSED_TAIL : MI_PATH_FUSED;
  p.wfb = p.tail ? ws.take<bf16_t>(dx * dy) : nullptr;
  p.xtfb = p.tail ? ws.take<bf16_t>(br * dx) : nullptr;
  p.dttfb = p.tail ? ws.take<bf16_t>(br * dy) : nullptr;
  // backward
  p.dt = ws.take<float>(br * dy);
  if (precision == MI_PREC_F32) p.g = ws.take<float>(br * b);
  else p.g = ws.take<bf16_t>(x3 * br * b);
  p.gb = (bf16_t*)p.g;
  p.gtb = ws.take<bf16_t>(x3 * br * b);
  p.dtb = ws.take<bf16_t>(x3 * br * dy);
  p.dttb = ws.take<bf16_t>(x3 * br * dy);
  int64_t tiles = ((dx + kTile - 1) / kTile) * ((dy + kTile - 1) / kTile);
  // split-K so that dW brings ~128 workgroups to the launch it shares with dX (measured at B = 4096, d = 512: 8 splits
  // 16.7 us, 16 splits 19.0 us, 4 splits 19.8 us for the pair)
  // (the fp8 mode launches dW on its own: 256 workgroups there -- 44 -> 2x fewer idle CUs at d = 1024)
  const int64_t dw_target = precision == MI_PREC_FP8 ? 256 : 128;
  int64_t splits = (dw_target + tiles - 1) / tiles;
  if (const char* e = getenv("MI_DW_SPLITS")) splits = atoi(e) > 0 ? atoi(e) : splits;  // A/B switch
  int64_t kchunk = (br + splits - 1) / splits;
  kchunk = (kchunk + kG2KT - 1) / kG2KT * kG2KT;
  splits = (br + kchunk - 1) / kchunk;
  p.dw_splits = (int)splits;
  p.dw_kchunk = kchunk;
  p.dw_slab = ws.take<float>(splits * dx * dy);
  {
    const int64_t t0 = ((br + kTile - 1) / kTile) * ((dy + kTile - 1) / kTile);
    int64_t sp = br < b ? (128 + t0 - 1) / t0 : 1;
    if (sp > 16) sp = 16;
    int64_t kc = (b + sp - 1) / sp;
    kc = (kc + kG2KT - 1) / kG2KT * kG2KT;
    sp = (b + kc - 1) / kc;
    p.dt_splits = (int)sp;
    p.dt_kchunk = kc;
    p.dt_slab = sp > 1 ? ws.take<float>(sp * br * dy) : nullptr;
  }
  if (precision == MI_PREC_F32) {
    int64_t need = generic_slab_floats(br, dy, dx);                      // T = X W
    const int64_t cand[3] = {generic_slab_floats(br, dy, b),             // dT = G Y
                             generic_slab_floats(b, dy, br),             // dY = G^T T
                             generic_slab_floats(dx, dy, br)};           // dW = X^T dT
    for (int64_t c : cand) need = c > need ? c : need;
    const int64_t c4 = generic_slab_floats(br, dx, dy);                  // dX = dT W^T
    need = c4 > need ? c4 : need;
    p.gen_slab_floats = need;
    p.gen_slab = need > 0 ? ws.take<float>(need) : nullptr;
  }
  p.bytes = ws.off;
  return p;
}

static GemmBf16Args one_problem(const bf16_t* a, int64_t lda, const bf16_t* b, int64_t ldb, int64_t m, int64_t n,
                                int64_t k, int64_t k_chunk = 0) {
  GemmBf16Args g{};
  g.p[0] = GemmBf16Problem{a, lda, b, ldb, m, n, k};
  g.p[1] = g.p[0];
  g.n_problems = 1;
  g.k_chunk = k_chunk > 0 ? k_chunk : k;
  return g;
}

// ------------------------------------------------------------------------------------------------ fast path
static int fast_prep_and_t(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                           const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                           const BilinearPlan& p, hipStream_t st, int part = 0) {
  // part 1 / part 2: a sharded run prepares what depends on its OWN rows only (the conversions of X and W, T = X W)
  // while the all-gather of the text embeddings is in flight (mi_bilinear_prep_local), and the rest -- the conversions of
  // the gathered Y, the equal-id flags -- behind it.  Fused-kernel shapes only (the callers check the plan's path).
  const bool fused = p.stage.fl.ok;
  if (part == 2) {
    CvtJobs rest{};
    rest.j[1] = CvtJob{y, b, dy, p.yb, nullptr, 0, 0, p.yfb};
    rest.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
    return launch_cvt_transpose3(rest, st, "bilinear prep Y, id flags");
  }
  // With the fused B x B kernel nobody reads Y^T or T^T any more; instead T and Y get a fragment-major copy (the
  // kernel's stationary operand, loaded straight into MFMA B fragments) and the equal-id tile flags ride along.
  if (fused) {
    // one launch: T tiles straight from the fp32 operands, the other conversions on the CUs the tiles leave free
    CvtJobs side{};
    // (with the two-launch tail nobody reads X^T row-major any more: only its fragment-major form, which the T tiles of
    // the whole step write themselves where the shape allows -- launch_prep_t drops job 0 then and X is read once)
    side.j[0] = CvtJob{x, br, dx, nullptr, p.tail ? nullptr : p.xtb, 0, 0, nullptr, 0, 0, p.xtfb};
    if (part == 0) side.j[1] = CvtJob{y, b, dy, p.yb, nullptr, 0, 0, p.yfb};
    side.j[2] = CvtJob{w, dx, dy, p.wb, nullptr, 0, 0, p.wfb};
    if (part == 0) side.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
    const int rc1 = launch_prep_t(x, w, br, dy, dx, p.tb, p.tfb, side, st, "bilinear prep + T = X W", false, nullptr, nullptr,
                                  p.tail && part == 0);
    if (rc1 != MI_EINVAL) return rc1;
  }
  const int x3 = p.x3;
  // G-materialising path in plain bf16 (widths outside the fused kernel, e.g. the reference's 768): the same single
  // launch -- T tiles (row-major and transposed) beside the conversions.  MI_NO_PREP_T=1: the two launches below.
  if (!fused && x3 == 1 && part == 0) {
    CvtJobs side{};
    side.j[0] = CvtJob{x, br, dx, nullptr, p.xtb, 0, 0, nullptr, 0, 0, p.xtfb};
    side.j[1] = CvtJob{y, b, dy, p.yb, p.ytb};
    side.j[2] = CvtJob{w, dx, dy, p.wb, p.wtb, 0, 0, p.wfb};
    const int rc1 = launch_prep_t(x, w, br, dy, dx, p.tb, nullptr, side, st, "bilinear prep + T = X W", false, nullptr, p.ttb);
    if (rc1 != MI_EINVAL) return rc1;
  }
  const int ra = x3 == 3 ? 1 : 0, rb = x3 == 3 ? 2 : 0;  // bf16x3 roles of A-side and B-side operands
  CvtJobs jobs{};
  jobs.j[0] = CvtJob{x, br, dx, p.xb, p.xtb, 0, 0, nullptr, ra, ra, p.xtfb};
  if (part == 0) jobs.j[1] = CvtJob{y, b, dy, p.yb, fused ? nullptr : p.ytb, 0, 0, fused ? p.yfb : nullptr, rb, rb};
  jobs.j[2] = CvtJob{w, dx, dy, p.wb, p.wtb, 0, 0, p.wfb, rb, rb};
  if (fused && part == 0) jobs.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
  int rc = launch_cvt_transpose3(jobs, st, "bilinear prep X Y W");
  if (rc) return rc;
  // T[i, c] = sum_a X[i, a] W[a, c]: A = Xb [br][dx], B = W^T [dy][dx]
  EpiStoreMulti e{};
  e.out[0] = EpiOut{nullptr, 0, 0, p.tb, dy, fused ? nullptr : p.ttb, br, fused ? p.tfb : nullptr, ra, rb};
  return launch_gemm_bf16(one_problem(p.xb, x3 * dx, p.wtb, x3 * dx, br, dy, x3 * dx), 1, e, st, "bilinear T = X W");
}

// The bf16 boundary: x [br][dx] and y [b][dy] arrive as bf16 (encoders under autocast).  Same launch as above minus the
// conversions: T tiles from the bf16 rows as they lie, X^T / Y fragment-major copies, W copies, the equal-id flags; the
// row-major bf16 copy of Y IS the input.
static int fast_prep_and_t_bf16(const bf16_t* x, const bf16_t* y, const float* w, const int64_t* sid_rows,
                                const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                                const BilinearPlan& p, hipStream_t st) {
  CvtJobs side{};
  side.j[0] = CvtJob{reinterpret_cast<const float*>(x), br, dx, nullptr, nullptr, 0, 0, nullptr, 0, 0, p.xtfb, 1};
  side.j[1] = CvtJob{reinterpret_cast<const float*>(y), b, dy, nullptr, nullptr, 0, 0, p.yfb, 0, 0, nullptr, 1};
  side.j[2] = CvtJob{w, dx, dy, p.wb, nullptr, 0, 0, p.wfb};
  side.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
  return launch_prep_t(reinterpret_cast<const float*>(x), w, br, dy, dx, p.tb, p.tfb, side, st,
                       "bilinear prep + T = X W (bf16 in)", true);
}

static int bilinear_bwd_small(int64_t br, int64_t dx, int64_t dy, float* grad_x, float* grad_w, const BilinearPlan& p,
                              hipStream_t st);
static int bilinear_bwd_from_g(int64_t br, int64_t b, int64_t dx, int64_t dy, float* grad_x, float* grad_y, float* grad_w,
                               bool has_w, const BilinearPlan& p, hipStream_t st);

// The backward's tail in two launches (mi_bilinear_tail.h): [partial sums -> dT rows, grad_y; dX = dT W^T; dT^T
// fragment-major] and [dW = X^T dT].  `merge` != null: the first launch also merges the fused kernel's records into the
// statistics and the loss (the one-call step: no finalize launch).
struct TailMerge {
  int estimator;
  float* loss_out;
  mi_stats* stats_out;
  float* partials_out;
  const float* records = nullptr;  // sharded: the raw records gathered from every rank (rank order), else the workspace's
  int64_t n_records = 0, n_pos = 0;
  int grads_bf16 = 0;              // grad_x / grad_y point to bf16 buffers (the bf16 boundary)
};
// One weight matrix behind the rows the tail reduces: its product dX = dT W^T in the first launch, dW = X^T dT in the second
struct TailSide {
  const bf16_t* w_frag;    // W [dx][d] fragment-major
  int64_t dx;
  float* grad;             // [rows][dx]
  bf16_t* dtt_frag;        // dT^T fragment-major: the first launch writes it, the second reads it
  const bf16_t* xt_frag;   // X^T fragment-major
  float* grad_w;           // [dx][d]
};
// The bilinear critic has one side (job 0: dT -> grad_x, dW; job 1 writes grad_y rows directly), the separable critic two
// (s1: dC -> grad_y, dWh; grad_y here is null).
static int bilinear_tail(const FusedStage& s, int64_t row_offset, const mi_stats* stats, const float* grad_out,
                         const TailSide& s0, const TailSide* s1, float* grad_y, const TailMerge* merge, hipStream_t st) {
  FlashTailArgs ta{};
  const bool gbf = merge && merge->grads_bf16;
  s.reduce_jobs(ta.j, row_offset, ReduceOut{},
                ReduceOut{gbf ? nullptr : grad_y, gbf ? reinterpret_cast<bf16_t*>(grad_y) : nullptr, nullptr});
  ta.stats = stats;
  ta.grad_out = grad_out;
  if (merge) {
    ta.merge_rec = merge->records ? (const Partial*)merge->records : s.rec[0];
    ta.n_merge = merge->records ? merge->n_records : s.fl.n_rec[0];
    ta.n_pos = merge->records ? merge->n_pos : s.b;
    ta.estimator = merge->estimator;
    ta.loss_out = merge->loss_out;
    ta.stats_out = merge->stats_out;
    ta.partials_out = merge->partials_out;
  }
  ta.w_frag = s0.w_frag, ta.dx = s0.dx, ta.dtt_frag = s0.dtt_frag;
#ifdef MI_STAMPS  // diagnostic library only (make STAMPS=1): a timing experiment that leaves grad_x / grad_w wrong
  static const bool diag_no_dx = getenv("MI_TAIL_DIAG_NO_DX") != nullptr;
  ta.grad_x = diag_no_dx ? nullptr : s0.grad;
#else
  ta.grad_x = s0.grad;
#endif
  if (gbf) {
    ta.grad_x_bf = reinterpret_cast<bf16_t*>(s0.grad);
    ta.grad_x = nullptr;
  }
  if (s1) ta.w_frag1 = s1->w_frag, ta.dx1 = s1->dx, ta.grad_x1 = s1->grad, ta.dtt_frag1 = s1->dtt_frag;
  const char* what = s1      ? "separable sums -> loss, dA, dC | dX = dA Wg^T | dY = dC Wh^T"
                     : merge ? "bilinear sums -> loss, dT, dY | dX = dT W^T"
                             : "bilinear sums -> dT, dY | dX = dT W^T";
  int rc = launch_flash_tail(ta, s.d, s.fl.slab_f16, merge != nullptr, st, what);
  if (rc) return rc;
  if (!s0.grad_w) return MI_OK;  // the caller launches dW itself (mi_bilinear_bwd_dw), e.g. behind a reduce-scatter's start
  const DwArgs g{s0.xt_frag, s0.dtt_frag, s0.dx, s.d, s.br, s0.grad_w};
  if (!s1) return launch_bilinear_dw(g, st, "bilinear dW = X^T dT");
  const DwArgs h{s1->xt_frag, s1->dtt_frag, s1->dx, s.d, s.b, s1->grad_w};
  return launch_bilinear_dw(g, st, "separable dWg = X^T dA | dWh = Y^T dC", &h);
}
static TailSide bilinear_side(const BilinearPlan& p, int64_t dx, float* grad_x, float* grad_w) {
  return TailSide{p.wfb, dx, grad_x, p.dttfb, p.xtfb, grad_w};
}

static int bilinear_fwd_fast(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                             const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                             int estimator, int need_grad, float* loss_out, mi_stats* stats, float* partials_out,
                             float* scores_out, const BilinearPlan& p, hipStream_t st) {
  // need_grad bit 2: mi_bilinear_prep_local already made the part of the preparation that needs neither Y nor the column ids
  const bool fused = p.path != MI_PATH_GEMMS;
  int rc = fast_prep_and_t(x, y, w, sid_rows, sid_cols, br, b, row_offset, dx, dy, p, st, (need_grad & 4) && fused ? 2 : 0);
  if (rc) return rc;
  if (fused) {
    // bit 0: gradients wanted (the fused launch then accumulates both contractions); bits 1-3 are flags (fp8 staged,
    // local part prepared, raw records)
    rc = p.stage.launch(sid_rows, sid_cols, row_offset, (need_grad & 1) != 0, st);
    if (rc) return rc;
    if (scores_out) {  // per-pair scores are a diagnostic output: the stand-alone score GEMM writes them
      rc = launch_gemm_bf16(one_problem(p.tb, dy, p.yb, dy, br, b, dy), 1,
                            EpiScoreLse2{sid_rows, sid_cols, row_offset, scores_out, p.partials}, st,
                            "bilinear score+LSE");
      if (rc) return rc;
    }
    // need_grad bit 3: the caller gathers the RAW per-wave records (mi_bilinear_raw_records) from every rank and hands
    // them to mi_bilinear_bwd_records, whose first launch merges them: no finalize launch, nothing written to loss / stats
    if ((need_grad & 8) && p.path == MI_PATH_FUSED_TAIL) return MI_OK;
    return launch_finalize(p.stage.rec[0], p.stage.fl.n_rec[0], b, estimator, loss_out, stats, partials_out, st);
  }
  const int x3 = p.x3;
  rc = launch_gemm_bf16(one_problem(p.tb, x3 * dy, p.yb, x3 * dy, br, b, x3 * dy), 1,
                        EpiScoreLse2{sid_rows, sid_cols, row_offset, scores_out, p.partials}, st, "bilinear score+LSE");
  if (rc) return rc;
  // the launcher picks 256 x 256 tiles for large score matrices: fewer partials than the plan reserved
  return launch_finalize(p.partials, gemm_bf16_n_partials(br, b, x3 * dy), b, estimator, loss_out, stats, partials_out,
                         st);
}

static int bilinear_bwd_fast(const int64_t* sid_rows, const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset,
                             int64_t dx, int64_t dy, const mi_stats* stats, const float* grad_out, float* grad_x,
                             float* grad_y, float* grad_w, const BilinearPlan& p, hipStream_t st) {
  int rc = MI_OK;
  if (p.path == MI_PATH_FUSED_TAIL)
    return bilinear_tail(p.stage, row_offset, stats, grad_out, bilinear_side(p, dx, grad_x, grad_w), nullptr, grad_y, nullptr,
                         st);
  if (p.path == MI_PATH_FUSED) {
    // the forward's fused launch left U, V as slabs: scale by exp(m_ref - lse), subtract the diagonal term, add the
    // slabs in a fixed order -> dT (bf16, both orientations, operands of dW | dX) and grad_y
    FlashReduceArgs ra{};
    p.stage.reduce_jobs(ra.j, row_offset, ReduceOut{nullptr, p.dtb, p.dttb}, ReduceOut{grad_y, nullptr, nullptr});
    ra.stats = stats;
    ra.grad_out = grad_out;
    rc = launch_flash_reduce(ra, 2, dy, p.stage.fl.slab_f16, st, "bilinear dT, dY from the fused sums");
    if (rc) return rc;
    return bilinear_bwd_small(br, dx, dy, grad_x, grad_w, p, st);
  }
  // G and G^T (bf16) from recomputed score tiles
  const int x3 = p.x3;
  rc = launch_gemm_bf16(one_problem(p.tb, x3 * dy, p.yb, x3 * dy, br, b, x3 * dy), 1,
                            EpiGradScore2{sid_rows, sid_cols, row_offset, stats, grad_out, p.gb, p.gtb, x3 == 3 ? 1 : 0}, st,
                            "bilinear G");
  if (rc) return rc;
  return bilinear_bwd_from_g(br, b, dx, dy, grad_x, grad_y, grad_w, true, p, st);
}

// The backward behind G, G^T (bf16, in the plan): dT = G Y | dY = G^T T, then dW | dX.  has_w == false (S = X Y^T on
// projected embeddings): dT is grad_x itself and there is no dW | dX launch.
static int bilinear_bwd_from_g(int64_t br, int64_t b, int64_t dx, int64_t dy, float* grad_x, float* grad_y, float* grad_w,
                               bool has_w, const BilinearPlan& p, hipStream_t st) {
  int rc = MI_OK;
  const int x3 = p.x3;
  const int ra = x3 == 3 ? 1 : 0, rbk = x3 == 3 ? 2 : 0;
  // problem 0: dT[i, c] = sum_j G[i, j] Y[j, c]   (A = G [br][b], B = Y^T [dy][b])  -> bf16 both orientations
  // problem 1: dY[j, c] = sum_i G[i, j] T[i, c]   (A = G^T [b][br], B = T^T [dy][br]) -> fp32 grad_y
  GemmBf16Args two{};
  two.p[0] = GemmBf16Problem{p.gb, x3 * b, p.ytb, x3 * b, br, dy, x3 * b};
  two.p[1] = GemmBf16Problem{p.gtb, x3 * br, p.ttb, x3 * br, b, dy, x3 * br};
  two.n_problems = 2;
  two.k_chunk = x3 * (b > br ? b : br);
  EpiStoreMulti e2{};
  e2.out[0] = has_w ? EpiOut{nullptr, 0, 0, p.dtb, dy, p.dttb, br, nullptr, ra, rbk} : EpiOut{grad_x, dy, 0, nullptr, 0, nullptr, 0};
  e2.out[1] = EpiOut{grad_y, dy, 0, nullptr, 0, nullptr, 0};
  bool split_done = false;
  if (p.dt_splits > 1 && x3 == 1 && has_w) {
    // sharded row block: dT partial sums over K chunks into fp32 slabs, beside dY; then one pass that adds the slabs and
    // writes the two bf16 orientations of dT
    EpiStoreMulti es{};
    es.out[0] = EpiOut{p.dt_slab, dy, br * dy, nullptr, 0, nullptr, 0};
    es.out[1] = e2.out[1];
    const int sp[2] = {p.dt_splits, 1};
    const int64_t ch[2] = {p.dt_kchunk, br};
    rc = launch_gemm_bf16_flat(two, sp, ch, es, st, "bilinear dT = G Y | dY = G^T T");
    if (rc == MI_OK) {
      CvtJobs jobs{};
      jobs.j[0] = CvtJob{p.dt_slab, br, dy, p.dtb, p.dttb, p.dt_splits, br * dy};
      rc = launch_cvt_transpose3(jobs, st, "bilinear dT slabs -> bf16");
      if (rc) return rc;
      split_done = true;
    } else if (rc != MI_EINVAL) {
      return rc;
    }
  }
  if (!split_done) {
    rc = launch_gemm_bf16(two, 1, e2, st, "bilinear dT = G Y | dY = G^T T");
    if (rc) return rc;
  }
  if (!has_w) return MI_OK;
  return bilinear_bwd_small(br, dx, dy, grad_x, grad_w, p, st);
}

// dW[a, c] = sum_i X[i, a] dT[i, c]: A = X^T [dx][rows], B = dT^T [dy][rows], split over i into slabs
// dX[i, a] = sum_c dT[i, c] W[a, c]: A = dT [rows][dy], B = W [dx][dy]
// Both only wait for dT: one launch (few tiles each; on their own they leave most CUs idle).  The separable critic runs it
// once per modality.  what[3]: the labels of the pair and, for shapes the LDS-DMA kernel does not take, of dW and dX alone.
struct DwDxPair {
  const bf16_t *xt, *dtt, *dt, *w;
  int64_t rows, dx, dy;
  int x3;
  float* slab;
  int splits;
  int64_t kchunk;
};
static int launch_dw_dx(const DwDxPair& q, float* grad_x, float* grad_w, hipStream_t st, const char* const (&what)[3]) {
  const int64_t x3 = q.x3, rows = q.rows, dx = q.dx, dy = q.dy;
  GemmBf16Args dwx{};
  dwx.p[0] = GemmBf16Problem{q.xt, x3 * rows, q.dtt, x3 * rows, dx, dy, x3 * rows};
  dwx.p[1] = GemmBf16Problem{q.dt, x3 * dy, q.w, x3 * dy, rows, dx, x3 * dy};
  dwx.n_problems = 2;
  EpiStoreMulti e3{};
  e3.out[0] = EpiOut{q.slab, dy, dx * dy, nullptr, 0, nullptr, 0};
  e3.out[1] = EpiOut{grad_x, dx, 0, nullptr, 0, nullptr, 0};
  const int splits[2] = {q.splits, 1};
  const int64_t chunks[2] = {x3 * q.kchunk, x3 * dy};
  int rc = launch_gemm_bf16_flat(dwx, splits, chunks, e3, st, what[0]);
  if (rc == MI_EINVAL) {  // one launch each
    EpiStoreMulti e4{};
    e4.out[0] = e3.out[0];
    rc = launch_gemm_bf16(one_problem(q.xt, x3 * rows, q.dtt, x3 * rows, dx, dy, x3 * rows, x3 * q.kchunk), q.splits, e4, st,
                          what[1]);
    if (rc) return rc;
    e4.out[0] = e3.out[1];
    rc = launch_gemm_bf16(one_problem(q.dt, x3 * dy, q.w, x3 * dy, rows, dx, x3 * dy), 1, e4, st, what[2]);
  }
  if (rc) return rc;
  return launch_slab_reduce_ld(q.slab, q.splits, dx, dy, grad_w, dy, st, "slab_reduce_ld_kernel");
}
static int bilinear_bwd_small(int64_t br, int64_t dx, int64_t dy, float* grad_x, float* grad_w, const BilinearPlan& p,
                              hipStream_t st) {
  return launch_dw_dx(DwDxPair{p.xtb, p.dttb, p.dtb, p.wb, br, dx, dy, p.x3, p.dw_slab, p.dw_splits, p.dw_kchunk}, grad_x,
                      grad_w, st, {"bilinear dW = X^T dT | dX = dT W^T", "bilinear dW = X^T dT", "bilinear dX = dT W^T"});
}

// ------------------------------------------------------------------------------------------------ fp8 path (mi_fp8.h)
// absmax -> scales -> e4m3 operands; T on the fp8 MFMA with its absmax in the epilogue; T quantised.  Three stages, so
// that a sharded run can make the scales GLOBAL between them (mi_bilinear_fp8_stage): the absmax of the local image rows
// and of the local rows of T differ between ranks; a MAX all-reduce of the four numbers makes every rank quantise with
// the scales a single GPU would have used.
static int fp8_stage0(const float* x, const float* y, const float* w, int64_t br, int64_t b, int64_t dx, int64_t dy,
                      const BilinearPlan& p, hipStream_t st) {
  const int rc0 = launch_zero_words(p.f8sc, sizeof(Fp8Scales), st, "zero_words_kernel(fp8 scales)");
  if (rc0) return rc0;
  AbsmaxJobs aj{};
  aj.in[0] = x; aj.n[0] = br * dx; aj.slot[0] = 0;
  aj.in[1] = y; aj.n[1] = b * dy; aj.slot[1] = 1;
  aj.in[2] = w; aj.n[2] = dx * dy; aj.slot[2] = 2;
  aj.sc = p.f8sc;
  {
    ProfScope prof_("fp8 absmax X Y W", st);
    hipLaunchKernelGGL(fp8_absmax_kernel, dim3(kAbsmaxBlocks, 3), dim3(256), 0, st, aj);
  }
  MI_LAUNCH_CHECK("fp8_absmax_kernel");
  return MI_OK;
}
static int fp8_stage1(const float* x, const float* y, const float* w, int64_t br, int64_t b, int64_t dx, int64_t dy,
                      const BilinearPlan& p, hipStream_t st) {
  QuantJobs qj{};
  qj.j[0] = QuantJob{x, br, dx, 0, p.qx8, nullptr, nullptr, p.xtb};   // A of T = X W; X^T (bf16) for dW
  qj.j[1] = QuantJob{y, b, dy, 1, p.qy8, nullptr, nullptr, p.ytb};    // B of S = T Y^T; Y^T (bf16) for dT
  qj.j[2] = QuantJob{w, dx, dy, 2, nullptr, p.qwt8, p.wb, nullptr};   // B of T = X W is W^T; W (bf16) for dX
  qj.sc = p.f8sc;
  int64_t rmax = br > b ? br : b, cmax = dx > dy ? dx : dy;
  if (dx > rmax) rmax = dx;
  {
    ProfScope prof_("fp8 quantize X Y W", st);
    hipLaunchKernelGGL(fp8_quantize_kernel, dim3((unsigned)((cmax + 63) / 64), (unsigned)((rmax + 63) / 64), 3), dim3(256),
                       0, st, qj);
  }
  MI_LAUNCH_CHECK("fp8_quantize_kernel");
  return launch_gemm_fp8(GemmF8Args{p.qx8, dx, p.qwt8, dx, br, dy, dx}, EpiT8{p.t, p.f8sc}, st, "fp8 T = X W");
}
static int fp8_stage2(int64_t br, int64_t dy, const BilinearPlan& p, hipStream_t st) {
  QuantJobs qt{};
  qt.j[0] = QuantJob{p.t, br, dy, 3, p.qt8, nullptr, nullptr, p.ttb};  // A of S; T^T (bf16) for dY
  qt.sc = p.f8sc;
  {
    ProfScope prof_("fp8 quantize T", st);
    hipLaunchKernelGGL(fp8_quantize_kernel, dim3((unsigned)((dy + 63) / 64), (unsigned)((br + 63) / 64), 1), dim3(256), 0, st,
                       qt);
  }
  MI_LAUNCH_CHECK("fp8_quantize_kernel");
  return MI_OK;
}
static int fp8_prep_and_t(const float* x, const float* y, const float* w, int64_t br, int64_t b, int64_t dx, int64_t dy,
                          const BilinearPlan& p, hipStream_t st) {
  int rc = fp8_stage0(x, y, w, br, b, dx, dy, p, st);
  if (rc) return rc;
  rc = fp8_stage1(x, y, w, br, b, dx, dy, p, st);
  if (rc) return rc;
  return fp8_stage2(br, dy, p, st);
}

static int bilinear_fwd_fp8(const float* x, const float* y, const float* w, const int64_t* sid_rows, const int64_t* sid_cols,
                            int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int estimator,
                            float* loss_out, mi_stats* stats, float* partials_out, float* scores_out,
                            const BilinearPlan& p, bool staged, hipStream_t st) {
  int rc = staged ? MI_OK : fp8_prep_and_t(x, y, w, br, b, dx, dy, p, st);  // staged: mi_bilinear_fp8_stage made them
  if (rc) return rc;
  EpiScaled<EpiScoreLse2> e{EpiScoreLse2{sid_rows, sid_cols, row_offset, scores_out, p.partials},
                            {&p.f8sc->scale[3], nullptr}, {&p.f8sc->scale[1], nullptr}, p.partials};
  rc = launch_gemm_fp8(GemmF8Args{p.qt8, dy, p.qy8, dy, br, b, dy}, e, st, "fp8 score+LSE");
  if (rc) return rc;
  return launch_finalize(p.partials, gemm_fp8_n_partials(br, b, dy), b, estimator, loss_out, stats, partials_out, st);
}

static int bilinear_bwd_fp8(const int64_t* sid_rows, const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset,
                            int64_t dx, int64_t dy, const mi_stats* stats, const float* grad_out, float* grad_x,
                            float* grad_y, float* grad_w, const BilinearPlan& p, hipStream_t st) {
  const float* sc = p.f8sc->scale;  // device addresses: x, y, w, T
  // G and G^T (bf16) from recomputed fp8 score tiles
  EpiScaled<EpiGradScore2> eg{EpiGradScore2{sid_rows, sid_cols, row_offset, stats, grad_out, p.gb, p.gtb, 0},
                              {sc + 3, nullptr}, {sc + 1, nullptr}};
  int rc = launch_gemm_fp8(GemmF8Args{p.qt8, dy, p.qy8, dy, br, b, dy}, eg, st, "fp8 G");
  if (rc) return rc;
  // dT = s_y (G y_q) -> bf16 both orientations | dY = s_t (G^T t_q) -> grad_y; operands: the quantised values as bf16
  GemmBf16Args two{};
  two.p[0] = GemmBf16Problem{p.gb, b, p.ytb, b, br, dy, b};
  two.p[1] = GemmBf16Problem{p.gtb, br, p.ttb, br, b, dy, br};
  two.n_problems = 2;
  two.k_chunk = b > br ? b : br;
  EpiScaled<EpiStoreMulti> e2{};
  e2.inner.out[0] = EpiOut{nullptr, 0, 0, p.dtb, dy, p.dttb, br};
  e2.inner.out[1] = EpiOut{grad_y, dy, 0, nullptr, 0, nullptr, 0};
  e2.sa[0] = sc + 1;
  e2.sa[1] = sc + 3;
  rc = launch_gemm_bf16(two, 1, e2, st, "fp8 mode dT = G Y | dY = G^T T");
  if (rc) return rc;
  // dW = s_x (x_q^T dT) (split-K slabs) | dX = s_w (dT W_q^T)
  EpiScaled<EpiStoreMulti> e3{};
  e3.inner.out[0] = EpiOut{p.dw_slab, dy, dx * dy, nullptr, 0, nullptr, 0};
  e3.sa[0] = sc + 0;
  rc = launch_gemm_bf16(one_problem(p.xtb, br, p.dttb, br, dx, dy, br, p.dw_kchunk), p.dw_splits, e3, st,
                        "fp8 mode dW = X^T dT");
  if (rc) return rc;
  EpiScaled<EpiStoreMulti> e4{};
  e4.inner.out[0] = EpiOut{grad_x, dx, 0, nullptr, 0, nullptr, 0};
  e4.sa[0] = sc + 2;
  rc = launch_gemm_bf16(one_problem(p.dtb, dy, p.wb, dy, br, dx, dy), 1, e4, st, "fp8 mode dX = dT W^T");
  if (rc) return rc;
  return launch_slab_reduce_ld(p.dw_slab, p.dw_splits, dx, dy, grad_w, dy, st, "slab_reduce_ld_kernel");
}

// ------------------------------------------------------------------------------------------------ generic path
// The operand type of the strided-operand kernels (mi_gemm.h): bf16, or float for exact fp32 products.  `f` is a generic
// lambda called with a null pointer of that type (OperandOf names it).  The bilinear critic and the chains run bf16
// operands in the bf16 mode only (bf16x3 falls back to exact products), the separable critic in every mode but f32.
template <typename F>
static int with_operand_type(bool bf16, F&& f) {
  return bf16 ? f((bf16_t*)nullptr) : f((float*)nullptr);
}
template <typename P>
using OperandOf = std::remove_pointer_t<P>;

// out [M][N] (ld) = A B^T with K split into slabs when the output has too few tiles (exact-fp32 mode only: the plan holds
// the slab buffer); the slabs are added in split order (fixed order: reproducible)
template <typename OpT, typename TA, typename TB>
static int generic_gemm_store(const Operand<TA>& A, const Operand<TB>& B, int64_t M, int64_t N, int64_t K, float* out,
                              int64_t ld, const BilinearPlan& p, hipStream_t st, const char* what) {
  int sp = 1;
  int64_t kc = K;
  static const bool off = getenv("MI_GENERIC_NO_SPLITK") != nullptr;  // A/B switch
  if (p.gen_slab && !off) generic_splitk(M, N, K, sp, kc);
  if (sp <= 1 || (int64_t)sp * M * N > p.gen_slab_floats)
    return launch_gemm<OpT>(A, B, M, N, K, EpiStore{out, ld, nullptr, 1.0f, 0}, st, what);
  EpiStore e{p.gen_slab, N, nullptr, 1.0f, 0};
  e.slab_stride = M * N;
  const int rc = launch_gemm<OpT>(A, B, M, N, K, e, st, what, sp, kc);
  if (rc) return rc;
  return launch_slab_reduce_ld(p.gen_slab, sp, M, N, out, ld, st, "slab_reduce_ld_kernel");
}

template <typename OpT>
static int bilinear_fwd_impl(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                             const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                             int estimator, float* loss_out, mi_stats* stats, float* partials_out, float* scores_out,
                             const BilinearPlan& p, hipStream_t st) {
  int rc = MI_OK;
  const float* t = x;  // w == nullptr: separable form, the caller passes the projected embeddings (d_img == d_txt)
  if (w) {
    rc = generic_gemm_store<OpT>(make_operand(x, dx, 1), make_operand(w, 1, dy), br, dy, dx, p.t, dy, p, st,
                                 "bilinear T = X W (generic)");
    if (rc) return rc;
    t = p.t;
  }
  rc = launch_gemm<OpT>(make_operand(t, dy, 1), make_operand(y, dy, 1), br, b, dy,
                        EpiScoreLse{sid_rows, sid_cols, row_offset, scores_out, p.partials}, st,
                        "bilinear score+LSE (generic)");
  if (rc) return rc;
  return launch_finalize(p.partials, p.n_partials, b, estimator, loss_out, stats, partials_out, st);
}

template <typename OpT, typename TG>
static int generic_bwd_from_g(const float* x, const float* y, const float* w, const float* t, const TG* g, int64_t br,
                              int64_t b, int64_t dx, int64_t dy, float* grad_x, float* grad_y, float* grad_w,
                              const BilinearPlan& p, hipStream_t st);

template <typename OpT, typename TG>
static int bilinear_bwd_impl(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                             const int64_t* sid_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                             const mi_stats* stats, const float* grad_out, float* grad_x, float* grad_y, float* grad_w,
                             const BilinearPlan& p, hipStream_t st) {
  TG* g = (TG*)p.g;
  int rc = MI_OK;
  const float* t = x;  // w == nullptr: dT is dX
  if (w) {
    rc = generic_gemm_store<OpT>(make_operand(x, dx, 1), make_operand(w, 1, dy), br, dy, dx, p.t, dy, p, st,
                                 "bilinear T = X W (generic, bwd)");
    if (rc) return rc;
    t = p.t;
  }
  rc = launch_gemm<OpT>(make_operand(t, dy, 1), make_operand(y, dy, 1), br, b, dy,
                        EpiGradScore<TG>{sid_rows, sid_cols, row_offset, stats, grad_out, g}, st, "bilinear G (generic)");
  if (rc) return rc;
  return generic_bwd_from_g<OpT, TG>(x, y, w, t, g, br, b, dx, dy, grad_x, grad_y, grad_w, p, st);
}

// The generic backward behind G [br][b] (TG): dT = G Y, dY = G^T T, dW = X^T dT, dX = dT W^T; w == nullptr: dT is dX.
template <typename OpT, typename TG>
static int generic_bwd_from_g(const float* x, const float* y, const float* w, const float* t, const TG* g, int64_t br,
                              int64_t b, int64_t dx, int64_t dy, float* grad_x, float* grad_y, float* grad_w,
                              const BilinearPlan& p, hipStream_t st) {
  float* dt = w ? p.dt : grad_x;
  int rc = generic_gemm_store<OpT>(make_operand((const TG*)g, b, 1), make_operand(y, 1, dy), br, dy, b, dt, dy, p, st,
                               "bilinear dT = G Y (generic)");
  if (rc) return rc;
  rc = generic_gemm_store<OpT>(make_operand((const TG*)g, 1, b), make_operand(t, 1, dy), b, dy, br, grad_y, dy, p, st,
                               "bilinear dY = G^T T (generic)");
  if (rc) return rc;
  if (!w) return MI_OK;
  rc = generic_gemm_store<OpT>(make_operand(x, 1, dx), make_operand((const float*)p.dt, 1, dy), dx, dy, br, grad_w, dy, p, st,
                               "bilinear dW = X^T dT (generic)");
  if (rc) return rc;
  return generic_gemm_store<OpT>(make_operand((const float*)p.dt, dy, 1), make_operand(w, dy, 1), br, dx, dy, grad_x, dx, p,
                                 st, "bilinear dX = dT W^T (generic)");
}

static int check_common(const char* fn, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy,
                        int precision) {
  MI_CHECK_ARG(br >= 1 && b >= 1 && br <= b, "%s: need 1 <= b_rows <= b (got %lld, %lld)", fn, (long long)br,
               (long long)b);
  MI_CHECK_ARG(row_offset >= 0 && row_offset + br <= b, "%s: row block [%lld, %lld) outside [0, %lld)", fn,
               (long long)row_offset, (long long)(row_offset + br), (long long)b);
  MI_CHECK_ARG(dx >= 1 && dy >= 1, "%s: embedding widths must be >= 1", fn);
  MI_CHECK_ARG(precision == MI_PREC_F32 || precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3 ||
                   precision == MI_PREC_FP8,
               "%s: unknown precision %d", fn, precision);
  return MI_OK;
}

// the plan's path of an fp8 call outside the fp8 kernels' shapes
static int fp8_shape_error(const char* fn) {
  set_error("%s: the fp8 mode needs a weight matrix, batch sizes that are multiples of 8 and widths that are multiples of 16",
            fn);
  return MI_ESHAPE;
}

}  // namespace mi

using namespace mi;

extern "C" {

size_t mi_bilinear_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return 0;  // (the planner divides by tile counts)
  Workspace ws(nullptr, 0);
  return plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true).bytes + 256;
}

int mi_bilinear_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows, const int64_t* sid_cols,
                    int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img, int64_t d_txt, int estimator,
                    int precision, int need_grad, float* loss_out, mi_stats* stats, float* partials_out,
                    float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && stats && workspace, "mi_bilinear_fwd: null pointer");
  MI_CHECK_ARG(w || d_img == d_txt, "mi_bilinear_fwd: w == NULL (separable form) needs d_img == d_txt");
  int rc = check_common("mi_bilinear_fwd", b_rows, b, row_offset, d_img, d_txt, precision);
  if (rc) return rc;
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_bilinear_fwd: unknown estimator %d", estimator);
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, w != nullptr);
  rc = ws_fits(ws, "mi_bilinear_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (p.path) {
    case MI_ESHAPE:
      return fp8_shape_error("mi_bilinear_fwd");
    case MI_PATH_FP8_GEMMS:
      return bilinear_fwd_fp8(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, estimator, loss_out, stats,
                              partials_out, scores_out, p, (need_grad & 2) != 0, st);
    case MI_PATH_GENERIC:
      return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
        return bilinear_fwd_impl<OperandOf<decltype(op)>>(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt,
                                                          estimator, loss_out, stats, partials_out, scores_out, p, st);
      });
    default:  // MI_PATH_GEMMS, MI_PATH_FUSED, MI_PATH_FUSED_TAIL
      return bilinear_fwd_fast(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, estimator, need_grad,
                               loss_out, stats, partials_out, scores_out, p, st);
  }
}

int mi_bilinear_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows, const int64_t* sid_cols,
                    int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img, int64_t d_txt, int precision,
                    const mi_stats* stats, const float* grad_out, float* grad_x, float* grad_y, float* grad_w,
                    void* workspace, size_t workspace_bytes, int workspace_from_forward, void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && stats && grad_x && grad_y && workspace,
               "mi_bilinear_bwd: null pointer");
  MI_CHECK_ARG((w && grad_w) || (!w && d_img == d_txt),
               "mi_bilinear_bwd: w == NULL (separable form) needs d_img == d_txt; w != NULL needs grad_w");
  int rc = check_common("mi_bilinear_bwd", b_rows, b, row_offset, d_img, d_txt, precision);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, w != nullptr);
  rc = ws_fits(ws, "mi_bilinear_bwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (p.path) {
    case MI_ESHAPE:
      return fp8_shape_error("mi_bilinear_bwd");
    case MI_PATH_FP8_GEMMS:
      if (!workspace_from_forward) {
        rc = fp8_prep_and_t(x, y, w, b_rows, b, d_img, d_txt, p, st);
        if (rc) return rc;
      }
      return bilinear_bwd_fp8(sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, stats, grad_out, grad_x, grad_y,
                              grad_w, p, st);
    case MI_PATH_GENERIC:
      return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
        using OpT = OperandOf<decltype(op)>;  // G is stored in the operand type
        return bilinear_bwd_impl<OpT, OpT>(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, stats, grad_out,
                                           grad_x, grad_y, grad_w, p, st);
      });
    default:  // MI_PATH_GEMMS, MI_PATH_FUSED, MI_PATH_FUSED_TAIL
      if (!workspace_from_forward) {  // rebuild the bf16 operand copies, T and the fused sums
        rc = fast_prep_and_t(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, p, st);
        if (rc) return rc;
        if (p.path != MI_PATH_GEMMS) {
          rc = p.stage.launch(sid_rows, sid_cols, row_offset, true, st);
          if (rc) return rc;
        }
      }
      return bilinear_bwd_fast(sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, stats, grad_out, grad_x, grad_y,
                               grad_w, p, st);
  }
}

/* Sharded batches without the finalize and merge launches.  The fused kernel leaves one 16-byte record per wave in the
 * workspace; mi_bilinear_raw_records says where (byte offset) and how many.  A rank runs mi_bilinear_fwd(need_grad | 8)
 * (no finalize: loss / stats / partials_out untouched), all-gathers that region from every rank (rank order) and calls
 * mi_bilinear_bwd_records, whose first launch merges ALL records in the gathered order on every workgroup (bit-identical
 * statistics and loss on every rank), writes loss / stats and goes on with the backward's tail.  0 records = the shape
 * does not take this path (use mi_bilinear_fwd / mi_merge_partials / mi_bilinear_bwd). */
size_t mi_bilinear_raw_records(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision,
                               size_t* offset_bytes) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  char* fake = reinterpret_cast<char*>(uintptr_t(1) << 20);  // only pointer differences are used
  Workspace ws(fake, ~size_t(0) >> 1);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true);
  if (p.path != MI_PATH_FUSED_TAIL) return 0;
  if (offset_bytes) *offset_bytes = (size_t)(reinterpret_cast<char*>(p.stage.rec[0]) - fake);
  return (size_t)p.stage.fl.n_rec[0];
}

int mi_bilinear_bwd_records(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                            const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                            int64_t d_txt, int precision, int estimator, const float* records, int64_t n_records,
                            int64_t n_pos, const float* grad_out, float* loss_out, mi_stats* stats_out, float* grad_x,
                            float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && w && sid_rows && sid_cols && records && stats_out && grad_x && grad_y && workspace,
               "mi_bilinear_bwd_records: null pointer");
  MI_CHECK_ARG(n_records > 0 && n_pos > 0, "mi_bilinear_bwd_records: n_records and n_pos must be positive");
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_bilinear_bwd_records: unknown estimator %d", estimator);
  int rc = check_common("mi_bilinear_bwd_records", b_rows, b, row_offset, d_img, d_txt, precision);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true);
  rc = ws_fits(ws, "mi_bilinear_bwd_records");
  if (rc) return rc;
  if (p.path != MI_PATH_FUSED_TAIL) {
    set_error("mi_bilinear_bwd_records: shape / precision outside the fused kernels (mi_bilinear_raw_records returns 0)");
    return MI_ESHAPE;
  }
  const TailMerge tm{estimator, loss_out, stats_out, nullptr, records, n_records, n_pos};
  const TailSide side = bilinear_side(p, d_img, grad_x, grad_w);
  return bilinear_tail(p.stage, row_offset, nullptr, grad_out, side, nullptr, grad_y, &tm, (hipStream_t)stream);
}

/* The second launch of the backward's tail on its own (dW = X^T dT from the fragment-major operands the first launch and
 * the forward left in the workspace).  For callers that ran mi_bilinear_bwd_records with grad_w == NULL: the reduce-scatter
 * of grad_y only needs the first launch, so a sharded step starts it (on RCCL's stream) BEFORE this launch and the two
 * overlap. */
int mi_bilinear_bwd_dw(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision, float* grad_w,
                       void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(grad_w && workspace, "mi_bilinear_bwd_dw: null pointer");
  int rc = check_common("mi_bilinear_bwd_dw", b_rows, b, 0, d_img, d_txt, precision);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true);
  rc = ws_fits(ws, "mi_bilinear_bwd_dw");
  if (rc) return rc;
  if (p.path != MI_PATH_FUSED_TAIL) {
    set_error("mi_bilinear_bwd_dw: shape / precision outside the fused kernels");
    return MI_ESHAPE;
  }
  return launch_bilinear_dw(DwArgs{p.xtfb, p.dttfb, d_img, d_txt, b_rows, grad_w}, (hipStream_t)stream, "bilinear dW = X^T dT");
}

/* Sharded batches: the part of the forward's preparation that depends on the rank's OWN rows only -- the bf16 copies of
 * X and W and T = X W -- so that it can run while the all-gather of the text embeddings is in flight.  Follow with
 * mi_bilinear_fwd(..., need_grad | 4, ...) on the same workspace (bit 2: the local part is prepared).  Returns
 * MI_ESHAPE where the shape does not take the fused kernels (the caller then simply calls mi_bilinear_fwd as usual). */
int mi_bilinear_prep_local(const float* x, const float* w, int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt,
                           int precision, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && w && workspace, "mi_bilinear_prep_local: null pointer");
  int rc = check_common("mi_bilinear_prep_local", b_rows, b, 0, d_img, d_txt, precision);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true);
  rc = ws_fits(ws, "mi_bilinear_prep_local");
  if (rc) return rc;
  if (p.path != MI_PATH_FUSED && p.path != MI_PATH_FUSED_TAIL) {
    set_error("mi_bilinear_prep_local: shape / precision outside the fused kernels (call mi_bilinear_fwd alone)");
    return MI_ESHAPE;
  }
  return fast_prep_and_t(x, nullptr, w, nullptr, nullptr, b_rows, b, 0, d_img, d_txt, p, (hipStream_t)stream, 1);
}

/* fp8 mode on a SHARDED batch: the per-tensor scales must be those of the whole batch.  The forward's preparation in
 * three stages around the caller's two MAX all-reduces of amax_io (4 floats, device):
 *   stage 0: local absmax of x (slot 0), y (1), w (2) -> amax_io[0..2]                    | all-reduce MAX amax_io
 *   stage 1: quantise x, y, w with amax_io[0..2]; T = x_q W_q; local absmax of T -> amax_io[3] | all-reduce MAX amax_io
 *   stage 2: quantise T with amax_io[3]
 * then mi_bilinear_fwd(..., need_grad | 2, ...) on the same workspace (bit 1: "the fp8 operands are staged"). */
int mi_bilinear_fp8_stage(const float* x, const float* y, const float* w, int64_t b_rows, int64_t b, int64_t d_img,
                          int64_t d_txt, int stage, float* amax_io, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && w && amax_io && workspace, "mi_bilinear_fp8_stage: null pointer");
  MI_CHECK_ARG(stage >= 0 && stage <= 2, "mi_bilinear_fp8_stage: stage %d outside 0..2", stage);
  int rc = check_common("mi_bilinear_fp8_stage", b_rows, b, 0, d_img, d_txt, MI_PREC_FP8);
  if (rc) return rc;
  if (!fp8_ok(b_rows, b, d_img, d_txt, MI_PREC_FP8, true)) {
    set_error("mi_bilinear_fp8_stage: the fp8 mode needs batch sizes that are multiples of 8 and widths that are multiples of 16");
    return MI_ESHAPE;
  }
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b_rows, b, d_img, d_txt, MI_PREC_FP8, true);
  rc = ws_fits(ws, "mi_bilinear_fp8_stage");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // non-negative floats and their bit patterns order alike: the absmax slots hold bit patterns, amax_io floats
  auto copy = [&](void* dst, const void* src, size_t n) {
    return launch_copy_words(dst, src, n, st, "copy_words_kernel(fp8 absmax)");
  };
  if (stage == 0) {
    rc = fp8_stage0(x, y, w, b_rows, b, d_img, d_txt, p, st);
    if (rc) return rc;
    return copy(amax_io, p.f8sc->amax_bits, 3 * sizeof(float));
  }
  if (stage == 1) {
    rc = copy(p.f8sc->amax_bits, amax_io, 3 * sizeof(float));
    if (rc) return rc;
    rc = fp8_stage1(x, y, w, b_rows, b, d_img, d_txt, p, st);
    if (rc) return rc;
    return copy(amax_io + 3, &p.f8sc->amax_bits[3], sizeof(float));
  }
  rc = copy(&p.f8sc->amax_bits[3], amax_io + 3, sizeof(float));
  if (rc) return rc;
  return fp8_stage2(b_rows, d_txt, p, st);
}

/* One critic step -- forward, loss and every gradient -- in one call (single GPU: b_rows == b).  Where the fused kernels
 * take the shape this is four launches: conversions + T, the fused B x B kernel, [records -> statistics and loss; partial
 * sums -> dT, grad_y; dX], dW.  Nothing needs the loss between the fused kernel and the gradients, so the statistics are
 * merged inside the third launch (no finalize launch).  Other shapes / precisions: the forward and the backward entry
 * points, one after the other.  grad_out may be NULL (dL/dloss = 1). */
int mi_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                     int64_t d_txt, int estimator, int precision, const float* grad_out, float* loss_out, mi_stats* stats,
                     float* partials_out, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                     size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && stats && grad_x && grad_y && workspace, "mi_bilinear_step: null pointer");
  MI_CHECK_ARG((w && grad_w) || (!w && d_img == d_txt),
               "mi_bilinear_step: w == NULL (separable form) needs d_img == d_txt; w != NULL needs grad_w");
  int rc = check_common("mi_bilinear_step", b, b, 0, d_img, d_txt, precision);
  if (rc) return rc;
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_bilinear_step: unknown estimator %d", estimator);
  Workspace ws(workspace, workspace_bytes);
  const BilinearPlan p = plan_bilinear(ws, b, b, d_img, d_txt, precision, w != nullptr);
  rc = ws_fits(ws, "mi_bilinear_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p.path == MI_PATH_FUSED_TAIL) {
    rc = fast_prep_and_t(x, y, w, sid, sid, b, b, 0, d_img, d_txt, p, st);
    if (rc) return rc;
    rc = p.stage.launch(sid, sid, 0, true, st);
    if (rc) return rc;
    const TailMerge m{estimator, loss_out, stats, partials_out};
    return bilinear_tail(p.stage, 0, stats, grad_out, bilinear_side(p, d_img, grad_x, grad_w), nullptr, grad_y, &m, st);
  }
  rc = mi_bilinear_fwd(x, y, w, sid, sid, b, b, 0, d_img, d_txt, estimator, precision, 1, loss_out, stats, partials_out,
                       nullptr, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return mi_bilinear_bwd(x, y, w, sid, sid, b, b, 0, d_img, d_txt, precision, stats, grad_out, grad_x, grad_y, grad_w,
                         workspace, workspace_bytes, 1, stream);
}

/* The same step at a bf16 boundary: x [b][d_img] and y [b][d_txt] are bf16 (what encoders under the autocast policy of
 * encoders.py emit), the gradients for them are written in bf16 when grads_bf16 != 0 (fp32 buffers otherwise); w, grad_w,
 * loss and statistics stay fp32.  The kernels round x and y to bf16 as their first act anyway: with bf16-representable
 * inputs the results are bit-identical to mi_bilinear_step(precision = MI_PREC_BF16), minus 25 MB of conversion traffic
 * per step.  Only where the fused kernels and the two-launch tail take the shape (mi_bilinear_path == MI_PATH_FUSED_TAIL);
 * MI_ESHAPE otherwise (convert and call mi_bilinear_step). */
int mi_bilinear_step_bf16(const void* x_bf16, const void* y_bf16, const float* w, const int64_t* sid, int64_t b,
                          int64_t d_img, int64_t d_txt, int estimator, const float* grad_out, float* loss_out,
                          mi_stats* stats, float* partials_out, void* grad_x, void* grad_y, int grads_bf16, float* grad_w,
                          void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x_bf16 && y_bf16 && w && sid && stats && grad_x && grad_y && grad_w && workspace,
               "mi_bilinear_step_bf16: null pointer");
  int rc = check_common("mi_bilinear_step_bf16", b, b, 0, d_img, d_txt, MI_PREC_BF16);
  if (rc) return rc;
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_bilinear_step_bf16: unknown estimator %d", estimator);
  Workspace ws(workspace, workspace_bytes);
  BilinearPlan p = plan_bilinear(ws, b, b, d_img, d_txt, MI_PREC_BF16, true);
  rc = ws_fits(ws, "mi_bilinear_step_bf16");
  if (rc) return rc;
  if (p.path != MI_PATH_FUSED_TAIL || (uintptr_t)x_bf16 % 16 != 0 ||
      (uintptr_t)y_bf16 % 16 != 0) {
    set_error("mi_bilinear_step_bf16: shape outside the fused kernels (mi_bilinear_path != MI_PATH_FUSED_TAIL) or "
              "embeddings not 16-byte aligned: convert to fp32 and call mi_bilinear_step");
    return MI_ESHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const bf16_t* xb = reinterpret_cast<const bf16_t*>(x_bf16);
  const bf16_t* yb = reinterpret_cast<const bf16_t*>(y_bf16);
  p.stage.rows[0] = yb;  // the streamed operand of problem 0: the input itself
  rc = fast_prep_and_t_bf16(xb, yb, w, sid, sid, b, b, 0, d_img, d_txt, p, st);
  if (rc) return rc == MI_EINVAL ? MI_ESHAPE : rc;
  rc = p.stage.launch(sid, sid, 0, true, st);
  if (rc) return rc;
  TailMerge m{estimator, loss_out, stats, partials_out};
  m.grads_bf16 = grads_bf16 ? 1 : 0;
  const TailSide side = bilinear_side(p, d_img, reinterpret_cast<float*>(grad_x), grad_w);
  return bilinear_tail(p.stage, 0, stats, grad_out, side, nullptr, reinterpret_cast<float*>(grad_y), &m, st);
}

/* Which kernels a bilinear-critic shape takes (host-side arithmetic only, nothing is launched): MI_PATH_*.  The Python
 * binding warns once per shape when a 16-bit call leaves the fused kernels. */
int mi_bilinear_path(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return MI_EINVAL;
  Workspace ws(nullptr, 0);
  return plan_bilinear(ws, b_rows, b, d_img, d_txt, precision, true).path;
}

/* Which kernel launch_gemm_bf16 issues for one m x n x k problem, n_splits = 1, a storing epilogue: MI_GEMM16_* (the
 * launcher switches on the same function; nothing is launched). */
int mi_gemm16_variant(int64_t m, int64_t n, int64_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return MI_EINVAL;
  static_assert(kGemm16Plain == MI_GEMM16_PLAIN && kGemm16Glds == MI_GEMM16_GLDS && kGemm16Glds4 == MI_GEMM16_GLDS4 &&
                    kGemm16Pipe128 == MI_GEMM16_PIPE128 && kGemm16Pipe256x128 == MI_GEMM16_PIPE256X128 &&
                    kGemm16Big == MI_GEMM16_BIG,
                "include/mi_critic.h out of step with GemmBf16Variant");
  const int64_t ks[2] = {k, 0};
  return gemm_bf16_variant(m, n, ks, 1, 1, k, false);
}

}  // extern "C"

// ================================================================================================ separable critic
// S = (X Wg)(Y Wh)^T  (BASELINE.json configs[1]; an extension: no reference code, oracle-pinned only).  Projections,
// the fused B x B stage and every gradient are this library's kernels:
//   forward : prep X, Y, Wg, Wh -> A = X Wg | C = Y Wh (one two-problem launch; bf16 row-major + fragment-major copies)
//             -> fused kernel (problem 0: A rows x C rows, problem 1: C rows x A rows) -> statistics
//   backward: slab reduce -> dA, dC (bf16, both orientations) -> {dWg = X^T dA | dX = dA Wg^T}, {dWh = Y^T dC | dY = dC Wh^T}
// Other shapes and the fp32 parity mode run on the generic strided-operand kernels (mi_gemm.h).
namespace mi {

struct SeparablePlan {
  int path;            // MI_PATH_GENERIC, MI_PATH_FUSED or MI_PATH_FUSED_TAIL
  FusedStage stage;    // the fused B x B stage on S = A C^T
  bf16_t *xb, *xtb, *yb, *ytb, *gb, *gtb, *hb, *htb;   // X, Y, Wg, Wh as bf16, row-major and transposed
  bf16_t *ab, *afb, *cb, *cfb;                          // projections, row-major and fragment-major
  bf16_t *dab, *datb, *dcb, *dctb;                      // their gradients, both orientations
  float *wg_slab, *wh_slab;
  int wg_splits, wh_splits;
  int64_t wg_kchunk, wh_kchunk;
  // the two-launch backward tail (mi_bilinear_tail.h, round 4): fragment-major Wg, Wh (B operands of dX = dA Wg^T and
  // dY = dC Wh^T inside the tail kernel), X^T, Y^T, dA^T, dC^T (operands of the one dWg | dWh launch)
  bool tail;
  bf16_t *gfb, *hfb, *xtfb, *ytfb, *datfb, *dctfb;
  // generic path
  float *a32, *c32, *da32, *dc32;
  void* g;
  Partial* partials;
  int64_t n_partials;
  size_t bytes;
};

static void split_plan(int64_t rows, int64_t m, int64_t n, int& splits, int64_t& kchunk) {
  const int64_t tiles = ((m + kTile - 1) / kTile) * ((n + kTile - 1) / kTile);
  int64_t sp = (128 + tiles - 1) / tiles;
  kchunk = (rows + sp - 1) / sp;
  kchunk = (kchunk + kG2KT - 1) / kG2KT * kG2KT;
  splits = (int)((rows + kchunk - 1) / kchunk);
}

static SeparablePlan plan_separable(Workspace& ws, int64_t br, int64_t b, int64_t dx, int64_t dy, int64_t k,
                                    int precision) {
  SeparablePlan p{};
  FusedStage& s = p.stage;
  if (precision == MI_PREC_BF16 && dx % 8 == 0 && dy % 8 == 0 && k % 64 == 0) s.fl = flash_plan(br, b, k);
  s.br = br, s.b = b, s.d = k;
  s.what_grad = "separable fused S | P C | P^T A", s.what_fwd = "separable fused S + LSE";
  if (s.fl.ok) {
    p.xb = ws.take<bf16_t>(br * dx);
    p.xtb = ws.take<bf16_t>(br * dx);
    p.yb = ws.take<bf16_t>(b * dy);
    p.ytb = ws.take<bf16_t>(b * dy);
    p.gb = ws.take<bf16_t>(dx * k);
    p.gtb = ws.take<bf16_t>(dx * k);
    p.hb = ws.take<bf16_t>(dy * k);
    p.htb = ws.take<bf16_t>(dy * k);
    p.ab = ws.take<bf16_t>(br * k);
    p.afb = ws.take<bf16_t>(br * k);
    p.cb = ws.take<bf16_t>(b * k);
    p.cfb = ws.take<bf16_t>(b * k);
    p.dab = ws.take<bf16_t>(br * k);
    p.datb = ws.take<bf16_t>(br * k);
    p.dcb = ws.take<bf16_t>(b * k);
    p.dctb = ws.take<bf16_t>(b * k);
    s.frag[0] = p.afb, s.rows[0] = p.cb;  // problem 0: the rows of C for every row of A
    s.frag[1] = p.cfb, s.rows[1] = p.ab;
    s.take(ws);
    split_plan(br, dx, k, p.wg_splits, p.wg_kchunk);
    split_plan(b, dy, k, p.wh_splits, p.wh_kchunk);
    p.wg_slab = ws.take<float>((int64_t)p.wg_splits * dx * k);
    p.wh_slab = ws.take<float>((int64_t)p.wh_splits * dy * k);
    static const bool no_tail = getenv("MI_NO_TAIL") != nullptr;  // A/B switch, as for the bilinear critic
    p.tail = !no_tail && flash_tail_ok(br, dx, k) && flash_tail_ok(b, dy, k) && s.fl.slab_f16;
    if (p.tail) {
      p.gfb = ws.take<bf16_t>(dx * k);
      p.hfb = ws.take<bf16_t>(dy * k);
      p.xtfb = ws.take<bf16_t>(br * dx);
      p.ytfb = ws.take<bf16_t>(b * dy);
      p.datfb = ws.take<bf16_t>(br * k);
      p.dctfb = ws.take<bf16_t>(b * k);
    }
  } else {
    p.a32 = ws.take<float>(br * k);
    p.c32 = ws.take<float>(b * k);
    p.da32 = ws.take<float>(br * k);
    p.dc32 = ws.take<float>(b * k);
    p.n_partials = ((b + kTile - 1) / kTile) * ((br + kTile - 1) / kTile);
    p.partials = ws.take<Partial>(p.n_partials);
    if (precision == MI_PREC_BF16) p.g = ws.take<bf16_t>(br * b);
    else p.g = ws.take<float>(br * b);
  }
  p.path = !s.fl.ok ? MI_PATH_GENERIC : p.tail ? MI_PATH_FUSED_TAIL : MI_PATH_FUSED;
  p.bytes = ws.off;
  return p;
}

static int separable_prep_project(const float* x, const float* y, const float* wg, const float* wh,
                                  const int64_t* sid_rows, const int64_t* sid_cols, int64_t br, int64_t b,
                                  int64_t row_offset, int64_t dx, int64_t dy, int64_t k, const SeparablePlan& p,
                                  hipStream_t st) {
  CvtJobs jobs{};
  jobs.j[0] = CvtJob{x, br, dx, p.xb, p.xtb, 0, 0, nullptr, 0, 0, p.tail ? p.xtfb : nullptr};
  jobs.j[1] = CvtJob{y, b, dy, p.yb, p.ytb, 0, 0, nullptr, 0, 0, p.tail ? p.ytfb : nullptr};
  jobs.j[2] = CvtJob{wg, dx, k, p.gb, p.gtb, 0, 0, p.tail ? p.gfb : nullptr};
  jobs.j[3] = CvtJob{wh, dy, k, p.hb, p.htb, 0, 0, p.tail ? p.hfb : nullptr};
  jobs.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
  int rc = launch_cvt_transpose3(jobs, st, "separable prep X Y Wg Wh");
  if (rc) return rc;
  // A[i, c] = sum_a X[i, a] Wg[a, c] (A operand Xb [br][dx], B operand Wg^T [k][dx]);  C likewise from Y, Wh
  GemmBf16Args two{};
  two.p[0] = GemmBf16Problem{p.xb, dx, p.gtb, dx, br, k, dx};
  two.p[1] = GemmBf16Problem{p.yb, dy, p.htb, dy, b, k, dy};
  two.n_problems = 2;
  two.k_chunk = dx > dy ? dx : dy;
  EpiStoreMulti e{};
  e.out[0] = EpiOut{nullptr, 0, 0, p.ab, k, nullptr, 0, p.afb};
  e.out[1] = EpiOut{nullptr, 0, 0, p.cb, k, nullptr, 0, p.cfb};
  return launch_gemm_bf16(two, 1, e, st, "separable A = X Wg | C = Y Wh");
}

// The one-call step's form of the above (mi_separable_step on the two-launch tail): conversions and BOTH projections in ONE
// launch (bilinear_prep_t_kernel with a second product) -- nobody reads the row-major / transposed bf16 copies of X, Y, Wg,
// Wh on that path, only the fragment-major ones.  MI_EINVAL: a shape the launch does not take (the caller falls back).
static int separable_prep_project_fused(const float* x, const float* y, const float* wg, const float* wh,
                                        const int64_t* sid_rows, const int64_t* sid_cols, int64_t br, int64_t b,
                                        int64_t row_offset, int64_t dx, int64_t dy, int64_t k, const SeparablePlan& p,
                                        hipStream_t st) {
  static const bool off = getenv("MI_SEP_NO_FUSED_PREP") != nullptr;  // A/B switch
  if (off) return MI_EINVAL;
  CvtJobs side{};
  side.j[0] = CvtJob{x, br, dx, nullptr, nullptr, 0, 0, nullptr, 0, 0, p.xtfb};
  side.j[1] = CvtJob{y, b, dy, nullptr, nullptr, 0, 0, nullptr, 0, 0, p.ytfb};
  side.j[2] = CvtJob{wg, dx, k, nullptr, nullptr, 0, 0, p.gfb};
  side.j[3] = CvtJob{wh, dy, k, nullptr, nullptr, 0, 0, p.hfb};
  side.dup = p.stage.dup_job(sid_rows, sid_cols, row_offset);
  const PrepTSecond c{y, wh, b, k, dy, p.cb, p.cfb};
  return launch_prep_t(x, wg, br, k, dx, p.ab, p.afb, side, st, "separable prep + A = X Wg | C = Y Wh", false, &c);
}

// The separable critic's projections on the strided-operand kernels (its generic path, and every shape of the InfoNCE /
// f-divergence chains): A = X Wg [br][k], C = Y Wh [b][k] (a row block projects all b text rows) and their gradients,
// bf16 operands in the bf16 mode, exact fp32 products otherwise.  The launch labels are the caller's.
struct SepLabels {
  const char *a, *c, *dx, *dwg, *dy, *dwh;
};
static constexpr SepLabels kSepFwd = {"separable A = X Wg (generic)", "separable C = Y Wh (generic)"};
static constexpr SepLabels kSepBwd = {"separable A = X Wg (generic, bwd)", "separable C = Y Wh (generic, bwd)",
                                      "separable dX = dA Wg^T (generic)", "separable dWg = X^T dA (generic)",
                                      "separable dY = dC Wh^T (generic)", "separable dWh = Y^T dC (generic)"};

static int separable_project(const SepLabels& l, bool bf, const float* x, const float* y, const float* wg,
                             const float* wh, int64_t br, int64_t b, int64_t dx, int64_t dy, int64_t k, float* a, float* c,
                             hipStream_t st) {
  return with_operand_type(bf, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    const int rc = launch_gemm<OpT>(make_operand(x, dx, 1), make_operand(wg, 1, k), br, k, dx,
                                    EpiStore{a, k, nullptr, 1.0f, 0}, st, l.a);
    if (rc) return rc;
    return launch_gemm<OpT>(make_operand(y, dy, 1), make_operand(wh, 1, k), b, k, dy, EpiStore{c, k, nullptr, 1.0f, 0},
                            st, l.c);
  });
}

// dA [br][k] -> dX = dA Wg^T and (the row block's part of) dWg = X^T dA; dC [b][k] -> (parts of) dY = dC Wh^T, dWh = Y^T dC
static int separable_project_back(const SepLabels& l, bool bf, const float* x, const float* y, const float* wg,
                                  const float* wh, int64_t br, int64_t b, int64_t dx, int64_t dy, int64_t k,
                                  const float* da, const float* dc, float* grad_x, float* grad_y, float* grad_wg,
                                  float* grad_wh, hipStream_t st) {
  return with_operand_type(bf, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    int rc = launch_gemm<OpT>(make_operand(da, k, 1), make_operand(wg, k, 1), br, dx, k,
                              EpiStore{grad_x, dx, nullptr, 1.0f, 0}, st, l.dx);
    if (rc) return rc;
    rc = launch_gemm<OpT>(make_operand(x, 1, dx), make_operand(da, 1, k), dx, k, br, EpiStore{grad_wg, k, nullptr, 1.0f, 0},
                          st, l.dwg);
    if (rc) return rc;
    rc = launch_gemm<OpT>(make_operand(dc, k, 1), make_operand(wh, k, 1), b, dy, k, EpiStore{grad_y, dy, nullptr, 1.0f, 0},
                          st, l.dy);
    if (rc) return rc;
    return launch_gemm<OpT>(make_operand(y, 1, dy), make_operand(dc, 1, k), dy, k, b,
                            EpiStore{grad_wh, k, nullptr, 1.0f, 0}, st, l.dwh);
  });
}

static int check_separable(const char* fn, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int64_t k,
                           int precision) {
  int rc = check_common(fn, br, b, row_offset, dx, dy, precision);
  if (rc) return rc;
  MI_CHECK_ARG(k >= 1, "%s: projection width must be >= 1", fn);
  // bf16x3 and fp8 exist for the bilinear critic only: the kernels below would run them as single-pass bf16
  MI_CHECK_ARG(precision == MI_PREC_F32 || precision == MI_PREC_BF16,
               "%s: precision %d is not available for the separable critic (f32, bf16)", fn, precision);
  return MI_OK;
}

}  // namespace mi

extern "C" {

size_t mi_separable_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                    int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_separable(ws, b_rows, b, d_img, d_txt, d_proj, precision).bytes + 256;
}

int mi_separable_fwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                     const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                     int64_t d_txt, int64_t d_proj, int estimator, int precision, int need_grad, float* loss_out,
                     mi_stats* stats, float* partials_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && stats && workspace, "mi_separable_fwd: null pointer");
  int rc = check_separable("mi_separable_fwd", b_rows, b, row_offset, d_img, d_txt, d_proj, precision);
  if (rc) return rc;
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_separable_fwd: unknown estimator %d", estimator);
  Workspace ws(workspace, workspace_bytes);
  const SeparablePlan p = plan_separable(ws, b_rows, b, d_img, d_txt, d_proj, precision);
  rc = ws_fits(ws, "mi_separable_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p.path != MI_PATH_GENERIC) {
    rc = separable_prep_project(x, y, wg, wh, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, d_proj, p, st);
    if (rc) return rc;
    rc = p.stage.launch(sid_rows, sid_cols, row_offset, need_grad != 0, st);
    if (rc) return rc;
    return launch_finalize(p.stage.rec[0], p.stage.fl.n_rec[0], b, estimator, loss_out, stats, partials_out, st);
  }
  // generic: projections on the strided-operand kernels (exact fp32 products in the parity mode), then the S = A C^T
  // score + LSE kernel of the bilinear path's generic form
  const bool bf = precision != MI_PREC_F32;
  rc = separable_project(kSepFwd, bf, x, y, wg, wh, b_rows, b, d_img, d_txt, d_proj, p.a32, p.c32, st);
  if (rc) return rc;
  rc = with_operand_type(bf, [&](auto* op) {
    return launch_gemm<OperandOf<decltype(op)>>(
        make_operand((const float*)p.a32, d_proj, 1), make_operand((const float*)p.c32, d_proj, 1), b_rows, b, d_proj,
        EpiScoreLse{sid_rows, sid_cols, row_offset, nullptr, p.partials}, st, "separable score+LSE (generic)");
  });
  if (rc) return rc;
  return launch_finalize(p.partials, p.n_partials, b, estimator, loss_out, stats, partials_out, st);
}

int mi_separable_bwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                     const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                     int64_t d_txt, int64_t d_proj, int precision, const mi_stats* stats, const float* grad_out,
                     float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                     size_t workspace_bytes, int workspace_from_forward, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && stats && grad_x && grad_y && grad_wg && grad_wh && workspace,
               "mi_separable_bwd: null pointer");
  int rc = check_separable("mi_separable_bwd", b_rows, b, row_offset, d_img, d_txt, d_proj, precision);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const SeparablePlan p = plan_separable(ws, b_rows, b, d_img, d_txt, d_proj, precision);
  rc = ws_fits(ws, "mi_separable_bwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t br = b_rows, k = d_proj;
  if (p.path != MI_PATH_GENERIC) {
    if (!workspace_from_forward) {
      rc = separable_prep_project(x, y, wg, wh, sid_rows, sid_cols, br, b, row_offset, d_img, d_txt, k, p, st);
      if (rc) return rc;
      rc = p.stage.launch(sid_rows, sid_cols, row_offset, true, st);
      if (rc) return rc;
    }
    FlashReduceArgs ra{};
    p.stage.reduce_jobs(ra.j, row_offset, ReduceOut{nullptr, p.dab, p.datb}, ReduceOut{nullptr, p.dcb, p.dctb});
    ra.stats = stats;
    ra.grad_out = grad_out;
    rc = launch_flash_reduce(ra, 2, k, p.stage.fl.slab_f16, st, "separable dA, dC from the fused sums");
    if (rc) return rc;
    // per modality: dW[a, c] = sum_i X[i, a] dA[i, c] (split over i into slabs) | dX[i, a] = sum_c dA[i, c] W[a, c]
    const char* const wg_what = "separable dWg = X^T dA | dX = dA Wg^T";
    const char* const wh_what = "separable dWh = Y^T dC | dY = dC Wh^T";
    rc = launch_dw_dx(DwDxPair{p.xtb, p.datb, p.dab, p.gb, br, d_img, k, 1, p.wg_slab, p.wg_splits, p.wg_kchunk}, grad_x,
                      grad_wg, st, {wg_what, wg_what, wg_what});
    if (rc) return rc;
    return launch_dw_dx(DwDxPair{p.ytb, p.dctb, p.dcb, p.hb, b, d_txt, k, 1, p.wh_slab, p.wh_splits, p.wh_kchunk}, grad_y,
                        grad_wh, st, {wh_what, wh_what, wh_what});
  }
  // generic path: recompute the projections (cheap), G from recomputed scores, dA = G C and dC = G^T A, back-projections
  const bool bf = precision != MI_PREC_F32;
  rc = separable_project(kSepBwd, bf, x, y, wg, wh, br, b, d_img, d_txt, k, p.a32, p.c32, st);
  if (rc) return rc;
  rc = with_operand_type(bf, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;  // G is stored in the operand type
    const float *a = p.a32, *c = p.c32;
    OpT* g = (OpT*)p.g;
    const EpiGradScore<OpT> eg{sid_rows, sid_cols, row_offset, stats, grad_out, g};
    int r = launch_gemm<OpT>(make_operand(a, k, 1), make_operand(c, k, 1), br, b, k, eg, st, "separable G (generic)");
    if (r) return r;
    r = launch_gemm<OpT>(make_operand((const OpT*)g, b, 1), make_operand(c, 1, k), br, k, b,
                         EpiStore{p.da32, k, nullptr, 1.0f, 0}, st, "separable dA = G C (generic)");
    if (r) return r;
    return launch_gemm<OpT>(make_operand((const OpT*)g, 1, b), make_operand(a, 1, k), b, k, br,
                            EpiStore{p.dc32, k, nullptr, 1.0f, 0}, st, "separable dC = G^T A (generic)");
  });
  if (rc) return rc;
  return separable_project_back(kSepBwd, bf, x, y, wg, wh, br, b, d_img, d_txt, k, p.da32, p.dc32, grad_x, grad_y,
                                grad_wg, grad_wh, st);
}

}  // extern "C"

/* One separable-critic step in ONE call (single GPU): prep + projections (one launch), the fused B x B kernel, then the two-launch tail
 * of the bilinear critic generalised to two products -- [records -> statistics and loss; partial sums -> dA, dC rows; dX =
 * dA Wg^T, dY = dC Wh^T on the matrix cores; dA^T, dC^T fragment-major] and [dWg = X^T dA | dWh = Y^T dC] -- four launches
 * (round 3: eight, with a finalize, a slab-reduce and two split-K reduce launches).  Shapes outside the fused kernels: the
 * forward and the backward entry points, one after the other. */
extern "C" int mi_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                                 int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int estimator, int precision,
                                 const float* grad_out, float* loss_out, mi_stats* stats, float* partials_out, float* grad_x,
                                 float* grad_y, float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  using namespace mi;
  MI_CHECK_ARG(x && y && wg && wh && sid && stats && grad_x && grad_y && grad_wg && grad_wh && workspace,
               "mi_separable_step: null pointer");
  int rc = check_separable("mi_separable_step", b, b, 0, d_img, d_txt, d_proj, precision);
  if (rc) return rc;
  MI_CHECK_ARG(estimator == MI_DV || estimator == MI_INFONCE, "mi_separable_step: unknown estimator %d", estimator);
  Workspace ws(workspace, workspace_bytes);
  const SeparablePlan p = plan_separable(ws, b, b, d_img, d_txt, d_proj, precision);
  rc = ws_fits(ws, "mi_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p.path == MI_PATH_FUSED_TAIL) {
    rc = separable_prep_project_fused(x, y, wg, wh, sid, sid, b, b, 0, d_img, d_txt, d_proj, p, st);
    if (rc == MI_EINVAL) rc = separable_prep_project(x, y, wg, wh, sid, sid, b, b, 0, d_img, d_txt, d_proj, p, st);
    if (rc) return rc;
    rc = p.stage.launch(sid, sid, 0, true, st);
    if (rc) return rc;
    const TailMerge m{estimator, loss_out, stats, partials_out};
    const TailSide g{p.gfb, d_img, grad_x, p.datfb, p.xtfb, grad_wg}, h{p.hfb, d_txt, grad_y, p.dctfb, p.ytfb, grad_wh};
    return bilinear_tail(p.stage, 0, stats, grad_out, g, &h, nullptr, &m, st);
  }
  rc = mi_separable_fwd(x, y, wg, wh, sid, sid, b, b, 0, d_img, d_txt, d_proj, estimator, precision, 1, loss_out, stats,
                        partials_out, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return mi_separable_bwd(x, y, wg, wh, sid, sid, b, b, 0, d_img, d_txt, d_proj, precision, stats, grad_out, grad_x, grad_y,
                          grad_wg, grad_wh, workspace, workspace_bytes, 1, stream);
}

extern "C" int mi_separable_path(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return MI_EINVAL;
  mi::Workspace ws(nullptr, 0);
  return mi::plan_separable(ws, b_rows, b, d_img, d_txt, d_proj, precision).path;
}

#ifdef MI_STAMPS
// diagnostic build only: where the stamped kernels of this translation unit write their s_memtime values
extern "C" int mi_debug_set_stamps(void* buf) {
  mi::g_stamp_buf = (unsigned long long*)buf;
  return 0;
}
// ... and their wall-clock stamps (mi_common.h, WallScope): 4 launches x kWallMaxWg workgroups x 2 x 2 words; null: off
extern "C" int mi_debug_set_wall(void* buf) {
  unsigned long long* p = (unsigned long long*)buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(mi::g_wall), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

// ================================================================================================ the G-materialising chain
// (mi_nce.h, mi_fdiv.h; DESIGN.md sections 8 and 9.)  The per-sample InfoNCE and the JSD / NWJ bounds on the bilinear
// critic, one row block [br] x [b] at a time (the whole batch: br == b, row_offset == 0, sid_rows == sid_cols):
//   16-bit chain (bf16 / bf16x3, batch sizes and widths multiples of 8):
//     prep + T = X W -> score GEMM with the estimator's statistics epilogue
//     [grads] G GEMM (recomputed scores -> G, G^T) -> dT = G Y | dY = G^T T -> dW = X^T dT | dX = dT W^T
//   generic kernels (MI_PREC_F32, other shapes): the same sequence on mi_gemm.h, G in fp32 (bf16 in the bf16 mode)
// Between the two halves each entry point runs its estimator's finish: nce_finish (row / column statistics, loss),
// nce_rank_part (a row block's part for the cross-rank merge) or launch_fdiv_finalize.  The fused B x B kernel is not
// used: per-row normalisation needs r_i before any row's P tile can be weighted, and the fdiv bounds keep one record per
// 64 x 64 score tile.  The separable critic runs the chain on its projections A = X Wg, C = Y Wh with W = I.
// The retrieval ranks (mi_rank.h) run the forward half alone, with the diagonal S[i, i] computed
// between prep / T and the score GEMM, whose epilogue counts the scores above it.
namespace mi {

// Est: what an estimator puts into the chain -- the statistics epilogue of the score GEMM and the gradient epilogue of
// the G GEMM (generic kernels' and 16-bit chain's forms), its mode check and its launch labels
struct NceEst {
  using StatsOut = NceStatsOut;
  using GradIn = NceGradIn;
  using Stats = EpiNceStats<false>;
  using Stats16 = EpiNceStats<true>;
  template <typename TG>
  using Grad = EpiNceGrad<TG>;
  using Grad16 = EpiNceGrad2;
  static int check_mode(const char* fn, int mode) {
    MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "%s: unknown mode %d", fn, mode);
    return MI_OK;
  }
  static constexpr const char* kName = "the per-sample InfoNCE";
  static constexpr const char* kT = "nce T = X W (generic)";
  static constexpr const char* kScores = "nce score + row / column records (generic)";
  static constexpr const char* kScores16 = "nce score + row / column records";
  static constexpr const char* kG = "nce G (generic)";
  static constexpr const char* kG16 = "nce G";
  static constexpr SepLabels kSep = {"nce separable A = X Wg",      "nce separable C = Y Wh",
                                     "nce separable dX = dA Wg^T",  "nce separable dWg = X^T dA",
                                     "nce separable dY = dC Wh^T",  "nce separable dWh = Y^T dC"};
};

struct FdivEst {
  using StatsOut = FdivStatsOut;
  using GradIn = FdivGradIn;
  using Stats = EpiFdivStats;
  using Stats16 = EpiFdivStats;
  template <typename TG>
  using Grad = EpiFdivGrad<TG>;
  using Grad16 = EpiFdivGrad2;
  static int check_mode(const char* fn, int mode) { return fdiv_check_mode(fn, mode); }
  static constexpr const char* kName = "the JSD / NWJ bounds on this critic";
  static constexpr const char* kT = "fdiv T = X W (generic)";
  static constexpr const char* kScores = "fdiv score + records (generic)";
  static constexpr const char* kScores16 = "fdiv score + records";
  static constexpr const char* kG = "fdiv G (generic)";
  static constexpr const char* kG16 = "fdiv G";
  static constexpr SepLabels kSep = {"fdiv separable A = X Wg",     "fdiv separable C = Y Wh",
                                     "fdiv separable dX = dA Wg^T", "fdiv separable dWg = X^T dA",
                                     "fdiv separable dY = dC Wh^T", "fdiv separable dWh = Y^T dC"};
};

// Retrieval ranks (mi_rank.h) are not an estimator, but they run the forward half of the chain:
// the score GEMM's epilogue counts instead of reducing.  No mode, no gradient half.
struct RankEst {
  using StatsOut = RankOut;
  using Stats = EpiRankCounts;
  using Stats16 = EpiRankCounts;
  static int check_mode(const char*, int) { return MI_OK; }
  static constexpr const char* kName = "the retrieval ranks";
  static constexpr const char* kT = "rank T = X W (generic)";
  static constexpr const char* kScores = "rank score + counts (generic)";
  static constexpr const char* kScores16 = "rank score + counts";
  static constexpr SepLabels kSep = {"rank separable A = X Wg", "rank separable C = Y Wh"};
};

// Top-k retrieval (mi_topk.h): the forward half again, the score GEMM's epilogue inserts into the
// queries' key lists.  Rectangular (n_img x n_txt), no ids in prep / T, no mode, no gradient half.
struct TopkEst {
  using StatsOut = TopkOut;
  using Stats = EpiTopkInsert;
  using Stats16 = EpiTopkInsert;
  static int check_mode(const char*, int) { return MI_OK; }
  static constexpr const char* kName = "the top-k retrieval";
  static constexpr const char* kT = "topk T = X W (generic)";
  static constexpr const char* kScores = "topk score + inserts (generic)";
  static constexpr const char* kScores16 = "topk score + inserts";
  static constexpr SepLabels kSep = {"topk separable A = X Wg", "topk separable C = Y Wh"};
};

// MI estimates (mi_estimates.h): the forward half once more, the score GEMM's epilogue writes one
// record per tile and the per-sample InfoNCE's row / column records.  No mode, no gradient half.
struct EstimatesEst {
  using StatsOut = EstStatsOut;
  using Stats = EpiEstStats<false>;
  using Stats16 = EpiEstStats<true>;
  static int check_mode(const char*, int) { return MI_OK; }
  static constexpr const char* kName = "the MI estimates";
  static constexpr const char* kT = "estimates T = X W (generic)";
  static constexpr const char* kScores = "estimates score + records (generic)";
  static constexpr const char* kScores16 = "estimates score + records";
  static constexpr SepLabels kSep = {"estimates separable A = X Wg", "estimates separable C = Y Wh"};
};

static bool chain_16bit_ok(int64_t br, int64_t b, int64_t dx, int64_t dy, int precision) {
  return (precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3) && br % 8 == 0 && b % 8 == 0 && dx % 8 == 0 &&
         dy % 8 == 0;
}

// sizes, the estimator's mode, the precision, then the row block [row_offset, row_offset + br) of [0, b)
template <typename Est>
static int chain_check(const char* fn, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int mode,
                       int precision) {
  MI_CHECK_ARG(b >= 1 && dx >= 1 && dy >= 1, "%s: sizes must be >= 1 (b %lld, widths %lld, %lld)", fn, (long long)b,
               (long long)dx, (long long)dy);
  const int rc = Est::check_mode(fn, mode);
  if (rc) return rc;
  MI_CHECK_ARG(precision == MI_PREC_F32 || precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3,
               "%s: precision %d is not available for %s (f32, bf16, bf16x3)", fn, precision, Est::kName);
  MI_CHECK_ARG(br >= 1 && br <= b, "%s: need 1 <= b_rows <= b (got %lld, %lld)", fn, (long long)br, (long long)b);
  MI_CHECK_ARG(row_offset >= 0 && row_offset + br <= b, "%s: row block [%lld, %lld) outside [0, %lld)", fn,
               (long long)row_offset, (long long)(row_offset + br), (long long)b);
  return MI_OK;
}

// The forward half, first part: prep / T = X W (w == nullptr: S = X Y^T), which leaves the score GEMM's operands in the
// workspace (16-bit chain: p.tb, p.yb) or in p.t (generic kernels with a weight)
template <typename Est>
static int chain_operands(const float* x, const float* y, const float* w, const int64_t* sid_rows, const int64_t* sid_cols,
                          int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int precision,
                          const BilinearPlan& p, hipStream_t st) {
  if (chain_16bit_ok(br, b, dx, dy, precision)) {
    if (w) return fast_prep_and_t(x, y, w, sid_rows, sid_cols, br, b, row_offset, dx, dy, p, st);  // (no fused stage in this plan)
    // X takes the place of T (A operand of the scores, B operand of dY = G^T T)
    const int ra = p.x3 == 3 ? 1 : 0, rb = p.x3 == 3 ? 2 : 0;
    CvtJobs jobs{};
    jobs.j[0] = CvtJob{x, br, dx, p.tb, p.ttb, 0, 0, nullptr, ra, rb};
    jobs.j[1] = CvtJob{y, b, dy, p.yb, p.ytb, 0, 0, nullptr, rb, rb};
    return launch_cvt_transpose3(jobs, st, "nce prep X Y");
  }
  if (!w) return MI_OK;
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    return generic_gemm_store<OpT>(make_operand(x, dx, 1), make_operand(w, 1, dy), br, dy, dx, p.t, dy, p, st, Est::kT);
  });
}

// ... second part: the score GEMM of the row block on those operands with Est's statistics epilogue writing to `so`
template <typename Est>
static int chain_sweep(const float* x, const float* y, const float* w, int64_t br, int64_t b, int64_t dx, int64_t dy,
                       int precision, const typename Est::StatsOut& so, const BilinearPlan& p, hipStream_t st) {
  if (chain_16bit_ok(br, b, dx, dy, precision)) {
    const int x3 = p.x3;
    return launch_gemm_bf16(one_problem(p.tb, x3 * dy, p.yb, x3 * dy, br, b, x3 * dy), 1, typename Est::Stats16{so}, st,
                            Est::kScores16);
  }
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    return launch_gemm<OpT>(make_operand(w ? p.t : x, dy, 1), make_operand(y, dy, 1), br, b, dy, typename Est::Stats{so},
                            st, Est::kScores);
  });
}

template <typename Est>
static int chain_scores(const float* x, const float* y, const float* w, const int64_t* sid_rows, const int64_t* sid_cols,
                        int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int precision,
                        const typename Est::StatsOut& so, const BilinearPlan& p, hipStream_t st) {
  const int rc = chain_operands<Est>(x, y, w, sid_rows, sid_cols, br, b, row_offset, dx, dy, precision, p, st);
  if (rc) return rc;
  return chain_sweep<Est>(x, y, w, br, b, dx, dy, precision, so, p, st);
}

// The gradient half: the G GEMM of the row block with Est's gradient epilogue (recomputed scores; T is chain_scores' in
// the same workspace), then dT = G Y | dY = G^T T and dW | dX.  w == nullptr: dT is grad_x and there is no grad_w.
template <typename Est>
static int chain_grads(const float* x, const float* y, const float* w, int64_t br, int64_t b, int64_t dx, int64_t dy,
                       int precision, const typename Est::GradIn& gi, float* grad_x, float* grad_y, float* grad_w,
                       const BilinearPlan& p, hipStream_t st) {
  if (chain_16bit_ok(br, b, dx, dy, precision)) {
    const int x3 = p.x3;
    const int rc = launch_gemm_bf16(one_problem(p.tb, x3 * dy, p.yb, x3 * dy, br, b, x3 * dy), 1,
                                    typename Est::Grad16{gi, p.gb, p.gtb, x3 == 3 ? 1 : 0}, st, Est::kG16);
    if (rc) return rc;
    return bilinear_bwd_from_g(br, b, dx, dy, grad_x, grad_y, grad_w, w != nullptr, p, st);
  }
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;  // G is stored in the operand type
    const float* t = w ? p.t : x;
    OpT* g = (OpT*)p.g;
    const int rc = launch_gemm<OpT>(make_operand(t, dy, 1), make_operand(y, dy, 1), br, b, dy,
                                    typename Est::template Grad<OpT>{gi, g}, st, Est::kG);
    if (rc) return rc;
    return generic_bwd_from_g<OpT, OpT>(x, y, w, t, g, br, b, dx, dy, grad_x, grad_y, grad_w, p, st);
  });
}

// The separable entry points' workspace: A, C, dA, dC, then the plan of the chain on (A, C)
template <typename Inner>
struct SeparableChainPlan {
  float *a, *c, *da, *dc;
  Inner n;
  size_t bytes;
};
template <typename PlanInner>
static auto plan_separable_chain(Workspace& ws, int64_t br, int64_t b, int64_t k, PlanInner plan_inner) {
  SeparableChainPlan<decltype(plan_inner())> s{};
  s.a = ws.take<float>(br * k);
  s.c = ws.take<float>(b * k);
  s.da = ws.take<float>(br * k);
  s.dc = ws.take<float>(b * k);
  s.n = plan_inner();
  s.bytes = ws.off;
  return s;
}

struct NceBilinearPlan {
  BilinearPlan p;
  NcePlan q;
  size_t bytes;
};
static NceBilinearPlan plan_nce_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision) {
  NceBilinearPlan n{};
  n.p = plan_bilinear(ws, b, b, dx, dy, precision, true, true);
  n.q = plan_nce(ws, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<NceBilinearPlan> plan_nce_separable(Workspace& ws, int64_t b, int64_t k, int precision) {
  return plan_separable_chain(ws, b, b, k, [&] { return plan_nce_bilinear(ws, b, k, k, precision); });
}

// A rank's row block [br] x [b]: the forward leaves T / the operand copies, the records and r in
// its workspace and writes the rank's part; the caller gathers the parts, mi_nce_merge_parts gives c and the loss; the
// backward reads r and the operands from the same workspace and the merged c from the caller.  br == b, row_offset == 0
// issues exactly the launches (and bits) of the whole-batch step plus the two small part / merge kernels.
struct NceShardBilinearPlan {
  BilinearPlan p;
  NceShardPlan q;
  size_t bytes;
};
static NceShardBilinearPlan plan_nce_shard_bilinear(Workspace& ws, int64_t br, int64_t b, int64_t dx, int64_t dy,
                                                    int precision) {
  NceShardBilinearPlan n{};
  n.p = plan_bilinear(ws, br, b, dx, dy, precision, true, true);
  n.q = plan_nce_shard(ws, br, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<NceShardBilinearPlan> plan_nce_shard_separable(Workspace& ws, int64_t br, int64_t b, int64_t k,
                                                                         int precision) {
  return plan_separable_chain(ws, br, b, k, [&] { return plan_nce_shard_bilinear(ws, br, b, k, k, precision); });
}

struct FdivBilinearPlan {
  BilinearPlan p;
  FdivRec* rec;  // [n_t][n_t]
  mi_stats* stats;
  int64_t n_t;
  size_t bytes;
};
static FdivBilinearPlan plan_fdiv_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision) {
  FdivBilinearPlan n{};
  n.p = plan_bilinear(ws, b, b, dx, dy, precision, true, true);
  n.n_t = (b + 63) / 64;
  n.rec = ws.take<FdivRec>(n.n_t * n.n_t);
  n.stats = ws.take<mi_stats>(1);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<FdivBilinearPlan> plan_fdiv_separable(Workspace& ws, int64_t b, int64_t k, int precision) {
  return plan_separable_chain(ws, b, b, k, [&] { return plan_fdiv_bilinear(ws, b, k, k, precision); });
}

// Retrieval ranks: the forward half's buffers only -- the operand copies and T of the 16-bit chain, or T and the split-K
// slabs of the generic kernels -- and the diagonal.  No G, no G^T, no tile records: linear in b.
struct RankBilinearPlan {
  BilinearPlan p;
  float* diag;  // [b]
  size_t bytes;
};
static RankBilinearPlan plan_rank_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision) {
  RankBilinearPlan n{};
  BilinearPlan& p = n.p;
  const int64_t x3 = precision == MI_PREC_BF16X3 ? 3 : 1;
  p.x3 = (int)x3;
  if (chain_16bit_ok(b, b, dx, dy, precision)) {
    p.xb = ws.take<bf16_t>(x3 * b * dx);
    p.xtb = ws.take<bf16_t>(x3 * b * dx);
    p.yb = ws.take<bf16_t>(x3 * b * dy);
    p.ytb = ws.take<bf16_t>(x3 * b * dy);
    p.wb = ws.take<bf16_t>(x3 * dx * dy);
    p.wtb = ws.take<bf16_t>(x3 * dx * dy);
    p.tb = ws.take<bf16_t>(x3 * b * dy);
    p.ttb = ws.take<bf16_t>(x3 * b * dy);
    p.path = MI_PATH_GEMMS;
  } else {
    p.t = ws.take<float>(b * dy);
    p.gen_slab_floats = precision == MI_PREC_F32 ? generic_slab_floats(b, dy, dx) : 0;  // T = X W
    p.gen_slab = p.gen_slab_floats > 0 ? ws.take<float>(p.gen_slab_floats) : nullptr;
    p.path = MI_PATH_GENERIC;
  }
  n.diag = ws.take<float>(b);
  p.bytes = n.bytes = ws.off;
  return n;
}

struct RankSeparablePlan {
  float *a, *c;  // the projections A = X Wg, C = Y Wh [b][k]
  RankBilinearPlan n;
  size_t bytes;
};
static RankSeparablePlan plan_rank_separable(Workspace& ws, int64_t b, int64_t k, int precision) {
  RankSeparablePlan s{};
  s.a = ws.take<float>(b * k);
  s.c = ws.take<float>(b * k);
  s.n = plan_rank_bilinear(ws, b, k, k, precision);
  s.bytes = ws.off;
  return s;
}

// prep / T, the diagonal from the sweep's operands (which zeroes the ranks), the sweep with the counting epilogue
static int rank_chain(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t dx,
                      int64_t dy, int precision, int* rank_i2t, int* rank_t2i, float* diag_out, const RankBilinearPlan& n,
                      hipStream_t st) {
  const BilinearPlan& p = n.p;
  const RankOut o = rank_out(sid, n.diag, rank_i2t, rank_t2i);
  int rc = chain_operands<RankEst>(x, y, w, sid, sid, b, b, 0, dx, dy, precision, p, st);
  if (rc) return rc;
  if (chain_16bit_ok(b, b, dx, dy, precision)) {
    rc = rank_diag_bf16(p.tb, p.yb, b, p.x3 * dy, o, diag_out, st);
  } else {
    rc = with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
      return rank_diag<OperandOf<decltype(op)>>(w ? p.t : x, y, b, dy, o, diag_out, st);
    });
  }
  if (rc) return rc;
  return chain_sweep<RankEst>(x, y, w, b, b, dx, dy, precision, o, p, st);
}

// ------------------------------------------------------------------------------------------------ MI estimates
// The forward half's buffers (plan_rank_bilinear) and the records: b^2 / 64 of them, no G, no G^T, no b x b floats
struct EstBilinearPlan {
  BilinearPlan p;
  EstPlan q;
  size_t bytes;
};
static EstBilinearPlan plan_est_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision) {
  EstBilinearPlan n{};
  n.p = plan_rank_bilinear(ws, b, dx, dy, precision).p;
  n.q = plan_est(ws, b);
  n.bytes = ws.off;
  return n;
}
struct EstSeparablePlan {
  float *a, *c;  // the projections A = X Wg, C = Y Wh [b][k]
  EstBilinearPlan n;
  size_t bytes;
};
static EstSeparablePlan plan_est_separable(Workspace& ws, int64_t b, int64_t k, int precision) {
  EstSeparablePlan s{};
  s.a = ws.take<float>(b * k);
  s.c = ws.take<float>(b * k);
  s.n = plan_est_bilinear(ws, b, k, k, precision);
  s.bytes = ws.off;
  return s;
}

// prep / T, the sweep with the statistics epilogue, merge and finalize
static int est_chain(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t dx, int64_t dy,
                     int precision, const EstTaus& taus, float* est_out, const EstBilinearPlan& n, hipStream_t st) {
  const int rc = chain_scores<EstimatesEst>(x, y, w, sid, sid, b, b, 0, dx, dy, precision, est_stats_out(n.q, sid, taus),
                                            n.p, st);
  if (rc) return rc;
  return est_finish(n.q, sid, b, taus, est_out, st);
}

// the arguments every estimates entry point shares: the batch size and the clips (read from the host array)
static int est_check(const char* fn, int64_t b, const float* taus_host, int n_tau, EstTaus& taus) {
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "%s: need 1 <= b < 2^31 (got %lld)", fn, (long long)b);
  return est_read_taus(fn, taus_host, n_tau, taus);
}

// ------------------------------------------------------------------------------------------------ top-k retrieval
// sizes and precision of a rectangular gallery call (chain_check ties b_rows to b: not for a gallery)
static int topk_check(const char* fn, int64_t n_img, int64_t n_txt, int64_t dx, int64_t dy, int precision, int k) {
  MI_CHECK_ARG(n_img >= 1 && n_txt >= 1 && dx >= 1 && dy >= 1, "%s: sizes must be >= 1 (n_img %lld, n_txt %lld, widths %lld, %lld)",
               fn, (long long)n_img, (long long)n_txt, (long long)dx, (long long)dy);
  const int64_t lim = (int64_t)1 << 31;
  MI_CHECK_ARG(n_img < lim && n_txt < lim && dx < lim && dy < lim, "%s: sizes must be below 2^31", fn);
  MI_CHECK_ARG(k >= 1 && k <= kTopkMaxK, "%s: k must be in [1, %d] (got %d)", fn, kTopkMaxK, k);
  MI_CHECK_ARG(precision == MI_PREC_F32 || precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3,
               "%s: precision %d is not available for %s (f32, bf16, bf16x3)", fn, precision, TopkEst::kName);
  return MI_OK;
}

// The forward half's buffers of an [n_img] x [n_txt] problem -- the operand copies and T of the 16-bit chain, or T and
// the split-K slabs of the generic kernels -- and the key lists of both directions: O((n_img + n_txt) k) on top.
struct TopkBilinearPlan {
  BilinearPlan p;
  topk_key_t* keys_i2t;  // [n_img][k]
  topk_key_t* keys_t2i;  // [n_txt][k], directly behind keys_i2t
  size_t bytes;
};
static TopkBilinearPlan plan_topk_bilinear(Workspace& ws, int64_t n_img, int64_t n_txt, int64_t dx, int64_t dy,
                                           int precision, int k) {
  TopkBilinearPlan n{};
  BilinearPlan& p = n.p;
  const int64_t x3 = precision == MI_PREC_BF16X3 ? 3 : 1;
  p.x3 = (int)x3;
  if (chain_16bit_ok(n_img, n_txt, dx, dy, precision)) {
    p.xb = ws.take<bf16_t>(x3 * n_img * dx);
    p.xtb = ws.take<bf16_t>(x3 * n_img * dx);
    p.yb = ws.take<bf16_t>(x3 * n_txt * dy);
    p.ytb = ws.take<bf16_t>(x3 * n_txt * dy);
    p.wb = ws.take<bf16_t>(x3 * dx * dy);
    p.wtb = ws.take<bf16_t>(x3 * dx * dy);
    p.tb = ws.take<bf16_t>(x3 * n_img * dy);
    p.ttb = ws.take<bf16_t>(x3 * n_img * dy);
    p.path = MI_PATH_GEMMS;
  } else {
    p.t = ws.take<float>(n_img * dy);
    p.gen_slab_floats = precision == MI_PREC_F32 ? generic_slab_floats(n_img, dy, dx) : 0;  // T = X W
    p.gen_slab = p.gen_slab_floats > 0 ? ws.take<float>(p.gen_slab_floats) : nullptr;
    p.path = MI_PATH_GENERIC;
  }
  n.keys_i2t = ws.take<topk_key_t>((n_img + n_txt) * k);
  n.keys_t2i = n.keys_i2t ? n.keys_i2t + n_img * k : nullptr;
  p.bytes = n.bytes = ws.off;
  return n;
}

struct TopkSeparablePlan {
  float *a, *c;  // the projections A = X Wg [n_img][k_proj], C = Y Wh [n_txt][k_proj]
  TopkBilinearPlan n;
  size_t bytes;
};
static TopkSeparablePlan plan_topk_separable(Workspace& ws, int64_t n_img, int64_t n_txt, int64_t k_proj, int precision,
                                             int k) {
  TopkSeparablePlan s{};
  s.a = ws.take<float>(n_img * k_proj);
  s.c = ws.take<float>(n_txt * k_proj);
  s.n = plan_topk_bilinear(ws, n_img, n_txt, k_proj, k_proj, precision, k);
  s.bytes = ws.off;
  return s;
}

struct TopkDirs {
  int32_t* idx_i2t;
  float* val_i2t;
  int32_t* idx_t2i;
  float* val_t2i;
};

// One direction's sweep.  The lane-owned side of the accumulator tile (its columns, the GEMM's B operand) is the query
// side: image -> report puts T (or X) there and streams Y as the A operand, report -> image the other way round.  Both
// read the same T from the workspace.
static int topk_sweep(bool i2t, const float* x, const float* y, const float* w, const int64_t* sid_img,
                      const int64_t* sid_txt, int64_t n_img, int64_t n_txt, int64_t dx, int64_t dy, int precision, int k,
                      const TopkBilinearPlan& n, hipStream_t st) {
  const BilinearPlan& p = n.p;
  const TopkOut o = i2t ? TopkOut{sid_img, sid_txt, n.keys_i2t, k} : TopkOut{sid_txt, sid_img, n.keys_t2i, k};
  if (chain_16bit_ok(n_img, n_txt, dx, dy, precision)) {
    const int64_t kk = p.x3 * dy;
    const GemmBf16Args g = i2t ? one_problem(p.yb, kk, p.tb, kk, n_txt, n_img, kk) : one_problem(p.tb, kk, p.yb, kk, n_img, n_txt, kk);
    return launch_gemm_bf16(g, 1, EpiTopkInsert{o}, st, TopkEst::kScores16);
  }
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    const auto img = make_operand(w ? (const float*)p.t : x, dy, 1), txt = make_operand(y, dy, 1);
    if (i2t) return launch_gemm<OpT>(txt, img, n_txt, n_img, dy, EpiTopkInsert{o}, st, TopkEst::kScores);
    return launch_gemm<OpT>(img, txt, n_img, n_txt, dy, EpiTopkInsert{o}, st, TopkEst::kScores);
  });
}

// prep / T without ids or a row offset (this plan has no fused stage, so no equal-id tile flags are written), the lists
// emptied, one sweep and one finish per direction asked for
static int topk_chain(const float* x, const float* y, const float* w, const int64_t* sid_img, const int64_t* sid_txt,
                      int64_t n_img, int64_t n_txt, int64_t dx, int64_t dy, int precision, int k, const TopkDirs& d,
                      const TopkBilinearPlan& n, hipStream_t st) {
  int rc = chain_operands<TopkEst>(x, y, w, nullptr, nullptr, n_img, n_txt, 0, dx, dy, precision, n.p, st);
  if (rc) return rc;
  const bool i2t = d.idx_i2t != nullptr, t2i = d.idx_t2i != nullptr;
  rc = topk_zero(i2t ? n.keys_i2t : n.keys_t2i, ((i2t ? n_img : 0) + (t2i ? n_txt : 0)) * k, st);
  if (rc) return rc;
  if (i2t) {
    rc = topk_sweep(true, x, y, w, sid_img, sid_txt, n_img, n_txt, dx, dy, precision, k, n, st);
    if (rc) return rc;
    rc = topk_finish(n.keys_i2t, n_img, k, d.idx_i2t, d.val_i2t, st);
    if (rc) return rc;
  }
  if (t2i) {
    rc = topk_sweep(false, x, y, w, sid_img, sid_txt, n_img, n_txt, dx, dy, precision, k, n, st);
    if (rc) return rc;
    rc = topk_finish(n.keys_t2i, n_txt, k, d.idx_t2i, d.val_t2i, st);
  }
  return rc;
}

// the pointer rules shared by the two chain entry points
static int topk_check_dirs(const char* fn, const int64_t* sid_img, const int64_t* sid_txt, const TopkDirs& d) {
  MI_CHECK_ARG((sid_img == nullptr) == (sid_txt == nullptr), "%s: pass sid_img and sid_txt, or neither", fn);
  MI_CHECK_ARG((d.idx_i2t == nullptr) == (d.val_i2t == nullptr) && (d.idx_t2i == nullptr) == (d.val_t2i == nullptr),
               "%s: idx and val of a direction go together", fn);
  MI_CHECK_ARG(d.idx_i2t || d.idx_t2i, "%s: pass the i2t outputs, the t2i outputs or both", fn);
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ hard-negative InfoNCE
// (mi_hardnce.h)  The top-k selection of the square batch with ids on both sides, the loss on the
// lists, and the gradient half of the chain with an epilogue that keeps G on the lists and the diagonal:
//   prep + T = X W -> lists emptied -> sweep image -> report (its epilogue also writes S[i, i]) + finish
//   [symmetric] sweep report -> image + finish -> hardnce_rows_kernel + nce_loss_kernel
//   [grads] G GEMM -> dT = G Y | dY = G^T T -> dW = X^T dT | dX = dT W^T
struct HardNceEst {
  using GradIn = HardNceGradIn;
  template <typename TG>
  using Grad = EpiHardNceGrad<TG>;
  using Grad16 = EpiHardNceGrad2;
  static int check_mode(const char* fn, int mode) { return NceEst::check_mode(fn, mode); }
  static constexpr const char* kName = "the hard-negative InfoNCE";
  static constexpr const char* kT = "hardnce T = X W (generic)";
  static constexpr const char* kScores = "hardnce score + inserts (generic)";
  static constexpr const char* kScores16 = "hardnce score + inserts";
  static constexpr const char* kG = "hardnce G (generic)";
  static constexpr const char* kG16 = "hardnce G";
  static constexpr SepLabels kSep = {"hardnce separable A = X Wg",     "hardnce separable C = Y Wh",
                                     "hardnce separable dX = dA Wg^T", "hardnce separable dWg = X^T dA",
                                     "hardnce separable dY = dC Wh^T", "hardnce separable dWh = Y^T dC"};
};

static int hardnce_check(const char* fn, int64_t b, int64_t dx, int64_t dy, int mode, int precision, int k) {
  const int rc = chain_check<HardNceEst>(fn, b, b, 0, dx, dy, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(b < ((int64_t)1 << 31), "%s: b must be below 2^31", fn);
  MI_CHECK_ARG(k >= 1 && k <= kTopkMaxK, "%s: k must be in [1, %d] (got %d)", fn, kTopkMaxK, k);
  return MI_OK;
}

// grads: the nce step's plan (with G and G^T); forward only: the forward half's buffers alone, linear in b
struct HardNceBilinearPlan {
  BilinearPlan p;
  float* diag;  // [b]
  HardNceLists q;
  size_t bytes;
};
static HardNceBilinearPlan plan_hardnce_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision, int k,
                                                 bool grads) {
  HardNceBilinearPlan n{};
  if (grads) {
    n.p = plan_bilinear(ws, b, b, dx, dy, precision, true, true);
    n.diag = ws.take<float>(b);
  } else {
    const RankBilinearPlan f = plan_rank_bilinear(ws, b, dx, dy, precision);
    n.p = f.p;
    n.diag = f.diag;
  }
  n.q = plan_hardnce_lists(ws, b, k);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<HardNceBilinearPlan> plan_hardnce_separable(Workspace& ws, int64_t b, int64_t kp, int precision,
                                                                      int k, bool grads) {
  return plan_separable_chain(ws, b, b, kp, [&] { return plan_hardnce_bilinear(ws, b, kp, kp, precision, k, grads); });
}

// One direction's sweep on the square batch, operands as topk_sweep: the query side is the GEMM's B operand.
static int hardnce_sweep(bool i2t, const float* x, const float* y, const float* w, const int64_t* sid, int64_t b,
                         int64_t dx, int64_t dy, int precision, int k, const HardNceBilinearPlan& n, hipStream_t st) {
  const BilinearPlan& p = n.p;
  const EpiHardNceInsert e{TopkOut{sid, sid, i2t ? n.q.keys : n.q.keys + b * k, k}, i2t ? n.diag : nullptr};
  if (chain_16bit_ok(b, b, dx, dy, precision)) {
    const int64_t kk = p.x3 * dy;
    const GemmBf16Args g = i2t ? one_problem(p.yb, kk, p.tb, kk, b, b, kk) : one_problem(p.tb, kk, p.yb, kk, b, b, kk);
    return launch_gemm_bf16(g, 1, e, st, HardNceEst::kScores16);
  }
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    const auto img = make_operand(w ? (const float*)p.t : x, dy, 1), txt = make_operand(y, dy, 1);
    if (i2t) return launch_gemm<OpT>(txt, img, b, b, dy, e, st, HardNceEst::kScores);
    return launch_gemm<OpT>(img, txt, b, b, dy, e, st, HardNceEst::kScores);
  });
}

// The whole step on (x, y, w); idx_rows / idx_cols: the caller's copies of the lists or null (the workspace's are used)
static int hardnce_chain(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t dx,
                         int64_t dy, int mode, int precision, int k, const float* grad_out, float* loss_out,
                         float* lse_rows, float* lse_cols, int32_t* idx_rows, int32_t* idx_cols, float* grad_x,
                         float* grad_y, float* grad_w, bool any_grad, const HardNceBilinearPlan& n, hipStream_t st) {
  const bool sym = mode == MI_NCE_SYMMETRIC;
  const HardNceLists& q = n.q;
  int32_t* ir = idx_rows ? idx_rows : q.idx;
  int32_t* ic = idx_cols ? idx_cols : q.idx + b * k;
  int rc = chain_operands<HardNceEst>(x, y, w, nullptr, nullptr, b, b, 0, dx, dy, precision, n.p, st);
  if (rc) return rc;
  rc = topk_zero(q.keys, (sym ? 2 : 1) * b * k, st);
  if (rc) return rc;
  rc = hardnce_sweep(true, x, y, w, sid, b, dx, dy, precision, k, n, st);
  if (rc) return rc;
  rc = topk_finish(q.keys, b, k, ir, q.val, st);
  if (rc) return rc;
  if (sym) {
    rc = hardnce_sweep(false, x, y, w, sid, b, dx, dy, precision, k, n, st);
    if (rc) return rc;
    rc = topk_finish(q.keys + b * k, b, k, ic, q.val + b * k, st);
    if (rc) return rc;
  }
  rc = hardnce_finish(q.val, q.val + b * k, n.diag, 1, b, k, mode, q, loss_out, lse_rows, lse_cols, st);
  if (rc || !any_grad) return rc;
  return chain_grads<HardNceEst>(x, y, w, b, b, dx, dy, precision, hardnce_grad_in(ir, ic, k, q.r, q.c, grad_out, b, mode),
                                 grad_x, grad_y, grad_w, n.p, st);
}

// ------------------------------------------------------------------------------------------------ study-positive InfoNCE
// (mi_posnce.h)  The chain of the per-sample InfoNCE with the epilogues that take every same-study
// pair as a positive:
//   prep + T = X W -> score GEMM + records -> posnce_merge_kernel -> nce_loss_kernel
//   [grads] G GEMM -> dT = G Y | dY = G^T T -> dW = X^T dT | dX = dT W^T
// A rank's row block runs the same chain in three calls, as the per-sample InfoNCE's:
//   fwd: prep + T -> score GEMM + records -> posnce_rank_part_kernel (r, 1 / n kept; the part)
//   merge of the gathered parts: posnce_merge_parts_kernel -> nce_loss_kernel
//   bwd: G GEMM from r, 1 / n and the merged c -> dT | dY -> dW | dX
struct PosNceEst {
  using StatsOut = PosNceStatsOut;
  using GradIn = PosNceGradIn;
  using Stats = EpiPosNceStats<false>;
  using Stats16 = EpiPosNceStats<true>;
  template <typename TG>
  using Grad = EpiPosNceGrad<TG>;
  using Grad16 = EpiPosNceGrad2;
  static int check_mode(const char* fn, int mode) { return NceEst::check_mode(fn, mode); }
  static constexpr const char* kName = "the study-positive InfoNCE";
  static constexpr const char* kT = "posnce T = X W (generic)";
  static constexpr const char* kScores = "posnce score + records (generic)";
  static constexpr const char* kScores16 = "posnce score + records";
  static constexpr const char* kG = "posnce G (generic)";
  static constexpr const char* kG16 = "posnce G";
  static constexpr SepLabels kSep = {"posnce separable A = X Wg",     "posnce separable C = Y Wh",
                                     "posnce separable dX = dA Wg^T", "posnce separable dWg = X^T dA",
                                     "posnce separable dY = dC Wh^T", "posnce separable dWh = Y^T dC"};
};

static int posnce_check(const char* fn, int64_t b, int64_t dx, int64_t dy, int mode, int precision) {
  const int rc = chain_check<PosNceEst>(fn, b, b, 0, dx, dy, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(b < ((int64_t)1 << 31), "%s: b must be below 2^31", fn);
  return MI_OK;
}

// grads: the nce step's buffers (with G and G^T); forward only: the forward half's buffers alone, no G
struct PosNceBilinearPlan {
  BilinearPlan p;
  PosNcePlan q;
  size_t bytes;
};
static PosNceBilinearPlan plan_posnce_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision,
                                               bool grads) {
  PosNceBilinearPlan n{};
  n.p = grads ? plan_bilinear(ws, b, b, dx, dy, precision, true, true) : plan_rank_bilinear(ws, b, dx, dy, precision).p;
  n.q = plan_posnce(ws, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<PosNceBilinearPlan> plan_posnce_separable(Workspace& ws, int64_t b, int64_t k, int precision,
                                                                    bool grads) {
  return plan_separable_chain(ws, b, b, k, [&] { return plan_posnce_bilinear(ws, b, k, k, precision, grads); });
}

// The whole step on (x, y, w); w == nullptr: S = X Y^T, dT is grad_x and there is no grad_w
static int posnce_chain(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t dx,
                        int64_t dy, int mode, int precision, const float* grad_out, float* loss_out, float* lse_rows,
                        float* lse_cols, int32_t* n_pos_out, float* grad_x, float* grad_y, float* grad_w, bool any_grad,
                        const PosNceBilinearPlan& n, hipStream_t st) {
  int rc = chain_scores<PosNceEst>(x, y, w, nullptr, nullptr, b, b, 0, dx, dy, precision, posnce_stats_out(n.q, sid), n.p,
                                   st);
  if (rc) return rc;
  rc = posnce_finish(n.q, b, mode, loss_out, lse_rows, lse_cols, n_pos_out, st);
  if (rc || !any_grad) return rc;
  return chain_grads<PosNceEst>(x, y, w, b, b, dx, dy, precision,
                                posnce_grad_in(sid, n.q.r, n.q.c, n.q.inv_n, nullptr, grad_out, b, mode), grad_x, grad_y,
                                grad_w, n.p, st);
}

// A rank's row block: the nce shard plan's buffers with the study-positive records, r and 1 / n
struct PosNceShardBilinearPlan {
  BilinearPlan p;
  PosNceShardPlan q;
  size_t bytes;
};
static PosNceShardBilinearPlan plan_posnce_shard_bilinear(Workspace& ws, int64_t br, int64_t b, int64_t dx, int64_t dy,
                                                          int precision) {
  PosNceShardBilinearPlan n{};
  n.p = plan_bilinear(ws, br, b, dx, dy, precision, true, true);
  n.q = plan_posnce_shard(ws, br, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<PosNceShardBilinearPlan> plan_posnce_shard_separable(Workspace& ws, int64_t br, int64_t b,
                                                                               int64_t k, int precision) {
  return plan_separable_chain(ws, br, b, k, [&] { return plan_posnce_shard_bilinear(ws, br, b, k, k, precision); });
}

// counts travel in the parts as floats: exact below 2^24
static int posnce_shard_check(const char* fn, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int mode,
                              int precision) {
  const int rc = chain_check<PosNceEst>(fn, br, b, row_offset, dx, dy, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(b < ((int64_t)1 << 24), "%s: b must be below 2^24 on a sharded batch", fn);
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ soft-target InfoNCE
// (mi_softnce.h)  The chain of the per-sample InfoNCE with the epilogues that weigh every pair by
// the similarity of its finding sets:
//   softnce_label_norm_kernel -> prep + T = X W -> score GEMM + records -> softnce_merge_kernel -> nce_loss_kernel
//   [grads] G GEMM -> dT = G Y | dY = G^T T -> dW = X^T dT | dX = dT W^T
// A rank's row block runs the same chain in three calls, as the per-sample InfoNCE's:
//   fwd: softnce_label_norm_kernel on the masks of ALL b samples -> prep + T -> score GEMM + records
//        -> softnce_rank_part_kernel (r, z, 1 / z, rs kept; the part)
//   merge of the gathered parts: softnce_merge_parts_kernel -> nce_loss_kernel
//   bwd: G GEMM from r, 1 / z, rs and the merged c -> dT | dY -> dW | dX
struct SoftNceEst {
  using StatsOut = SoftNceStatsOut;
  using GradIn = SoftNceGradIn;
  using Stats = EpiSoftNceStats<false>;
  using Stats16 = EpiSoftNceStats<true>;
  template <typename TG>
  using Grad = EpiSoftNceGrad<TG>;
  using Grad16 = EpiSoftNceGrad2;
  static int check_mode(const char* fn, int mode) { return NceEst::check_mode(fn, mode); }
  static constexpr const char* kName = "the soft-target InfoNCE";
  static constexpr const char* kT = "softnce T = X W (generic)";
  static constexpr const char* kScores = "softnce score + records (generic)";
  static constexpr const char* kScores16 = "softnce score + records";
  static constexpr const char* kG = "softnce G (generic)";
  static constexpr const char* kG16 = "softnce G";
  static constexpr SepLabels kSep = {"softnce separable A = X Wg",     "softnce separable C = Y Wh",
                                     "softnce separable dX = dA Wg^T", "softnce separable dWg = X^T dA",
                                     "softnce separable dY = dC Wh^T", "softnce separable dWh = Y^T dC"};
};

// b, mode, tau and mix of every soft-target entry point (NaN fails both range tests)
static int softnce_check_targets(const char* fn, int64_t b, int mode, float tau, float mix) {
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "%s: b must be in [1, 2^31)", fn);
  const int rc = SoftNceEst::check_mode(fn, mode);
  if (rc) return rc;
  MI_CHECK_ARG(std::isfinite(tau) && tau > 0.0f, "%s: tau must be finite and > 0 (got %g)", fn, (double)tau);
  MI_CHECK_ARG(mix >= 0.0f && mix <= 1.0f, "%s: mix must be in [0, 1] (got %g)", fn, (double)mix);
  return MI_OK;
}

static int softnce_check(const char* fn, int64_t b, int64_t dx, int64_t dy, int mode, int precision, float tau, float mix) {
  const int rc = chain_check<SoftNceEst>(fn, b, b, 0, dx, dy, mode, precision);
  if (rc) return rc;
  return softnce_check_targets(fn, b, mode, tau, mix);
}

// grads: the nce step's buffers (with G and G^T); forward only: the forward half's buffers alone, no G
struct SoftNceBilinearPlan {
  BilinearPlan p;
  SoftNcePlan q;
  size_t bytes;
};
static SoftNceBilinearPlan plan_softnce_bilinear(Workspace& ws, int64_t b, int64_t dx, int64_t dy, int precision,
                                                 bool grads) {
  SoftNceBilinearPlan n{};
  n.p = grads ? plan_bilinear(ws, b, b, dx, dy, precision, true, true) : plan_rank_bilinear(ws, b, dx, dy, precision).p;
  n.q = plan_softnce(ws, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<SoftNceBilinearPlan> plan_softnce_separable(Workspace& ws, int64_t b, int64_t k, int precision,
                                                                      bool grads) {
  return plan_separable_chain(ws, b, b, k, [&] { return plan_softnce_bilinear(ws, b, k, k, precision, grads); });
}

// The whole step on (x, y, w); w == nullptr: S = X Y^T, dT is grad_x and there is no grad_w
static int softnce_chain(const float* x, const float* y, const float* w, const int64_t* lab, int64_t b, int64_t dx,
                         int64_t dy, int mode, int precision, float tau, float mix, const float* grad_out, float* loss_out,
                         float* lse_rows, float* lse_cols, float* target_norm, float* grad_x, float* grad_y, float* grad_w,
                         bool any_grad, const SoftNceBilinearPlan& n, hipStream_t st) {
  int rc = softnce_label_norm(lab, b, tau, chain_16bit_ok(b, b, dx, dy, precision), n.q, target_norm, st);
  if (rc) return rc;
  rc = chain_scores<SoftNceEst>(x, y, w, nullptr, nullptr, b, b, 0, dx, dy, precision,
                                softnce_stats_out(n.q, lab, tau, mix), n.p, st);
  if (rc) return rc;
  rc = softnce_finish(n.q, b, mode, loss_out, lse_rows, lse_cols, st);
  if (rc || !any_grad) return rc;
  return chain_grads<SoftNceEst>(x, y, w, b, b, dx, dy, precision,
                                 softnce_grad_in(lab, n.q.rs, n.q.inv_z, nullptr, n.q.r, n.q.c, grad_out, b, mode, tau, mix),
                                 grad_x, grad_y, grad_w, n.p, st);
}

// A rank's row block: the nce shard plan's buffers with the soft-target records, r and the label norms of all b samples
struct SoftNceShardBilinearPlan {
  BilinearPlan p;
  SoftNceShardPlan q;
  size_t bytes;
};
static SoftNceShardBilinearPlan plan_softnce_shard_bilinear(Workspace& ws, int64_t br, int64_t b, int64_t dx, int64_t dy,
                                                            int precision) {
  SoftNceShardBilinearPlan n{};
  n.p = plan_bilinear(ws, br, b, dx, dy, precision, true, true);
  n.q = plan_softnce_shard(ws, br, b);
  n.bytes = ws.off;
  return n;
}
static SeparableChainPlan<SoftNceShardBilinearPlan> plan_softnce_shard_separable(Workspace& ws, int64_t br, int64_t b,
                                                                                 int64_t k, int precision) {
  return plan_separable_chain(ws, br, b, k, [&] { return plan_softnce_shard_bilinear(ws, br, b, k, k, precision); });
}

static int softnce_shard_check(const char* fn, int64_t br, int64_t b, int64_t row_offset, int64_t dx, int64_t dy, int mode,
                               int precision, float tau, float mix) {
  int rc = chain_check<SoftNceEst>(fn, br, b, row_offset, dx, dy, mode, precision);
  if (rc) return rc;
  rc = softnce_check_targets(fn, b, mode, tau, mix);
  if (rc) return rc;
  MI_CHECK_ARG(b < ((int64_t)1 << 24), "%s: b must be below 2^24 on a sharded batch", fn);
  return MI_OK;
}

// the label norms of all b samples (z of the rank's rows to target_norm), the rank's scores and records, its part
static int softnce_shard_fwd_chain(const float* x, const float* y, const float* w, const int64_t* lab_rows,
                                   const int64_t* lab_cols, int64_t br, int64_t b, int64_t row_offset, int64_t dx,
                                   int64_t dy, int precision, float tau, float mix, float* part_out, float* lse_rows,
                                   float* target_norm, const SoftNceShardBilinearPlan& n, hipStream_t st) {
  const SoftNceShardPlan& q = n.q;
  int rc = softnce_label_norm(lab_cols, b, tau, chain_16bit_ok(br, b, dx, dy, precision), q.z, q.inv_z, q.rs, target_norm,
                              row_offset, br, st);
  if (rc) return rc;
  rc = chain_scores<SoftNceEst>(x, y, w, nullptr, nullptr, br, b, 0, dx, dy, precision,
                                softnce_stats_out(q, lab_rows, lab_cols, row_offset, tau, mix), n.p, st);
  if (rc) return rc;
  return softnce_rank_part(q, br, b, part_out, lse_rows, st);
}

// ------------------------------------------------------------------------------------------------ memory-bank InfoNCE
// (mi_banknce.h)  The per-sample InfoNCE of the batch against the batch and a bank of past
// embeddings: an L-shaped score matrix, a top block [b] x [b + m] (a row block of the chain: br = b, row_offset = 0, the
// reports of batch and bank behind each other) and, in the symmetric mode, a left block [m] x [b] (bank images against the
// batch's reports; the GEMM launchers take any m, so it runs as it lies, no transposed formulation).
//   16-bit chain (bf16 / bf16x3; b, m and the widths multiples of 8):
//     prep (batch and bank rows converted at their row offsets) -> T = X W [-> U = bank_x W]
//     -> score GEMM top [-> score GEMM left] -> merge records -> loss
//     [grads] G top [-> G left] -> dT = G Y_all | dY = G^T T [-> dT slabs -> bf16]
//             [sym: dU = G_left Y | dY_left = G_left^T U -> dY = top + left (two slabs, fixed order)]
//             -> dW = X^T dT | dX = dT W^T [sym: dW_bank = bank_x^T dU split-K behind slab 0 = the batch's dW -> reduce]
//   generic kernels (other shapes, MI_PREC_F32): the same sequence on mi_gemm.h; the reports of batch and bank are
//     gathered into one fp32 operand first (these kernels read the caller's fp32 rows directly), the two blocks'
//     contributions to dY and dW are added by the store epilogue's accumulate slot, launch after launch
// grad_bank_t / grad_bank_y: dS/d(bank image rows of T) and d/d(bank report rows), fp32 [m][dy], for the separable critic
// whose bank projections depend on Wg, Wh; null for the bilinear critic (the bank is a constant).
struct BankNceEst {
  static constexpr const char* kName = "the memory-bank InfoNCE";
  static constexpr SepLabels kSep = {"banknce separable A = X Wg",      "banknce separable C = Y Wh",
                                     "banknce separable dX = dA Wg^T",  "banknce separable dWg = X^T dA",
                                     "banknce separable dY = dC Wh^T",  "banknce separable dWh = Y^T dC"};
};

struct BankNcePlan {
  BilinearPlan p;  // the top block: operand copies, T, G, G^T, dT and the slabs of a [b] x [b + m] row block
  BankNceRecords q;
  bool c16, sym;
  float* yall;  // generic kernels: the reports of batch and bank, fp32 [b + m][dy]
  // the bank's image side (symmetric mode): operand copies, U = bank_x W, G_left, dU
  bf16_t *bxb, *bxtb, *ub, *utb, *ytb0, *glb, *gltb, *dub, *dutb;
  float *u, *du;
  void* gl;
  float* dy_slab;   // [2][b][dy]: dY of the top and of the left block
  float* dwb_slab;  // [1 + dwb_splits][dx][dy]: the batch's dW, then the split-K slabs of bank_x^T dU
  int dwb_splits;
  int64_t dwb_kchunk;
  size_t bytes;
};

// The layout does not depend on w (the workspace query has none).  Forward only: the forward half's buffers alone.
static BankNcePlan plan_banknce(Workspace& ws, int64_t b, int64_t m, int64_t dx, int64_t dy, int mode, int precision,
                                bool grads) {
  BankNcePlan n{};
  const int64_t nn = b + m;
  const int64_t x3 = precision == MI_PREC_BF16X3 ? 3 : 1;
  n.sym = mode == MI_NCE_SYMMETRIC;
  n.c16 = chain_16bit_ok(b, m, dx, dy, precision);
  if (grads) {
    n.p = plan_bilinear(ws, b, nn, dx, dy, precision, true, true);
  } else {
    BilinearPlan& p = n.p;
    p.x3 = (int)x3;
    if (n.c16) {
      p.xb = ws.take<bf16_t>(x3 * b * dx);
      p.xtb = ws.take<bf16_t>(x3 * b * dx);
      p.yb = ws.take<bf16_t>(x3 * nn * dy);
      p.ytb = ws.take<bf16_t>(x3 * nn * dy);
      p.wb = ws.take<bf16_t>(x3 * dx * dy);
      p.wtb = ws.take<bf16_t>(x3 * dx * dy);
      p.tb = ws.take<bf16_t>(x3 * b * dy);
      p.ttb = ws.take<bf16_t>(x3 * b * dy);
    } else {
      p.t = ws.take<float>(b * dy);
      p.gen_slab_floats = precision == MI_PREC_F32 ? generic_slab_floats(b, dy, dx) : 0;
      p.gen_slab = p.gen_slab_floats > 0 ? ws.take<float>(p.gen_slab_floats) : nullptr;
    }
  }
  n.q = plan_banknce_records(ws, b, m, n.sym);
  if (!n.c16) n.yall = ws.take<float>(nn * dy);
  if (n.sym) {
    if (n.c16) {
      n.bxb = ws.take<bf16_t>(x3 * m * dx);
      n.bxtb = ws.take<bf16_t>(x3 * m * dx);
      n.ub = ws.take<bf16_t>(x3 * m * dy);
      n.utb = ws.take<bf16_t>(x3 * m * dy);
    } else {
      n.u = ws.take<float>(m * dy);
    }
    if (grads && n.c16) {
      n.ytb0 = ws.take<bf16_t>(x3 * b * dy);
      n.glb = ws.take<bf16_t>(x3 * m * b);
      n.gltb = ws.take<bf16_t>(x3 * m * b);
      n.dub = ws.take<bf16_t>(x3 * m * dy);
      n.dutb = ws.take<bf16_t>(x3 * m * dy);
      n.dy_slab = ws.take<float>(2 * b * dy);
      // split-K of dW_bank = bank_x^T dU as plan_bilinear's dW: ~128 workgroups, K chunks multiples of the K tile
      const int64_t tiles = ((dx + kTile - 1) / kTile) * ((dy + kTile - 1) / kTile);
      int64_t splits = (128 + tiles - 1) / tiles;
      int64_t kchunk = (m + splits - 1) / splits;
      kchunk = (kchunk + kG2KT - 1) / kG2KT * kG2KT;
      splits = (m + kchunk - 1) / kchunk;
      n.dwb_splits = (int)splits;
      n.dwb_kchunk = kchunk;
      n.dwb_slab = ws.take<float>((1 + splits) * dx * dy);
    } else if (grads) {
      if (precision == MI_PREC_BF16) n.gl = ws.take<bf16_t>(m * b);  // G_left in the operand type, as the top block's G
      else n.gl = ws.take<float>(m * b);
      n.du = ws.take<float>(m * dy);
    }
  }
  n.bytes = ws.off;
  return n;
}

static int banknce_check(const char* fn, int64_t b, int64_t m, int64_t dx, int64_t dy, int mode, int precision) {
  MI_CHECK_ARG(b >= 1 && m >= 1 && dx >= 1 && dy >= 1, "%s: sizes must be >= 1 (b %lld, m %lld, widths %lld, %lld)", fn,
               (long long)b, (long long)m, (long long)dx, (long long)dy);
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "%s: unknown mode %d", fn, mode);
  MI_CHECK_ARG(precision == MI_PREC_F32 || precision == MI_PREC_BF16 || precision == MI_PREC_BF16X3,
               "%s: precision %d is not available for %s (f32, bf16, bf16x3)", fn, precision, BankNceEst::kName);
  const int64_t lim = (int64_t)1 << 31;
  MI_CHECK_ARG(b < lim && m < lim && b + m < lim, "%s: b + m must be below 2^31", fn);
  return MI_OK;
}

// The gradient half on the 16-bit chain, behind G, G^T (top) and G_left, G_left^T in the plan
static int banknce_bwd16(bool has_w, int64_t b, int64_t m, int64_t dx, int64_t dy, float* grad_x, float* grad_y,
                         float* grad_w, float* grad_bank_t, float* grad_bank_y, const BankNcePlan& n, hipStream_t st) {
  const BilinearPlan& p = n.p;
  const int64_t nn = b + m;
  const int x3 = p.x3;
  const int ra = x3 == 3 ? 1 : 0, rb = x3 == 3 ? 2 : 0;
  int rc = MI_OK;
  // problem 0: dT[i, c] = sum_j G[i, j] Y_all[j, c] (K = b + m); problem 1: dY[j, c] = sum_i G[i, j] T[i, c] for the
  // batch's reports j < b alone (the first b rows of G^T): no dY of bank rows
  GemmBf16Args two{};
  two.p[0] = GemmBf16Problem{p.gb, x3 * nn, p.ytb, x3 * nn, b, dy, x3 * nn};
  two.p[1] = GemmBf16Problem{p.gtb, x3 * b, p.ttb, x3 * b, b, dy, x3 * b};
  two.n_problems = 2;
  two.k_chunk = x3 * nn;
  float* dy_top = n.sym ? n.dy_slab : grad_y;
  EpiStoreMulti e2{};
  e2.out[0] = has_w ? EpiOut{nullptr, 0, 0, p.dtb, dy, p.dttb, b, nullptr, ra, rb} : EpiOut{grad_x, dy, 0, nullptr, 0, nullptr, 0};
  e2.out[1] = EpiOut{dy_top, dy, 0, nullptr, 0, nullptr, 0};
  bool split_done = false;
  if (p.dt_splits > 1 && x3 == 1 && has_w) {
    // short, wide block: dT partial sums over K chunks into fp32 slabs beside dY, then one pass that adds the slabs in
    // slab order and writes the two bf16 orientations of dT (bilinear_bwd_from_g's split)
    EpiStoreMulti es{};
    es.out[0] = EpiOut{p.dt_slab, dy, b * dy, nullptr, 0, nullptr, 0};
    es.out[1] = e2.out[1];
    const int sp[2] = {p.dt_splits, 1};
    const int64_t ch[2] = {p.dt_kchunk, b};
    rc = launch_gemm_bf16_flat(two, sp, ch, es, st, "banknce dT = G Y | dY = G^T T");
    if (rc == MI_OK) {
      CvtJobs jobs{};
      jobs.j[0] = CvtJob{p.dt_slab, b, dy, p.dtb, p.dttb, p.dt_splits, b * dy};
      rc = launch_cvt_transpose3(jobs, st, "banknce dT slabs -> bf16");
      if (rc) return rc;
      split_done = true;
    } else if (rc != MI_EINVAL) {
      return rc;
    }
  }
  if (!split_done) {
    rc = launch_gemm_bf16(two, 1, e2, st, "banknce dT = G Y | dY = G^T T");
    if (rc) return rc;
  }
  if (grad_bank_y) {
    // the bank reports' rows of G^T: dY_bank[mm, c] = sum_i G[i, b + mm] T[i, c]
    EpiStoreMulti e{};
    e.out[0] = EpiOut{grad_bank_y, dy, 0, nullptr, 0, nullptr, 0};
    rc = launch_gemm_bf16(one_problem(p.gtb + b * x3 * b, x3 * b, p.ttb, x3 * b, m, dy, x3 * b), 1, e, st,
                          "banknce dY_bank = G^T T");
    if (rc) return rc;
  }
  const bool need_du = has_w || grad_bank_t != nullptr;
  if (n.sym) {
    // problem 0: dU[mm, c] = sum_j G_left[mm, j] Y[j, c] (K = b); problem 1: dY_left[j, c] = sum_mm G_left[mm, j] U[mm, c]
    const EpiOut du_out = has_w ? EpiOut{nullptr, 0, 0, n.dub, dy, n.dutb, m, nullptr, ra, rb}
                                : EpiOut{grad_bank_t, dy, 0, nullptr, 0, nullptr, 0};
    const EpiOut dyl_out = EpiOut{n.dy_slab + b * dy, dy, 0, nullptr, 0, nullptr, 0};
    EpiStoreMulti e{};
    if (need_du) {
      GemmBf16Args l{};
      l.p[0] = GemmBf16Problem{n.glb, x3 * b, n.ytb0, x3 * b, m, dy, x3 * b};
      l.p[1] = GemmBf16Problem{n.gltb, x3 * m, n.utb, x3 * m, b, dy, x3 * m};
      l.n_problems = 2;
      l.k_chunk = x3 * (b > m ? b : m);
      e.out[0] = du_out;
      e.out[1] = dyl_out;
      rc = launch_gemm_bf16(l, 1, e, st, "banknce dU = G_left Y | dY_left = G_left^T U");
    } else {
      e.out[0] = dyl_out;
      rc = launch_gemm_bf16(one_problem(n.gltb, x3 * m, n.utb, x3 * m, b, dy, x3 * m), 1, e, st,
                            "banknce dY_left = G_left^T U");
    }
    if (rc) return rc;
    rc = launch_slab_reduce_ld(n.dy_slab, 2, b, dy, grad_y, dy, st, "banknce dY = top + left");
    if (rc) return rc;
  }
  if (!has_w) return MI_OK;
  // dW = X^T dT | dX = dT W^T; symmetric: the batch's dW lands in slab 0 of the bank's slabs, which are reduced in order
  rc = launch_dw_dx(DwDxPair{p.xtb, p.dttb, p.dtb, p.wb, b, dx, dy, x3, p.dw_slab, p.dw_splits, p.dw_kchunk}, grad_x,
                    n.sym ? n.dwb_slab : grad_w, st,
                    {"banknce dW = X^T dT | dX = dT W^T", "banknce dW = X^T dT", "banknce dX = dT W^T"});
  if (rc || !n.sym) return rc;
  EpiStoreMulti e{};
  e.out[0] = EpiOut{n.dwb_slab + dx * dy, dy, dx * dy, nullptr, 0, nullptr, 0};
  rc = launch_gemm_bf16(one_problem(n.bxtb, x3 * m, n.dutb, x3 * m, dx, dy, x3 * m, x3 * n.dwb_kchunk), n.dwb_splits, e, st,
                        "banknce dW_bank = bank_x^T dU");
  if (rc) return rc;
  return launch_slab_reduce_ld(n.dwb_slab, 1 + n.dwb_splits, dx, dy, grad_w, dy, st, "banknce dW = batch + bank");
}

// The whole step.  w == nullptr: S = X Y^T (d_img == d_txt); then T is X, U is bank_x, dT is grad_x.
static int banknce_chain(const float* x, const float* y, const float* w, const int64_t* sid, const float* bank_x,
                         const float* bank_y, const int64_t* bank_sid, int64_t b, int64_t m, int64_t dx, int64_t dy,
                         int mode, int precision, const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols,
                         float* grad_x, float* grad_y, float* grad_w, float* grad_bank_t, float* grad_bank_y, bool any_grad,
                         const BankNcePlan& n, hipStream_t st) {
  const BilinearPlan& p = n.p;
  const BankNceRecords& q = n.q;
  const int64_t nn = b + m;
  const bool sym = n.sym;
  const BankStatsOut so_top = banknce_stats_top(q, sid, bank_sid, b), so_left = banknce_stats_left(q, sid, bank_sid, b);
  const BankGradIn gi_top = banknce_grad_top(q, sid, bank_sid, b, grad_out, mode);
  const BankGradIn gi_left = banknce_grad_left(q, sid, bank_sid, b, grad_out);
  int rc = MI_OK;
  if (n.c16) {
    const int x3 = p.x3;
    const int ra = x3 == 3 ? 1 : 0, rb = x3 == 3 ? 2 : 0;
    const int64_t kk = x3 * dy;
    BankCvtJobs jobs{};
    if (w) {
      jobs.j[0] = BankCvtJob{x, b, nullptr, 0, dx, p.xb, p.xtb, ra, ra, nullptr};
      jobs.j[2] = BankCvtJob{w, dx, nullptr, 0, dy, p.wb, p.wtb, rb, rb, nullptr};
      if (sym) jobs.j[3] = BankCvtJob{bank_x, m, nullptr, 0, dx, n.bxb, n.bxtb, ra, ra, nullptr};
    } else {
      jobs.j[0] = BankCvtJob{x, b, nullptr, 0, dx, p.tb, p.ttb, ra, rb, nullptr};
      if (sym) jobs.j[3] = BankCvtJob{bank_x, m, nullptr, 0, dx, n.ub, n.utb, ra, rb, nullptr};
    }
    jobs.j[1] = BankCvtJob{y, b, bank_y, m, dy, p.yb, p.ytb, rb, rb, nullptr};
    if (sym && any_grad) jobs.j[4] = BankCvtJob{y, b, nullptr, 0, dy, nullptr, n.ytb0, 0, rb, nullptr};
    rc = launch_bank_cvt(jobs, st, "banknce prep batch + bank");
    if (rc) return rc;
    if (w) {
      // T[i, c] = sum_a X[i, a] W[a, c]: A = Xb [b][dx], B = W^T [dy][dx]; U likewise on the bank's images
      EpiStoreMulti e{};
      e.out[0] = EpiOut{nullptr, 0, 0, p.tb, dy, p.ttb, b, nullptr, ra, rb};
      rc = launch_gemm_bf16(one_problem(p.xb, x3 * dx, p.wtb, x3 * dx, b, dy, x3 * dx), 1, e, st, "banknce T = X W");
      if (rc) return rc;
      if (sym) {
        e.out[0] = EpiOut{nullptr, 0, 0, n.ub, dy, n.utb, m, nullptr, ra, rb};
        rc = launch_gemm_bf16(one_problem(n.bxb, x3 * dx, p.wtb, x3 * dx, m, dy, x3 * dx), 1, e, st, "banknce U = bank_x W");
        if (rc) return rc;
      }
    }
    rc = launch_gemm_bf16(one_problem(p.tb, kk, p.yb, kk, b, nn, kk), 1, EpiBankStats<true>{so_top}, st,
                          "banknce score + records (top)");
    if (rc) return rc;
    if (sym) {
      rc = launch_gemm_bf16(one_problem(n.ub, kk, p.yb, kk, m, b, kk), 1, EpiBankStats<true>{so_left}, st,
                            "banknce score + records (left)");
      if (rc) return rc;
    }
    rc = banknce_finish(q, b, mode, loss_out, lse_rows, lse_cols, st);
    if (rc || !any_grad) return rc;
    rc = launch_gemm_bf16(one_problem(p.tb, kk, p.yb, kk, b, nn, kk), 1,
                          EpiBankGrad2{gi_top, p.gb, p.gtb, grad_bank_y ? nn : b, x3 == 3 ? 1 : 0}, st, "banknce G (top)");
    if (rc) return rc;
    if (sym) {
      rc = launch_gemm_bf16(one_problem(n.ub, kk, p.yb, kk, m, b, kk), 1,
                            EpiBankGrad2{gi_left, n.glb, n.gltb, b, x3 == 3 ? 1 : 0}, st, "banknce G (left)");
      if (rc) return rc;
    }
    return banknce_bwd16(w != nullptr, b, m, dx, dy, grad_x, grad_y, grad_w, grad_bank_t, grad_bank_y, n, st);
  }
  return with_operand_type(precision == MI_PREC_BF16, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;  // G is stored in the operand type
    BankCvtJobs jobs{};
    jobs.j[0] = BankCvtJob{y, b, bank_y, m, dy, nullptr, nullptr, 0, 0, n.yall};
    int rc = launch_bank_cvt(jobs, st, "banknce gather Y (generic)");
    if (rc) return rc;
    const float* t = x;
    const float* u = bank_x;
    if (w) {
      rc = generic_gemm_store<OpT>(make_operand(x, dx, 1), make_operand(w, 1, dy), b, dy, dx, p.t, dy, p, st,
                                   "banknce T = X W (generic)");
      if (rc) return rc;
      t = p.t;
      if (sym) {
        rc = generic_gemm_store<OpT>(make_operand(bank_x, dx, 1), make_operand(w, 1, dy), m, dy, dx, n.u, dy, p, st,
                                     "banknce U = bank_x W (generic)");
        if (rc) return rc;
        u = n.u;
      }
    }
    const auto top_a = make_operand(t, dy, 1), all_y = make_operand((const float*)n.yall, dy, 1);
    rc = launch_gemm<OpT>(top_a, all_y, b, nn, dy, EpiBankStats<false>{so_top}, st, "banknce score + records (top, generic)");
    if (rc) return rc;
    if (sym) {
      rc = launch_gemm<OpT>(make_operand(u, dy, 1), all_y, m, b, dy, EpiBankStats<false>{so_left}, st,
                            "banknce score + records (left, generic)");
      if (rc) return rc;
    }
    rc = banknce_finish(q, b, mode, loss_out, lse_rows, lse_cols, st);
    if (rc || !any_grad) return rc;
    OpT* g = (OpT*)p.g;
    OpT* gl = (OpT*)n.gl;
    rc = launch_gemm<OpT>(top_a, all_y, b, nn, dy, EpiBankGrad<OpT>{gi_top, g}, st, "banknce G (top, generic)");
    if (rc) return rc;
    if (sym) {
      rc = launch_gemm<OpT>(make_operand(u, dy, 1), all_y, m, b, dy, EpiBankGrad<OpT>{gi_left, gl}, st,
                            "banknce G (left, generic)");
      if (rc) return rc;
    }
    // dT = G Y_all; dY = G^T T over the batch's reports [+ G_left^T U, accumulated]; dU = G_left Y
    float* dt = w ? p.dt : grad_x;
    rc = generic_gemm_store<OpT>(make_operand((const OpT*)g, nn, 1), make_operand((const float*)n.yall, 1, dy), b, dy, nn, dt,
                                 dy, p, st, "banknce dT = G Y (generic)");
    if (rc) return rc;
    rc = generic_gemm_store<OpT>(make_operand((const OpT*)g, 1, nn), make_operand(t, 1, dy), b, dy, b, grad_y, dy, p, st,
                                 "banknce dY = G^T T (generic)");
    if (rc) return rc;
    if (grad_bank_y) {
      rc = generic_gemm_store<OpT>(make_operand((const OpT*)g + b, 1, nn), make_operand(t, 1, dy), m, dy, b, grad_bank_y, dy, p,
                                   st, "banknce dY_bank = G^T T (generic)");
      if (rc) return rc;
    }
    float* du = w ? n.du : grad_bank_t;
    if (sym) {
      rc = launch_gemm<OpT>(make_operand((const OpT*)gl, 1, b), make_operand(u, 1, dy), b, dy, m,
                            EpiStore{grad_y, dy, nullptr, 1.0f, 1}, st, "banknce dY += G_left^T U (generic)");
      if (rc) return rc;
      if (du) {
        rc = generic_gemm_store<OpT>(make_operand((const OpT*)gl, b, 1), make_operand((const float*)n.yall, 1, dy), m, dy, b,
                                     du, dy, p, st, "banknce dU = G_left Y (generic)");
        if (rc) return rc;
      }
    }
    if (!w) return MI_OK;
    rc = generic_gemm_store<OpT>(make_operand(x, 1, dx), make_operand((const float*)p.dt, 1, dy), dx, dy, b, grad_w, dy, p, st,
                                 "banknce dW = X^T dT (generic)");
    if (rc) return rc;
    if (sym) {
      rc = launch_gemm<OpT>(make_operand(bank_x, 1, dx), make_operand((const float*)n.du, 1, dy), dx, dy, m,
                            EpiStore{grad_w, dy, nullptr, 1.0f, 1}, st, "banknce dW += bank_x^T dU (generic)");
      if (rc) return rc;
    }
    return generic_gemm_store<OpT>(make_operand((const float*)p.dt, dy, 1), make_operand(w, dy, 1), b, dx, dy, grad_x, dx, p,
                                   st, "banknce dX = dT W^T (generic)");
  });
}

// The separable entry point's workspace: the projections of batch and bank and their gradients, then the chain's plan
struct BankNceSeparablePlan {
  float *a, *c, *ab, *cb, *da, *dc, *dab, *dcb;
  BankNcePlan n;
  size_t bytes;
};
static BankNceSeparablePlan plan_banknce_separable(Workspace& ws, int64_t b, int64_t m, int64_t kp, int mode, int precision,
                                                   bool grads) {
  BankNceSeparablePlan s{};
  const bool sym = mode == MI_NCE_SYMMETRIC;
  s.a = ws.take<float>(b * kp);
  s.c = ws.take<float>(b * kp);
  s.ab = sym ? ws.take<float>(m * kp) : nullptr;
  s.cb = ws.take<float>(m * kp);
  if (grads) {
    s.da = ws.take<float>(b * kp);
    s.dc = ws.take<float>(b * kp);
    s.dab = sym ? ws.take<float>(m * kp) : nullptr;
    s.dcb = ws.take<float>(m * kp);
  }
  s.n = plan_banknce(ws, b, m, kp, kp, mode, precision, grads);
  s.bytes = ws.off;
  return s;
}

}  // namespace mi

extern "C" {

// ------------------------------------------------------------------------------------------------ per-sample InfoNCE
size_t mi_nce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_nce_bilinear(ws, b, d_img, d_txt, precision).bytes + 256;
}

int mi_nce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                         int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out, float* lse_rows,
                         float* lse_cols, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                         size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && loss_out && workspace, "mi_nce_bilinear_step: null pointer");
  int rc = chain_check<NceEst>("mi_nce_bilinear_step", b, b, 0, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_nce_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_nce_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const NceBilinearPlan n = plan_nce_bilinear(ws, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_nce_bilinear_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = chain_scores<NceEst>(x, y, w, sid, sid, b, b, 0, d_img, d_txt, precision, nce_stats_out(n.q, sid), n.p, st);
  if (rc) return rc;
  rc = nce_finish(n.q, b, mode, loss_out, lse_rows, lse_cols, st);
  if (rc || !any_grad) return rc;
  return chain_grads<NceEst>(x, y, w, b, b, d_img, d_txt, precision, nce_grad_in(sid, n.q.r, n.q.c, grad_out, b, mode),
                             grad_x, grad_y, grad_w, n.p, st);
}

size_t mi_nce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_nce_separable(ws, b, d_proj, precision).bytes + 256;
}

int mi_nce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                          int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, const float* grad_out,
                          float* loss_out, float* lse_rows, float* lse_cols, float* grad_x, float* grad_y,
                          float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && loss_out && workspace, "mi_nce_separable_step: null pointer");
  int rc = chain_check<NceEst>("mi_nce_separable_step", b, b, 0, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_nce_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_nce_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_nce_separable(ws, b, d_proj, precision);
  rc = ws_fits(ws, "mi_nce_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const NceBilinearPlan& n = sp.n;
  const bool bf = precision == MI_PREC_BF16;
  rc = separable_project(NceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  rc = chain_scores<NceEst>(sp.a, sp.c, nullptr, sid, sid, b, b, 0, k, k, precision, nce_stats_out(n.q, sid), n.p, st);
  if (rc) return rc;
  rc = nce_finish(n.q, b, mode, loss_out, lse_rows, lse_cols, st);
  if (rc || !any_grad) return rc;
  rc = chain_grads<NceEst>(sp.a, sp.c, nullptr, b, b, k, k, precision, nce_grad_in(sid, n.q.r, n.q.c, grad_out, b, mode),
                           sp.da, sp.dc, nullptr, n.p, st);
  if (rc) return rc;
  return separable_project_back(NceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.da, sp.dc, grad_x, grad_y, grad_wg,
                                grad_wh, st);
}

/* Row blocks of a sharded batch (include/mi_critic.h): forward -> part, merge of the gathered parts -> loss and c,
 * backward from the forward's workspace and the merged c. */
size_t mi_nce_part_floats(int64_t b_rows, int64_t b) {
  if (b_rows <= 0 || b <= 0) return 0;
  return (size_t)nce_part_floats(b_rows, b);
}

size_t mi_nce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_nce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision).bytes + 256;
}

int mi_nce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                              const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                              int64_t d_txt, int mode, int precision, float* part_out, float* lse_rows, void* workspace,
                              size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && part_out && workspace, "mi_nce_bilinear_shard_fwd: null pointer");
  int rc = chain_check<NceEst>("mi_nce_bilinear_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_nce_bilinear_shard_fwd: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const NceShardBilinearPlan n = plan_nce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_nce_bilinear_shard_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = chain_scores<NceEst>(x, y, w, sid_rows, sid_cols, b_rows, b, row_offset, d_img, d_txt, precision,
                            nce_stats_out(n.q, sid_rows, sid_cols, row_offset), n.p, st);
  if (rc) return rc;
  return nce_rank_part(n.q, b_rows, b, part_out, lse_rows, st);
}

int mi_nce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                              const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                              int64_t d_txt, int mode, int precision, const float* lse_cols, const float* grad_out,
                              float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                              void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && grad_x && grad_y && workspace, "mi_nce_bilinear_shard_bwd: null pointer");
  int rc = chain_check<NceEst>("mi_nce_bilinear_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_nce_bilinear_shard_bwd: the symmetric mode needs lse_cols");
  MI_CHECK_ARG((w && grad_w) || (!w && !grad_w && d_img == d_txt),
               "mi_nce_bilinear_shard_bwd: w != NULL needs grad_w; w == NULL (S = X Y^T) needs d_img == d_txt, no grad_w");
  Workspace ws(workspace, workspace_bytes);
  const NceShardBilinearPlan n = plan_nce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_nce_bilinear_shard_bwd");
  if (rc) return rc;
  return chain_grads<NceEst>(x, y, w, b_rows, b, d_img, d_txt, precision,
                             nce_grad_in(sid_rows, sid_cols, row_offset, n.q.r, lse_cols, grad_out, b, mode), grad_x,
                             grad_y, grad_w, n.p, (hipStream_t)stream);
}

size_t mi_nce_merge_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  return (size_t)(2 * b) * sizeof(float) + 256;
}

int mi_nce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                       float* lse_cols, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(parts && loss_out && lse_cols && workspace, "mi_nce_merge_parts: null pointer");
  MI_CHECK_ARG(n_ranks >= 1 && b_rows >= 1 && b == n_ranks * b_rows,
               "mi_nce_merge_parts: need b == n_ranks * b_rows >= 1 (got %lld ranks of %lld rows, b %lld)",
               (long long)n_ranks, (long long)b_rows, (long long)b);
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_nce_merge_parts: unknown mode %d", mode);
  Workspace ws(workspace, workspace_bytes);
  float* terms = ws.take<float>(2 * b);
  const int rc = ws_fits(ws, "mi_nce_merge_parts");
  if (rc) return rc;
  return nce_merge_parts(parts, n_ranks, b_rows, b, mode, loss_out, lse_cols, terms, (hipStream_t)stream);
}

size_t mi_nce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                              int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_nce_shard_separable(ws, b_rows, b, d_proj, precision).bytes + 256;
}

int mi_nce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                               const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                               int64_t d_txt, int64_t d_proj, int mode, int precision, float* part_out, float* lse_rows,
                               void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && part_out && workspace,
               "mi_nce_separable_shard_fwd: null pointer");
  int rc = chain_check<NceEst>("mi_nce_separable_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_nce_separable_shard_fwd: projection width must be >= 1");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_nce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_nce_separable_shard_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = separable_project(NceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.a, sp.c,
                         st);
  if (rc) return rc;
  rc = chain_scores<NceEst>(sp.a, sp.c, nullptr, sid_rows, sid_cols, b_rows, b, row_offset, k, k, precision,
                            nce_stats_out(sp.n.q, sid_rows, sid_cols, row_offset), sp.n.p, st);
  if (rc) return rc;
  return nce_rank_part(sp.n.q, b_rows, b, part_out, lse_rows, st);
}

int mi_nce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                               const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                               int64_t d_txt, int64_t d_proj, int mode, int precision, const float* lse_cols,
                               const float* grad_out, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                               void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && grad_x && grad_y && grad_wg && grad_wh && workspace,
               "mi_nce_separable_shard_bwd: null pointer");
  int rc = chain_check<NceEst>("mi_nce_separable_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_nce_separable_shard_bwd: projection width must be >= 1");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_nce_separable_shard_bwd: the symmetric mode needs lse_cols");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_nce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_nce_separable_shard_bwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = chain_grads<NceEst>(sp.a, sp.c, nullptr, b_rows, b, k, k, precision,
                           nce_grad_in(sid_rows, sid_cols, row_offset, sp.n.q.r, lse_cols, grad_out, b, mode), sp.da,
                           sp.dc, nullptr, sp.n.p, st);
  if (rc) return rc;
  // dA -> the rank's dX and its partial dWg; the rank's partial dC (all b text rows) -> partial dY and dWh
  return separable_project_back(NceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.da, sp.dc,
                                        grad_x, grad_y, grad_wg, grad_wh, st);
}

size_t mi_matrix_nce_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  Workspace ws(nullptr, 0);
  plan_nce(ws, b);
  return ws.off + 256;
}

int mi_matrix_nce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, float* loss_out, float* lse_rows,
                      float* lse_cols, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && sid && loss_out && workspace, "mi_matrix_nce_fwd: null pointer");
  MI_CHECK_ARG(b >= 1, "mi_matrix_nce_fwd: b must be >= 1");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_nce_fwd: unknown mode %d", mode);
  Workspace ws(workspace, workspace_bytes);
  const NcePlan q = plan_nce(ws, b);
  const int rc = ws_fits(ws, "mi_matrix_nce_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("nce_matrix_stats_kernel", st);
    hipLaunchKernelGGL(nce_matrix_stats_kernel, dim3((unsigned)q.n_t, (unsigned)q.n_t), dim3(64), 0, st, scores, b,
                       nce_stats_out(q, sid));
  }
  MI_LAUNCH_CHECK("nce_matrix_stats_kernel");
  return nce_finish(q, b, mode, loss_out, lse_rows, lse_cols, st);
}

int mi_matrix_nce_bwd(const float* scores, const int64_t* sid, int64_t b, int mode, const float* lse_rows,
                      const float* lse_cols, const float* grad_out, float* grad_scores, void* stream) {
  MI_CHECK_ARG(scores && sid && lse_rows && grad_scores, "mi_matrix_nce_bwd: null pointer");
  MI_CHECK_ARG(b >= 1, "mi_matrix_nce_bwd: b must be >= 1");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_nce_bwd: unknown mode %d", mode);
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_matrix_nce_bwd: the symmetric mode needs lse_cols");
  const int64_t nt = (b + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("nce_matrix_grad_kernel", st);
    hipLaunchKernelGGL(nce_matrix_grad_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(64), 0, st, scores, b,
                       nce_grad_in(sid, lse_rows, lse_cols, grad_out, b, mode), grad_scores);
  }
  MI_LAUNCH_CHECK("nce_matrix_grad_kernel");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ Jensen-Shannon and NWJ
size_t mi_fdiv_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_fdiv_bilinear(ws, b, d_img, d_txt, precision).bytes + 256;
}

int mi_fdiv_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                          int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out, float* terms_out,
                          mi_stats* stats, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                          size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && loss_out && workspace, "mi_fdiv_bilinear_step: null pointer");
  int rc = chain_check<FdivEst>("mi_fdiv_bilinear_step", b, b, 0, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_fdiv_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_fdiv_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const FdivBilinearPlan n = plan_fdiv_bilinear(ws, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_fdiv_bilinear_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!stats) stats = n.stats;  // the G epilogue reads the statistics: the caller's block or the workspace's
  rc = chain_scores<FdivEst>(x, y, w, sid, sid, b, b, 0, d_img, d_txt, precision,
                             FdivStatsOut{sid, sid, 0, mode, n.rec, n.n_t}, n.p, st);
  if (rc) return rc;
  rc = launch_fdiv_finalize(n.rec, n.n_t * n.n_t, b, mode, loss_out, terms_out, stats, st);
  if (rc || !any_grad) return rc;
  return chain_grads<FdivEst>(x, y, w, b, b, d_img, d_txt, precision, FdivGradIn{sid, sid, 0, mode, stats, grad_out},
                              grad_x, grad_y, grad_w, n.p, st);
}

size_t mi_fdiv_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_fdiv_separable(ws, b, d_proj, precision).bytes + 256;
}

int mi_fdiv_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                           int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                           const float* grad_out, float* loss_out, float* terms_out, mi_stats* stats, float* grad_x,
                           float* grad_y, float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes,
                           void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && loss_out && workspace, "mi_fdiv_separable_step: null pointer");
  int rc = chain_check<FdivEst>("mi_fdiv_separable_step", b, b, 0, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_fdiv_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_fdiv_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_fdiv_separable(ws, b, d_proj, precision);
  rc = ws_fits(ws, "mi_fdiv_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const FdivBilinearPlan& n = sp.n;
  const bool bf = precision == MI_PREC_BF16;
  if (!stats) stats = n.stats;
  rc = separable_project(FdivEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  rc = chain_scores<FdivEst>(sp.a, sp.c, nullptr, sid, sid, b, b, 0, k, k, precision,
                             FdivStatsOut{sid, sid, 0, mode, n.rec, n.n_t}, n.p, st);
  if (rc) return rc;
  rc = launch_fdiv_finalize(n.rec, n.n_t * n.n_t, b, mode, loss_out, terms_out, stats, st);
  if (rc || !any_grad) return rc;
  rc = chain_grads<FdivEst>(sp.a, sp.c, nullptr, b, b, k, k, precision, FdivGradIn{sid, sid, 0, mode, stats, grad_out},
                            sp.da, sp.dc, nullptr, n.p, st);
  if (rc) return rc;
  return separable_project_back(FdivEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.da, sp.dc, grad_x, grad_y, grad_wg,
                                grad_wh, st);
}

// ------------------------------------------------------------------------------------------------ retrieval ranks
size_t mi_rank_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_rank_bilinear(ws, b, d_img, d_txt, precision).bytes + 256;
}

int mi_rank_bilinear(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                     int64_t d_txt, int precision, int32_t* rank_i2t, int32_t* rank_t2i, float* diag_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && workspace, "mi_rank_bilinear: null pointer");
  int rc = chain_check<RankEst>("mi_rank_bilinear", b, b, 0, d_img, d_txt, 0, precision);
  if (rc) return rc;
  MI_CHECK_ARG(rank_i2t || rank_t2i, "mi_rank_bilinear: pass rank_i2t, rank_t2i or both");
  MI_CHECK_ARG(w || d_img == d_txt, "mi_rank_bilinear: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const RankBilinearPlan n = plan_rank_bilinear(ws, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_rank_bilinear");
  if (rc) return rc;
  return rank_chain(x, y, w, sid, b, d_img, d_txt, precision, rank_i2t, rank_t2i, diag_out, n, (hipStream_t)stream);
}

size_t mi_rank_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_rank_separable(ws, b, d_proj, precision).bytes + 256;
}

int mi_rank_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                      int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, int32_t* rank_i2t, int32_t* rank_t2i,
                      float* diag_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && workspace, "mi_rank_separable: null pointer");
  int rc = chain_check<RankEst>("mi_rank_separable", b, b, 0, d_img, d_txt, 0, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_rank_separable: projection width must be >= 1");
  MI_CHECK_ARG(rank_i2t || rank_t2i, "mi_rank_separable: pass rank_i2t, rank_t2i or both");
  Workspace ws(workspace, workspace_bytes);
  const RankSeparablePlan sp = plan_rank_separable(ws, b, d_proj, precision);
  rc = ws_fits(ws, "mi_rank_separable");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = separable_project(RankEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  return rank_chain(sp.a, sp.c, nullptr, sid, b, k, k, precision, rank_i2t, rank_t2i, diag_out, sp.n, st);
}

// ------------------------------------------------------------------------------------------------ MI estimates
size_t mi_estimates_matrix_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  Workspace ws(nullptr, 0);
  plan_est(ws, b);
  return ws.off + 256;
}

int mi_estimates_matrix(const float* scores, const int64_t* sid, int64_t b, const float* taus_host, int n_tau,
                        float* est_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && sid && est_out && workspace, "mi_estimates_matrix: null pointer");
  EstTaus taus;
  int rc = est_check("mi_estimates_matrix", b, taus_host, n_tau, taus);
  if (rc) return rc;
  MI_CHECK_ARG((b + 63) / 64 <= 65535, "mi_estimates_matrix: b %lld needs more than 65535 tile rows", (long long)b);
  Workspace ws(workspace, workspace_bytes);
  const EstPlan q = plan_est(ws, b);
  rc = ws_fits(ws, "mi_estimates_matrix");
  if (rc) return rc;
  return est_matrix(scores, sid, b, taus, est_out, q, (hipStream_t)stream);
}

size_t mi_estimates_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_est_bilinear(ws, b, d_img, d_txt, precision).bytes + 256;
}

int mi_estimates_bilinear(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                          int64_t d_txt, int precision, const float* taus_host, int n_tau, float* est_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && est_out && workspace, "mi_estimates_bilinear: null pointer");
  int rc = chain_check<EstimatesEst>("mi_estimates_bilinear", b, b, 0, d_img, d_txt, 0, precision);
  if (rc) return rc;
  EstTaus taus;
  rc = est_check("mi_estimates_bilinear", b, taus_host, n_tau, taus);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_estimates_bilinear: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const EstBilinearPlan n = plan_est_bilinear(ws, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_estimates_bilinear");
  if (rc) return rc;
  return est_chain(x, y, w, sid, b, d_img, d_txt, precision, taus, est_out, n, (hipStream_t)stream);
}

size_t mi_estimates_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_est_separable(ws, b, d_proj, precision).bytes + 256;
}

int mi_estimates_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                           int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, const float* taus_host, int n_tau,
                           float* est_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && est_out && workspace, "mi_estimates_separable: null pointer");
  int rc = chain_check<EstimatesEst>("mi_estimates_separable", b, b, 0, d_img, d_txt, 0, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_estimates_separable: projection width must be >= 1");
  EstTaus taus;
  rc = est_check("mi_estimates_separable", b, taus_host, n_tau, taus);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const EstSeparablePlan sp = plan_est_separable(ws, b, d_proj, precision);
  rc = ws_fits(ws, "mi_estimates_separable");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = separable_project(EstimatesEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  return est_chain(sp.a, sp.c, nullptr, sid, b, k, k, precision, taus, est_out, sp.n, st);
}

// ------------------------------------------------------------------------------------------------ top-k retrieval
size_t mi_topk_matrix_workspace_bytes(int64_t n_rows, int64_t n_cols, int k, int axis) {
  if (n_rows <= 0 || n_cols <= 0 || k < 1 || k > kTopkMaxK || (axis != 0 && axis != 1)) return 0;
  return (size_t)(axis == 0 ? n_rows : n_cols) * k * sizeof(topk_key_t) + 256;
}

int mi_topk_matrix(const float* scores, int64_t n_rows, int64_t n_cols, const int64_t* sid_rows, const int64_t* sid_cols,
                   int k, int axis, int32_t* idx, float* val, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && idx && val && workspace, "mi_topk_matrix: null pointer");
  MI_CHECK_ARG(n_rows >= 1 && n_cols >= 1, "mi_topk_matrix: sizes must be >= 1 (got %lld x %lld)", (long long)n_rows,
               (long long)n_cols);
  MI_CHECK_ARG(n_rows < ((int64_t)1 << 31) && n_cols < ((int64_t)1 << 31), "mi_topk_matrix: sizes must be below 2^31");
  MI_CHECK_ARG(k >= 1 && k <= kTopkMaxK, "mi_topk_matrix: k must be in [1, %d] (got %d)", kTopkMaxK, k);
  MI_CHECK_ARG(axis == 0 || axis == 1, "mi_topk_matrix: axis must be 0 (rows' columns) or 1 (columns' rows), got %d", axis);
  MI_CHECK_ARG((sid_rows == nullptr) == (sid_cols == nullptr), "mi_topk_matrix: pass sid_rows and sid_cols, or neither");
  Workspace ws(workspace, workspace_bytes);
  const int64_t n_q = axis == 0 ? n_rows : n_cols;
  topk_key_t* keys = ws.take<topk_key_t>(n_q * k);
  int rc = ws_fits(ws, "mi_topk_matrix");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = topk_zero(keys, n_q * k, st);
  if (rc) return rc;
  rc = topk_matrix(scores, sid_rows, sid_cols, n_rows, n_cols, axis, keys, k, st);
  if (rc) return rc;
  return topk_finish(keys, n_q, k, idx, val, st);
}

size_t mi_topk_bilinear_workspace_bytes(int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int precision, int k) {
  if (n_img <= 0 || n_txt <= 0 || d_img <= 0 || d_txt <= 0 || k < 1 || k > kTopkMaxK) return 0;
  Workspace ws(nullptr, 0);
  return plan_topk_bilinear(ws, n_img, n_txt, d_img, d_txt, precision, k).bytes + 256;
}

int mi_topk_bilinear(const float* x, const float* y, const float* w, const int64_t* sid_img, const int64_t* sid_txt,
                     int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int precision, int k, int32_t* idx_i2t,
                     float* val_i2t, int32_t* idx_t2i, float* val_t2i, void* workspace, size_t workspace_bytes,
                     void* stream) {
  MI_CHECK_ARG(x && y && workspace, "mi_topk_bilinear: null pointer");
  int rc = topk_check("mi_topk_bilinear", n_img, n_txt, d_img, d_txt, precision, k);
  if (rc) return rc;
  const TopkDirs d{idx_i2t, val_i2t, idx_t2i, val_t2i};
  rc = topk_check_dirs("mi_topk_bilinear", sid_img, sid_txt, d);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_topk_bilinear: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const TopkBilinearPlan n = plan_topk_bilinear(ws, n_img, n_txt, d_img, d_txt, precision, k);
  rc = ws_fits(ws, "mi_topk_bilinear");
  if (rc) return rc;
  return topk_chain(x, y, w, sid_img, sid_txt, n_img, n_txt, d_img, d_txt, precision, k, d, n, (hipStream_t)stream);
}

size_t mi_topk_separable_workspace_bytes(int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                         int precision, int k) {
  if (n_img <= 0 || n_txt <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0 || k < 1 || k > kTopkMaxK) return 0;
  Workspace ws(nullptr, 0);
  return plan_topk_separable(ws, n_img, n_txt, d_proj, precision, k).bytes + 256;
}

int mi_topk_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_img,
                      const int64_t* sid_txt, int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int64_t d_proj,
                      int precision, int k, int32_t* idx_i2t, float* val_i2t, int32_t* idx_t2i, float* val_t2i,
                      void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && workspace, "mi_topk_separable: null pointer");
  int rc = topk_check("mi_topk_separable", n_img, n_txt, d_img, d_txt, precision, k);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1 && d_proj < ((int64_t)1 << 31), "mi_topk_separable: projection width must be in [1, 2^31)");
  const TopkDirs d{idx_i2t, val_i2t, idx_t2i, val_t2i};
  rc = topk_check_dirs("mi_topk_separable", sid_img, sid_txt, d);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const TopkSeparablePlan sp = plan_topk_separable(ws, n_img, n_txt, d_proj, precision, k);
  rc = ws_fits(ws, "mi_topk_separable");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = separable_project(TopkEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, n_img, n_txt, d_img, d_txt, d_proj, sp.a,
                         sp.c, st);
  if (rc) return rc;
  return topk_chain(sp.a, sp.c, nullptr, sid_img, sid_txt, n_img, n_txt, d_proj, d_proj, precision, k, d, sp.n, st);
}

// ------------------------------------------------------------------------------------------------ hard-negative InfoNCE
size_t mi_hardnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int k, int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || k < 1 || k > kTopkMaxK) return 0;
  Workspace ws(nullptr, 0);
  return plan_hardnce_bilinear(ws, b, d_img, d_txt, precision, k, with_grads != 0).bytes + 256;
}

int mi_hardnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                             int64_t d_txt, int mode, int precision, int k, const float* grad_out, float* loss_out,
                             float* lse_rows, float* lse_cols, int32_t* idx_rows, int32_t* idx_cols, float* grad_x,
                             float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && loss_out && workspace, "mi_hardnce_bilinear_step: null pointer");
  int rc = hardnce_check("mi_hardnce_bilinear_step", b, d_img, d_txt, mode, precision, k);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_hardnce_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_hardnce_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const HardNceBilinearPlan n = plan_hardnce_bilinear(ws, b, d_img, d_txt, precision, k, any_grad);
  rc = ws_fits(ws, "mi_hardnce_bilinear_step");
  if (rc) return rc;
  return hardnce_chain(x, y, w, sid, b, d_img, d_txt, mode, precision, k, grad_out, loss_out, lse_rows, lse_cols, idx_rows,
                       idx_cols, grad_x, grad_y, grad_w, any_grad, n, (hipStream_t)stream);
}

size_t mi_hardnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, int k,
                                            int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0 || k < 1 || k > kTopkMaxK) return 0;
  Workspace ws(nullptr, 0);
  return plan_hardnce_separable(ws, b, d_proj, precision, k, with_grads != 0).bytes + 256;
}

int mi_hardnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                              int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, int k,
                              const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, int32_t* idx_rows,
                              int32_t* idx_cols, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                              void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && loss_out && workspace, "mi_hardnce_separable_step: null pointer");
  int rc = hardnce_check("mi_hardnce_separable_step", b, d_img, d_txt, mode, precision, k);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_hardnce_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_hardnce_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_hardnce_separable(ws, b, d_proj, precision, k, any_grad);
  rc = ws_fits(ws, "mi_hardnce_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t kp = d_proj;
  const bool bf = precision == MI_PREC_BF16;
  rc = separable_project(HardNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, kp, sp.a, sp.c, st);
  if (rc) return rc;
  rc = hardnce_chain(sp.a, sp.c, nullptr, sid, b, kp, kp, mode, precision, k, grad_out, loss_out, lse_rows, lse_cols,
                     idx_rows, idx_cols, sp.da, sp.dc, nullptr, any_grad, sp.n, st);
  if (rc || !any_grad) return rc;
  return separable_project_back(HardNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, kp, sp.da, sp.dc, grad_x, grad_y,
                                grad_wg, grad_wh, st);
}

size_t mi_matrix_hardnce_workspace_bytes(int64_t b, int k) {
  if (b <= 0 || k < 1 || k > kTopkMaxK) return 0;
  Workspace ws(nullptr, 0);
  plan_hardnce_lists(ws, b, k);
  return ws.off + 256;
}

int mi_matrix_hardnce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, int k, float* loss_out,
                          float* lse_rows, float* lse_cols, int32_t* idx_rows, int32_t* idx_cols, void* workspace,
                          size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && sid && loss_out && workspace, "mi_matrix_hardnce_fwd: null pointer");
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "mi_matrix_hardnce_fwd: b must be in [1, 2^31)");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_hardnce_fwd: unknown mode %d", mode);
  MI_CHECK_ARG(k >= 1 && k <= kTopkMaxK, "mi_matrix_hardnce_fwd: k must be in [1, %d] (got %d)", kTopkMaxK, k);
  Workspace ws(workspace, workspace_bytes);
  const HardNceLists q = plan_hardnce_lists(ws, b, k);
  int rc = ws_fits(ws, "mi_matrix_hardnce_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool sym = mode == MI_NCE_SYMMETRIC;
  rc = topk_zero(q.keys, (sym ? 2 : 1) * b * k, st);
  if (rc) return rc;
  rc = topk_matrix(scores, sid, sid, b, b, 0, q.keys, k, st);
  if (rc) return rc;
  rc = topk_finish(q.keys, b, k, idx_rows ? idx_rows : q.idx, q.val, st);
  if (rc) return rc;
  if (sym) {
    rc = topk_matrix(scores, sid, sid, b, b, 1, q.keys + b * k, k, st);
    if (rc) return rc;
    rc = topk_finish(q.keys + b * k, b, k, idx_cols ? idx_cols : q.idx + b * k, q.val + b * k, st);
    if (rc) return rc;
  }
  return hardnce_finish(q.val, q.val + b * k, scores, b + 1, b, k, mode, q, loss_out, lse_rows, lse_cols, st);
}

int mi_matrix_hardnce_bwd(const float* scores, int64_t b, int mode, int k, const int32_t* idx_rows, const int32_t* idx_cols,
                          const float* lse_rows, const float* lse_cols, const float* grad_out, float* grad_scores,
                          void* stream) {
  MI_CHECK_ARG(scores && idx_rows && lse_rows && grad_scores, "mi_matrix_hardnce_bwd: null pointer");
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "mi_matrix_hardnce_bwd: b must be in [1, 2^31)");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_hardnce_bwd: unknown mode %d", mode);
  MI_CHECK_ARG(k >= 1 && k <= kTopkMaxK, "mi_matrix_hardnce_bwd: k must be in [1, %d] (got %d)", kTopkMaxK, k);
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || (idx_cols && lse_cols),
               "mi_matrix_hardnce_bwd: the symmetric mode needs idx_cols and lse_cols");
  const int64_t nt = (b + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("hardnce_matrix_grad_kernel", st);
    hipLaunchKernelGGL(hardnce_matrix_grad_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(64), 0, st, scores, b,
                       hardnce_grad_in(idx_rows, idx_cols, k, lse_rows, lse_cols, grad_out, b, mode), grad_scores);
  }
  MI_LAUNCH_CHECK("hardnce_matrix_grad_kernel");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ study-positive InfoNCE
size_t mi_posnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_posnce_bilinear(ws, b, d_img, d_txt, precision, with_grads != 0).bytes + 256;
}

int mi_posnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                            int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out,
                            float* lse_rows, float* lse_cols, int32_t* n_pos_out, float* grad_x, float* grad_y,
                            float* grad_w, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && loss_out && workspace, "mi_posnce_bilinear_step: null pointer");
  int rc = posnce_check("mi_posnce_bilinear_step", b, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_posnce_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_posnce_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const PosNceBilinearPlan n = plan_posnce_bilinear(ws, b, d_img, d_txt, precision, any_grad);
  rc = ws_fits(ws, "mi_posnce_bilinear_step");
  if (rc) return rc;
  return posnce_chain(x, y, w, sid, b, d_img, d_txt, mode, precision, grad_out, loss_out, lse_rows, lse_cols, n_pos_out,
                      grad_x, grad_y, grad_w, any_grad, n, (hipStream_t)stream);
}

size_t mi_posnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision,
                                           int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_posnce_separable(ws, b, d_proj, precision, with_grads != 0).bytes + 256;
}

int mi_posnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                             int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                             const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, int32_t* n_pos_out,
                             float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                             size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && loss_out && workspace, "mi_posnce_separable_step: null pointer");
  int rc = posnce_check("mi_posnce_separable_step", b, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_posnce_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_posnce_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_posnce_separable(ws, b, d_proj, precision, any_grad);
  rc = ws_fits(ws, "mi_posnce_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const bool bf = precision == MI_PREC_BF16;
  rc = separable_project(PosNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  rc = posnce_chain(sp.a, sp.c, nullptr, sid, b, k, k, mode, precision, grad_out, loss_out, lse_rows, lse_cols, n_pos_out,
                    sp.da, sp.dc, nullptr, any_grad, sp.n, st);
  if (rc || !any_grad) return rc;
  return separable_project_back(PosNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.da, sp.dc, grad_x, grad_y,
                                grad_wg, grad_wh, st);
}

size_t mi_matrix_posnce_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  Workspace ws(nullptr, 0);
  plan_posnce(ws, b);
  return ws.off + 256;
}

int mi_matrix_posnce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, float* loss_out, float* lse_rows,
                         float* lse_cols, int32_t* n_pos, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && sid && loss_out && workspace, "mi_matrix_posnce_fwd: null pointer");
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "mi_matrix_posnce_fwd: b must be in [1, 2^31)");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_posnce_fwd: unknown mode %d", mode);
  Workspace ws(workspace, workspace_bytes);
  const PosNcePlan q = plan_posnce(ws, b);
  const int rc = ws_fits(ws, "mi_matrix_posnce_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("posnce_matrix_stats_kernel", st);
    hipLaunchKernelGGL(posnce_matrix_stats_kernel, dim3((unsigned)q.n_t, (unsigned)q.n_t), dim3(64), 0, st, scores, b,
                       posnce_stats_out(q, sid));
  }
  MI_LAUNCH_CHECK("posnce_matrix_stats_kernel");
  return posnce_finish(q, b, mode, loss_out, lse_rows, lse_cols, n_pos, st);
}

int mi_matrix_posnce_bwd(const float* scores, const int64_t* sid, int64_t b, int mode, const float* lse_rows,
                         const float* lse_cols, const int32_t* n_pos, const float* grad_out, float* grad_scores,
                         void* stream) {
  MI_CHECK_ARG(scores && sid && lse_rows && n_pos && grad_scores, "mi_matrix_posnce_bwd: null pointer");
  MI_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31), "mi_matrix_posnce_bwd: b must be in [1, 2^31)");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_matrix_posnce_bwd: unknown mode %d", mode);
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_matrix_posnce_bwd: the symmetric mode needs lse_cols");
  const int64_t nt = (b + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("posnce_matrix_grad_kernel", st);
    hipLaunchKernelGGL(posnce_matrix_grad_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(64), 0, st, scores, b,
                       posnce_grad_in(sid, lse_rows, lse_cols, nullptr, n_pos, grad_out, b, mode), grad_scores);
  }
  MI_LAUNCH_CHECK("posnce_matrix_grad_kernel");
  return MI_OK;
}

/* Row blocks of a sharded batch (include/mi_critic.h): forward -> part, merge of the gathered parts -> loss and c,
 * backward from the forward's workspace and the merged c. */
size_t mi_posnce_part_floats(int64_t b_rows, int64_t b) {
  if (b_rows <= 0 || b <= 0) return 0;
  return (size_t)posnce_part_floats(b_rows, b);
}

size_t mi_posnce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_posnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision).bytes + 256;
}

int mi_posnce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                                 const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                 int64_t d_txt, int mode, int precision, float* part_out, float* lse_rows,
                                 int32_t* n_pos_out, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && part_out && workspace, "mi_posnce_bilinear_shard_fwd: null pointer");
  int rc = posnce_shard_check("mi_posnce_bilinear_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_posnce_bilinear_shard_fwd: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const PosNceShardBilinearPlan n = plan_posnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_posnce_bilinear_shard_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = chain_scores<PosNceEst>(x, y, w, nullptr, nullptr, b_rows, b, 0, d_img, d_txt, precision,
                               posnce_stats_out(n.q, sid_rows, sid_cols), n.p, st);
  if (rc) return rc;
  return posnce_rank_part(n.q, b_rows, b, part_out, lse_rows, n_pos_out, st);
}

int mi_posnce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                                 const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                 int64_t d_txt, int mode, int precision, const float* lse_cols, const float* grad_out,
                                 float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  MI_CHECK_ARG(x && y && sid_rows && sid_cols && grad_x && grad_y && workspace,
               "mi_posnce_bilinear_shard_bwd: null pointer");
  int rc = posnce_shard_check("mi_posnce_bilinear_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_posnce_bilinear_shard_bwd: the symmetric mode needs lse_cols");
  MI_CHECK_ARG((w && grad_w) || (!w && !grad_w && d_img == d_txt),
               "mi_posnce_bilinear_shard_bwd: w != NULL needs grad_w; w == NULL (S = X Y^T) needs d_img == d_txt, no "
               "grad_w");
  Workspace ws(workspace, workspace_bytes);
  const PosNceShardBilinearPlan n = plan_posnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_posnce_bilinear_shard_bwd");
  if (rc) return rc;
  return chain_grads<PosNceEst>(x, y, w, b_rows, b, d_img, d_txt, precision,
                                posnce_grad_in(sid_rows, sid_cols, n.q.r, lse_cols, n.q.inv_n, nullptr, grad_out, b, mode),
                                grad_x, grad_y, grad_w, n.p, (hipStream_t)stream);
}

size_t mi_posnce_merge_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  return (size_t)(2 * b) * sizeof(float) + 256;
}

int mi_posnce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                          float* lse_cols, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(parts && loss_out && lse_cols && workspace, "mi_posnce_merge_parts: null pointer");
  MI_CHECK_ARG(n_ranks >= 1 && b_rows >= 1 && b == n_ranks * b_rows,
               "mi_posnce_merge_parts: need b == n_ranks * b_rows >= 1 (got %lld ranks of %lld rows, b %lld)",
               (long long)n_ranks, (long long)b_rows, (long long)b);
  MI_CHECK_ARG(b < ((int64_t)1 << 24), "mi_posnce_merge_parts: b must be below 2^24 on a sharded batch");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_posnce_merge_parts: unknown mode %d", mode);
  Workspace ws(workspace, workspace_bytes);
  float* terms = ws.take<float>(2 * b);
  const int rc = ws_fits(ws, "mi_posnce_merge_parts");
  if (rc) return rc;
  return posnce_merge_parts(parts, n_ranks, b_rows, b, mode, loss_out, lse_cols, terms, (hipStream_t)stream);
}

size_t mi_posnce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                                 int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_posnce_shard_separable(ws, b_rows, b, d_proj, precision).bytes + 256;
}

int mi_posnce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh,
                                  const int64_t* sid_rows, const int64_t* sid_cols, int64_t b_rows, int64_t b,
                                  int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                                  float* part_out, float* lse_rows, int32_t* n_pos_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && part_out && workspace,
               "mi_posnce_separable_shard_fwd: null pointer");
  int rc = posnce_shard_check("mi_posnce_separable_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_posnce_separable_shard_fwd: projection width must be >= 1");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_posnce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_posnce_separable_shard_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = separable_project(PosNceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.a, sp.c,
                         st);
  if (rc) return rc;
  rc = chain_scores<PosNceEst>(sp.a, sp.c, nullptr, nullptr, nullptr, b_rows, b, 0, k, k, precision,
                               posnce_stats_out(sp.n.q, sid_rows, sid_cols), sp.n.p, st);
  if (rc) return rc;
  return posnce_rank_part(sp.n.q, b_rows, b, part_out, lse_rows, n_pos_out, st);
}

int mi_posnce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh,
                                  const int64_t* sid_rows, const int64_t* sid_cols, int64_t b_rows, int64_t b,
                                  int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                                  const float* lse_cols, const float* grad_out, float* grad_x, float* grad_y,
                                  float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid_rows && sid_cols && grad_x && grad_y && grad_wg && grad_wh && workspace,
               "mi_posnce_separable_shard_bwd: null pointer");
  int rc = posnce_shard_check("mi_posnce_separable_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_posnce_separable_shard_bwd: projection width must be >= 1");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_posnce_separable_shard_bwd: the symmetric mode needs lse_cols");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_posnce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_posnce_separable_shard_bwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = chain_grads<PosNceEst>(sp.a, sp.c, nullptr, b_rows, b, k, k, precision,
                              posnce_grad_in(sid_rows, sid_cols, sp.n.q.r, lse_cols, sp.n.q.inv_n, nullptr, grad_out, b,
                                             mode),
                              sp.da, sp.dc, nullptr, sp.n.p, st);
  if (rc) return rc;
  // dA -> the rank's dX and its partial dWg; the rank's partial dC (all b text rows) -> partial dY and dWh
  return separable_project_back(PosNceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.da,
                                sp.dc, grad_x, grad_y, grad_wg, grad_wh, st);
}

// ------------------------------------------------------------------------------------------------ soft-target InfoNCE
size_t mi_softnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_softnce_bilinear(ws, b, d_img, d_txt, precision, with_grads != 0).bytes + 256;
}

int mi_softnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* label_mask, int64_t b,
                             int64_t d_img, int64_t d_txt, int mode, int precision, float tau, float mix,
                             const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, float* target_norm,
                             float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                             void* stream) {
  MI_CHECK_ARG(x && y && label_mask && loss_out && workspace, "mi_softnce_bilinear_step: null pointer");
  int rc = softnce_check("mi_softnce_bilinear_step", b, d_img, d_txt, mode, precision, tau, mix);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_softnce_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_softnce_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const SoftNceBilinearPlan n = plan_softnce_bilinear(ws, b, d_img, d_txt, precision, any_grad);
  rc = ws_fits(ws, "mi_softnce_bilinear_step");
  if (rc) return rc;
  return softnce_chain(x, y, w, label_mask, b, d_img, d_txt, mode, precision, tau, mix, grad_out, loss_out, lse_rows,
                       lse_cols, target_norm, grad_x, grad_y, grad_w, any_grad, n, (hipStream_t)stream);
}

size_t mi_softnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision,
                                            int with_grads) {
  if (b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_softnce_separable(ws, b, d_proj, precision, with_grads != 0).bytes + 256;
}

int mi_softnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* label_mask,
                              int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, float tau,
                              float mix, const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols,
                              float* target_norm, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                              void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && label_mask && loss_out && workspace, "mi_softnce_separable_step: null pointer");
  int rc = softnce_check("mi_softnce_separable_step", b, d_img, d_txt, mode, precision, tau, mix);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_softnce_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_softnce_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_softnce_separable(ws, b, d_proj, precision, any_grad);
  rc = ws_fits(ws, "mi_softnce_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const bool bf = precision == MI_PREC_BF16;
  rc = separable_project(SoftNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  rc = softnce_chain(sp.a, sp.c, nullptr, label_mask, b, k, k, mode, precision, tau, mix, grad_out, loss_out, lse_rows,
                     lse_cols, target_norm, sp.da, sp.dc, nullptr, any_grad, sp.n, st);
  if (rc || !any_grad) return rc;
  return separable_project_back(SoftNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.da, sp.dc, grad_x, grad_y,
                                grad_wg, grad_wh, st);
}

size_t mi_matrix_softnce_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  Workspace ws(nullptr, 0);
  plan_softnce(ws, b);
  return ws.off + 256;
}

int mi_matrix_softnce_fwd(const float* scores, const int64_t* label_mask, int64_t b, int mode, float tau, float mix,
                          float* loss_out, float* lse_rows, float* lse_cols, float* target_norm, void* workspace,
                          size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(scores && label_mask && loss_out && workspace, "mi_matrix_softnce_fwd: null pointer");
  int rc = softnce_check_targets("mi_matrix_softnce_fwd", b, mode, tau, mix);
  if (rc) return rc;
  Workspace ws(workspace, workspace_bytes);
  const SoftNcePlan q = plan_softnce(ws, b);
  rc = ws_fits(ws, "mi_matrix_softnce_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = softnce_label_norm(label_mask, b, tau, false, q, target_norm, st);
  if (rc) return rc;
  {
    ProfScope prof_("softnce_matrix_stats_kernel", st);
    hipLaunchKernelGGL(softnce_matrix_stats_kernel, dim3((unsigned)q.n_t, (unsigned)q.n_t), dim3(64), 0, st, scores, b,
                       softnce_stats_out(q, label_mask, tau, mix));
  }
  MI_LAUNCH_CHECK("softnce_matrix_stats_kernel");
  return softnce_finish(q, b, mode, loss_out, lse_rows, lse_cols, st);
}

int mi_matrix_softnce_bwd(const float* scores, const int64_t* label_mask, int64_t b, int mode, float tau, float mix,
                          const float* lse_rows, const float* lse_cols, const float* target_norm, const float* grad_out,
                          float* grad_scores, void* stream) {
  MI_CHECK_ARG(scores && label_mask && lse_rows && grad_scores, "mi_matrix_softnce_bwd: null pointer");
  MI_CHECK_ARG(target_norm, "mi_matrix_softnce_bwd: target_norm (the forward's z) is required");
  const int rc = softnce_check_targets("mi_matrix_softnce_bwd", b, mode, tau, mix);
  if (rc) return rc;
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_matrix_softnce_bwd: the symmetric mode needs lse_cols");
  const int64_t nt = (b + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof_("softnce_matrix_grad_kernel", st);
    hipLaunchKernelGGL(softnce_matrix_grad_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(64), 0, st, scores, b,
                       softnce_grad_in(label_mask, nullptr, nullptr, target_norm, lse_rows, lse_cols, grad_out, b, mode,
                                       tau, mix),
                       grad_scores);
  }
  MI_LAUNCH_CHECK("softnce_matrix_grad_kernel");
  return MI_OK;
}

/* Row blocks of a sharded batch (include/mi_critic.h): forward -> part, merge of the gathered parts -> loss and c,
 * backward from the forward's workspace and the merged c. */
size_t mi_softnce_part_floats(int64_t b_rows, int64_t b) {
  if (b_rows <= 0 || b <= 0) return 0;
  return (size_t)softnce_part_floats(b_rows, b);
}

size_t mi_softnce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_softnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision).bytes + 256;
}

int mi_softnce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* label_rows,
                                  const int64_t* label_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                  int64_t d_txt, int mode, int precision, float tau, float mix, float* part_out,
                                  float* lse_rows, float* target_norm, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  MI_CHECK_ARG(x && y && label_rows && label_cols && part_out && workspace, "mi_softnce_bilinear_shard_fwd: null pointer");
  int rc = softnce_shard_check("mi_softnce_bilinear_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision, tau,
                               mix);
  if (rc) return rc;
  MI_CHECK_ARG(w || d_img == d_txt, "mi_softnce_bilinear_shard_fwd: w == NULL (S = X Y^T) needs d_img == d_txt");
  Workspace ws(workspace, workspace_bytes);
  const SoftNceShardBilinearPlan n = plan_softnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_softnce_bilinear_shard_fwd");
  if (rc) return rc;
  return softnce_shard_fwd_chain(x, y, w, label_rows, label_cols, b_rows, b, row_offset, d_img, d_txt, precision, tau, mix,
                                 part_out, lse_rows, target_norm, n, (hipStream_t)stream);
}

int mi_softnce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* label_rows,
                                  const int64_t* label_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                  int64_t d_txt, int mode, int precision, float tau, float mix, const float* lse_cols,
                                  const float* grad_out, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && label_rows && label_cols && grad_x && grad_y && workspace,
               "mi_softnce_bilinear_shard_bwd: null pointer");
  int rc = softnce_shard_check("mi_softnce_bilinear_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision, tau,
                               mix);
  if (rc) return rc;
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_softnce_bilinear_shard_bwd: the symmetric mode needs lse_cols");
  MI_CHECK_ARG((w && grad_w) || (!w && !grad_w && d_img == d_txt),
               "mi_softnce_bilinear_shard_bwd: w != NULL needs grad_w; w == NULL (S = X Y^T) needs d_img == d_txt, no "
               "grad_w");
  Workspace ws(workspace, workspace_bytes);
  const SoftNceShardBilinearPlan n = plan_softnce_shard_bilinear(ws, b_rows, b, d_img, d_txt, precision);
  rc = ws_fits(ws, "mi_softnce_bilinear_shard_bwd");
  if (rc) return rc;
  return chain_grads<SoftNceEst>(x, y, w, b_rows, b, d_img, d_txt, precision,
                                 softnce_grad_in(label_rows, label_cols, row_offset, n.q.rs, n.q.inv_z, nullptr, n.q.r,
                                                 lse_cols, grad_out, b, mode, tau, mix),
                                 grad_x, grad_y, grad_w, n.p, (hipStream_t)stream);
}

size_t mi_softnce_merge_workspace_bytes(int64_t b) {
  if (b <= 0) return 0;
  return (size_t)(2 * b) * sizeof(float) + 256;
}

int mi_softnce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                           float* lse_cols, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(parts && loss_out && lse_cols && workspace, "mi_softnce_merge_parts: null pointer");
  MI_CHECK_ARG(n_ranks >= 1 && b_rows >= 1 && b == n_ranks * b_rows,
               "mi_softnce_merge_parts: need b == n_ranks * b_rows >= 1 (got %lld ranks of %lld rows, b %lld)",
               (long long)n_ranks, (long long)b_rows, (long long)b);
  MI_CHECK_ARG(b < ((int64_t)1 << 24), "mi_softnce_merge_parts: b must be below 2^24 on a sharded batch");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || mode == MI_NCE_SYMMETRIC, "mi_softnce_merge_parts: unknown mode %d", mode);
  Workspace ws(workspace, workspace_bytes);
  float* terms = ws.take<float>(2 * b);
  const int rc = ws_fits(ws, "mi_softnce_merge_parts");
  if (rc) return rc;
  return softnce_merge_parts(parts, n_ranks, b_rows, b, mode, loss_out, lse_cols, terms, (hipStream_t)stream);
}

size_t mi_softnce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                                  int precision) {
  if (b_rows <= 0 || b <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_softnce_shard_separable(ws, b_rows, b, d_proj, precision).bytes + 256;
}

int mi_softnce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh,
                                   const int64_t* label_rows, const int64_t* label_cols, int64_t b_rows, int64_t b,
                                   int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                   int precision, float tau, float mix, float* part_out, float* lse_rows,
                                   float* target_norm, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && label_rows && label_cols && part_out && workspace,
               "mi_softnce_separable_shard_fwd: null pointer");
  int rc = softnce_shard_check("mi_softnce_separable_shard_fwd", b_rows, b, row_offset, d_img, d_txt, mode, precision, tau,
                               mix);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_softnce_separable_shard_fwd: projection width must be >= 1");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_softnce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_softnce_separable_shard_fwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  rc = separable_project(SoftNceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.a, sp.c,
                         st);
  if (rc) return rc;
  return softnce_shard_fwd_chain(sp.a, sp.c, nullptr, label_rows, label_cols, b_rows, b, row_offset, k, k, precision, tau,
                                 mix, part_out, lse_rows, target_norm, sp.n, st);
}

int mi_softnce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh,
                                   const int64_t* label_rows, const int64_t* label_cols, int64_t b_rows, int64_t b,
                                   int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                   int precision, float tau, float mix, const float* lse_cols, const float* grad_out,
                                   float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && label_rows && label_cols && grad_x && grad_y && grad_wg && grad_wh && workspace,
               "mi_softnce_separable_shard_bwd: null pointer");
  int rc = softnce_shard_check("mi_softnce_separable_shard_bwd", b_rows, b, row_offset, d_img, d_txt, mode, precision, tau,
                               mix);
  if (rc) return rc;
  MI_CHECK_ARG(d_proj >= 1, "mi_softnce_separable_shard_bwd: projection width must be >= 1");
  MI_CHECK_ARG(mode == MI_NCE_ROWWISE || lse_cols, "mi_softnce_separable_shard_bwd: the symmetric mode needs lse_cols");
  Workspace ws(workspace, workspace_bytes);
  const auto sp = plan_softnce_shard_separable(ws, b_rows, b, d_proj, precision);
  rc = ws_fits(ws, "mi_softnce_separable_shard_bwd");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const SoftNceShardPlan& q = sp.n.q;
  rc = chain_grads<SoftNceEst>(sp.a, sp.c, nullptr, b_rows, b, k, k, precision,
                               softnce_grad_in(label_rows, label_cols, row_offset, q.rs, q.inv_z, nullptr, q.r, lse_cols,
                                               grad_out, b, mode, tau, mix),
                               sp.da, sp.dc, nullptr, sp.n.p, st);
  if (rc) return rc;
  // dA -> the rank's dX and its partial dWg; the rank's partial dC (all b text rows) -> partial dY and dWh
  return separable_project_back(SoftNceEst::kSep, precision == MI_PREC_BF16, x, y, wg, wh, b_rows, b, d_img, d_txt, k, sp.da,
                                sp.dc, grad_x, grad_y, grad_wg, grad_wh, st);
}

// ------------------------------------------------------------------------------------------------ memory-bank InfoNCE
size_t mi_banknce_bilinear_workspace_bytes(int64_t b, int64_t m, int64_t d_img, int64_t d_txt, int mode, int precision,
                                           int with_grads) {
  if (b <= 0 || m <= 0 || d_img <= 0 || d_txt <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_banknce(ws, b, m, d_img, d_txt, mode, precision, with_grads != 0).bytes + 256;
}

int mi_banknce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, const float* bank_x,
                             const float* bank_y, const int64_t* bank_sid, int64_t b, int64_t m, int64_t d_img,
                             int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out,
                             float* lse_rows, float* lse_cols, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                             size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && sid && bank_y && bank_sid && loss_out && workspace, "mi_banknce_bilinear_step: null pointer");
  int rc = banknce_check("mi_banknce_bilinear_step", b, m, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(bank_x || mode == MI_NCE_ROWWISE, "mi_banknce_bilinear_step: the symmetric mode needs bank_x");
  MI_CHECK_ARG(w || d_img == d_txt, "mi_banknce_bilinear_step: w == NULL (S = X Y^T) needs d_img == d_txt");
  const bool any_grad = grad_x || grad_y || grad_w;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && (w ? grad_w != nullptr : grad_w == nullptr)),
               "mi_banknce_bilinear_step: pass grad_x, grad_y and (with w) grad_w, or none of them");
  Workspace ws(workspace, workspace_bytes);
  const BankNcePlan n = plan_banknce(ws, b, m, d_img, d_txt, mode, precision, any_grad);
  rc = ws_fits(ws, "mi_banknce_bilinear_step");
  if (rc) return rc;
  return banknce_chain(x, y, w, sid, bank_x, bank_y, bank_sid, b, m, d_img, d_txt, mode, precision, grad_out, loss_out,
                       lse_rows, lse_cols, grad_x, grad_y, grad_w, nullptr, nullptr, any_grad, n, (hipStream_t)stream);
}

size_t mi_banknce_separable_workspace_bytes(int64_t b, int64_t m, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                            int precision, int with_grads) {
  if (b <= 0 || m <= 0 || d_img <= 0 || d_txt <= 0 || d_proj <= 0) return 0;
  Workspace ws(nullptr, 0);
  return plan_banknce_separable(ws, b, m, d_proj, mode, precision, with_grads != 0).bytes + 256;
}

int mi_banknce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                              const float* bank_x, const float* bank_y, const int64_t* bank_sid, int64_t b, int64_t m,
                              int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, const float* grad_out,
                              float* loss_out, float* lse_rows, float* lse_cols, float* grad_x, float* grad_y,
                              float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(x && y && wg && wh && sid && bank_y && bank_sid && loss_out && workspace,
               "mi_banknce_separable_step: null pointer");
  int rc = banknce_check("mi_banknce_separable_step", b, m, d_img, d_txt, mode, precision);
  if (rc) return rc;
  MI_CHECK_ARG(bank_x || mode == MI_NCE_ROWWISE, "mi_banknce_separable_step: the symmetric mode needs bank_x");
  MI_CHECK_ARG(d_proj >= 1, "mi_banknce_separable_step: projection width must be >= 1");
  const bool any_grad = grad_x || grad_y || grad_wg || grad_wh;
  MI_CHECK_ARG(!any_grad || (grad_x && grad_y && grad_wg && grad_wh),
               "mi_banknce_separable_step: pass all four gradients or none of them");
  Workspace ws(workspace, workspace_bytes);
  const BankNceSeparablePlan sp = plan_banknce_separable(ws, b, m, d_proj, mode, precision, any_grad);
  rc = ws_fits(ws, "mi_banknce_separable_step");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t k = d_proj;
  const bool bf = precision == MI_PREC_BF16, sym = mode == MI_NCE_SYMMETRIC;
  // the projections of the batch, then the bank's (recomputed every call: they depend on Wg, Wh)
  rc = separable_project(BankNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.a, sp.c, st);
  if (rc) return rc;
  rc = with_operand_type(bf, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    if (sym) {
      const int r = launch_gemm<OpT>(make_operand(bank_x, d_img, 1), make_operand(wg, 1, k), m, k, d_img,
                                     EpiStore{sp.ab, k, nullptr, 1.0f, 0}, st, "banknce separable A_bank = bank_x Wg");
      if (r) return r;
    }
    return launch_gemm<OpT>(make_operand(bank_y, d_txt, 1), make_operand(wh, 1, k), m, k, d_txt,
                            EpiStore{sp.cb, k, nullptr, 1.0f, 0}, st, "banknce separable C_bank = bank_y Wh");
  });
  if (rc) return rc;
  rc = banknce_chain(sp.a, sp.c, nullptr, sid, sp.ab, sp.cb, bank_sid, b, m, k, k, mode, precision, grad_out, loss_out,
                     lse_rows, lse_cols, sp.da, sp.dc, nullptr, sp.dab, sp.dcb, any_grad, sp.n, st);
  if (rc || !any_grad) return rc;
  rc = separable_project_back(BankNceEst::kSep, bf, x, y, wg, wh, b, b, d_img, d_txt, k, sp.da, sp.dc, grad_x, grad_y,
                              grad_wg, grad_wh, st);
  if (rc) return rc;
  // the bank rows' share of dWg, dWh, added behind the batch's by the store epilogue's accumulate slot
  return with_operand_type(bf, [&](auto* op) {
    using OpT = OperandOf<decltype(op)>;
    if (sym) {
      const int r = launch_gemm<OpT>(make_operand(bank_x, 1, d_img), make_operand((const float*)sp.dab, 1, k), d_img, k, m,
                                     EpiStore{grad_wg, k, nullptr, 1.0f, 1}, st, "banknce separable dWg += bank_x^T dA_bank");
      if (r) return r;
    }
    return launch_gemm<OpT>(make_operand(bank_y, 1, d_txt), make_operand((const float*)sp.dcb, 1, k), d_txt, k, m,
                            EpiStore{grad_wh, k, nullptr, 1.0f, 1}, st, "banknce separable dWh += bank_y^T dC_bank");
  });
}

}  // extern "C"
