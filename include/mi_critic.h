/*
 * mi_critic.h -- C ABI of the MI355X-native mutual-information critic path (libmi_critic_hip.so).
 *
 * The reference (vnoz/Mutual-Information-MultiModal) is pure Python and has no FFI; the interface each entry
 * point replaces is therefore a Python callable.  Citations are file:line relative to the reference root.
 *
 *   mi_bound_*            <- mutual_info_img_txt/mi_critics.py:3-12  (dv_bound_loss)
 *                            mutual_info_img_txt/mi_critics.py:14-23 (infonce_bound_loss)
 *   mi_pair_index,
 *   mi_create_pairs*      <- MultiModalManager.create_mi_pairs, mutual_info_img_txt/main_utils.py:80-110
 *   mi_concat_mlp_*       <- the call site mutual_info_img_txt/main_utils.py:220-226:
 *                            create_mi_pairs -> mi_discriminator (make_mlp(1536,[1024,512]), model.py:18-32,
 *                            instantiated main_utils.py:77) -> mi_critic -> loss.backward()
 *   mi_separable_*        <- same call site with the separable critic S = (X Wg)(Y Wh)^T (BASELINE.json configs[1])
 *   mi_bilinear_*         <- same call site with the bilinear critic S = (X W) Y^T named by BASELINE.json
 *                            (an extension: the reference has no bilinear critic; the bound, the masking and the
 *                            pair semantics applied to its scores are the reference's)
 *   mi_nce_*, mi_matrix_nce_* <- an extension: the per-sample (CPC / ConVIRT / CLIP) InfoNCE on the bilinear and
 *                            separable critics and on materialised scores, with the reference's masking rule
 *                            (main_utils.py:105); the reference has no such loss
 *   mi_fdiv_*             <- an extension: the Jensen-Shannon (Deep InfoMax) and NWJ bounds on the reference's pairs
 *                            (main_utils.py:88-110), for every critic; the reference has "dv" and "infonce" only
 *   mi_rank_*             <- an extension: image-report retrieval ranks (for recall@K, median rank, MRR) of every
 *                            critic under the same masking rule; an evaluation, not an estimator
 *   mi_topk_*             <- an extension: the k best reports of an image and the k best images of a report over a
 *                            gallery (n_img != n_txt allowed), optionally without equal-id candidates; an evaluation too
 *   mi_posnce_*, mi_matrix_posnce_* <- an extension: the per-sample InfoNCE with every same-study pair as a positive
 *                            (the dataset pairs each image with its study's report, so such pairs are true matches)
 *   mi_softnce_*, mi_matrix_softnce_* <- an extension: the per-sample InfoNCE with soft targets from the CheXpert /
 *                            NegBio finding labels of the dataset's label table (the reference ships the table; no
 *                            loss of it reads it)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; all tensors are dense row-major
 *   - embeddings, parameters, scores and gradients are float32 (the reference is fp32 throughout);
 *     study ids are int64 codes (equal code <=> equal study id; the reference compares ids with != only,
 *     main_utils.py:105)
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work on it and never synchronise
 *     (the reference synchronises only at loss.item(), main_utils.py:233); the only exception is
 *     mi_pairs_count_host, which returns a host integer
 *   - the callee never allocates or frees: outputs, saved statistics and workspace are caller-owned;
 *     query sizes with the *_workspace_bytes functions (pure host arithmetic; 0 for a non-positive size)
 *   - return value: 0 on success, negative MI_E* code on failure; mi_last_error() describes the last failure
 *     on the calling thread.  No C++ exception crosses this boundary.
 *   - re-entrant: forward and backward may be called from different host threads (autograd does).  Process-wide state is
 *     limited to (a) per-device caches of kernel attributes (atomic, raised under a mutex) and (b) the optional
 *     profiling hook mi_profile_begin/end, which is NOT thread-safe (single-threaded benchmarking only).  The library
 *     never sets the device: the caller makes the tensors' device current (the Python binding does).
 *
 * estimator: MI_DV = 0 (loss = LSE(neg) - log N_neg - mean(pos)), MI_INFONCE = 1 (no log N_neg term).
 * precision: MI_PREC_F32 = 0 (fp32-input MFMA, exact fp32 products, parity mode),
 *            MI_PREC_BF16 = 1 (bf16 MFMA operands, fp32 accumulate),
 *            MI_PREC_BF16X3 = 2 (bilinear critic with a weight matrix only: every operand split into two bf16 parts,
 *            three bf16 MFMAs per product, fp32 accumulate -- products good to ~2^-16 at a third of the bf16 rate;
 *            mi_separable_fwd / _bwd / _step and the concat-MLP entry points reject it),
 *            MI_PREC_FP8 = 3 (bilinear critic with a weight matrix only; widths multiples of 16: x, y, W and T = x W are
 *            quantised to OCP e4m3 with per-tensor scales absmax / 448 computed on the device, both forward products
 *            run on the fp8 MFMA with fp32 accumulation, the backward is straight-through on the quantised values
 *            with bf16 MFMA operands; other entry points reject it),
 *            MI_PREC_F16 = 4 (concat-MLP critic only: fp16 MFMA operands -- U, V, W2 and w3 W2 scaled by powers of two
 *            derived on the device from their absmax, the generated operand relu(U_i + V_j) formed by packed fp16
 *            arithmetic -- fp32 accumulate; the fast mode of the reference's critic, csrc/mi_concat_f16.h).
 */
#ifndef MI_CRITIC_H
#define MI_CRITIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument (null pointer, negative size, unknown enum) */
#define MI_ESHAPE (-2)   /* shape not supported by the fused kernels */
#define MI_EWORKSPACE (-3) /* workspace too small */
#define MI_EHIP (-4)     /* a HIP runtime call failed */

#define MI_DV 0
#define MI_INFONCE 1

#define MI_PREC_F32 0
#define MI_PREC_BF16 1
#define MI_PREC_BF16X3 2
#define MI_PREC_FP8 3
#define MI_PREC_F16 4   /* concat-MLP critic: fp16 MFMA operands with power-of-two tensor scales, fp32 accumulate */
#define MI_PREC_F16X3 5 /* concat-MLP critic: every operand as two fp16 parts, three MFMAs per product (fp32 tolerances) */

/* Statistics block written by every forward call and read by the matching backward call (64 bytes). */
typedef struct mi_stats {
  float lse;          /* log-sum-exp over the negative scores                                  */
  float pos_mean;     /* mean of the positive scores                                           */
  float loss_dv;      /* lse - log(n_neg) - pos_mean      (mi_critics.py:10,12)                */
  float loss_infonce; /* lse - pos_mean                   (mi_critics.py:21,23)                */
  float log_n_neg;    /* logf((float)n_neg), float32 as in the reference (mi_critics.py:10)    */
  float neg_max;      /* running maximum of the negative scores                                */
  float reserved0, reserved1;
  int64_t n_neg;      /* number of negative rows N - pos_size                                  */
  int64_t n_pos;      /* pos_size                                                              */
  int64_t reserved2, reserved3;
} mi_stats;

/* Kernel paths reported by mi_bilinear_path / mi_separable_path (host-side queries; nothing is launched) */
#define MI_PATH_GENERIC 0    /* strided-operand kernels of mi_gemm.h (fp32 parity mode, odd shapes)            */
#define MI_PATH_GEMMS 1      /* 16-bit GEMM chain with G / G^T materialised (widths outside the fused kernel) */
#define MI_PATH_FUSED 2      /* fused B x B kernel + the three-launch backward tail                          */
#define MI_PATH_FUSED_TAIL 3 /* fused B x B kernel + the two-launch tail (the four-launch step)              */
#define MI_PATH_FP8_GEMMS 4  /* fp8 forward products + bf16 backward chain                                   */

int mi_abi_version(void);  /* 4: bf16 / fp16 boundary, path queries, MI_PREC_F16 / MI_PREC_F16X3 */
const char* mi_last_error(void);

/* Optional per-kernel timing (bench.py's roofline leg): between mi_profile_begin and mi_profile_end every kernel
 * launch of this library is bracketed by HIP events on its stream.  mi_profile_end synchronises the device and returns
 * up to `capacity` (name, milliseconds) records in launch order; names is a NUL-separated list.  Not thread-safe. */
int mi_profile_begin(void);
int mi_profile_end(char* names, size_t names_bytes, float* ms, int capacity, int* n_out);

/* ---- a3 / a4: bound on materialised logits (mi_critics.py:3-23) ------------------------------------ */
size_t mi_bound_workspace_bytes(int64_t n);
/* logits[n] (the reference's [N,1] tensor), first pos_size rows positive.  Writes *stats and loss_out[0]. */
int mi_bound_fwd(const float* logits, int64_t n, int64_t pos_size, int estimator, float* loss_out,
                 mi_stats* stats, void* workspace, size_t workspace_bytes, void* stream);
/* grad_logits[r] = grad_out[0] * (r < pos ? -1/pos : exp(logits[r] - lse)); identical for both estimators. */
int mi_bound_bwd(const float* logits, int64_t n, int64_t pos_size, const mi_stats* stats, const float* grad_out,
                 float* grad_logits, void* stream);

/* ---- bound on a B x B score matrix with study-id masking ------------------------------------------- */
/* positives = diagonal; negatives = (i != j and sid[i] != sid[j]); other pairs are dropped (main_utils.py:105) */
size_t mi_matrix_bound_workspace_bytes(int64_t b);
int mi_matrix_bound_fwd(const float* scores, const int64_t* sid, int64_t b, int estimator, float* loss_out,
                        mi_stats* stats, void* workspace, size_t workspace_bytes, void* stream);
/* grad_scores[i,j] = grad_out[0] * dloss/dS[i,j] */
int mi_matrix_bound_bwd(const float* scores, const int64_t* sid, int64_t b, const mi_stats* stats,
                        const float* grad_out, float* grad_scores, void* stream);

/* ---- a1: pair builder (main_utils.py:80-110) ------------------------------------------------------- */
/* number of rows N of mi_input for these ids (host result; synchronises the stream) */
int mi_pairs_count_host(const int64_t* sid, int64_t b, int64_t* n_rows_host, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t mi_pair_index_workspace_bytes(int64_t b);
/* pair_i/pair_j[capacity] receive the (i,j) of every row in reference order (positives first, then gap-major /
 * i-minor negatives); n_rows_dev[0] receives N.  rowpos (optional, [b*(b-1)] int32) receives for every (gap,i)
 * the output row or -1 when the pair is dropped. */
int mi_pair_index(const int64_t* sid, int64_t b, int32_t* pair_i, int32_t* pair_j, int64_t capacity,
                  int64_t* n_rows_dev, int32_t* rowpos, void* workspace, size_t workspace_bytes, void* stream);
/* out[n_rows, d_img + d_txt] = [img[pair_i[r]] ; txt[pair_j[r]]] */
int mi_create_pairs(const float* embedding_img, const float* embedding_txt, const int32_t* pair_i,
                    const int32_t* pair_j, int64_t n_rows, int64_t d_img, int64_t d_txt, float* out, void* stream);
/* grad_img[i] = sum of grad_out rows whose image index is i (left part), same for txt (right part); fixed
 * summation order (positive row, then gaps ascending). */
int mi_create_pairs_bwd(const float* grad_out, const int32_t* rowpos, int64_t b, int64_t d_img, int64_t d_txt,
                        float* grad_img, float* grad_txt, void* stream);

/* ---- fused bilinear critic: S = (X W) Y^T, bound, all gradients ------------------------------------- */
/* X [b_rows, d_img] (the local row block), Y [b, d_txt] (all columns), W [d_img, d_txt], sid_rows [b_rows],
 * sid_cols [b]; row_offset = global index of local row 0 (diagonal of the global B x B matrix).  Single GPU:
 * b_rows = b, row_offset = 0.  scores_out (optional) [b_rows, b].  w == NULL selects the separable form
 * S = X Y^T on already-projected embeddings (d_img == d_txt; grad_w unused).
 * need_grad bit 0: the forward's fused B x B launch also accumulates the two gradient contractions (the loss has one
 * global log-sum-exp, so they only need a scale once it is known); the matching backward then never recomputes scores. */
size_t mi_bilinear_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_bilinear_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                    const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                    int64_t d_txt, int estimator, int precision, int need_grad, float* loss_out, mi_stats* stats,
                    float* partials_out, float* scores_out, void* workspace, size_t workspace_bytes, void* stream);
/* stats must hold the GLOBAL lse / n_pos (after the cross-rank merge when sharded). grad_out[0] = dL/dloss.
 * Outputs: grad_x [b_rows, d_img], grad_y [b, d_txt] (partial over this row block), grad_w [d_img, d_txt].
 * workspace_from_forward != 0: `workspace` is the buffer the matching mi_bilinear_fwd call wrote (same inputs,
 * need_grad != 0); the backward then reuses the operand copies, T and the fused sums found there instead of
 * rebuilding them. */
int mi_bilinear_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                    const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                    int64_t d_txt, int precision, const mi_stats* stats, const float* grad_out, float* grad_x,
                    float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                    int workspace_from_forward, void* stream);

/* Sharded batches (b_rows < b): the part of the forward's preparation that depends on the rank's own rows only (bf16
 * copies of X and W, T = X W), so that it runs while the all-gather of the text embeddings is in flight (SURVEY.md 8e:
 * "overlap the gather with local work").  Then mi_bilinear_fwd(..., need_grad | 4, ...) on the SAME workspace (bit 2 of
 * need_grad: the local part is prepared).  MI_ESHAPE where the shape does not take the fused kernels: call
 * mi_bilinear_fwd alone then. */
int mi_bilinear_prep_local(const float* x, const float* w, int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt,
                           int precision, void* workspace, size_t workspace_bytes, void* stream);

/* Sharded batches without the finalize and merge launches: mi_bilinear_fwd(..., need_grad | 8, ...) leaves one 16-byte
 * record per wave of the fused kernel in the workspace and writes no loss / stats / partials_out;
 * mi_bilinear_raw_records returns their count (0: the shape does not take this path) and, through offset_bytes, where
 * they start in the workspace.  All-gather that region from every rank (rank order) and call mi_bilinear_bwd_records on
 * the forward's workspace: its first launch merges all n_records records in the given order on every workgroup
 * (bit-identical loss / stats on every rank; n_pos = the global batch), then computes the gradients as mi_bilinear_bwd. */
size_t mi_bilinear_raw_records(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision,
                               size_t* offset_bytes);
int mi_bilinear_bwd_records(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                            const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                            int64_t d_txt, int precision, int estimator, const float* records, int64_t n_records,
                            int64_t n_pos, const float* grad_out, float* loss_out, mi_stats* stats_out, float* grad_x,
                            float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes, void* stream);
/* mi_bilinear_bwd_records with grad_w == NULL stops after its first launch (statistics, loss, grad_x, the partial grad_y);
 * mi_bilinear_bwd_dw then launches dW = X^T dT from the same workspace.  Between the two a sharded step starts the
 * reduce-scatter of grad_y, which so overlaps the dW launch (ABI 4). */
int mi_bilinear_bwd_dw(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision, float* grad_w,
                       void* workspace, size_t workspace_bytes, void* stream);


/* fp8 mode (MI_PREC_FP8) on a sharded batch: the per-tensor scales must be the whole batch's.  The forward's preparation
 * in three stages around the caller's two MAX all-reduces of amax_io (4 floats on the device: x, y, w, T):
 *   stage 0 -> amax_io[0..2] | all-reduce MAX | stage 1 -> amax_io[3] | all-reduce MAX | stage 2,
 * then mi_bilinear_fwd(..., need_grad | 2, ...) on the SAME workspace (bit 1 of need_grad: the fp8 operands are staged)
 * and mi_bilinear_bwd(..., workspace_from_forward = 1).  BASELINE.json configs[4] (fp8, 8 GPUs). */
int mi_bilinear_fp8_stage(const float* x, const float* y, const float* w, int64_t b_rows, int64_t b, int64_t d_img,
                          int64_t d_txt, int stage, float* amax_io, void* workspace, size_t workspace_bytes, void* stream);

/* One critic step in ONE call (single GPU; the sharded case needs the cross-rank merge between the forward and the
 * backward and uses the two calls above): forward, statistics, loss and every gradient of  grad_out[0] * loss
 * (grad_out == NULL: 1).  Same inputs, outputs and workspace as mi_bilinear_fwd + mi_bilinear_bwd with b_rows == b,
 * row_offset == 0; replaces the whole call site main_utils.py:220-226 (pairs -> critic -> bound -> loss.backward()).
 * Where the fused kernels take the shape it saves the finalize launch: nothing needs the loss between the fused B x B
 * kernel and the gradients, so the per-wave records are merged by the launch that also turns the partial sums into
 * dT / grad_y / grad_x.  loss_out, *stats and partials_out (optional) are valid when the call's work has completed. */
int mi_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                     int64_t d_txt, int estimator, int precision, const float* grad_out, float* loss_out,
                     mi_stats* stats, float* partials_out, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The step at a bf16 boundary (ABI 4): x_bf16 [b][d_img], y_bf16 [b][d_txt] hold bfloat16 -- what the encoders emit under
 * autocast (model.py:540-555 run in bf16) --; grad_x / grad_y are bfloat16 buffers when grads_bf16 != 0, float32 buffers
 * otherwise; w, grad_w, the loss and the statistics are float32.  The kernels' first act on fp32 embeddings is to round
 * them to bf16, so this entry point computes the same bits as mi_bilinear_step(precision = MI_PREC_BF16) on the same
 * bf16-representable values; what it saves is the 25 MB of conversion traffic per step at B = 4096, d = 512.  Shapes:
 * mi_bilinear_path(b, b, d_img, d_txt, MI_PREC_BF16) == MI_PATH_FUSED_TAIL, 16-byte aligned embeddings; else MI_ESHAPE. */
int mi_bilinear_step_bf16(const void* x_bf16, const void* y_bf16, const float* w, const int64_t* sid, int64_t b,
                          int64_t d_img, int64_t d_txt, int estimator, const float* grad_out, float* loss_out,
                          mi_stats* stats, float* partials_out, void* grad_x, void* grad_y, int grads_bf16,
                          float* grad_w, void* workspace, size_t workspace_bytes, void* stream);

/* Which kernels a shape takes: one of MI_PATH_* (or a negative MI_E* code).  Host-side arithmetic on the plan only; the
 * Python binding uses it to warn once per shape when a 16-bit call leaves the fused kernels. */
int mi_bilinear_path(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_separable_path(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision);

/* Which kernel the 16-bit GEMM launcher issues for one m x n problem of depth k without split-K and with a storing (not
 * partial-reducing) epilogue -- the score GEMM of every loss family on the 16-bit chain, where k is d_txt (bf16) or
 * 3 * d_txt (bf16x3): one of MI_GEMM16_*, or MI_EINVAL on a size < 1.  The launcher switches on the same host function;
 * nothing is launched and no GPU is needed. */
#define MI_GEMM16_PLAIN 0       /* 128 x 128 tiles, operands staged through registers (k % 64 != 0)        */
#define MI_GEMM16_GLDS 1        /* 128 x 128 tiles, LDS-DMA, two stages                                     */
#define MI_GEMM16_GLDS4 2       /* 128 x 128 tiles, LDS-DMA, four stages (k >= 256, at most 512 tiles)      */
#define MI_GEMM16_PIPE128 3     /* 128 x 128 tiles, ping-pong K groups (k >= 2048, at most 256 tiles)       */
#define MI_GEMM16_PIPE256X128 4 /* 256 x 128 tiles, ping-pong K groups (k >= 2048, 160 .. 256 such tiles)   */
#define MI_GEMM16_BIG 5         /* 256 x 256 tiles (at least 192 of them)                                   */
int mi_gemm16_variant(int64_t m, int64_t n, int64_t k);

/* ---- fused separable critic: S = (X Wg)(Y Wh)^T, bound, all gradients ------------------------------- */
/* BASELINE.json configs[1] (an extension: the reference has no separable critic; bound, masking and pair semantics are
 * the reference's).  X [b_rows, d_img], Y [b, d_txt], Wg [d_img, d_proj], Wh [d_txt, d_proj].  The projections run on
 * this library's MFMA kernels (no library GEMM).  Sharding arguments as for mi_bilinear_*.
 * precision: MI_PREC_F32 (exact fp32 products on the generic kernels) or MI_PREC_BF16 (the fused kernels where
 * mi_separable_path says so, bf16 operands on the generic kernels otherwise).  mi_separable_fwd / _bwd / _step answer
 * every other code with MI_EINVAL before anything touches the device; the two host queries still take the codes of the
 * bilinear critic and report the generic plan for them. */
size_t mi_separable_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                    int precision);
int mi_separable_fwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                     const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                     int64_t d_txt, int64_t d_proj, int estimator, int precision, int need_grad, float* loss_out,
                     mi_stats* stats, float* partials_out, void* workspace, size_t workspace_bytes, void* stream);
/* grad_y [b, d_txt] is the partial over this row block; grad_wg / grad_wh are this row block's contributions. */
int mi_separable_bwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                     const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                     int64_t d_txt, int64_t d_proj, int precision, const mi_stats* stats, const float* grad_out,
                     float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                     size_t workspace_bytes, int workspace_from_forward, void* stream);

/* One separable-critic step in one call (single GPU; ABI 4): as mi_bilinear_step.  Five launches where the fused kernels
 * take the shape (mi_separable_path == MI_PATH_FUSED_TAIL): conversions, the two projections, the fused B x B kernel,
 * [statistics + dA, dC rows + dX, dY on the matrix cores], [dWg | dWh]. */
int mi_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                      int64_t d_img, int64_t d_txt, int64_t d_proj, int estimator, int precision, const float* grad_out,
                      float* loss_out, mi_stats* stats, float* partials_out, float* grad_x, float* grad_y,
                      float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused concat-MLP critic (the reference's mi_discriminator) ------------------------------------ */
/* params in PyTorch [out,in] layout: w1 [h1, d_img+d_txt], b1 [h1], w2 [h2, h1], b2 [h2], w3 [h2], b3 [1]. */
size_t mi_concat_mlp_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t h1,
                                     int64_t h2, int precision, int need_grad);
int mi_concat_mlp_fwd(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, const int64_t* sid_rows,
                      const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                      int64_t d_txt, int64_t h1, int64_t h2, int estimator, int precision, int need_grad,
                      float* loss_out, mi_stats* stats, float* partials_out, float* scores_out /* [b_rows,b] */,
                      void* workspace, size_t workspace_bytes, void* stream);
int mi_concat_mlp_bwd(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, const int64_t* sid_rows,
                      const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                      int64_t d_txt, int64_t h1, int64_t h2, int precision, const mi_stats* stats,
                      const float* grad_out, const float* scores /* [b_rows,b] from fwd */, float* grad_x,
                      float* grad_y, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                      float* grad_w3, float* grad_b3, void* workspace, size_t workspace_bytes, void* stream);
/* The critic as a differentiable score matrix: any loss on S, written in any framework, trains it on the fused kernels.
 * The forward runs the score kernels alone (no study ids, no reduction, no loss) and writes scores_out [b_rows, b],
 * b_rows <= b, local row i being sample i; with need_grad it leaves the sign-bit images and operand copies in the
 * workspace (mi_concat_mlp_workspace_bytes) as the forward above does.  The backward takes grad_scores = dL/dS [b_rows, b]
 * -- dropped pairs are whatever the caller put there, normally 0 -- and the workspace of a forward made with need_grad = 1
 * (MI_EWORKSPACE otherwise), and writes the eight gradients.  stats_scratch: 64 bytes of device memory the call overwrites
 * (max|grad_scores|, from which the fp16 modes derive the power-of-two scale of g; 0 or a non-finite maximum: scale 1).
 * Deterministic: fixed reduction orders, no float atomics. */
int mi_concat_mlp_scores_fwd(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* w3, const float* b3, int64_t b_rows, int64_t b,
                             int64_t d_img, int64_t d_txt, int64_t h1, int64_t h2, int precision, int need_grad,
                             float* scores_out /* [b_rows,b] */, void* workspace, size_t workspace_bytes, void* stream);
int mi_concat_mlp_bwd_from_g(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* w3, const float* b3, int64_t b_rows, int64_t b,
                             int64_t d_img, int64_t d_txt, int64_t h1, int64_t h2, int precision,
                             const float* grad_scores /* [b_rows,b] */, mi_stats* stats_scratch /* 64 bytes */,
                             float* grad_x, float* grad_y, float* grad_w1, float* grad_b1, float* grad_w2,
                             float* grad_b2, float* grad_w3, float* grad_b3, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- cross-rank merge of per-rank partial statistics (global-batch negatives) -------- */
/* partials [n_ranks][4] = (neg_max, sum exp(s - neg_max), sum of positives, n_neg as float pair) gathered in
 * rank order; writes the global stats and loss.  Merging in rank order makes every rank compute identical bits. */
int mi_merge_partials(const float* partials, int64_t n_ranks, int64_t n_pos_global, int estimator,
                      float* loss_out, mi_stats* stats, void* stream);

/* ---- per-sample InfoNCE (row-wise and symmetric image-report contrastive loss) ----------------------- */
/* Scores S[i,j] = critic(img_i, txt_j) over a batch of b; a pair i != j with equal study ids is dropped.
 *   r_i = log sum_{j in C_i} exp S[i,j],  C_i = {i} u {j : sid_j != sid_i}      (row LSE, lse_rows)
 *   c_j = log sum_{i in R_j} exp S[i,j],  R_j = {j} u {i : sid_i != sid_j}      (column LSE, lse_cols)
 *   MI_NCE_ROWWISE:   loss = (1/b) sum_i (r_i - S[i,i])                        (image -> report cross-entropy)
 *   MI_NCE_SYMMETRIC: loss = 1/2 (1/b) sum_i (r_i - S[i,i]) + 1/2 (1/b) sum_j (c_j - S[j,j])
 * A row whose only candidate is its own positive contributes 0 (a batch without negatives gives loss 0).  Not the
 * reference's "infonce" estimator (MI_INFONCE: one LSE over every negative pair): a separate family of entry points whose
 * `mode` codes are not estimator codes.  Deterministic: partial records merged in a fixed order, no float atomics.
 * precision: MI_PREC_BF16 / MI_PREC_BF16X3 run the 16-bit GEMM chain where b and the widths are multiples of 8, every
 * other shape and MI_PREC_F32 the generic kernels; MI_PREC_FP8 / F16 / F16X3 are rejected (MI_EINVAL).
 * grad_out may be NULL (dL/dloss = 1); lse_rows / lse_cols ([b], optional) receive r and c. */
#define MI_NCE_ROWWISE 0
#define MI_NCE_SYMMETRIC 1
/* S = (X W) Y^T, or S = X Y^T when w == NULL (projected embeddings, d_img == d_txt).  grad_x, grad_y (and grad_w when
 * w != NULL) all NULL: forward only, no backward launches; otherwise all of them are written. */
size_t mi_nce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_nce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                         int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out, float* lse_rows,
                         float* lse_cols, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                         size_t workspace_bytes, void* stream);
/* S = (X Wg)(Y Wh)^T; wg [d_img, d_proj], wh [d_txt, d_proj].  The four gradients all NULL: forward only. */
size_t mi_nce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision);
int mi_nce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                          int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, const float* grad_out,
                          float* loss_out, float* lse_rows, float* lse_cols, float* grad_x, float* grad_y,
                          float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream);
/* on a caller's fp32 [b, b] score matrix (any critic): forward writes loss_out[0] and the optional lse_rows / lse_cols;
 * backward reads lse_rows (and lse_cols in the symmetric mode) and writes grad_scores = grad_out[0] * dloss/dS */
size_t mi_matrix_nce_workspace_bytes(int64_t b);
int mi_matrix_nce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, float* loss_out, float* lse_rows,
                      float* lse_cols, void* workspace, size_t workspace_bytes, void* stream);
int mi_matrix_nce_bwd(const float* scores, const int64_t* sid, int64_t b, int mode, const float* lse_rows,
                      const float* lse_cols, const float* grad_out, float* grad_scores, void* stream);

/* ---- per-sample InfoNCE on a sharded batch (row blocks, global-batch normalisation) ---------------------- */
/* Rank g of n_ranks owns rows [row_offset, row_offset + b_rows) of the global b x b matrix, row_offset = g * b_rows,
 * b = n_ranks * b_rows: x [b_rows, d_img] and sid_rows [b_rows] are its own rows, y [b, d_txt] and sid_cols [b] every
 * rank's (all-gathered in rank order).  Masking and loss are those above at the global b (weights 1/b).  Per step:
 *   1. *_shard_fwd: the rank's scores, r_i of its rows (lse_rows [b_rows], optional) and its PART, part_out[P] with
 *      P = mi_nce_part_floats(b_rows, b) = 2 b + 2 b_rows floats:
 *        [0, 2b)                   (max, sum exp(S - max)) of column j over this rank's candidate rows, j = 0 .. b-1
 *        [2b, 2b + b_rows)         row terms r_i - S[i, row_offset + i]
 *        [2b + b_rows, 2b + 2 b_rows) the diagonal scores S[i, row_offset + i]
 *      The workspace keeps what the backward needs (operand copies, T, r): pass the SAME workspace to *_shard_bwd.
 *   2. all-gather the parts in rank order -> parts [n_ranks][P]; mi_nce_merge_parts merges every column in rank order
 *      (c_j, lse_cols [b]) and reduces the 2b per-sample terms in a fixed order: every rank computes identical bits, and
 *      n_ranks == 1 gives the bits of mi_nce_*_step.  Its workspace: mi_nce_merge_workspace_bytes(b).
 *   3. *_shard_bwd with the merged lse_cols (may be NULL in MI_NCE_ROWWISE): gradients of grad_out[0] * loss.
 *      grad_x [b_rows, d_img] is complete; grad_y [b, d_txt] and grad_w / grad_wg / grad_wh are this rank's PARTIAL sums
 *      (reduce-scatter grad_y, all-reduce the parameter gradients).
 * Precisions and paths as for mi_nce_*_step (16-bit chain where b_rows, b and the widths are multiples of 8). */
size_t mi_nce_part_floats(int64_t b_rows, int64_t b);
size_t mi_nce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_nce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                              const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                              int64_t d_txt, int mode, int precision, float* part_out, float* lse_rows, void* workspace,
                              size_t workspace_bytes, void* stream);
int mi_nce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                              const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                              int64_t d_txt, int mode, int precision, const float* lse_cols, const float* grad_out,
                              float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t mi_nce_merge_workspace_bytes(int64_t b);
int mi_nce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                       float* lse_cols, void* workspace, size_t workspace_bytes, void* stream);
size_t mi_nce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                              int precision);
int mi_nce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                               const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                               int64_t d_txt, int64_t d_proj, int mode, int precision, float* part_out, float* lse_rows,
                               void* workspace, size_t workspace_bytes, void* stream);
int mi_nce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_rows,
                               const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                               int64_t d_txt, int64_t d_proj, int mode, int precision, const float* lse_cols,
                               const float* grad_out, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- Jensen-Shannon and NWJ bounds ------------------------------------------------------ */
/* The reference's pairs (positives (i, i), negatives i != j with sid_i != sid_j; other pairs dropped), sp(x) = log(1 + e^x):
 *   MI_FDIV_JSD: loss = mean_pos sp(-s) + mean_neg sp(s)                 (Deep InfoMax; -loss + 2 log 2 = JS divergence)
 *   MI_FDIV_NWJ: loss = exp(LSE_neg - log n_neg - 1) - mean_pos s        (NWJ / f-GAN KL; -loss is the NWJ lower bound)
 * A separate family: `mode` codes are not estimator codes.  "jsd" stays finite for any finite scores; NWJ overflows where
 * e^s does (fp32).  No negatives: the loss is NaN.  Deterministic: partial records merged in a fixed order.
 * Every forward writes loss_out[0] and, when terms_out != NULL, terms_out[0] = the positive-pair term and terms_out[1] =
 * the negative-pair term (their sum is the loss):  JSD: mean_pos sp(-s), mean_neg sp(s);  NWJ: -mean_pos s,
 * exp(LSE_neg - log n_neg - 1).  The statistics block (same struct, fields read as follows) is what the backward reads:
 *   lse          NWJ: 1 + logf(n_neg), the normaliser of the DV-form gradient exp(s - lse); JSD: 0
 *   pos_mean     the positive-pair term          reserved0   the negative-pair term
 *   loss_dv, loss_infonce   both the loss        log_n_neg   logf((float)n_neg)
 *   neg_max      NWJ: maximum negative score; JSD: 0          n_neg, n_pos   the pair counts; reserved1..3: 0
 * Backward: grad = grad_out[0] * dloss/ds (grad_out NULL: 1), positives -sigma(-s)/n_pos (JSD) or -1/n_pos (NWJ),
 * negatives sigma(s)/n_neg (JSD) or exp(s - lse) (NWJ), dropped pairs 0. */
#define MI_FDIV_JSD 0
#define MI_FDIV_NWJ 1
/* logits[n] (the reference's [N, 1] mi_output), first pos_size rows positive, the rest negative */
size_t mi_fdiv_bound_workspace_bytes(int64_t n);
int mi_fdiv_bound_fwd(const float* logits, int64_t n, int64_t pos_size, int mode, float* loss_out, float* terms_out,
                      mi_stats* stats, void* workspace, size_t workspace_bytes, void* stream);
int mi_fdiv_bound_bwd(const float* logits, int64_t n, int64_t pos_size, int mode, const mi_stats* stats,
                      const float* grad_out, float* grad_logits, void* stream);
/* a caller's fp32 [b, b] score matrix with study-id masking */
size_t mi_fdiv_matrix_workspace_bytes(int64_t b);
int mi_fdiv_matrix_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, float* loss_out, float* terms_out,
                       mi_stats* stats, void* workspace, size_t workspace_bytes, void* stream);
int mi_fdiv_matrix_bwd(const float* scores, const int64_t* sid, int64_t b, int mode, const mi_stats* stats,
                       const float* grad_out, float* grad_scores, void* stream);
/* Bilinear S = (X W) Y^T (w == NULL: X Y^T, d_img == d_txt) and separable S = (X Wg)(Y Wh)^T critics, whole batch, on the
 * G-materialising GEMM chain (the fused B x B kernel is not used).  stats (optional) receives the block above.  All
 * gradient pointers NULL: forward only; otherwise every one of them is written (gradients of grad_out[0] * loss).
 * precision: MI_PREC_F32 (exact fp32 products), MI_PREC_BF16 / MI_PREC_BF16X3 (16-bit chain where b and the widths are
 * multiples of 8, generic kernels otherwise); MI_PREC_FP8 / F16 / F16X3 are rejected (MI_EINVAL). */
size_t mi_fdiv_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_fdiv_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                          int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out, float* terms_out,
                          mi_stats* stats, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t mi_fdiv_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision);
int mi_fdiv_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                           int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                           const float* grad_out, float* loss_out, float* terms_out, mi_stats* stats, float* grad_x,
                           float* grad_y, float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Concat-MLP critic (make_mlp(d_img + d_txt, [h1, h2])): arguments, row block, precisions and workspace
 * (mi_concat_mlp_workspace_bytes) as mi_concat_mlp_fwd / _bwd.  The forward writes scores_out [b_rows, b], the sign-bit
 * images (need_grad) and *stats; the backward reads them, the same workspace and the same mode.  n_pos of the row block
 * is b (the global batch's positives). */
int mi_fdiv_concat_mlp_fwd(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, const int64_t* sid_rows,
                           const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                           int64_t d_txt, int64_t h1, int64_t h2, int mode, int precision, int need_grad,
                           float* loss_out, float* terms_out, mi_stats* stats, float* scores_out, void* workspace,
                           size_t workspace_bytes, void* stream);
int mi_fdiv_concat_mlp_bwd(const float* x, const float* y, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, const int64_t* sid_rows,
                           const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                           int64_t d_txt, int64_t h1, int64_t h2, int mode, int precision, const mi_stats* stats,
                           const float* grad_out, const float* scores, float* grad_x, float* grad_y, float* grad_w1,
                           float* grad_b1, float* grad_w2, float* grad_b2, float* grad_w3, float* grad_b3,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- image-report retrieval ranks -------------------------------------------------------- */
/* S[i, j] = critic(img_i, txt_j) over b pairs, positives (i, i); a pair i != j with sid_i == sid_j is dropped (neither a
 * hit nor a miss), as everywhere above:
 *   rank_i2t[i] = #{ j : sid_j != sid_i and S[i, j] > S[i, i] }      image -> report
 *   rank_t2i[j] = #{ i : sid_i != sid_j and S[i, j] > S[j, j] }      report -> image
 * 0-based int32 [b]; strictly greater, so a tie counts for the true pair; every id equal: all zeros.  recall@K is the
 * mean of rank < K.  Integer counts: exact and identical from call to call.  rank_i2t and rank_t2i may each be NULL (one
 * direction alone); both NULL is MI_EINVAL.  Not an estimator: no mode, no loss, no gradients. */
/* a caller's fp32 [b, b] score matrix (any critic); no workspace */
int mi_rank_matrix(const float* scores, const int64_t* sid, int64_t b, int32_t* rank_i2t, int32_t* rank_t2i, void* stream);
/* Bilinear S = (X W) Y^T (w == NULL: X Y^T, d_img == d_txt) and separable S = (X Wg)(Y Wh)^T critics on the forward half
 * of the GEMM chain of mi_nce_*_step: prep and T = X W, the diagonal S[i, i] from the score GEMM's own operands (bf16:
 * bf16 T and Y, fp32 accumulation; bf16x3: the split parts), then the score sweep, whose epilogue counts per 64 x 64 tile
 * and adds the counts to the ranks.  No score matrix, G or per-tile buffer: the workspace grows linearly in b.
 * diag_out (optional, [b]) receives S[i, i].  precision: MI_PREC_F32 (exact fp32 products), MI_PREC_BF16 /
 * MI_PREC_BF16X3 (16-bit chain where b and the widths are multiples of 8, generic kernels otherwise); MI_PREC_FP8 / F16
 * / F16X3 are rejected (MI_EINVAL). */
size_t mi_rank_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_rank_bilinear(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                     int64_t d_txt, int precision, int32_t* rank_i2t, int32_t* rank_t2i, float* diag_out, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t mi_rank_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision);
int mi_rank_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                      int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, int32_t* rank_i2t, int32_t* rank_t2i,
                      float* diag_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- top-k retrieval over a gallery ------------------------------------------------------ */
/* Queries q and candidates g with scores S[q, g]; with ids, a candidate whose id equals the query's is excluded.  The
 * result of a query is its first k candidates in the total order "score descending, then candidate index ascending"
 * (-0.0 counts as +0.0): idx int32 [n_q, k] and val float32 [n_q, k], val = the kernel's own fp32 score of idx.  Where
 * fewer than k candidates remain the tail is idx = -1, val = -inf.  The order is total, so the result is unique and
 * identical from call to call; NaN scores carry no ordering promise (indices stay in range).  The two id pointers are
 * both NULL (nothing excluded) or both given.  k in [1, MI_TOPK_MAX_K], every size below 2^31, else MI_EINVAL.  Not an
 * estimator: no mode, no loss, no gradients. */
#define MI_TOPK_MAX_K 32
/* a caller's fp32 [n_rows, n_cols] score matrix.  axis 0: each row's top-k columns (idx, val [n_rows, k], sid_rows the
 * queries' ids); axis 1: each column's top-k rows (idx, val [n_cols, k], sid_cols the queries' ids). */
size_t mi_topk_matrix_workspace_bytes(int64_t n_rows, int64_t n_cols, int k, int axis);
int mi_topk_matrix(const float* scores, int64_t n_rows, int64_t n_cols, const int64_t* sid_rows, const int64_t* sid_cols,
                   int k, int axis, int32_t* idx, float* val, void* workspace, size_t workspace_bytes, void* stream);
/* Bilinear S = (X W) Y^T (w == NULL: X Y^T, d_img == d_txt) of x [n_img, d_img] against y [n_txt, d_txt], n_img != n_txt
 * allowed, on the forward half of the GEMM chain as mi_rank_bilinear: prep and T = X W once, then one score sweep per
 * direction whose epilogue inserts into per-query key lists (image -> report: idx_i2t / val_i2t [n_img, k] index the
 * reports; report -> image: idx_t2i / val_t2i [n_txt, k] index the images), then a small sort.  A direction whose two
 * pointers are NULL is skipped; both directions NULL is MI_EINVAL.  No score matrix and no per-tile buffer: the workspace
 * is the forward half's operand copies and T plus 8 (n_img + n_txt) k bytes of lists.  precision: MI_PREC_F32 (exact
 * fp32 products), MI_PREC_BF16 / MI_PREC_BF16X3 (16-bit chain where n_img, n_txt and the widths are multiples of 8,
 * generic kernels otherwise); MI_PREC_FP8 / F16 / F16X3 are rejected (MI_EINVAL). */
size_t mi_topk_bilinear_workspace_bytes(int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int precision, int k);
int mi_topk_bilinear(const float* x, const float* y, const float* w, const int64_t* sid_img, const int64_t* sid_txt,
                     int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int precision, int k, int32_t* idx_i2t,
                     float* val_i2t, int32_t* idx_t2i, float* val_t2i, void* workspace, size_t workspace_bytes,
                     void* stream);
/* separable S = (X Wg)(Y Wh)^T: projects first, then the w == NULL form on the projections, as mi_rank_separable */
size_t mi_topk_separable_workspace_bytes(int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                         int precision, int k);
int mi_topk_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid_img,
                      const int64_t* sid_txt, int64_t n_img, int64_t n_txt, int64_t d_img, int64_t d_txt, int64_t d_proj,
                      int precision, int k, int32_t* idx_i2t, float* val_i2t, int32_t* idx_t2i, float* val_t2i,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- hard-negative InfoNCE ---------------------------------------------------------------- */
/* The per-sample InfoNCE above on each query's top-k negatives.  H_i = the image -> report list of mi_topk_* for row i of
 * the square batch with sid on both sides (the first min(k, #negatives) negatives in "score descending, index
 * ascending"), H'_j = the report -> image list of column j:
 *   r_i = log(exp S[i, i] + sum_{j in H_i} exp S[i, j]),   c_j = log(exp S[j, j] + sum_{i in H'_j} exp S[i, j])
 *   MI_NCE_ROWWISE:   L = (1/b) sum_i (r_i - S[i, i])
 *   MI_NCE_SYMMETRIC: half of that plus half of (1/b) sum_j (c_j - S[j, j])
 * The selection is a constant of the gradient (its derivative almost everywhere): dL/dS is nonzero exactly on the
 * diagonal and at the listed indices.  A row or column without negatives contributes exactly 0; k >= every row's (and
 * column's) negative count gives the loss of mi_nce_*.  A TRAINING LOSS, NOT AN MI BOUND: the candidates were chosen by
 * score, so log(k + 1) - L bounds nothing.  Deterministic: integer selection, fixed-order reductions, no float atomics.
 * k in [1, MI_TOPK_MAX_K]; precisions and paths as mi_nce_*_step (MI_PREC_FP8 / F16 / F16X3: MI_EINVAL).
 * Outputs: loss_out [1]; optional lse_rows [b], idx_rows int32 [b, k] (H_i, tail -1); in the symmetric mode also the
 * optional lse_cols [b], idx_cols [b, k] (H'_j) -- MI_NCE_ROWWISE takes no column side and leaves both untouched.
 * Gradient pointers all NULL: the forward launches only, and the workspace query with with_grads == 0 (linear in b: no
 * G) suffices; otherwise every gradient is written (of grad_out[0] * loss; grad_out NULL: 1) and the workspace is that of
 * with_grads != 0 (the nce step's plus the lists: 8 k 2b bytes of keys, idx / val, O(b) floats). */
size_t mi_hardnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int k, int with_grads);
int mi_hardnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                             int64_t d_txt, int mode, int precision, int k, const float* grad_out, float* loss_out,
                             float* lse_rows, float* lse_cols, int32_t* idx_rows, int32_t* idx_cols, float* grad_x,
                             float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes, void* stream);
size_t mi_hardnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, int k,
                                            int with_grads);
int mi_hardnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                              int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, int k,
                              const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, int32_t* idx_rows,
                              int32_t* idx_cols, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                              void* workspace, size_t workspace_bytes, void* stream);
/* on a caller's fp32 [b, b] score matrix (any critic): the lists by mi_topk_matrix's kernel on both axes.  The backward
 * reads the forward's idx_rows and lse_rows (and idx_cols, lse_cols in the symmetric mode) and writes the dense
 * grad_scores [b, b] = grad_out[0] * dloss/dS, zero outside the lists and the diagonal. */
size_t mi_matrix_hardnce_workspace_bytes(int64_t b, int k);
int mi_matrix_hardnce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, int k, float* loss_out,
                          float* lse_rows, float* lse_cols, int32_t* idx_rows, int32_t* idx_cols, void* workspace,
                          size_t workspace_bytes, void* stream);
int mi_matrix_hardnce_bwd(const float* scores, int64_t b, int mode, int k, const int32_t* idx_rows, const int32_t* idx_cols,
                          const float* lse_rows, const float* lse_cols, const float* grad_out, float* grad_scores,
                          void* stream);

/* Per-sample InfoNCE against a memory bank of past embeddings.  Batch x [b, d_img], y [b, d_txt],
 * ids sid [b]; bank bank_x [m, d_img], bank_y [m, d_txt], ids bank_sid [m], m >= 1.  The bank is a constant: it gets no
 * gradient.  S[i, j] = critic(img_i, txt_j) with the current parameters; index b + k is bank entry k on either side.
 *   C_i = {i} u {j < b : sid_j != sid_i} u {b + k : bank_sid_k != sid_i},  r_i = log sum_{j in C_i} exp S[i, j]
 *   R_j = {j} u {i < b : sid_i != sid_j} u {b + k : bank_sid_k != sid_j},  c_j = log sum_{i in R_j} exp S[i, j]
 *   MI_NCE_ROWWISE:   loss = (1/b) sum_i (r_i - S[i,i])                  (reads bank_y only; bank_x may be NULL)
 *   MI_NCE_SYMMETRIC: loss = 1/2 (1/b) sum_i (r_i - S[i,i]) + 1/2 (1/b) sum_j (c_j - S[j,j])
 * A bank entry of the query's own study is never a candidate; bank entries have no row or column terms of their own; a
 * row (column) whose only candidate is its positive contributes exactly 0.  With unique ids and bank entries drawn from
 * the marginal, log(b + m) - loss(rowwise) is the InfoNCE bound with b + m candidates (ceiling log(b + m)); embeddings
 * of a training queue are stale, then it is a training loss with that ceiling.
 * Conventions of mi_nce_*_step: w == NULL is S = X Y^T (d_img == d_txt); all gradients NULL runs the forward launches
 * alone; lse_rows / lse_cols are [b] and optional, lse_cols is not written in the row-wise mode; grad_out scales every
 * gradient.  Bilinear: grad_w includes bank_x^T (G_left Y), grad_y includes G_left^T (bank_x W).  Separable: the bank's
 * projections are recomputed in the call and grad_wg / grad_wh include the bank rows' share.
 * precision: MI_PREC_F32 / BF16 / BF16X3; the 16-bit chain where b, m and the widths are multiples of 8, else the generic
 * kernels; MI_PREC_FP8 / F16 / F16X3 give MI_EINVAL.  MI_EINVAL also for null required pointers, b < 1, m < 1, bank_x ==
 * NULL in the symmetric mode, an unknown mode, a partial gradient set, b + m >= 2^31; MI_EWORKSPACE for a short workspace.
 * The workspace holds G [b, b + m] (and [m, b] in the symmetric mode) in the chain's G type; everything else is linear in
 * b + m.  No float atomics: two calls give identical bits. */
size_t mi_banknce_bilinear_workspace_bytes(int64_t b, int64_t m, int64_t d_img, int64_t d_txt, int mode, int precision,
                                           int with_grads);
int mi_banknce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, const float* bank_x,
                             const float* bank_y, const int64_t* bank_sid, int64_t b, int64_t m, int64_t d_img,
                             int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out,
                             float* lse_rows, float* lse_cols, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                             size_t workspace_bytes, void* stream);
size_t mi_banknce_separable_workspace_bytes(int64_t b, int64_t m, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                            int precision, int with_grads);
int mi_banknce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                              const float* bank_x, const float* bank_y, const int64_t* bank_sid, int64_t b, int64_t m,
                              int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, const float* grad_out,
                              float* loss_out, float* lse_rows, float* lse_cols, float* grad_x, float* grad_y,
                              float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream);

/* ---- study-positive InfoNCE ---------------------------------------------------------------- */
/* The per-sample InfoNCE with every same-study pair as a positive (multi-positive InfoNCE: SupCon's L_out, UniCL).
 * Batch x [b, d_img], y [b, d_txt], id codes sid [b], S[i, j] = critic(img_i, txt_j):
 *   P_i = {j : sid_j == sid_i} (contains i),  n_i = |P_i| >= 1
 *   r_i = log sum_{j < b} exp S[i, j],  c_j = log sum_{i < b} exp S[i, j]                     (nothing is masked)
 *   row term t_i = r_i - (1/n_i) sum_{p in P_i} S[i, p],  column term t'_j = c_j - (1/n_j) sum_{p in P_j} S[p, j]
 *   MI_NCE_ROWWISE:   L = (1/b) sum_i t_i
 *   MI_NCE_SYMMETRIC: L = 1/2 (1/b) sum_i t_i + 1/2 (1/b) sum_j t'_j
 *   dL/dS[i, j] = w_r exp(S[i,j] - r_i) + w_c exp(S[i,j] - c_j) - (w_r + w_c) 1[sid_i == sid_j] / n_i,
 *   (w_r, w_c) = (1/b, 0) or (1/(2b), 1/(2b)); each row's share of dL/dS sums to zero.
 * With unique ids this IS the loss of mi_nce_*: same r, c, loss and gradients.  With duplicates it differs from it in two
 * ways: same-study pairs enter the denominators, and they share the positive weight.  With all ids equal t_i = r_i -
 * mean_j S[i, j] >= log b: the loss is not zero.  b == 1 gives loss exactly 0.0 and exact-zero gradients.
 * A TRAINING LOSS, NOT AN MI BOUND: log b - L bounds nothing once some n_i > 1; `mode` codes are those of mi_nce_*, not
 * estimator codes.  Only this averaged-outside form exists (in the image -> report direction the positives of a row are
 * the same report repeated, so the log-of-sum-over-positives form gains nothing).  Row blocks of a sharded batch: the
 * mi_posnce_*_shard_* calls below.
 * Outputs: loss_out [1]; optional lse_rows [b], lse_cols [b] (r and c, both written in either mode), n_pos_out int32 [b]
 * (n_i).  grad_out may be NULL (1).  Gradient pointers all NULL: the forward launches only, and the workspace query with
 * with_grads == 0 (no G) suffices; otherwise every gradient is written and the workspace is that of with_grads != 0.
 * w == NULL is S = X Y^T (d_img == d_txt, no grad_w).  precision: MI_PREC_BF16 / BF16X3 run the 16-bit GEMM chain where b
 * and the widths are multiples of 8, every other shape and MI_PREC_F32 the generic kernels; MI_PREC_FP8 / F16 / F16X3:
 * MI_EINVAL.  MI_EINVAL also for null required pointers, sizes < 1, b >= 2^31, an unknown mode, a partial gradient set;
 * MI_EWORKSPACE for a short workspace.  Deterministic: records merged in tile order, no float atomics. */
size_t mi_posnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int with_grads);
int mi_posnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                            int64_t d_txt, int mode, int precision, const float* grad_out, float* loss_out,
                            float* lse_rows, float* lse_cols, int32_t* n_pos_out, float* grad_x, float* grad_y,
                            float* grad_w, void* workspace, size_t workspace_bytes, void* stream);
/* S = (X Wg)(Y Wh)^T: projects, runs the w == NULL form on the projections, projects the gradients back */
size_t mi_posnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision,
                                           int with_grads);
int mi_posnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid,
                             int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                             const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, int32_t* n_pos_out,
                             float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                             size_t workspace_bytes, void* stream);
/* on a caller's fp32 [b, b] score matrix (any critic, exact expf): the forward writes loss_out[0] and the optional
 * lse_rows / lse_cols / n_pos; the backward reads lse_rows, n_pos (and lse_cols in the symmetric mode) and writes the
 * dense grad_scores [b, b] = grad_out[0] * dloss/dS */
size_t mi_matrix_posnce_workspace_bytes(int64_t b);
int mi_matrix_posnce_fwd(const float* scores, const int64_t* sid, int64_t b, int mode, float* loss_out, float* lse_rows,
                         float* lse_cols, int32_t* n_pos, void* workspace, size_t workspace_bytes, void* stream);
int mi_matrix_posnce_bwd(const float* scores, const int64_t* sid, int64_t b, int mode, const float* lse_rows,
                         const float* lse_cols, const int32_t* n_pos, const float* grad_out, float* grad_scores,
                         void* stream);

/* ---- study-positive InfoNCE on a sharded batch (row blocks, global-batch normalisation) ----------------------------- */
/* The convention of mi_nce_*_shard_*: rank g of n_ranks owns rows [row_offset, row_offset + b_rows) of the global b x b
 * matrix, row_offset = g * b_rows, b = n_ranks * b_rows; x [b_rows, d_img] and sid_rows [b_rows] are its own rows, y [b,
 * d_txt] and sid_cols [b] every rank's (all-gathered in rank order).  Positives are sid_rows[i] == sid_cols[j]; the loss
 * is the one above at the global b (weights 1/b).  Per step:
 *   1. *_shard_fwd: the rank's scores; r_i, n_i and the row term t_i of its rows are complete on this rank (a row has
 *      all of its columns): optional lse_rows [b_rows], n_pos_out int32 [b_rows].  Its PART, part_out[P] with
 *      P = mi_posnce_part_floats(b_rows, b) = 3 b + 2 b_rows floats:
 *        [0, 2b)                        (max, sum exp(S - max)) of column j over this rank's rows, j = 0 .. b-1
 *        [2b, 3b)                       sum of S[p, j] over this rank's rows p with sid_p == sid_j
 *        [3b, 3b + b_rows)              row terms t_i
 *        [3b + b_rows, 3b + 2 b_rows)   n_i as floats (exact: b < 2^24 is required); n_i is also the positive count of
 *                                       column row_offset + i, the same sample
 *      The workspace keeps what the backward needs (operand copies, T, r, 1/n): pass the SAME workspace to *_shard_bwd.
 *   2. all-gather the parts in rank order -> parts [n_ranks][P]; mi_posnce_merge_parts walks every column's partials in
 *      rank order from an empty start (c_j -> lse_cols [b], the column terms) and reduces the 2b per-sample terms in a
 *      fixed order: every rank computes identical bits, and n_ranks == 1 gives the bits of mi_posnce_*_step.  Its
 *      workspace: mi_posnce_merge_workspace_bytes(b).
 *   3. *_shard_bwd with the merged lse_cols (may be NULL in MI_NCE_ROWWISE): gradients of grad_out[0] * loss (grad_out
 *      may be NULL: 1).  grad_x [b_rows, d_img] is complete; grad_y [b, d_txt] and grad_w / grad_wg / grad_wh are this
 *      rank's PARTIAL sums (reduce-scatter grad_y, all-reduce the parameter gradients).
 * Precisions and paths as mi_posnce_*_step (16-bit chain where b_rows, b and the widths are multiples of 8).  MI_EINVAL,
 * before anything touches the device: null required pointers, sizes < 1, b_rows > b, a row block outside [0, b),
 * b >= 2^24, an unknown mode, MI_PREC_FP8 / F16 / F16X3, w == NULL with d_img != d_txt, w without grad_w (or grad_w
 * without w), the symmetric backward without lse_cols, b != n_ranks * b_rows in the merge.  No float atomics. */
size_t mi_posnce_part_floats(int64_t b_rows, int64_t b);
size_t mi_posnce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_posnce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                                 const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                 int64_t d_txt, int mode, int precision, float* part_out, float* lse_rows,
                                 int32_t* n_pos_out, void* workspace, size_t workspace_bytes, void* stream);
int mi_posnce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* sid_rows,
                                 const int64_t* sid_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                 int64_t d_txt, int mode, int precision, const float* lse_cols, const float* grad_out,
                                 float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t mi_posnce_merge_workspace_bytes(int64_t b);
int mi_posnce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                          float* lse_cols, void* workspace, size_t workspace_bytes, void* stream);
/* the separable form projects A = X Wg for the rank's rows and C = Y Wh for all b text rows */
size_t mi_posnce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                                 int precision);
int mi_posnce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh,
                                  const int64_t* sid_rows, const int64_t* sid_cols, int64_t b_rows, int64_t b,
                                  int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                                  float* part_out, float* lse_rows, int32_t* n_pos_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
int mi_posnce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh,
                                  const int64_t* sid_rows, const int64_t* sid_cols, int64_t b_rows, int64_t b,
                                  int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision,
                                  const float* lse_cols, const float* grad_out, float* grad_x, float* grad_y,
                                  float* grad_wg, float* grad_wh, void* workspace, size_t workspace_bytes, void* stream);

/* ---- soft-target InfoNCE from finding-label bit masks --------------------------------------- */
/* The row-wise / symmetric InfoNCE with soft targets: the target distribution of row i puts weight on every report in
 * proportion to how similar its finding set is to that of image i (SoftCLIP, label-aware contrast).  Batch x [b, d_img],
 * y [b, d_txt], one label mask per sample label_mask [b] (int64; the low MI_SOFTNCE_MAX_LABELS bits are a multi-hot set
 * of findings; bit 63 cannot be checked on the host and is IGNORED -- masked off -- on the device), floats tau > 0 and
 * mix in [0, 1]; no study ids.  S[i, j] = critic(img_i, txt_j):
 *   n_i   = popcount(lab_i)
 *   a_ij  = popcount(lab_i & lab_j) / sqrt(n_i n_j)   (0 where n_i n_j = 0);  a_ii := 1 always
 *   k_ij  = exp((a_ij - 1) / tau)                      (<= 1, k_ii = 1, k_ij == k_ji bit for bit)
 *   z_i   = sum_j k_ij                                 (>= 1; serves rows and, k being symmetric, columns)
 *   qr_ij = (1 - mix) delta_ij + mix k_ij / z_i        qc_ij = (1 - mix) delta_ij + mix k_ij / z_j
 *   r_i = log sum_{j < b} exp S[i, j],  c_j = log sum_{i < b} exp S[i, j]                     (nothing is masked)
 *   row term t_i = r_i - sum_j qr_ij S[i, j],  column term t'_j = c_j - sum_i qc_ij S[i, j]
 *   MI_NCE_ROWWISE:   L = (1/b) sum_i t_i
 *   MI_NCE_SYMMETRIC: L = 1/2 (1/b) sum_i t_i + 1/2 (1/b) sum_j t'_j
 *   dL/dS[i, j] = w_r (exp(S[i,j] - r_i) - qr_ij) + w_c (exp(S[i,j] - c_j) - qc_ij),
 *   (w_r, w_c) = (1/b, 0) or (1/(2b), 1/(2b)); each row's share of dL/dS sums to zero.
 * a_ij is formed in fp32 as popcount * (rs_i * rs_j), rs = 1 / sqrt(n).  mix = 0 IS the loss of mi_nce_* on unique ids.
 * Every mask equal and mix = 1: the loss of mi_posnce_* with all ids equal.  One distinct bit per study, mix = 1 and a
 * small tau (0.02): the loss of mi_posnce_* with those ids.  All masks zero: uniform smoothing of weight exp(-1/tau) off
 * the diagonal.  b == 1 gives loss exactly 0.0 and exact-zero gradients.
 * A TRAINING LOSS, NOT AN MI BOUND: log b - L bounds nothing once mix > 0; `mode` codes are those of mi_nce_*, not
 * estimator codes.  Row blocks of a sharded batch: the mi_softnce_*_shard_* calls below.  No b x b target matrix exists:
 * both GEMM epilogues recompute
 * the pair weights from the masks and the per-sample z and rs that one launch ahead of the score GEMM writes.
 * Outputs: loss_out [1]; optional lse_rows [b], lse_cols [b] (r and c, both written in either mode), target_norm [b]
 * (z).  grad_out may be NULL (1).  Gradient pointers all NULL: the forward launches only, and the workspace query with
 * with_grads == 0 (no G) suffices; otherwise every gradient is written and the workspace is that of with_grads != 0.
 * w == NULL is S = X Y^T (d_img == d_txt, no grad_w).  precision: MI_PREC_BF16 / BF16X3 run the 16-bit GEMM chain where b
 * and the widths are multiples of 8, every other shape and MI_PREC_F32 the generic kernels; MI_PREC_FP8 / F16 / F16X3:
 * MI_EINVAL.  MI_EINVAL also for null required pointers, sizes < 1, b >= 2^31, an unknown mode, a partial gradient set,
 * tau not finite or <= 0, mix outside [0, 1] or NaN; MI_EWORKSPACE for a short workspace; all before anything touches
 * the device.  Deterministic: z summed and records merged in fixed order, no float atomics. */
#define MI_SOFTNCE_MAX_LABELS 63
size_t mi_softnce_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision, int with_grads);
int mi_softnce_bilinear_step(const float* x, const float* y, const float* w, const int64_t* label_mask, int64_t b,
                             int64_t d_img, int64_t d_txt, int mode, int precision, float tau, float mix,
                             const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols, float* target_norm,
                             float* grad_x, float* grad_y, float* grad_w, void* workspace, size_t workspace_bytes,
                             void* stream);
/* S = (X Wg)(Y Wh)^T: projects, runs the w == NULL form on the projections, projects the gradients back */
size_t mi_softnce_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision,
                                            int with_grads);
int mi_softnce_separable_step(const float* x, const float* y, const float* wg, const float* wh, const int64_t* label_mask,
                              int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode, int precision, float tau,
                              float mix, const float* grad_out, float* loss_out, float* lse_rows, float* lse_cols,
                              float* target_norm, float* grad_x, float* grad_y, float* grad_wg, float* grad_wh,
                              void* workspace, size_t workspace_bytes, void* stream);
/* on a caller's fp32 [b, b] score matrix (any critic, exact expf): the forward writes loss_out[0] and the optional
 * lse_rows / lse_cols / target_norm; the backward reads lse_rows, target_norm (required: MI_EINVAL without it; and
 * lse_cols in the symmetric mode) and writes the dense grad_scores [b, b] = grad_out[0] * dloss/dS */
size_t mi_matrix_softnce_workspace_bytes(int64_t b);
int mi_matrix_softnce_fwd(const float* scores, const int64_t* label_mask, int64_t b, int mode, float tau, float mix,
                          float* loss_out, float* lse_rows, float* lse_cols, float* target_norm, void* workspace,
                          size_t workspace_bytes, void* stream);
int mi_matrix_softnce_bwd(const float* scores, const int64_t* label_mask, int64_t b, int mode, float tau, float mix,
                          const float* lse_rows, const float* lse_cols, const float* target_norm, const float* grad_out,
                          float* grad_scores, void* stream);

/* ---- soft-target InfoNCE on a sharded batch (row blocks, global-batch normalisation) ------------------------------- */
/* The convention of mi_nce_*_shard_*: rank g of n_ranks owns rows [row_offset, row_offset + b_rows) of the global b x b
 * matrix, row_offset = g * b_rows, b = n_ranks * b_rows; x [b_rows, d_img] and label_rows [b_rows] are its own rows, y
 * [b, d_txt] and label_cols [b] every rank's (all-gathered in rank order).  The loss is the one above at the global b:
 * z_i sums over all b samples, the diagonal rule a_ii := 1 holds where row_offset + i == j.  Per step:
 *   1. *_shard_fwd: z, 1/z and rs of ALL b samples from label_cols (every rank: same inputs, same order, same bits; row
 *      weights take z of the row, column weights z of the column), then the rank's scores.  r_i and the row term t_i of
 *      its rows are complete on this rank: optional lse_rows [b_rows], target_norm [b_rows] (z of the rank's rows).  Its
 *      PART, part_out[P] with P = mi_softnce_part_floats(b_rows, b) = 3 b + b_rows floats:
 *        [0, 2b)               (max, sum exp(S - max)) of column j over this rank's rows, j = 0 .. b-1
 *        [2b, 3b)              sum of qc_ij S[i, j] over this rank's rows i
 *        [3b, 3b + b_rows)     row terms t_i
 *      The workspace keeps what the backward needs (operand copies, T, r, 1/z, rs): pass the SAME workspace to
 *      *_shard_bwd.
 *   2. all-gather the parts in rank order -> parts [n_ranks][P]; mi_softnce_merge_parts walks every column's partials in
 *      rank order from an empty start (c_j -> lse_cols [b], the column terms) and reduces the 2b per-sample terms in a
 *      fixed order: every rank computes identical bits, and n_ranks == 1 gives the bits of mi_softnce_*_step.  Its
 *      workspace: mi_softnce_merge_workspace_bytes(b).
 *   3. *_shard_bwd with the same masks, tau, mix and the merged lse_cols (may be NULL in MI_NCE_ROWWISE): gradients of
 *      grad_out[0] * loss (grad_out may be NULL: 1).  grad_x [b_rows, d_img] is complete; grad_y [b, d_txt] and grad_w /
 *      grad_wg / grad_wh are this rank's PARTIAL sums (reduce-scatter grad_y, all-reduce the parameter gradients).
 * Precisions and paths as mi_softnce_*_step (16-bit chain where b_rows, b and the widths are multiples of 8).  MI_EINVAL,
 * before anything touches the device: null required pointers, sizes < 1, b_rows > b, a row block outside [0, b),
 * b >= 2^24 (the limit of the study-positive parts, kept for both), an unknown mode, tau not finite or <= 0, mix outside
 * [0, 1] or NaN, MI_PREC_FP8 / F16 / F16X3, w == NULL with d_img != d_txt, w without grad_w (or grad_w without w), the
 * symmetric backward without lse_cols, b != n_ranks * b_rows in the merge.  No float atomics. */
size_t mi_softnce_part_floats(int64_t b_rows, int64_t b);
size_t mi_softnce_bilinear_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_softnce_bilinear_shard_fwd(const float* x, const float* y, const float* w, const int64_t* label_rows,
                                  const int64_t* label_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                  int64_t d_txt, int mode, int precision, float tau, float mix, float* part_out,
                                  float* lse_rows, float* target_norm, void* workspace, size_t workspace_bytes,
                                  void* stream);
int mi_softnce_bilinear_shard_bwd(const float* x, const float* y, const float* w, const int64_t* label_rows,
                                  const int64_t* label_cols, int64_t b_rows, int64_t b, int64_t row_offset, int64_t d_img,
                                  int64_t d_txt, int mode, int precision, float tau, float mix, const float* lse_cols,
                                  const float* grad_out, float* grad_x, float* grad_y, float* grad_w, void* workspace,
                                  size_t workspace_bytes, void* stream);
size_t mi_softnce_merge_workspace_bytes(int64_t b);
int mi_softnce_merge_parts(const float* parts, int64_t n_ranks, int64_t b_rows, int64_t b, int mode, float* loss_out,
                           float* lse_cols, void* workspace, size_t workspace_bytes, void* stream);
/* the separable form projects A = X Wg for the rank's rows and C = Y Wh for all b text rows */
size_t mi_softnce_separable_shard_workspace_bytes(int64_t b_rows, int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj,
                                                  int precision);
int mi_softnce_separable_shard_fwd(const float* x, const float* y, const float* wg, const float* wh,
                                   const int64_t* label_rows, const int64_t* label_cols, int64_t b_rows, int64_t b,
                                   int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                   int precision, float tau, float mix, float* part_out, float* lse_rows,
                                   float* target_norm, void* workspace, size_t workspace_bytes, void* stream);
int mi_softnce_separable_shard_bwd(const float* x, const float* y, const float* wg, const float* wh,
                                   const int64_t* label_rows, const int64_t* label_cols, int64_t b_rows, int64_t b,
                                   int64_t row_offset, int64_t d_img, int64_t d_txt, int64_t d_proj, int mode,
                                   int precision, float tau, float mix, const float* lse_cols, const float* grad_out,
                                   float* grad_x, float* grad_y, float* grad_wg, float* grad_wh, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- MI estimates from one forward sweep -------------------------------------------------- */
/* How much mutual information a trained critic has found on a batch: every bound of the package and SMILE (Song & Ermon
 * 2020: DV with the negatives' scores clipped to [-tau, tau]) from ONE pass over S[i, j] = critic(img_i, txt_j).  Pairs as
 * everywhere above: n_pos = b positives (i, i), n_neg negatives i != j with sid_i != sid_j, equal-id off-diagonal pairs
 * dropped.  sp(x) = log(1 + e^x).  ESTIMATES, not losses: higher means more MI, in nats.  est_out [MI_EST_FLOATS], device:
 *   MI_EST_DV         mean_pos s - (LSE_neg s - log n_neg)
 *   MI_EST_NWJ        mean_pos s - exp(LSE_neg s - log n_neg - 1)
 *   MI_EST_JSD        -(mean_pos sp(-s) + mean_neg sp(s))                      (+ 2 log 2: the JS divergence)
 *   MI_EST_NCE_I2T    (1/b) sum_i (S_ii - r_i + log |C_i|)                     r_i, C_i of mi_nce_* above
 *   MI_EST_NCE_T2I    (1/b) sum_j (S_jj - c_j + log |R_j|)                     |C_i| = |R_i| = b + 1 - #{j : sid_j == sid_i}
 *   MI_EST_POS_MEAN   mean_pos s          MI_EST_NEG_MEAN   mean_neg s          MI_EST_LOG_N_NEG   logf((float)n_neg)
 *   MI_EST_SMILE + k  mean_pos s - (log sum_neg exp(clip(s, -tau_k, tau_k)) - log n_neg)   for k < n_tau, NaN for k >= n_tau
 * With unique ids nce_i2t = log b - (the row-wise loss of mi_nce_*); tau >= max |s_neg| makes SMILE equal DV.  Without
 * negatives (every id equal, b == 1) dv, nwj, jsd, neg_mean and smile are NaN, log_n_neg is -inf and nce_* is exactly 0.
 * taus_host is a HOST array of n_tau clips, read during the call and copied by value into the kernel arguments (NULL
 * allowed with n_tau == 0).  n_tau in [0, MI_EST_MAX_TAUS]; every tau finite, 0 < tau <= 40: the terms exp(clip(s)) of
 * the clipped sum then lie in [e^-40, e^40], normal fp32 numbers whose sum over fewer than 2^62 pairs stays finite, so it
 * needs no running maximum.
 * Forward only: no gradients, no mode, not an estimator of the training entry points.  Every one of the MI_EST_FLOATS
 * outputs is written.  Fixed-order reductions, integer counts (64-bit in total), no float atomics: identical bits from
 * call to call.  MI_EINVAL before anything touches the device: null required pointers, sizes < 1, b >= 2^31, n_tau or a
 * tau out of range, MI_PREC_FP8 / F16 / F16X3, w == NULL with d_img != d_txt; MI_EWORKSPACE: workspace too small. */
#define MI_EST_DV 0
#define MI_EST_NWJ 1
#define MI_EST_JSD 2
#define MI_EST_NCE_I2T 3
#define MI_EST_NCE_T2I 4
#define MI_EST_POS_MEAN 5
#define MI_EST_NEG_MEAN 6
#define MI_EST_LOG_N_NEG 7
#define MI_EST_SMILE 8
#define MI_EST_MAX_TAUS 4
#define MI_EST_FLOATS 12
/* a caller's fp32 [b, b] score matrix (any critic): one wave per 64 x 64 tile, exact expf; the workspace holds the tile
 * and row / column records, 16 b ceil(b / 64) + 48 ceil(b / 64)^2 bytes and O(b) floats */
size_t mi_estimates_matrix_workspace_bytes(int64_t b);
int mi_estimates_matrix(const float* scores, const int64_t* sid, int64_t b, const float* taus_host, int n_tau,
                        float* est_out, void* workspace, size_t workspace_bytes, void* stream);
/* Bilinear S = (X W) Y^T (w == NULL: X Y^T, d_img == d_txt) on the forward half of the GEMM chain, as mi_rank_bilinear:
 * prep and T = X W, the score sweep with the statistics epilogue, merge, finalize.  The workspace is the forward half's
 * operand copies and T plus the records of the matrix call: no G, no G^T, no b x b float buffer.  Precisions and paths as
 * mi_rank_*: MI_PREC_F32 (exact fp32 products), MI_PREC_BF16 / MI_PREC_BF16X3 (16-bit chain where b and the widths are
 * multiples of 8, generic kernels otherwise). */
size_t mi_estimates_bilinear_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int precision);
int mi_estimates_bilinear(const float* x, const float* y, const float* w, const int64_t* sid, int64_t b, int64_t d_img,
                          int64_t d_txt, int precision, const float* taus_host, int n_tau, float* est_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* separable S = (X Wg)(Y Wh)^T: projects first, then the w == NULL form on the projections, as mi_rank_separable */
size_t mi_estimates_separable_workspace_bytes(int64_t b, int64_t d_img, int64_t d_txt, int64_t d_proj, int precision);
int mi_estimates_separable(const float* x, const float* y, const float* wg, const float* wh, const int64_t* sid, int64_t b,
                           int64_t d_img, int64_t d_txt, int64_t d_proj, int precision, const float* taus_host, int n_tau,
                           float* est_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_CRITIC_H */
