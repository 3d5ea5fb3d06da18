"""Study-positive InfoNCE: the per-sample image-report contrastive loss with every same-study pair as a positive
(the multi-positive InfoNCE of SupCon -- its "L_out" form -- and UniCL).

The dataset pairs every image with the report of its study, and a study usually has several images, so a batch holds
off-diagonal pairs ``(i, j)`` with equal study ids that are true image-report matches.  The other losses of the package
drop them; this one trains on them.  With ``S[i, j] = critic(img_i, txt_j)`` over a batch of B pairs:

    P_i = {j : sid_j == sid_i}  (contains i),   n_i = |P_i| >= 1
    r_i = log sum_{j < B} exp S[i, j]                 c_j = log sum_{i < B} exp S[i, j]        (nothing is masked)
    row term     t_i  = r_i - (1/n_i) sum_{p in P_i} S[i, p]
    column term  t'_j = c_j - (1/n_j) sum_{p in P_j} S[p, j]
    row-wise:  L = mean_i t_i            symmetric:  L = 1/2 mean_i t_i + 1/2 mean_j t'_j
    dL/dS[i, j] = w_r exp(S[i, j] - r_i) + w_c exp(S[i, j] - c_j) - (w_r + w_c) 1[sid_i == sid_j] / n_i

- With unique ids this IS the loss of ``fused_mi_bound(..., "infonce_rowwise" / "infonce_symmetric")``: the same r, c,
  loss and gradients.
- With duplicates it differs from that loss in two ways: same-study pairs enter the denominators, and same-study pairs
  share the positive weight.
- With all ids equal ``t_i = r_i - mean_j S[i, j] >= log B``: the loss is not zero.
- ``B = 1`` gives loss exactly 0.0 and exact-zero gradients.
- Each row's share of dL/dS sums to zero.
- Only the averaged-outside form is built: in the image -> report direction the positives of a row are the same report
  repeated, so the log-of-sum-over-positives form gains nothing.

THIS IS A TRAINING LOSS, NOT A MUTUAL-INFORMATION BOUND: ``log B - L`` bounds nothing once some ``n_i > 1``.  It is
therefore not an estimator name of ``fused_mi_bound``; it is a switch on the row-wise and symmetric losses, reached
through the two functions below (and ``MultiModalManager(study_positives=True)`` / ``train.py --study_positives``).  It
runs eagerly on one GPU: there is no graphed and no sharded form.

Loss and every gradient are HIP kernels behind the C ABI (``mi_posnce_*`` / ``mi_matrix_posnce_*`` in
``include/mi_critic.h``): the score matrix is never materialised, the per-row and per-column statistics are an epilogue
of the score GEMM, the gradient weights an epilogue of the G GEMM; no float atomics anywhere, identical bits from call
to call.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _hip
from .critic_ops import OPS, posnce_matrix_bwd, posnce_matrix_fwd, resolve_critic
from .mi_critics import _batch_codes, _critic_kind, _f32_inputs, _grad_scalar, study_id_codes

__all__ = ["study_positive_infonce", "matrix_study_positive_infonce"]

_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def _mode(symmetric: bool) -> int:
    return _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE


class _PosNceFn(torch.autograd.Function):
    """The study-positive InfoNCE of the bilinear or separable critic in one library call (``ops.posnce_step``), as
    ``hard_negatives._HardNceFn``: with ``need_grad`` the call also writes every gradient for dL/dloss = 1 and the
    backward only scales them.  Returns (loss [1], lse_rows, lse_cols, n_pos)."""

    @staticmethod
    def forward(ctx, kind: str, sid, mode: int, precision: int, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        loss, r, c, n_pos, grads = OPS[kind]().posnce_step(x, y, params, sid, mode, precision, need_grad)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(r, c, n_pos)
        return loss, r, c, n_pos

    @staticmethod
    def backward(ctx, grad_loss, *_):
        saved = ctx.saved_tensors
        if not saved:
            raise RuntimeError("_PosNceFn: the forward ran without gradients (need_grad=False)")
        go = grad_loss.reshape(-1)[:1].to(torch.float32)
        return (None,) * 5 + tuple(g * go for g in saved)


class _MatrixPosNceFn(torch.autograd.Function):
    """The study-positive InfoNCE of a [B, B] score matrix (mi_matrix_posnce_fwd / _bwd); the backward reads the
    forward's LSEs and positive counts and writes the dense gradient of the scores."""

    @staticmethod
    def forward(ctx, scores, sid, mode: int):
        s = _hip.f32c(scores, "scores")
        loss, r, c, n_pos = posnce_matrix_fwd(s, sid, mode)
        ctx.save_for_backward(s, sid, r, c, n_pos)
        ctx.mode = mode
        ctx.mark_non_differentiable(r, c, n_pos)
        return loss, r, c, n_pos

    @staticmethod
    def backward(ctx, grad_loss, *_):
        s, sid, r, c, n_pos = ctx.saved_tensors
        return posnce_matrix_bwd(s, sid, ctx.mode, r, c, n_pos, _grad_scalar(grad_loss)), None, None


def study_positive_infonce(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic,
                           symmetric: bool = True, precision: str = "f32", return_stats: bool = False):
    """The study-positive InfoNCE (module docstring) of the batch under ``critic``, a 0-d tensor carrying autograd to the
    embeddings and the critic's parameters.  A training loss, not an MI bound.

    ``critic``: a ``BilinearCritic`` or a ``SeparableCritic``.  One library call runs prep and T = X W, the score GEMM
    whose epilogue writes the row / column records (LSE parts over every column, sums and counts over the same-study
    ones), the merge, the loss, and -- when an input needs a gradient -- the G GEMM whose epilogue applies the formula
    above, followed by the backward products of the per-sample InfoNCE.  The backward pass only scales the saved
    gradients.  A ``make_mlp`` critic has no GEMM form and raises ValueError: take its differentiable score matrix from
    ``fused_scores.fused_critic_scores`` (the fused kernels, no pair matrix) and call
    ``matrix_study_positive_infonce(scores, study_id)`` -- ``fused_scores.concat_study_positive_infonce`` does both.

    ``precision`` as for the per-sample InfoNCE of ``fused_mi_bound``: "f32" (bf16x3 on the bilinear critic where every
    size is a multiple of 8, exact fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8", "f16" and "f16x3"
    raise ValueError.

    ``return_stats=True``: ``(loss, {"lse_rows": r, "lse_cols": c, "n_pos": n})`` -- float32 [B], float32 [B] and the
    int32 [B] count of each sample's positives (itself included)."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a BilinearCritic or a SeparableCritic")
    if _critic_kind(critic) == "concat_mlp":
        raise ValueError("study_positive_infonce is implemented for the bilinear and separable critics only; for scores "
                         "you compute yourself (e.g. a make_mlp critic applied to every pair) use "
                         "matrix_study_positive_infonce(scores, study_id)")
    x = embedding_img.float() if embedding_img.dtype == torch.float64 else embedding_img
    y = embedding_txt.float() if embedding_txt.dtype == torch.float64 else embedding_txt
    sid = _batch_codes(x, y, study_id)
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    if prec not in _CHAIN_PRECISIONS:
        raise ValueError(f'precision="{precision}" is not available for the study-positive InfoNCE of the {kind} critic '
                         '(use "f32", "f32_exact", "bf16" or "bf16x3")')
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    loss, r, c, n_pos = _PosNceFn.apply(kind, sid, _mode(symmetric), prec, need_grad, x, y, *params)
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "n_pos": n_pos}) if return_stats else loss


def matrix_study_positive_infonce(scores: torch.Tensor, study_id, symmetric: bool = True, return_stats: bool = False):
    """The study-positive InfoNCE (module docstring) of a float32 [B, B] score matrix you computed, S[i, j] =
    critic(img_i, txt_j): a 0-d tensor with gradients to ``scores`` (dense).  The way to this loss for any critic, e.g. a
    ``make_mlp`` critic applied to every pair.  A training loss, not an MI bound.  ``return_stats`` as in
    ``study_positive_infonce``."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    loss, r, c, n_pos = _MatrixPosNceFn.apply(scores, sid, _mode(symmetric))
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "n_pos": n_pos}) if return_stats else loss
