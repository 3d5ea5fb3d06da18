"""The reference's make_mlp critic as a differentiable score matrix on the fused kernels.

``fused_critic_scores(embedding_img, embedding_txt, critic)`` returns S [n_img, n_txt], S[i, j] = critic([img_i ; txt_j]),
without materialising the [n_img * n_txt, d_img + d_txt] pair matrix, and carries autograd: whatever loss is applied to S
-- the matrix functions of this package (``matrix_bound_loss``, ``matrix_hard_negative_infonce``,
``matrix_study_positive_infonce``, ``matrix_soft_target_infonce``) or plain torch -- its dL/dS goes back through the
fused backward kernels to both embeddings and the six parameters of the critic (mi_concat_mlp_scores_fwd /
mi_concat_mlp_bwd_from_g).  The DV, "infonce", JSD and NWJ bounds of this critic stay with
``fused_mi_bound``, which forms their gradient inside the kernels and never reads a [B, B] gradient matrix.

Four one-line compositions for the losses ``fused_mi_bound`` and its siblings do not take for this critic:

* ``concat_infonce``                 -- per-sample InfoNCE (row-wise / symmetric), or any estimator of ``matrix_bound_loss``
* ``concat_hard_negative_infonce``   -- hard-negative InfoNCE on each query's top-k negatives
* ``concat_study_positive_infonce``  -- same-study pairs as positives
* ``concat_soft_target_infonce``     -- soft targets from the studies' finding-label masks
"""
from __future__ import annotations

import torch

from . import _hip
from .critic_ops import NOT_MAKE_MLP, HipConcatMlpOps, resolve_critic
from .hard_negatives import matrix_hard_negative_infonce
from .mi_critics import _critic_kind, _f32_inputs, matrix_bound_loss
from .soft_targets import matrix_soft_target_infonce
from .study_positives import matrix_study_positive_infonce

__all__ = ["fused_critic_scores", "concat_infonce", "concat_hard_negative_infonce", "concat_study_positive_infonce",
           "concat_soft_target_infonce"]


class _ScoresFn(torch.autograd.Function):
    """S [n_img, n_txt] of the make_mlp critic.  With ``need_grad`` the forward leaves the sign-bit images and operand
    copies in its workspace, which ``ctx`` keeps: the backward reads it and may run more than once."""

    @staticmethod
    def forward(ctx, precision: int, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        scores, saved = HipConcatMlpOps().scores_forward(x, y, params, precision, need_grad)
        ctx.save_for_backward(x, y, saved[-1], *params)
        ctx.precision, ctx.need_grad = precision, need_grad
        return scores

    @staticmethod
    def backward(ctx, grad_scores):
        if not ctx.need_grad:
            raise RuntimeError("_ScoresFn: the forward ran without gradients (need_grad=False)")
        x, y, ws, *params = ctx.saved_tensors
        g = grad_scores.to(torch.float32).contiguous()
        gx, gy, gp = HipConcatMlpOps().scores_backward((x, y, params, ctx.precision, ws), g)
        return (None, None, gx, gy, *gp)


def fused_critic_scores(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, critic,
                        precision: str = "f32") -> torch.Tensor:
    """S [n_img, n_txt], S[i, j] = critic([img_i ; txt_j]), float32, differentiable in both embeddings and in the six
    parameters of ``critic``; n_img <= n_txt (a row block of images against every report; n_img == n_txt is a batch).

    ``critic``: the reference's ``make_mlp(d_img + d_txt, [h1, h2])`` of the fused shapes (h1 % 64 == 0, h2 in {256,
    512}); anything else raises ValueError.  ``precision`` as for the DV bound of this critic in ``fused_mi_bound``: "f32"
    (the two-part fp16 scheme, fp32-grade results), "f32_exact", "bf16", "f16"; the scores are bit-identical to the ones
    ``fused_mi_bound(..., return_scores=True)`` returns.  Under ``torch.no_grad()``, or when nothing requires a gradient,
    only the forward kernels run and no sign-bit image is written.

    The backward reads ``grad_scores`` [n_img, n_txt] (64 MB at B = 4096); pairs a loss drops carry a zero there.  In the
    fp16 modes g is scaled by a power of two taken from max|grad_scores|, so loss scaling by any power of two changes
    nothing but the exponent of the result."""
    x = embedding_img.float() if torch.is_tensor(embedding_img) and embedding_img.dtype == torch.float64 else embedding_img
    y = embedding_txt.float() if torch.is_tensor(embedding_txt) and embedding_txt.dtype == torch.float64 else embedding_txt
    if not torch.is_tensor(x) or not torch.is_tensor(y) or x.dim() != 2 or y.dim() != 2:
        raise ValueError("embedding_img / embedding_txt must be [n_img, d_img] / [n_txt, d_txt]")
    if x.shape[0] > y.shape[0] or x.shape[0] < 1:
        raise ValueError(f"fused_critic_scores needs 1 <= n_img <= n_txt (got {x.shape[0]} images, {y.shape[0]} reports)")
    if critic is None or _critic_kind(critic) != "concat_mlp" or not isinstance(critic, torch.nn.Sequential):
        raise ValueError(NOT_MAKE_MLP)
    _kind, params, prec = resolve_critic(critic, precision, y.shape[0], x.shape[1], y.shape[1])
    if prec in (_hip.MI_PREC_BF16X3, _hip.MI_PREC_FP8):
        raise ValueError(f'precision="{precision}" is implemented for BilinearCritic only')
    _hip.require_device(x, "embedding_img")
    _hip.require_device(y, "embedding_txt")
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    return _ScoresFn.apply(prec, need_grad, x, y, *params)


def concat_infonce(embedding_img, embedding_txt, study_id, critic, estimator: str = "infonce_symmetric",
                   precision: str = "f32") -> torch.Tensor:
    """``matrix_bound_loss`` (per-sample InfoNCE "infonce_rowwise" / "infonce_symmetric", or any other estimator it takes)
    on the fused scores of a make_mlp critic; a batch: n_img == n_txt."""
    return matrix_bound_loss(fused_critic_scores(embedding_img, embedding_txt, critic, precision), study_id, estimator)


def concat_hard_negative_infonce(embedding_img, embedding_txt, study_id, critic, k: int, symmetric: bool = True,
                                 precision: str = "f32", return_lists: bool = False):
    """``matrix_hard_negative_infonce`` on the fused scores of a make_mlp critic; a batch: n_img == n_txt."""
    return matrix_hard_negative_infonce(fused_critic_scores(embedding_img, embedding_txt, critic, precision), study_id, k,
                                        symmetric=symmetric, return_lists=return_lists)


def concat_study_positive_infonce(embedding_img, embedding_txt, study_id, critic, symmetric: bool = True,
                                  precision: str = "f32", return_stats: bool = False):
    """``matrix_study_positive_infonce`` on the fused scores of a make_mlp critic; a batch: n_img == n_txt."""
    return matrix_study_positive_infonce(fused_critic_scores(embedding_img, embedding_txt, critic, precision), study_id,
                                         symmetric=symmetric, return_stats=return_stats)


def concat_soft_target_infonce(embedding_img, embedding_txt, labels, critic, *, tau, mix, symmetric: bool = True,
                               precision: str = "f32", return_stats: bool = False):
    """``matrix_soft_target_infonce`` on the fused scores of a make_mlp critic; a batch: n_img == n_txt."""
    return matrix_soft_target_infonce(fused_critic_scores(embedding_img, embedding_txt, critic, precision), labels,
                                      tau=tau, mix=mix, symmetric=symmetric, return_stats=return_stats)
