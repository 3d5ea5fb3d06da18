"""Hard-negative InfoNCE: the per-sample image-report contrastive loss trained on each query's top-k negatives
(DESIGN.md section 12).

With ``S[i, j] = critic(img_i, txt_j)`` over a batch of B pairs and the package's masking (a pair ``i != j`` with equal
study ids is never a negative), ``H_i`` is the image -> report list of ``retrieval.retrieval_topk`` called with the study
ids on both sides -- the first ``min(k, #negatives)`` negatives of row i in "score descending, then index ascending" --
and ``H'_j`` the report -> image list of column j:

    r_i = log(exp S[i, i] + sum_{j in H_i} exp S[i, j])          c_j = log(exp S[j, j] + sum_{i in H'_j} exp S[i, j])
    row-wise:  L = mean_i (r_i - S[i, i])            symmetric:  L = 1/2 mean_i (r_i - S[i, i]) + 1/2 mean_j (c_j - S[j, j])

The selection is a constant of the gradient (its derivative almost everywhere), so dL/dS is nonzero exactly on the
diagonal and at the listed indices.  A row or column without negatives contributes exactly 0; with ``k`` at least every
row's (column's) negative count the loss is that of ``fused_mi_bound(..., "infonce_rowwise" / "infonce_symmetric")``.

THIS IS A TRAINING LOSS, NOT A MUTUAL-INFORMATION BOUND: the k candidates were chosen by score, not drawn from the
marginal, so ``log(k + 1) - L`` bounds nothing.  It is therefore not an estimator name of ``fused_mi_bound``; it is a
parameter ``k`` of the row-wise and symmetric losses, reached through the two functions below (and
``MultiModalManager(hard_negatives=k)`` / ``train.py --hard_negatives k``).  It runs eagerly on one GPU: there is no
graphed and no sharded form.

Selection, loss and every gradient are HIP kernels behind the C ABI (``mi_hardnce_*`` / ``mi_matrix_hardnce_*`` in
``include/mi_critic.h``): one score computation serves selection and loss, no float atomics anywhere, identical bits
from call to call.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _hip
from .critic_ops import OPS, hardnce_matrix_bwd, hardnce_matrix_fwd, resolve_critic
from .mi_critics import _batch_codes, _critic_kind, _f32_inputs, _grad_scalar, study_id_codes

__all__ = ["hard_negative_infonce", "matrix_hard_negative_infonce"]

_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def check_k(k) -> int:
    """``k`` as an int in [1, MI_TOPK_MAX_K]; ValueError otherwise."""
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f"k must be an integer in [1, {_hip.MI_TOPK_MAX_K}] (got {k!r})")
    k = int(k)
    if not 1 <= k <= _hip.MI_TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {_hip.MI_TOPK_MAX_K}] (got {k})")
    return k


def _mode(symmetric: bool) -> int:
    return _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE


class _HardNceFn(torch.autograd.Function):
    """The hard-negative InfoNCE of the bilinear or separable critic in one library call (``ops.hardnce_step``), as
    ``mi_critics._ChainFn``: with ``need_grad`` the call also writes every gradient for dL/dloss = 1 and the backward only
    scales them.  Returns (loss [1], lse_rows, lse_cols, idx_rows, idx_cols); the column side is None in the row-wise
    mode."""

    @staticmethod
    def forward(ctx, kind: str, sid, mode: int, precision: int, k: int, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        loss, r, c, ir, ic, grads = OPS[kind]().hardnce_step(x, y, params, sid, mode, precision, k, need_grad)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(*[t for t in (r, c, ir, ic) if t is not None])
        return loss, r, c, ir, ic

    @staticmethod
    def backward(ctx, grad_loss, *_):
        saved = ctx.saved_tensors
        if not saved:
            raise RuntimeError("_HardNceFn: the forward ran without gradients (need_grad=False)")
        go = grad_loss.reshape(-1)[:1].to(torch.float32)
        return (None,) * 6 + tuple(g * go for g in saved)


class _MatrixHardNceFn(torch.autograd.Function):
    """The hard-negative InfoNCE of a [B, B] score matrix (mi_matrix_hardnce_fwd / _bwd); the backward reads the
    forward's lists and LSEs and writes the dense gradient of the scores."""

    @staticmethod
    def forward(ctx, scores, sid, mode: int, k: int):
        s = _hip.f32c(scores, "scores")
        loss, r, c, ir, ic = hardnce_matrix_fwd(s, sid, mode, k)
        ctx.save_for_backward(*[t for t in (s, r, ir, c, ic) if t is not None])
        ctx.mode, ctx.k = mode, k
        ctx.mark_non_differentiable(*[t for t in (r, c, ir, ic) if t is not None])
        return loss, r, c, ir, ic

    @staticmethod
    def backward(ctx, grad_loss, *_):
        s, r, ir, *cols = ctx.saved_tensors
        c, ic = cols if cols else (None, None)
        return hardnce_matrix_bwd(s, ctx.mode, ctx.k, r, c, ir, ic, _grad_scalar(grad_loss)), None, None, None


def hard_negative_infonce(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic, k: int,
                          symmetric: bool = True, precision: str = "f32", return_lists: bool = False):
    """The hard-negative InfoNCE (module docstring) of the batch under ``critic``, a 0-d tensor carrying autograd to the
    embeddings and the critic's parameters.  A training loss, not an MI bound.

    ``critic``: a ``BilinearCritic`` or a ``SeparableCritic``.  One library call runs prep and T = X W, the top-k sweep
    with the ids (image -> report; in the symmetric mode also report -> image), a small kernel that forms the loss from
    the lists, and -- when an input needs a gradient -- the G GEMM whose epilogue keeps G on the lists and the diagonal
    followed by the backward products of the per-sample InfoNCE.  The backward pass only scales the saved gradients.  A
    ``make_mlp`` critic has no GEMM form and raises ValueError: take its differentiable score matrix from
    ``fused_scores.fused_critic_scores`` (the fused kernels, no pair matrix) and call
    ``matrix_hard_negative_infonce(scores, study_id, k)`` -- ``fused_scores.concat_hard_negative_infonce`` does both.

    ``k`` in [1, 32].  ``precision`` as for the per-sample InfoNCE of ``fused_mi_bound``: "f32" (bf16x3 on the bilinear
    critic where every size is a multiple of 8, exact fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8",
    "f16" and "f16x3" raise ValueError.

    ``return_lists=True``: ``(loss, {"i2t": idx_rows, "t2i": idx_cols})``, the int32 [B, k] lists the loss used (tail
    -1) -- ``torch.equal`` to ``retrieval_topk(..., img_ids=study_id, txt_ids=study_id)`` on the same inputs and
    precision; "t2i" is None in the row-wise mode, which selects no column side."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a BilinearCritic or a SeparableCritic")
    if _critic_kind(critic) == "concat_mlp":
        raise ValueError("hard_negative_infonce is implemented for the bilinear and separable critics only; for scores you "
                         "compute yourself (e.g. a make_mlp critic applied to every pair) use "
                         "matrix_hard_negative_infonce(scores, study_id, k)")
    k = check_k(k)
    x = embedding_img.float() if embedding_img.dtype == torch.float64 else embedding_img
    y = embedding_txt.float() if embedding_txt.dtype == torch.float64 else embedding_txt
    sid = _batch_codes(x, y, study_id)
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    if prec not in _CHAIN_PRECISIONS:
        raise ValueError(f'precision="{precision}" is not available for the hard-negative InfoNCE of the {kind} critic '
                         '(use "f32", "f32_exact", "bf16" or "bf16x3")')
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    loss, _r, _c, ir, ic = _HardNceFn.apply(kind, sid, _mode(symmetric), prec, k, need_grad, x, y, *params)
    loss = loss.reshape(())
    return (loss, {"i2t": ir, "t2i": ic}) if return_lists else loss


def matrix_hard_negative_infonce(scores: torch.Tensor, study_id, k: int, symmetric: bool = True,
                                 return_lists: bool = False):
    """The hard-negative InfoNCE (module docstring) of a float32 [B, B] score matrix you computed, S[i, j] =
    critic(img_i, txt_j): a 0-d tensor with gradients to ``scores`` (dense, zero outside the lists and the diagonal).
    The way to this loss for any critic, e.g. a ``make_mlp`` critic applied to every pair.  A training loss, not an MI
    bound.  ``return_lists`` as in ``hard_negative_infonce``."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    k = check_k(k)
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    loss, _r, _c, ir, ic = _MatrixHardNceFn.apply(scores, sid, _mode(symmetric), k)
    loss = loss.reshape(())
    return (loss, {"i2t": ir, "t2i": ic}) if return_lists else loss
