"""The soft-target InfoNCE over the sharded global batch: the row-block protocol of
``distributed.GlobalBatchNceFn`` / ``GlobalBatchPosNceFn`` with the epilogues that weigh every pair
by the similarity of its finding sets.  A module of its own beside ``distributed`` (which holds the collectives and the
shared helpers it uses): a training loss, not an estimator, and nothing in ``global_batch_mi_bound`` or the graphed step
knows about it.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.distributed as dist

from . import _hip
from .distributed import _all_gather_rows, _block_loss_setup, _exchange_block_gradients, _gather_block_inputs
from .soft_targets import check_tau_mix

__all__ = ["GlobalBatchSoftNceFn", "global_batch_soft_target_infonce"]


class GlobalBatchSoftNceFn(torch.autograd.Function):
    """Soft-target InfoNCE over the GLOBAL batch from this rank's row block.
    Returns (loss [1], lse_rows [b_rows], lse_cols [B], target_norm [b_rows]).

    forward : all-gather Y and the label masks; every rank forms z of ALL samples from the gathered masks; the rank's
              scores -> one flat part (column LSE partials, column q-weighted score partials, row terms); all-gather the
              parts; merge them in rank order -> c, loss (identical bits on every rank).
    backward: the rank's gradients from its r, the label norms and the merged c -> dX complete, dY partial
              (reduce-scatter), parameter gradients partial (one flat all-reduce).  Five collectives per step."""

    @staticmethod
    def forward(ctx, ops, group, mode: int, precision: int, tau: float, mix: float, lab_rows, x, y, *params):
        rank = dist.get_rank(group)
        br = x.shape[0]
        x = x.contiguous()
        params_c = [p.contiguous() for p in params]
        y_all, lab_all = _gather_block_inputs(group, y, lab_rows)
        part, lse_rows, z, saved = ops.softnce_forward(x, y_all, params_c, lab_rows.contiguous(), lab_all, rank * br, mode,
                                                       precision, tau, mix)
        parts = _all_gather_rows(part.reshape(1, -1), group)  # [G, P], rank order
        loss, lse_cols = ops.softnce_merge(parts, br, mode)
        ctx.ops, ctx.group, ctx.saved = ops, group, saved
        ctx.param_like = [p.detach() for p in params]
        ctx.save_for_backward(lse_cols)
        ctx.mark_non_differentiable(lse_rows, lse_cols, z)
        return loss, lse_rows, lse_cols, z

    @staticmethod
    def backward(ctx, grad_loss, *_):
        (lse_cols,) = ctx.saved_tensors
        go = grad_loss.reshape(-1)[:1].to(lse_cols.dtype).contiguous()
        gx, gy_partial, gparams = ctx.ops.softnce_backward(ctx.saved, lse_cols, go)
        return (None,) * 7 + _exchange_block_gradients(ctx.group, ctx.param_like, gx, gy_partial, gparams)


def global_batch_soft_target_infonce(embedding_img, embedding_txt, label_masks, critic_params: Sequence[torch.Tensor], *,
                                     tau, mix, symmetric: bool = True, precision: str = "f32", critic: str = "bilinear",
                                     group=None, ops=None, return_stats: bool = False):
    """``soft_targets.soft_target_infonce`` at B = world_size * local_batch with this rank's [B/G, d] embeddings: the
    target of a row spreads over the similar reports of the GLOBAL batch (GlobalBatchSoftNceFn).  ``label_masks``: int64
    tensor [B/G], one finding-set mask per sample (``soft_targets.label_masks`` packs multi-hot labels); ``tau`` and
    ``mix`` are required keywords, as on one GPU.  ``critic`` "bilinear" (``critic_params`` = [W]) or "separable"
    ([Wg, Wh]).  Every rank returns the same 0-d loss; ``.backward()`` leaves the gradient of the global loss w.r.t. the
    local embeddings and the (all-reduced) gradient w.r.t. the critic parameters.  A training loss, not an MI bound, and
    not an estimator name.

    ``return_stats=True``: ``(loss, {"lse_rows": r [B/G], "lse_cols": c [B], "target_norm": z [B/G]})``."""
    tau, mix = check_tau_mix(tau, mix)
    ops, prec = _block_loss_setup("the soft-target InfoNCE", embedding_img, embedding_txt, label_masks, critic_params,
                                  precision, critic, ops)
    mode = _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE
    loss, r, c, z = GlobalBatchSoftNceFn.apply(ops, group, mode, prec, tau, mix, label_masks, embedding_img, embedding_txt,
                                               *critic_params)
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "target_norm": z}) if return_stats else loss
