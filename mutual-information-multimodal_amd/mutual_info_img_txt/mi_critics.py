"""MI355X-native drop-in for the reference's ``mutual_info_img_txt/mi_critics.py``.

Same two callables with the same signatures and return shapes as the reference:

* ``dv_bound_loss(discriminator_logits, pos_size, device)``      -- reference mi_critics.py:3-12,  returns shape [1]
* ``infonce_bound_loss(discriminator_logits, pos_size, device)`` -- reference mi_critics.py:14-23, returns shape []

plus the fused entry point that replaces lines ``main_utils.py:220-224`` of the reference training step
(create_mi_pairs -> mi_discriminator -> mi_critic) without materialising ``mi_input`` / ``mi_output``:

* ``fused_mi_bound(embedding_img, embedding_txt, study_id, critic, estimator, ...)``

Besides the reference's two estimators, ``fused_mi_bound`` (bilinear and separable critics) and ``matrix_bound_loss``
take the per-sample InfoNCE of CPC / ConVIRT / CLIP: ``"infonce_rowwise"`` (image -> report cross-entropy) and
``"infonce_symmetric"`` (its mean with report -> image), with the reference's masking of equal-id pairs (DESIGN.md
section 8), and every critic and ``matrix_bound_loss`` take the Jensen-Shannon bound ``"jsd"`` and the NWJ bound ``"nwj"``
(DESIGN.md section 9), also as reference-style callables on logits:

* ``jsd_bound_loss(discriminator_logits, pos_size, device)``, ``nwj_bound_loss(...)`` -- returns shape []

Every function runs hand-written HIP kernels through the C ABI in ``include/mi_critic.h`` (loaded with ctypes,
wrapped in ``torch.autograd.Function``).  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

from . import _hip
from ._hip import ESTIMATORS, FDIV_ESTIMATORS, NCE_ESTIMATORS
from .critic_ops import (HipBilinearOps, HipConcatMlpOps, HipSeparableOps, _concat_params,  # noqa: F401 (re-exported)
                         _precision_code, fwd_outputs, resolve_critic)

__all__ = ["dv_bound_loss", "infonce_bound_loss", "matrix_bound_loss", "fused_mi_bound", "study_id_codes",
           "BilinearCriticFn", "SeparableCriticFn", "ConcatMlpCriticFn", "NceBilinearFn", "NceSeparableFn",
           "check_estimator", "jsd_bound_loss", "nwj_bound_loss", "FdivBilinearFn", "FdivSeparableFn",
           "FdivConcatMlpFn"]


# ----------------------------------------------------------------------------------------------------------
# study ids: list[str] in the reference (model_utils.py:212); compared with != only (main_utils.py:105)
# ----------------------------------------------------------------------------------------------------------
def study_id_codes(study_id: Union[Sequence, torch.Tensor], device) -> torch.Tensor:
    """int64 device tensor with equal code <=> equal study id.  The codes are a pure function of each id
    (``utils.study_id_to_int64``: the numeric value of ids like "50414267", a 62-bit hash otherwise), hence identical in
    every process of a sharded run -- a first-seen numbering would not be."""
    from .utils import study_ids_to_tensor
    return study_ids_to_tensor(study_id, device)


def _estimator_code(estimator: str) -> int:
    if estimator not in ESTIMATORS:
        # the reference leaves mi_critic unbound for an unknown estimator (main_utils.py:141-144, UnboundLocalError
        # at :224); here it is rejected eagerly
        raise ValueError(f"unknown mi_estimator {estimator!r}: expected one of {sorted(ESTIMATORS)}")
    return ESTIMATORS[estimator]


def check_estimator(estimator: str, critic_kind: str) -> None:
    """Eager validation of an estimator name for a critic kind ("concat_mlp", "bilinear", "separable"): the reference's
    "dv" / "infonce" and the Jensen-Shannon / NWJ bounds "jsd" / "nwj" for every critic, the per-sample
    "infonce_rowwise" / "infonce_symmetric" for the bilinear and separable critics only."""
    if estimator in FDIV_ESTIMATORS:
        return
    if estimator in NCE_ESTIMATORS:
        if critic_kind not in ("bilinear", "separable"):
            raise ValueError(f"mi_estimator {estimator!r} is implemented for the bilinear and separable critics only "
                             f"(got critic {critic_kind!r})")
        return
    if estimator not in ESTIMATORS:
        raise ValueError(f"unknown mi_estimator {estimator!r}: expected one of "
                         f"{sorted(ESTIMATORS) + sorted(NCE_ESTIMATORS) + sorted(FDIV_ESTIMATORS)}")


def _grad_scalar(grad: torch.Tensor) -> torch.Tensor:
    return grad.reshape(-1)[:1].to(torch.float32).contiguous()


# ----------------------------------------------------------------------------------------------------------
# a3 / a4: bound on materialised logits
# ----------------------------------------------------------------------------------------------------------
class _BoundFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, pos_size: int, estimator: int):
        lib = _hip.load()
        flat = _hip.f32c(logits, "discriminator_logits").reshape(-1)
        n = flat.numel()
        dev = flat.device
        ws = _hip.workspace(lib.mi_bound_workspace_bytes(n), dev)
        stats = _hip.new_stats(dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("mi_bound_fwd", dev, flat.data_ptr(), n, int(pos_size), estimator, loss.data_ptr(), stats.data_ptr(),
                                    ws.data_ptr(), ws.numel())
        ctx.save_for_backward(flat, stats)
        ctx.pos_size = int(pos_size)
        ctx.in_shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _hip.load()
        flat, stats = ctx.saved_tensors
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(flat)
        _hip.call("mi_bound_bwd", flat.device, flat.data_ptr(), flat.numel(), ctx.pos_size, stats.data_ptr(), go.data_ptr(),
                                    grad.data_ptr())
        return grad.reshape(ctx.in_shape), None, None


def _bound(discriminator_logits, pos_size, estimator):
    _hip.require_device(discriminator_logits, "discriminator_logits")
    n = discriminator_logits.shape[0]
    if discriminator_logits.numel() != n:
        raise ValueError("discriminator_logits must be [N] or [N, 1] (one score per pair row)")
    if not 0 <= int(pos_size) <= n:
        raise ValueError(f"pos_size={pos_size} outside [0, {n}]")
    return _BoundFn.apply(discriminator_logits, int(pos_size), estimator)


def dv_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """Donsker-Varadhan bound, reference mi_critics.py:3-12: ``LSE(logits[pos:]) - log(N - pos) - mean(logits[:pos])``.
    ``device`` is kept for signature compatibility (the reference only uses it for the log-N constant)."""
    loss = _bound(discriminator_logits, pos_size, _hip.MI_DV)
    return loss.reshape(discriminator_logits.shape[1:])  # [N,1] -> [1] as in the reference


def infonce_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """The reference's "InfoNCE" bound, mi_critics.py:14-23: ``LSE(logits[pos:]) - mean(logits[:pos])`` (no log-N term;
    not a row-wise softmax cross-entropy).  Returns shape []."""
    return _bound(discriminator_logits, pos_size, _hip.MI_INFONCE).reshape(())


class _FdivBoundFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, pos_size: int, mode: int):
        lib = _hip.load()
        flat = _hip.f32c(logits, "discriminator_logits").reshape(-1)
        n, dev = flat.numel(), flat.device
        ws = _hip.workspace(lib.mi_fdiv_bound_workspace_bytes(n), dev)
        stats = _hip.new_stats(dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("mi_fdiv_bound_fwd", dev, flat.data_ptr(), n, int(pos_size), mode, loss.data_ptr(), None,
                  stats.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(flat, stats)
        ctx.pos_size, ctx.mode, ctx.in_shape = int(pos_size), mode, logits.shape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        flat, stats = ctx.saved_tensors
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(flat)
        _hip.call("mi_fdiv_bound_bwd", flat.device, flat.data_ptr(), flat.numel(), ctx.pos_size, ctx.mode,
                  stats.data_ptr(), go.data_ptr(), grad.data_ptr())
        return grad.reshape(ctx.in_shape), None, None


def _fdiv_bound(discriminator_logits, pos_size, mode):
    _hip.require_device(discriminator_logits, "discriminator_logits")
    n = discriminator_logits.shape[0]
    if discriminator_logits.numel() != n:
        raise ValueError("discriminator_logits must be [N] or [N, 1] (one score per pair row)")
    if not 0 <= int(pos_size) <= n:
        raise ValueError(f"pos_size={pos_size} outside [0, {n}]")
    return _FdivBoundFn.apply(discriminator_logits, int(pos_size), mode).reshape(())


def jsd_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """Jensen-Shannon bound (Deep InfoMax) on the reference's logits layout (the first ``pos_size`` rows positive):
    ``mean(softplus(-logits[:pos])) + mean(softplus(logits[pos:]))``, shape [].  Finite for any finite logits.  ``device``
    is kept for the signature of the reference's callables."""
    return _fdiv_bound(discriminator_logits, pos_size, _hip.MI_FDIV_JSD)


def nwj_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """NWJ bound (f-GAN KL, "MINE-f") on the reference's logits layout: ``exp(LSE(logits[pos:]) - log(N - pos) - 1) -
    mean(logits[:pos])``, shape []; ``-loss`` is the NWJ lower bound on the MI."""
    return _fdiv_bound(discriminator_logits, pos_size, _hip.MI_FDIV_NWJ)


# ----------------------------------------------------------------------------------------------------------
# bound on a B x B score matrix with study-id masking
# ----------------------------------------------------------------------------------------------------------
class _MatrixBoundFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: torch.Tensor, sid: torch.Tensor, estimator: int):
        lib = _hip.load()
        s = _hip.f32c(scores, "scores")
        b = s.shape[0]
        dev = s.device
        ws = _hip.workspace(lib.mi_matrix_bound_workspace_bytes(b), dev)
        stats = _hip.new_stats(dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("mi_matrix_bound_fwd", dev, s.data_ptr(), sid.data_ptr(), b, estimator, loss.data_ptr(),
                                           stats.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(s, sid, stats)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _hip.load()
        s, sid, stats = ctx.saved_tensors
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(s)
        _hip.call("mi_matrix_bound_bwd", s.device, s.data_ptr(), sid.data_ptr(), s.shape[0], stats.data_ptr(), go.data_ptr(),
                                           grad.data_ptr())
        return grad, None, None


class _MatrixNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: torch.Tensor, sid: torch.Tensor, mode: int):
        lib = _hip.load()
        s = _hip.f32c(scores, "scores")
        b = s.shape[0]
        dev = s.device
        ws = _hip.workspace(lib.mi_matrix_nce_workspace_bytes(b), dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        r = torch.empty(b, dtype=torch.float32, device=dev)
        c = torch.empty(b, dtype=torch.float32, device=dev)
        _hip.call("mi_matrix_nce_fwd", dev, s.data_ptr(), sid.data_ptr(), b, mode, loss.data_ptr(), r.data_ptr(),
                  c.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(s, sid, r, c)
        ctx.mode = mode
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        s, sid, r, c = ctx.saved_tensors
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(s)
        _hip.call("mi_matrix_nce_bwd", s.device, s.data_ptr(), sid.data_ptr(), s.shape[0], ctx.mode, r.data_ptr(),
                  c.data_ptr(), go.data_ptr(), grad.data_ptr())
        return grad, None, None


class _MatrixFdivFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: torch.Tensor, sid: torch.Tensor, mode: int):
        lib = _hip.load()
        s = _hip.f32c(scores, "scores")
        b, dev = s.shape[0], s.device
        ws = _hip.workspace(lib.mi_fdiv_matrix_workspace_bytes(b), dev)
        stats = _hip.new_stats(dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("mi_fdiv_matrix_fwd", dev, s.data_ptr(), sid.data_ptr(), b, mode, loss.data_ptr(), None,
                  stats.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(s, sid, stats)
        ctx.mode = mode
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        s, sid, stats = ctx.saved_tensors
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(s)
        _hip.call("mi_fdiv_matrix_bwd", s.device, s.data_ptr(), sid.data_ptr(), s.shape[0], ctx.mode, stats.data_ptr(),
                  go.data_ptr(), grad.data_ptr())
        return grad, None, None


def matrix_bound_loss(scores: torch.Tensor, study_id, estimator: str = "dv") -> torch.Tensor:
    """The reference loss on a [B,B] score matrix S[i,j] = critic(img_i, txt_j): positives are the diagonal, negatives
    the pairs with i != j and different study ids (main_utils.py:99-108).  Shape [1] (dv) / [] (infonce).

    "infonce_rowwise" / "infonce_symmetric": the per-sample InfoNCE on the same scores and masking,
    shape [], gradients to ``scores``.  The way to that loss for any critic whose scores you compute yourself.

    "jsd" / "nwj": the Jensen-Shannon and NWJ bounds on the same pairs, shape []."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    if estimator in FDIV_ESTIMATORS:
        sid = study_id_codes(study_id, scores.device)
        if sid.numel() != scores.shape[0]:
            raise ValueError("study_id length must equal B")
        return _MatrixFdivFn.apply(scores, sid, FDIV_ESTIMATORS[estimator]).reshape(())
    if estimator in NCE_ESTIMATORS:
        sid = study_id_codes(study_id, scores.device)
        if sid.numel() != scores.shape[0]:
            raise ValueError("study_id length must equal B")
        return _MatrixNceFn.apply(scores, sid, NCE_ESTIMATORS[estimator]).reshape(())
    code = _estimator_code(estimator)
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    loss = _MatrixBoundFn.apply(scores, sid, code)
    return loss if estimator == "dv" else loss.reshape(())


# ----------------------------------------------------------------------------------------------------------
# fused critics: thin autograd Functions over the ops objects of critic_ops (whole batch: b_rows = b, row_offset = 0)
# ----------------------------------------------------------------------------------------------------------
def _critic_forward(ctx, ops, x, y, params, sid, estimator, precision, scores):
    loss, stats, _, scores = out = fwd_outputs(x.device, scores)
    _, saved = ops.forward(x, y, params, sid, sid, 0, estimator, precision, any(ctx.needs_input_grad), out=out)
    ctx.save_for_backward(x, y, sid, stats, scores, saved[-1], *params)
    ctx.ops, ctx.precision = ops, precision
    ctx.mark_non_differentiable(*[t for t in (stats, scores) if t is not None])
    return loss, stats, scores


def _critic_backward(ctx, grad_loss):
    """(grad_x, grad_y, [grad_params...]) of grad_loss * loss."""
    x, y, sid, stats, scores, ws, *params = ctx.saved_tensors
    return ctx.ops.backward((x, y, params, sid, sid, 0, ctx.precision, scores, ws), stats, _grad_scalar(grad_loss))


class BilinearCriticFn(torch.autograd.Function):
    """loss = bound(S), S = (X W) Y^T (W None: X Y^T) with study-id masking; all gradients by the HIP backward."""

    @staticmethod
    def forward(ctx, x, y, w, sid, estimator: int, precision: int, want_scores: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [] if w is None else [_hip.f32c(w, "bilinear weight")]
        b = x.shape[0]
        if params:
            _hip.note_path("bilinear", (b, b, x.shape[1], y.shape[1]), precision)
        scores = torch.empty(b, b, dtype=torch.float32, device=x.device) if want_scores else None
        return _critic_forward(ctx, HipBilinearOps(), x, y, params, sid, estimator, precision, scores)

    @staticmethod
    def backward(ctx, grad_loss, _gs, _gsc):
        gx, gy, gp = _critic_backward(ctx, grad_loss)
        return gx, gy, (gp[0] if gp else None), None, None, None, None


class SeparableCriticFn(torch.autograd.Function):
    """loss = bound(S), S = (X Wg)(Y Wh)^T with study-id masking; projections, fused B x B stage and all gradients by
    the HIP library (BASELINE.json configs[1]).  Projection shapes are checked by ``resolve_critic``."""

    @staticmethod
    def forward(ctx, x, y, wg, wh, sid, estimator: int, precision: int):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [_hip.f32c(wg, "image projection"), _hip.f32c(wh, "text projection")]
        b = x.shape[0]
        _hip.note_path("separable", (b, b, x.shape[1], y.shape[1], wg.shape[1]), precision)
        return _critic_forward(ctx, HipSeparableOps(), x, y, params, sid, estimator, precision, None)

    @staticmethod
    def backward(ctx, grad_loss, _gs, _gsc):
        gx, gy, gp = _critic_backward(ctx, grad_loss)
        return (gx, gy, *gp, None, None, None)


class ConcatMlpCriticFn(torch.autograd.Function):
    """loss = bound(S), S[i,j] = MLP([x_i ; y_j]) with the reference critic make_mlp(d,[h1,h2]) (model.py:18-32)."""

    @staticmethod
    def forward(ctx, x, y, w1, b1, w2, b2, w3, b3, sid, estimator: int, precision: int, want_scores: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [_hip.f32c(p, f"critic param {n}") for n, p in enumerate((w1, b1, w2, b2, w3, b3))]
        scores = torch.empty(x.shape[0], x.shape[0], dtype=torch.float32, device=x.device)  # the backward reads them
        return _critic_forward(ctx, HipConcatMlpOps(), x, y, params, sid, estimator, precision, scores)

    @staticmethod
    def backward(ctx, grad_loss, _gs, _gsc):
        gx, gy, gp = _critic_backward(ctx, grad_loss)
        return (gx, gy, *gp, None, None, None, None)


def _nce_forward(ctx, ops, x, y, params, sid, mode, precision, need_grad):
    loss, r, c, grads = ops.nce_step(x, y, params, sid, mode, precision, need_grad)
    ctx.save_for_backward(*grads)
    ctx.mark_non_differentiable(r, c)
    return loss, r, c


def _nce_backward(ctx, grad_loss, name):
    """The gradients the forward call wrote for dL/dloss = 1, scaled by grad_loss."""
    saved = ctx.saved_tensors
    if not saved:
        raise RuntimeError(f"{name}: the forward ran without gradients (need_grad=False)")
    go = grad_loss.reshape(-1)[:1].to(torch.float32)
    return (*(g * go for g in saved), *[None] * (len(ctx.needs_input_grad) - len(saved)))


class NceBilinearFn(torch.autograd.Function):
    """Per-sample InfoNCE of S = (X W) Y^T (W None: S = X Y^T) in one library call (mi_nce_bilinear_step).  With
    ``need_grad`` the call also writes every gradient for dL/dloss = 1; the backward only scales them by grad_loss.
    Returns (loss [1], lse_rows [B], lse_cols [B])."""

    @staticmethod
    def forward(ctx, x, y, w, sid, mode: int, precision: int, need_grad: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [] if w is None else [_hip.f32c(w, "bilinear weight")]
        return _nce_forward(ctx, HipBilinearOps(), x, y, params, sid, mode, precision, need_grad)

    @staticmethod
    def backward(ctx, grad_loss, _gr, _gc):
        return _nce_backward(ctx, grad_loss, "NceBilinearFn")


class NceSeparableFn(torch.autograd.Function):
    """Per-sample InfoNCE of S = (X Wg)(Y Wh)^T in one library call (mi_nce_separable_step); see NceBilinearFn."""

    @staticmethod
    def forward(ctx, x, y, wg, wh, sid, mode: int, precision: int, need_grad: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [_hip.f32c(wg, "image projection"), _hip.f32c(wh, "text projection")]
        return _nce_forward(ctx, HipSeparableOps(), x, y, params, sid, mode, precision, need_grad)

    @staticmethod
    def backward(ctx, grad_loss, _gr, _gc):
        return _nce_backward(ctx, grad_loss, "NceSeparableFn")


def _fdiv_step_forward(ctx, ops, x, y, params, sid, mode, precision, need_grad):
    loss, terms, grads = ops.fdiv_step(x, y, params, sid, mode, precision, need_grad)
    ctx.save_for_backward(*grads)
    ctx.mark_non_differentiable(terms)
    return loss, terms


class FdivBilinearFn(torch.autograd.Function):
    """Jensen-Shannon / NWJ bound of S = (X W) Y^T (W None: S = X Y^T) in one library call (mi_fdiv_bilinear_step); with
    ``need_grad`` the call also writes every gradient for dL/dloss = 1, the backward scales them.  Returns (loss [1],
    terms [2])."""

    @staticmethod
    def forward(ctx, x, y, w, sid, mode: int, precision: int, need_grad: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [] if w is None else [_hip.f32c(w, "bilinear weight")]
        return _fdiv_step_forward(ctx, HipBilinearOps(), x, y, params, sid, mode, precision, need_grad)

    @staticmethod
    def backward(ctx, grad_loss, _gt):
        return _nce_backward(ctx, grad_loss, "FdivBilinearFn")


class FdivSeparableFn(torch.autograd.Function):
    """Jensen-Shannon / NWJ bound of S = (X Wg)(Y Wh)^T in one library call (mi_fdiv_separable_step); see
    FdivBilinearFn."""

    @staticmethod
    def forward(ctx, x, y, wg, wh, sid, mode: int, precision: int, need_grad: bool):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [_hip.f32c(wg, "image projection"), _hip.f32c(wh, "text projection")]
        return _fdiv_step_forward(ctx, HipSeparableOps(), x, y, params, sid, mode, precision, need_grad)

    @staticmethod
    def backward(ctx, grad_loss, _gt):
        return _nce_backward(ctx, grad_loss, "FdivSeparableFn")


class FdivConcatMlpFn(torch.autograd.Function):
    """Jensen-Shannon / NWJ bound of S[i,j] = MLP([x_i ; y_j]) (make_mlp(d,[h1,h2])): the fused forward writes scores,
    sign-bit images and statistics; the backward kernels run under the mode's gradient rule.  Returns (loss [1],
    terms [2], scores [B, B])."""

    @staticmethod
    def forward(ctx, x, y, w1, b1, w2, b2, w3, b3, sid, mode: int, precision: int):
        x, y = _hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt")
        params = [_hip.f32c(p, f"critic param {n}") for n, p in enumerate((w1, b1, w2, b2, w3, b3))]
        need_grad = any(ctx.needs_input_grad)
        loss, terms, saved = HipConcatMlpOps().fdiv_forward(x, y, params, sid, sid, 0, mode, precision, need_grad)
        scores, stats, ws = saved[8:]
        ctx.save_for_backward(x, y, sid, scores, stats, ws, *params)
        ctx.mode, ctx.precision = mode, precision
        ctx.mark_non_differentiable(terms, scores)
        return loss, terms, scores

    @staticmethod
    def backward(ctx, grad_loss, _gt, _gs):
        x, y, sid, scores, stats, ws, *params = ctx.saved_tensors
        saved = (x, y, params, sid, sid, 0, ctx.mode, ctx.precision, scores, stats, ws)
        gx, gy, gp = HipConcatMlpOps().fdiv_backward(saved, _grad_scalar(grad_loss))
        return (gx, gy, *gp, None, None, None)


def _fused_fdiv(x, y, study_id, critic, estimator, precision, return_scores, return_stats):
    """fused_mi_bound for "jsd" / "nwj" (every critic)."""
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    sid = _batch_codes(x, y, study_id)
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    mode = FDIV_ESTIMATORS[estimator]
    scores = None
    if kind == "concat_mlp":
        w1, b1, w2, b2, w3, b3 = params
        loss, terms, scores = FdivConcatMlpFn.apply(x, y, w1, b1, w2, b2, w3.reshape(-1), b3, sid, mode, prec)
    else:
        # "f32": bf16x3 on the bilinear critic where every size is a multiple of 8, exact fp32 products otherwise (the
        # library rejects fp8 / f16 / f16x3 for these critics)
        need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
        fn = FdivBilinearFn if kind == "bilinear" else FdivSeparableFn
        loss, terms = fn.apply(x, y, *params, sid, mode, prec, need_grad)
        if return_scores:  # diagnostic output: no gradient flows through it
            with torch.no_grad():
                a, c, w = (x, y, critic.weight) if kind == "bilinear" else (critic.project_img(x), critic.project_txt(y), None)
                scores = BilinearCriticFn.apply(a, c, w, sid, _hip.MI_DV, prec, True)[2]
    out = [loss.reshape(())]
    if return_scores:
        out.append(scores)
    if return_stats:
        out.append((terms[0], terms[1]))
    return out[0] if len(out) == 1 else tuple(out)


def _batch_codes(embedding_img, embedding_txt, study_id) -> torch.Tensor:
    """Shape checks of one batch; its study-id codes."""
    if embedding_img.dim() != 2 or embedding_txt.dim() != 2 or embedding_img.shape[0] != embedding_txt.shape[0]:
        raise ValueError("embedding_img / embedding_txt must be [B, d_img] / [B, d_txt]")
    sid = study_id_codes(study_id, embedding_img.device)
    if sid.numel() != embedding_img.shape[0]:
        raise ValueError("study_id length must equal the batch size")
    return sid


def _fused_nce(x, y, study_id, critic, estimator, precision, return_scores, return_stats):
    """fused_mi_bound for "infonce_rowwise" / "infonce_symmetric"."""
    from . import model as _model

    if not isinstance(critic, (_model.BilinearCritic, _model.SeparableCritic)):
        raise ValueError(f"mi_estimator {estimator!r} is implemented for BilinearCritic and SeparableCritic only; for "
                         "scores you compute yourself (e.g. a make_mlp critic applied to every pair) use "
                         "matrix_bound_loss(scores, study_id, estimator)")
    sid = _batch_codes(x, y, study_id)
    # "f32": bf16x3 on the bilinear critic where every size is a multiple of 8, exact fp32 products otherwise (the library
    # rejects fp8 / f16 / f16x3 for this loss)
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    fn = NceBilinearFn if kind == "bilinear" else NceSeparableFn
    loss, r, c = fn.apply(x, y, *params, sid, NCE_ESTIMATORS[estimator], prec, need_grad)
    out = [loss.reshape(())]
    if return_scores:  # diagnostic output, as for the reference's estimators: no gradient flows through it
        with torch.no_grad():
            if kind == "bilinear":
                s = BilinearCriticFn.apply(x, y, critic.weight, sid, _hip.MI_DV, prec, True)[2]
            else:
                s = BilinearCriticFn.apply(critic.project_img(x), critic.project_txt(y), None, sid, _hip.MI_DV, prec,
                                           True)[2]
        out.append(s)
    if return_stats:
        out.append((r, c))
    return out[0] if len(out) == 1 else tuple(out)


def fused_mi_bound(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic, estimator: str = "dv",
                   precision: str = "f32", return_scores: bool = False, return_stats: bool = False):
    """Fused replacement of the reference lines main_utils.py:220-224:

        mi_input  = self.create_mi_pairs(embedding_img, embedding_txt, study_id, device)
        mi_output = self.mi_discriminator(mi_input)
        loss      = mi_critic(mi_output, args.batch_size, device)

    ``critic`` is the reference's ``make_mlp(d_img+d_txt,[h1,h2])`` nn.Sequential, or a ``BilinearCritic`` /
    ``SeparableCritic`` from ``mutual_info_img_txt.model`` (extensions).  Returns the loss (shape [1] for "dv",
    [] for "infonce", as the reference) and optionally the [B,B] score matrix S[i,j] = critic(img_i, txt_j).

    ``precision`` defaults to "f32": the reference critic is fp32 throughout and this is the mode whose results match it
    within the stated fp32 tolerances.  For the concat-MLP and separable critics it means exact fp32
    products on the fp32-input MFMA; for ``BilinearCritic`` (sizes multiples of 8) it runs the "bf16x3" scheme below, which
    meets the same tolerances at several times the speed -- pass "f32_exact" to insist on exact fp32 products.  "bf16" (bf16 MFMA operands, fp32
    accumulate) is the fast mode; it moves the gradients of this heavily cancelling loss by up to a few percent of
    max|grad| against the fp32 reference and must be asked for explicitly.  "bf16x3" (BilinearCritic only) splits every
    operand into two bf16 parts and spends three bf16 MFMAs per product: fp32-grade gradients at several times the speed
    of "f32".  "fp8" (BilinearCritic only) quantises the embeddings, the weight and T = x W to e4m3 with per-tensor scales
    and runs both forward products on the fp8 MFMA (BASELINE configs[4]); its results match an oracle fed the same
    quantised values, not the fp32 reference.  Embeddings in float64 are cast to float32 (the reference would run them in fp64; this path computes in
    fp32).

    ``estimator`` = "infonce_rowwise" / "infonce_symmetric" (BilinearCritic, SeparableCritic): the per-sample InfoNCE
    (DESIGN.md section 8), loss of shape [], precisions "f32" / "f32_exact" / "bf16" / "bf16x3";
    ``return_stats=True`` then gives ``(lse_rows, lse_cols)``, the row and column log-sum-exps.  A make_mlp critic raises
    ValueError: apply it to the pairs yourself and call ``matrix_bound_loss(scores, study_id, estimator)``.

    ``estimator`` = "jsd" / "nwj" (every critic): the Jensen-Shannon and NWJ bounds, loss of shape
    []; ``return_stats=True`` then gives ``(positive-pair term, negative-pair term)``, two 0-d tensors whose sum is the loss.
    """
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if embedding_img.dtype == torch.float64:
        embedding_img = embedding_img.float()
    if embedding_txt.dtype == torch.float64:
        embedding_txt = embedding_txt.float()
    if estimator in FDIV_ESTIMATORS:
        return _fused_fdiv(embedding_img, embedding_txt, study_id, critic, estimator, precision, return_scores,
                           return_stats)
    if estimator in NCE_ESTIMATORS:
        return _fused_nce(embedding_img, embedding_txt, study_id, critic, estimator, precision, return_scores, return_stats)
    code = _estimator_code(estimator)
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    sid = _batch_codes(embedding_img, embedding_txt, study_id)
    kind, params, prec = resolve_critic(critic, precision, embedding_img.shape[0], embedding_img.shape[1],
                                        embedding_txt.shape[1])
    if prec in (_hip.MI_PREC_BF16X3, _hip.MI_PREC_FP8) and kind != "bilinear":
        raise ValueError(f'precision="{precision}" is implemented for BilinearCritic only')
    if prec in (_hip.MI_PREC_F16, _hip.MI_PREC_F16X3) and kind != "concat_mlp":
        raise ValueError(f'precision="{precision}" is the fp16-operand mode of the make_mlp critic (its generated operand '
                         'relu(U_i + V_j) is formed by packed fp16 arithmetic); use "bf16" for this critic')
    if kind == "bilinear":
        loss, stats, scores = BilinearCriticFn.apply(embedding_img, embedding_txt, *params, sid, code, prec,
                                                     bool(return_scores))
    elif kind == "separable" and return_scores:  # per-pair scores are a diagnostic output: eager projections + the
        a, c = critic.project_img(embedding_img), critic.project_txt(embedding_txt)
        loss, stats, scores = BilinearCriticFn.apply(a, c, None, sid, code, prec, True)  # bilinear form with W = None
    elif kind == "separable":
        loss, stats, scores = SeparableCriticFn.apply(embedding_img, embedding_txt, *params, sid, code, prec)
    else:
        w1, b1, w2, b2, w3, b3 = params
        loss, stats, scores = ConcatMlpCriticFn.apply(embedding_img, embedding_txt, w1, b1, w2, b2, w3.reshape(-1), b3,
                                                      sid, code, prec, bool(return_scores))
    loss = loss if estimator == "dv" else loss.reshape(())
    out = [loss]
    if return_scores:
        out.append(scores)
    if return_stats:
        out.append(stats)
    return out[0] if len(out) == 1 else tuple(out)
