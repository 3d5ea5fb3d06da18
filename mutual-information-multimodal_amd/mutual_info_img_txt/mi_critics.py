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

from typing import Sequence, Union

import torch

from . import _hip
from ._hip import ESTIMATOR_TABLE, ESTIMATORS, check_estimator  # noqa: F401 (check_estimator: re-exported)
from .critic_ops import (OPS, HipBilinearOps, HipConcatMlpOps, HipSeparableOps, _concat_params,  # noqa: F401 (re-exported)
                         _precision_code, fwd_outputs, resolve_critic)

__all__ = ["dv_bound_loss", "infonce_bound_loss", "matrix_bound_loss", "fused_mi_bound", "study_id_codes",
           "check_estimator", "jsd_bound_loss", "nwj_bound_loss"]


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
    """The estimator code of the DV entry points; ValueError for the names of the other families and unknown names."""
    if estimator not in ESTIMATORS:
        raise ValueError(f"unknown mi_estimator {estimator!r}: expected one of {sorted(ESTIMATORS)}")
    return ESTIMATORS[estimator]


def _grad_scalar(grad: torch.Tensor) -> torch.Tensor:
    return grad.reshape(-1)[:1].to(torch.float32).contiguous()


# ----------------------------------------------------------------------------------------------------------
# bound on scores computed elsewhere: the reference's logits layout, or a B x B score matrix with study-id masking
# ----------------------------------------------------------------------------------------------------------
class _BoundFn(torch.autograd.Function):
    """loss [1] of the estimator ``est`` on logits [N] whose first ``pos_size`` rows are the positive pairs (``sid``
    None; ``est.bound_entry``) or on a [B, B] score matrix with its study-id codes (``est.matrix_entry``).  For the
    backward the forward keeps the statistics block (families "dv" and "fdiv"; "fdiv" leaves its terms pointer NULL) or
    the row and column log-sum-exps ("nce")."""

    @staticmethod
    def forward(ctx, scores: torch.Tensor, sid, pos_size: int, est):
        lib = _hip.load()
        if sid is None:
            s = _hip.f32c(scores, "discriminator_logits").reshape(-1)
            entry, head = est.bound_entry, (s.numel(), pos_size)
        else:
            s = _hip.f32c(scores, "scores")
            entry, head = est.matrix_entry, (sid.data_ptr(), s.shape[0])
        dev = s.device
        ws = _hip.workspace(getattr(lib, f"{entry}_workspace_bytes")(s.shape[0]), dev)
        if est.family == "nce":
            kept = [torch.empty(s.shape[0], dtype=torch.float32, device=dev) for _ in range(2)]
        else:
            kept = [_hip.new_stats(dev)]
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        outs = [None] * (est.family == "fdiv") + [t.data_ptr() for t in kept]
        _hip.call(f"{entry}_fwd", dev, s.data_ptr(), *head, est.code, loss.data_ptr(), *outs, ws.data_ptr(), ws.numel())
        ctx.save_for_backward(s, sid, *kept)
        ctx.entry, ctx.head, ctx.est, ctx.in_shape = entry, head, est, scores.shape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        s, _sid, *kept = ctx.saved_tensors  # (sid saved: ctx.head holds its address)
        go = _grad_scalar(grad_loss)
        grad = torch.empty_like(s)
        mode = [ctx.est.code] * (ctx.est.family != "dv")  # the DV backward takes the estimator from the statistics
        _hip.call(f"{ctx.entry}_bwd", s.device, s.data_ptr(), *ctx.head, *mode, *[t.data_ptr() for t in kept],
                  go.data_ptr(), grad.data_ptr())
        return grad.reshape(ctx.in_shape), None, None, None


def _bound(discriminator_logits, pos_size, est):
    _hip.require_device(discriminator_logits, "discriminator_logits")
    n = discriminator_logits.shape[0]
    if discriminator_logits.numel() != n:
        raise ValueError("discriminator_logits must be [N] or [N, 1] (one score per pair row)")
    if not 0 <= int(pos_size) <= n:
        raise ValueError(f"pos_size={pos_size} outside [0, {n}]")
    return _BoundFn.apply(discriminator_logits, None, int(pos_size), est)


def dv_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """Donsker-Varadhan bound, reference mi_critics.py:3-12: ``LSE(logits[pos:]) - log(N - pos) - mean(logits[:pos])``.
    ``device`` is kept for signature compatibility (the reference only uses it for the log-N constant)."""
    loss = _bound(discriminator_logits, pos_size, ESTIMATOR_TABLE["dv"])
    return loss.reshape(discriminator_logits.shape[1:])  # [N,1] -> [1] as in the reference


def infonce_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """The reference's "InfoNCE" bound, mi_critics.py:14-23: ``LSE(logits[pos:]) - mean(logits[:pos])`` (no log-N term;
    not a row-wise softmax cross-entropy).  Returns shape []."""
    return _bound(discriminator_logits, pos_size, ESTIMATOR_TABLE["infonce"]).reshape(())


def jsd_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """Jensen-Shannon bound (Deep InfoMax) on the reference's logits layout (the first ``pos_size`` rows positive):
    ``mean(softplus(-logits[:pos])) + mean(softplus(logits[pos:]))``, shape [].  Finite for any finite logits.  ``device``
    is kept for the signature of the reference's callables."""
    return _bound(discriminator_logits, pos_size, ESTIMATOR_TABLE["jsd"]).reshape(())


def nwj_bound_loss(discriminator_logits: torch.Tensor, pos_size: int, device=None) -> torch.Tensor:
    """NWJ bound (f-GAN KL, "MINE-f") on the reference's logits layout: ``exp(LSE(logits[pos:]) - log(N - pos) - 1) -
    mean(logits[:pos])``, shape []; ``-loss`` is the NWJ lower bound on the MI."""
    return _bound(discriminator_logits, pos_size, ESTIMATOR_TABLE["nwj"]).reshape(())


def matrix_bound_loss(scores: torch.Tensor, study_id, estimator: str = "dv") -> torch.Tensor:
    """The reference loss on a [B,B] score matrix S[i,j] = critic(img_i, txt_j): positives are the diagonal, negatives
    the pairs with i != j and different study ids (main_utils.py:99-108).  Shape [1] (dv) / [] (infonce).

    "infonce_rowwise" / "infonce_symmetric": the per-sample InfoNCE on the same scores and masking,
    shape [], gradients to ``scores``.  The way to that loss for any critic whose scores you compute yourself.

    "jsd" / "nwj": the Jensen-Shannon and NWJ bounds on the same pairs, shape []."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    est = check_estimator(estimator)
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    return est.shape_loss(_BoundFn.apply(scores, sid, 0, est))


# ----------------------------------------------------------------------------------------------------------
# fused critics: thin autograd Functions over the ops objects of critic_ops (whole batch: b_rows = b, row_offset = 0)
# ----------------------------------------------------------------------------------------------------------
def _f32_inputs(x, y, params):
    return (_hip.f32c(x, "embedding_img"), _hip.f32c(y, "embedding_txt"),
            [_hip.f32c(p, f"critic param {n}") for n, p in enumerate(params)])


class _CriticFn(torch.autograd.Function):
    """loss = bound(S) of the DV entry points with study-id masking, S from the critic ``kind`` of critic_ops: (X W) Y^T
    (no params: X Y^T), (X Wg)(Y Wh)^T or MLP([x_i ; y_j]) of make_mlp(d,[h1,h2]) (model.py:18-32); forward and all
    gradients by the HIP library.  Returns (loss [1], statistics, scores [B, B] or None)."""

    @staticmethod
    def forward(ctx, kind: str, sid, estimator: int, precision: int, want_scores: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        b = x.shape[0]
        if kind == "bilinear" and params:
            _hip.note_path("bilinear", (b, b, x.shape[1], y.shape[1]), precision)
        elif kind == "separable":
            _hip.note_path("separable", (b, b, x.shape[1], y.shape[1], params[0].shape[1]), precision)
        scores = None
        if want_scores or kind == "concat_mlp":  # the concat-MLP backward reads them
            scores = torch.empty(b, b, dtype=torch.float32, device=x.device)
        ops = OPS[kind]()
        loss, stats, _, scores = out = fwd_outputs(x.device, scores)
        _, saved = ops.forward(x, y, params, sid, sid, 0, estimator, precision, any(ctx.needs_input_grad), out=out)
        ctx.save_for_backward(x, y, sid, stats, scores, saved[-1], *params)
        ctx.ops, ctx.precision = ops, precision
        ctx.mark_non_differentiable(*[t for t in (stats, scores) if t is not None])
        return loss, stats, scores

    @staticmethod
    def backward(ctx, grad_loss, _gs, _gsc):
        x, y, sid, stats, scores, ws, *params = ctx.saved_tensors
        gx, gy, gp = ctx.ops.backward((x, y, params, sid, sid, 0, ctx.precision, scores, ws), stats,
                                      _grad_scalar(grad_loss))
        return (None,) * 5 + (gx, gy, *gp)


class _ChainFn(torch.autograd.Function):
    """The per-sample InfoNCE ("mi_nce") or the Jensen-Shannon / NWJ bound ("mi_fdiv") of the bilinear or separable
    critic in one library call (``ops.chain_step``).  With ``need_grad`` the call also writes every gradient for
    dL/dloss = 1; the backward only scales them by grad_loss.  Returns (loss [1], lse_rows [B], lse_cols [B]) or
    (loss [1], terms [2], None)."""

    @staticmethod
    def forward(ctx, kind: str, entry: str, sid, mode: int, precision: int, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        loss, a, b, grads = OPS[kind]().chain_step(entry, x, y, params, sid, mode, precision, need_grad)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(*[t for t in (a, b) if t is not None])
        return loss, a, b

    @staticmethod
    def backward(ctx, grad_loss, _ga, _gb):
        saved = ctx.saved_tensors
        if not saved:
            raise RuntimeError("_ChainFn: the forward ran without gradients (need_grad=False)")
        go = grad_loss.reshape(-1)[:1].to(torch.float32)
        return (None,) * 6 + tuple(g * go for g in saved)


class _FdivConcatFn(torch.autograd.Function):
    """Jensen-Shannon / NWJ bound of S[i,j] = MLP([x_i ; y_j]) (make_mlp(d,[h1,h2])): the fused forward writes scores,
    sign-bit images and statistics; the backward kernels run under the mode's gradient rule.  Returns (loss [1],
    terms [2], scores [B, B])."""

    @staticmethod
    def forward(ctx, sid, mode: int, precision: int, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
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
        return (None,) * 3 + (gx, gy, *gp)


def _batch_codes(embedding_img, embedding_txt, study_id) -> torch.Tensor:
    """Shape checks of one batch; its study-id codes."""
    if embedding_img.dim() != 2 or embedding_txt.dim() != 2 or embedding_img.shape[0] != embedding_txt.shape[0]:
        raise ValueError("embedding_img / embedding_txt must be [B, d_img] / [B, d_txt]")
    sid = study_id_codes(study_id, embedding_img.device)
    if sid.numel() != embedding_img.shape[0]:
        raise ValueError("study_id length must equal the batch size")
    return sid


def _critic_kind(critic):
    """The critic kind a critic is checked as: anything but a BilinearCritic or a SeparableCritic -- None included, which
    fused_mi_bound then rejects for the estimators of every critic -- is taken for a make_mlp critic (resolve_critic then
    checks that it is one)."""
    from . import model as _model
    if isinstance(critic, _model.BilinearCritic):
        return "bilinear"
    if isinstance(critic, _model.SeparableCritic):
        return "separable"
    return "concat_mlp"


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
    ValueError: take its differentiable score matrix from ``fused_scores.fused_critic_scores`` (the fused kernels, no pair
    matrix) and call ``matrix_bound_loss(scores, study_id, estimator)`` -- ``fused_scores.concat_infonce`` does both.

    ``estimator`` = "jsd" / "nwj" (every critic): the Jensen-Shannon and NWJ bounds, loss of shape
    []; ``return_stats=True`` then gives ``(positive-pair term, negative-pair term)``, two 0-d tensors whose sum is the loss.
    """
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if embedding_img.dtype == torch.float64:
        embedding_img = embedding_img.float()
    if embedding_txt.dtype == torch.float64:
        embedding_txt = embedding_txt.float()
    x, y = embedding_img, embedding_txt
    est = check_estimator(estimator, _critic_kind(critic))
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    sid = _batch_codes(x, y, study_id)
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    scores = None
    if est.family == "dv":
        if prec in (_hip.MI_PREC_BF16X3, _hip.MI_PREC_FP8) and kind != "bilinear":
            raise ValueError(f'precision="{precision}" is implemented for BilinearCritic only')
        if prec in (_hip.MI_PREC_F16, _hip.MI_PREC_F16X3) and kind != "concat_mlp":
            raise ValueError(f'precision="{precision}" is the fp16-operand mode of the make_mlp critic (its generated '
                             'operand relu(U_i + V_j) is formed by packed fp16 arithmetic); use "bf16" for this critic')
        if kind == "separable" and return_scores:  # per-pair scores are a diagnostic output: eager projections + the
            kind, x, y, params = "bilinear", critic.project_img(x), critic.project_txt(y), []  # bilinear form, W = None
        loss, stats, scores = _CriticFn.apply(kind, sid, est.code, prec, bool(return_scores), x, y, *params)
    elif kind == "concat_mlp":
        loss, terms, scores = _FdivConcatFn.apply(sid, est.code, prec, x, y, *params)
        stats = (terms[0], terms[1])
    else:
        # "f32": bf16x3 on the bilinear critic where every size is a multiple of 8, exact fp32 products otherwise (the
        # library rejects fp8 / f16 / f16x3 for these critics)
        need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
        loss, a, b = _ChainFn.apply(kind, est.chain_entry, sid, est.code, prec, need_grad, x, y, *params)
        stats = (a, b) if b is not None else (a[0], a[1])
        if return_scores:  # diagnostic output: no gradient flows through it
            with torch.no_grad():
                a, c, w = ((x, y, [critic.weight]) if kind == "bilinear" else
                           (critic.project_img(x), critic.project_txt(y), []))  # the projections, as for "dv"
                scores = _CriticFn.apply("bilinear", sid, _hip.MI_DV, prec, True, a, c, *w)[2]
    out = [est.shape_loss(loss)]
    if return_scores:
        out.append(scores)
    if return_stats:
        out.append(stats)
    return out[0] if len(out) == 1 else tuple(out)
