"""Soft-target InfoNCE from finding-label bit masks: the per-sample image-report contrastive loss whose targets follow
the similarity of the studies' finding sets (soft targets as in SoftCLIP and label-aware
contrast, or label smoothing with structure).

Every other contrastive loss of the package takes two different studies for a true negative.  On chest X-rays that is
often wrong: many studies carry the same findings ("No Finding", "Support Devices" plus "Pleural Effusion", ...), their
reports are near-paraphrases, and the loss spends its gradient pushing them apart.  The dataset ships a CheXpert / NegBio
label table with 14 findings per study (``load_label_table``); this loss reads it.  With ``S[i, j] = critic(img_i,
txt_j)`` over a batch of B pairs, one label mask per sample ``lab_i`` (an int64 whose low 63 bits are a multi-hot set of
findings) and two floats ``tau > 0`` and ``mix`` in [0, 1]:

    n_i   = popcount(lab_i)
    a_ij  = popcount(lab_i & lab_j) / sqrt(n_i n_j)      (0 where n_i n_j = 0);   a_ii := 1 always
    k_ij  = exp((a_ij - 1) / tau)                         (<= 1, k_ii = 1, k_ij == k_ji bit for bit)
    z_i   = sum_j k_ij                                    (>= 1; serves rows and, k being symmetric, columns)
    qr_ij = (1 - mix) delta_ij + mix k_ij / z_i           qc_ij = (1 - mix) delta_ij + mix k_ij / z_j
    r_i   = log sum_j exp S[i, j]     c_j = log sum_i exp S[i, j]          (nothing is masked)
    row term     t_i  = r_i - sum_j qr_ij S[i, j]
    column term  t'_j = c_j - sum_i qc_ij S[i, j]
    row-wise:  L = mean_i t_i            symmetric:  L = 1/2 mean_i t_i + 1/2 mean_j t'_j
    dL/dS[i, j] = w_r (exp(S[i, j] - r_i) - qr_ij) + w_c (exp(S[i, j] - c_j) - qc_ij)

- ``mix = 0`` IS the loss of ``fused_mi_bound(..., "infonce_rowwise" / "infonce_symmetric")`` on unique ids: the same r,
  c, loss and gradients.
- Every mask equal and ``mix = 1``: the study-positive loss (``study_positives``) with all ids equal,
  ``t_i = r_i - mean_j S[i, j]``.
- One distinct bit per study (at most 63 studies), ``mix = 1`` and a small ``tau`` (0.02): the study-positive loss with
  those study ids.
- All masks zero gives uniform smoothing of weight ``exp(-1 / tau)`` off the diagonal.
- ``B = 1`` gives loss exactly 0.0 and exact-zero gradients.
- Each row's share of dL/dS sums to zero.

Labels are multi-hot SETS, not float label vectors, on purpose: the similarity of a pair is then one AND, one popcount
and one multiply against two per-sample ``1 / sqrt(n)`` values, cheap enough to recompute in both GEMM epilogues, so no
B x B target matrix ever exists.  A caller with soft label scores thresholds them (``label_masks(scores > 0.5)``); float
label vectors are out of scope.  Bit 63 of a mask is ignored on the device; ``label_masks`` rejects it.

THIS IS A TRAINING LOSS, NOT A MUTUAL-INFORMATION BOUND: ``log B - L`` bounds nothing once ``mix > 0``.  It is therefore
not an estimator name of ``fused_mi_bound``; it is a switch on the row-wise and symmetric losses, reached through the
functions below (and ``MultiModalManager(soft_targets=...)`` / ``train.py --soft_targets``).  It runs eagerly on one GPU:
there is no graphed and no sharded form.

Loss and every gradient are HIP kernels behind the C ABI (``mi_softnce_*`` / ``mi_matrix_softnce_*`` in
``include/mi_critic.h``): one launch turns the masks into z, the score matrix is never materialised, the per-row and
per-column statistics are an epilogue of the score GEMM, the gradient weights an epilogue of the G GEMM; no float atomics
anywhere, identical bits from call to call.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import csv
import math

import torch

from . import _hip
from .critic_ops import OPS, resolve_critic, softnce_matrix_bwd, softnce_matrix_fwd
from .mi_critics import _critic_kind, _f32_inputs, _grad_scalar
from .utils import study_id_to_int64

__all__ = ["label_masks", "load_label_table", "label_key", "soft_target_infonce", "matrix_soft_target_infonce"]

MAX_LABELS = _hip.MI_SOFTNCE_MAX_LABELS
_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def _mode(symmetric: bool) -> int:
    return _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE


def check_tau_mix(tau, mix):
    """(tau, mix) as floats; ValueError unless tau is finite and > 0 and mix lies in [0, 1]."""
    if isinstance(tau, bool) or isinstance(mix, bool):
        raise TypeError("tau and mix must be numbers")
    tau, mix = float(tau), float(mix)
    if not (math.isfinite(tau) and tau > 0.0):
        raise ValueError(f"tau must be finite and > 0 (got {tau})")
    if not 0.0 <= mix <= 1.0:
        raise ValueError(f"mix must be in [0, 1] (got {mix})")
    return tau, mix


def label_masks(labels) -> torch.Tensor:
    """int64 [B] label masks (bit f set <=> finding f present) on the device of ``labels`` (CPU for arrays and lists).

    ``labels`` is either a bool / 0-1 ``[B, n_lab]`` tensor or array with ``n_lab <= 63`` (any other value raises), or an
    int64 ``[B]`` tensor of ready masks (a negative value -- bit 63 -- raises).  Soft label scores are thresholded by the
    caller: ``label_masks(scores > 0.5)``."""
    t = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
    if t.dim() == 1:
        if t.dtype != torch.int64:
            raise TypeError(f"ready label masks must be int64 [B] (got {t.dtype}); multi-hot labels are [B, n_lab]")
        if t.numel() and bool((t < 0).any()):
            raise ValueError("label masks must be non-negative: bit 63 is not a label (at most 63 findings)")
        return t.contiguous()
    if t.dim() != 2:
        raise ValueError("labels must be a multi-hot [B, n_lab] tensor or an int64 [B] tensor of masks")
    if t.shape[1] > MAX_LABELS:
        raise ValueError(f"at most {MAX_LABELS} labels fit a mask (got {t.shape[1]})")
    if t.dtype != torch.bool:
        if t.numel() and not bool(((t == 0) | (t == 1)).all()):
            raise ValueError("multi-hot labels must be bool or hold only 0 and 1 (threshold soft label scores first)")
        t = t != 0
    weights = torch.ones(t.shape[1], dtype=torch.int64, device=t.device) << torch.arange(t.shape[1], device=t.device)
    return (t.to(torch.int64) * weights).sum(dim=1)


def label_key(study_id) -> str:
    """The key of a study id in a label table: the normalisation of ``mi_critics.study_id_codes`` (the numeric value of
    ids like "50414267"), after dropping the "s" of MIMIC-CXR folder names, so "s50414267" and 50414267 meet."""
    if torch.is_tensor(study_id):
        study_id = study_id.item()
    if isinstance(study_id, float) and study_id.is_integer():
        study_id = int(study_id)
    if isinstance(study_id, str):
        study_id = study_id.strip()
        if len(study_id) > 1 and study_id[0] in "sS" and study_id[1:].isdigit():
            study_id = study_id[1:]
    return str(study_id_to_int64(study_id))


def load_label_table(csv_path, uncertain_positive: bool = False) -> dict:
    """``{study id string: mask}`` from a CheXpert / NegBio label table (``training_label_negbio.csv``), or any CSV with
    a ``study_id`` column: every other column except ``subject_id`` is a finding, in file order (more than 63 raise).  A
    cell > 0 sets the finding's bit, a cell == -1 (uncertain) sets it only with ``uncertain_positive``, blank or 0 leaves
    it clear.  Keys are ``label_key`` of the ids."""
    table = {}
    with open(csv_path, newline="") as f:
        reader = csv.reader(f)
        header = [h.strip() for h in next(reader, [])]
        if "study_id" not in header:
            raise ValueError(f"{csv_path}: no study_id column")
        sid_col = header.index("study_id")
        findings = [n for n, h in enumerate(header) if n != sid_col and h != "subject_id"]
        if len(findings) > MAX_LABELS:
            raise ValueError(f"{csv_path}: {len(findings)} finding columns, at most {MAX_LABELS} fit a mask")
        for line, row in enumerate(reader, start=2):
            if not row or all(not c.strip() for c in row):
                continue
            mask = 0
            for bit, col in enumerate(findings):
                cell = row[col].strip() if col < len(row) else ""
                if not cell:
                    continue
                try:
                    v = float(cell)
                except ValueError:
                    raise ValueError(f"{csv_path} line {line}: label {cell!r} in column {header[col]!r}") from None
                if v > 0.0 or (uncertain_positive and v == -1.0):
                    mask |= 1 << bit
            table[label_key(row[sid_col])] = mask
    return table


def _device_masks(labels, device, b: int) -> torch.Tensor:
    lab = label_masks(labels).to(device)
    if lab.numel() != b:
        raise ValueError("labels length must equal the batch size B")
    return lab


class _SoftNceFn(torch.autograd.Function):
    """The soft-target InfoNCE of the bilinear or separable critic in one library call (``ops.softnce_step``), as
    ``study_positives._PosNceFn``: with ``need_grad`` the call also writes every gradient for dL/dloss = 1 and the
    backward only scales them.  Returns (loss [1], lse_rows, lse_cols, target_norm)."""

    @staticmethod
    def forward(ctx, kind: str, lab, mode: int, precision: int, tau: float, mix: float, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        loss, r, c, z, grads = OPS[kind]().softnce_step(x, y, params, lab, mode, precision, tau, mix, need_grad)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(r, c, z)
        return loss, r, c, z

    @staticmethod
    def backward(ctx, grad_loss, *_):
        saved = ctx.saved_tensors
        if not saved:
            raise RuntimeError("_SoftNceFn: the forward ran without gradients (need_grad=False)")
        go = grad_loss.reshape(-1)[:1].to(torch.float32)
        return (None,) * 7 + tuple(g * go for g in saved)


class _MatrixSoftNceFn(torch.autograd.Function):
    """The soft-target InfoNCE of a [B, B] score matrix (mi_matrix_softnce_fwd / _bwd); the backward reads the forward's
    LSEs and target norms and writes the dense gradient of the scores."""

    @staticmethod
    def forward(ctx, scores, lab, mode: int, tau: float, mix: float):
        s = _hip.f32c(scores, "scores")
        loss, r, c, z = softnce_matrix_fwd(s, lab, mode, tau, mix)
        ctx.save_for_backward(s, lab, r, c, z)
        ctx.mode, ctx.tau, ctx.mix = mode, tau, mix
        ctx.mark_non_differentiable(r, c, z)
        return loss, r, c, z

    @staticmethod
    def backward(ctx, grad_loss, *_):
        s, lab, r, c, z = ctx.saved_tensors
        g = softnce_matrix_bwd(s, lab, ctx.mode, ctx.tau, ctx.mix, r, c, z, _grad_scalar(grad_loss))
        return g, None, None, None, None


def soft_target_infonce(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, labels, critic, *, tau, mix,
                        symmetric: bool = True, precision: str = "f32", return_stats: bool = False):
    """The soft-target InfoNCE (module docstring) of the batch under ``critic``, a 0-d tensor carrying autograd to the
    embeddings and the critic's parameters.  A training loss, not an MI bound.

    ``labels``: anything ``label_masks`` takes -- a multi-hot ``[B, n_lab]`` tensor / array (threshold soft label scores
    first) or int64 ``[B]`` masks.  ``tau`` and ``mix`` are required keywords: ``tau > 0`` is the temperature of the label
    similarity, ``mix`` in [0, 1] the weight of the soft targets against the one-hot target.

    ``critic``: a ``BilinearCritic`` or a ``SeparableCritic``.  One library call runs the label-norm launch, prep and
    T = X W, the score GEMM whose epilogue writes the row / column records (LSE parts and the q-weighted score sums), the
    merge, the loss, and -- when an input needs a gradient -- the G GEMM whose epilogue applies the formula above,
    followed by the backward products of the per-sample InfoNCE.  The backward pass only scales the saved gradients.  A
    ``make_mlp`` critic has no GEMM form and raises ValueError: take its differentiable score matrix from
    ``fused_scores.fused_critic_scores`` and call ``matrix_soft_target_infonce(scores, labels, tau=..., mix=...)`` --
    ``fused_scores.concat_soft_target_infonce`` does both.

    ``precision`` as for the per-sample InfoNCE of ``fused_mi_bound``: "f32" (bf16x3 on the bilinear critic where every
    size is a multiple of 8, exact fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8", "f16" and "f16x3"
    raise ValueError.

    ``return_stats=True``: ``(loss, {"lse_rows": r, "lse_cols": c, "target_norm": z})`` -- float32 [B] each."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a BilinearCritic or a SeparableCritic")
    if _critic_kind(critic) == "concat_mlp":
        raise ValueError("soft_target_infonce is implemented for the bilinear and separable critics only; for scores you "
                         "compute yourself (e.g. a make_mlp critic applied to every pair) use "
                         "matrix_soft_target_infonce(scores, labels, tau=..., mix=...)")
    tau, mix = check_tau_mix(tau, mix)
    x = embedding_img.float() if embedding_img.dtype == torch.float64 else embedding_img
    y = embedding_txt.float() if embedding_txt.dtype == torch.float64 else embedding_txt
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
        raise ValueError("embedding_img / embedding_txt must be [B, d_img] / [B, d_txt]")
    lab = _device_masks(labels, x.device, x.shape[0])
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    if prec not in _CHAIN_PRECISIONS:
        raise ValueError(f'precision="{precision}" is not available for the soft-target InfoNCE of the {kind} critic '
                         '(use "f32", "f32_exact", "bf16" or "bf16x3")')
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    loss, r, c, z = _SoftNceFn.apply(kind, lab, _mode(symmetric), prec, tau, mix, need_grad, x, y, *params)
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "target_norm": z}) if return_stats else loss


def matrix_soft_target_infonce(scores: torch.Tensor, labels, *, tau, mix, symmetric: bool = True,
                               return_stats: bool = False):
    """The soft-target InfoNCE (module docstring) of a float32 [B, B] score matrix you computed, S[i, j] =
    critic(img_i, txt_j): a 0-d tensor with gradients to ``scores`` (dense).  The way to this loss for any critic, e.g. a
    ``make_mlp`` critic applied to every pair.  A training loss, not an MI bound.  ``labels``, ``tau``, ``mix`` and
    ``return_stats`` as in ``soft_target_infonce``."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    tau, mix = check_tau_mix(tau, mix)
    lab = _device_masks(labels, scores.device, scores.shape[0])
    loss, r, c, z = _MatrixSoftNceFn.apply(scores, lab, _mode(symmetric), tau, mix)
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "target_norm": z}) if return_stats else loss
