"""How much mutual information has a trained critic found?  Every bound of the package and SMILE, as ESTIMATES (higher
means more MI, in nats; none of them is a loss), from one forward sweep over the scores of a validation batch.

With ``S[i, j] = critic(img_i, txt_j)`` over a batch of B pairs and the package's pairs -- positives ``(i, i)``, negatives
``i != j`` with different study ids (``n_neg`` of them), equal-id off-diagonal pairs dropped -- and ``sp(x) = log(1 +
e^x)``:

    dv        mean_pos s - (LSE_neg s - log n_neg)                      Donsker-Varadhan
    nwj       mean_pos s - exp(LSE_neg s - log n_neg - 1)               Nguyen-Wainwright-Jordan ("MINE-f")
    jsd       -(mean_pos sp(-s) + mean_neg sp(s))                       add 2 log 2 for the Jensen-Shannon divergence
    nce_i2t   (1/B) sum_i (S_ii - r_i + log |C_i|)                      per-sample InfoNCE, image -> report
    nce_t2i   (1/B) sum_j (S_jj - c_j + log |R_j|)                      ... report -> image
    pos_mean  mean_pos s        neg_mean  mean_neg s        log_n_neg  log n_neg
    smile[k]  mean_pos s - (log sum_neg exp(clip(s, -tau_k, tau_k)) - log n_neg)    Song & Ermon 2020: clipped DV

``r_i``, ``c_j`` are the row and column log-sum-exps of the per-sample InfoNCE over the candidates ``C_i``, ``R_j``
(DESIGN.md section 8); with unique ids ``nce_i2t = log B - infonce_rowwise``.  A clip at or above every negative score
makes SMILE equal DV.  Without negatives (every id equal, B == 1) ``dv``, ``nwj``, ``jsd``, ``neg_mean`` and ``smile``
are NaN, ``log_n_neg`` is -inf and ``nce_*`` is exactly 0.

The values come from HIP kernels through the C ABI (``mi_estimates_*`` in ``include/mi_critic.h``); there is no CPU
path: CPU tensors raise.  Forward only: the inputs are detached and nothing here takes part in autograd.  These are not
estimator names of ``fused_mi_bound``.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import torch

from . import _hip
from .critic_ops import OPS, estimates_matrix, resolve_critic
from .mi_critics import _batch_codes, _f32_inputs, study_id_codes

__all__ = ["mi_estimates", "matrix_mi_estimates", "ESTIMATE_NAMES"]

# name -> slot of the scalar outputs (``smile`` is the [n_tau] tail from _hip.MI_EST_SMILE on)
ESTIMATE_NAMES = {"dv": _hip.MI_EST_DV, "nwj": _hip.MI_EST_NWJ, "jsd": _hip.MI_EST_JSD, "nce_i2t": _hip.MI_EST_NCE_I2T,
                  "nce_t2i": _hip.MI_EST_NCE_T2I, "pos_mean": _hip.MI_EST_POS_MEAN, "neg_mean": _hip.MI_EST_NEG_MEAN,
                  "log_n_neg": _hip.MI_EST_LOG_N_NEG}

_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)
_CONCAT_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_F16, _hip.MI_PREC_F16X3)


def _check_taus(taus) -> Tuple[float, ...]:
    """The clips as floats: at most MI_EST_MAX_TAUS of them, each finite with 0 < tau <= 40 (ValueError otherwise)."""
    try:
        out = tuple(float(t) for t in taus)
    except TypeError:
        raise ValueError(f"taus must be a sequence of at most {_hip.MI_EST_MAX_TAUS} clips (got {taus!r})") from None
    if len(out) > _hip.MI_EST_MAX_TAUS:
        raise ValueError(f"at most {_hip.MI_EST_MAX_TAUS} clips per call (got {len(out)})")
    for t in out:
        if not (math.isfinite(t) and 0.0 < t <= 40.0):
            raise ValueError(f"every tau must be finite with 0 < tau <= 40 (got {t})")
    return out


def _as_dict(est: torch.Tensor, n_tau: int) -> Dict[str, torch.Tensor]:
    """Views of the one output tensor: 0-dim per name, ``smile`` [n_tau]."""
    out = {name: est[slot] for name, slot in ESTIMATE_NAMES.items()}
    out["smile"] = est[_hip.MI_EST_SMILE:_hip.MI_EST_SMILE + n_tau]
    return out


def mi_estimates(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic,
                 taus: Sequence[float] = (1.0, 5.0), precision: str = "f32") -> Dict[str, torch.Tensor]:
    """``{"dv", "nwj", "jsd", "nce_i2t", "nce_t2i", "pos_mean", "neg_mean", "log_n_neg"}`` -> 0-dim float32 tensors and
    ``"smile"`` -> float32 [len(taus)], of the batch under ``critic``; all of them views of one device tensor, nothing
    synchronises.

    ``critic`` and ``precision`` resolve as in ``retrieval.retrieval_ranks``: a ``BilinearCritic`` or ``SeparableCritic``
    runs the forward half of the GEMM chain with a statistics epilogue (``mi_estimates_bilinear`` /
    ``mi_estimates_separable``: one score sweep, no [B, B] matrix) -- precisions "f32" (bf16x3 on the bilinear critic
    where every size is a multiple of 8, exact fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8", "f16" and
    "f16x3" raise ValueError.  A ``make_mlp`` critic has no GEMM form: its fused forward gives the [B, B] fp32 scores
    ("f32", "f32_exact", "bf16", "f16"), which ``mi_estimates_matrix`` then reads once.

    ``taus``: at most 4 SMILE clips, each in (0, 40]."""
    taus = _check_taus(taus)
    if not torch.is_tensor(embedding_img) or not torch.is_tensor(embedding_txt):
        raise TypeError("embedding_img / embedding_txt must be torch.Tensors")
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    if embedding_img.dim() != 2 or embedding_txt.dim() != 2 or embedding_img.shape[0] != embedding_txt.shape[0]:
        raise ValueError("embedding_img / embedding_txt must be [B, d_img] / [B, d_txt]")
    kind, params, prec = resolve_critic(critic, precision, embedding_img.shape[0], embedding_img.shape[1],
                                        embedding_txt.shape[1])
    allowed = _CONCAT_PRECISIONS if kind == "concat_mlp" else _CHAIN_PRECISIONS
    if prec not in allowed:
        names = '"f32", "f32_exact", "bf16" or "f16"' if kind == "concat_mlp" else '"f32", "f32_exact", "bf16" or "bf16x3"'
        raise ValueError(f'precision="{precision}" is not available for the MI estimates of the {kind} critic (use {names})')
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    with torch.no_grad():
        x, y = embedding_img.detach().float(), embedding_txt.detach().float()
        sid = _batch_codes(x, y, study_id)
        x, y, params = _f32_inputs(x, y, [p.detach() for p in params])
        if kind == "concat_mlp":
            scores, _saved = OPS[kind]().scores_forward(x, y, params, prec, need_grad=False)
            est = estimates_matrix(scores, sid, taus)
        else:
            est = OPS[kind]().estimates_step(x, y, params, sid, prec, taus)
    return _as_dict(est, len(taus))


def matrix_mi_estimates(scores: torch.Tensor, study_id, taus: Sequence[float] = (1.0, 5.0)) -> Dict[str, torch.Tensor]:
    """The dict of ``mi_estimates`` for a [B, B] score matrix you computed: S[i, j] = critic(img_i, txt_j)."""
    taus = _check_taus(taus)
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    with torch.no_grad():
        est = estimates_matrix(_hip.f32c(scores.detach(), "scores"), sid, taus)
    return _as_dict(est, len(taus))
