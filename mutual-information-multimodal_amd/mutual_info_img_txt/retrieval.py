"""Image-report retrieval: where does each image's own report rank among all reports, and each report's image among all
images (ConVIRT, CLIP and the chest X-ray retrieval literature); recall@K, median rank and MRR summarise it.

With ``S[i, j] = critic(img_i, txt_j)`` over a batch of B pairs, positives ``(i, i)``, and the package's masking -- a
pair ``i != j`` with equal study ids is dropped, neither a hit nor a miss:

    rank_i2t[i] = #{ j : sid_j != sid_i and S[i, j] > S[i, i] }        image  -> report
    rank_t2i[j] = #{ i : sid_i != sid_j and S[i, j] > S[j, j] }        report -> image

0-based int32; strictly greater, so a tie counts for the true pair.  The counts are taken by HIP kernels through the C
ABI (``mi_rank_*`` in ``include/mi_critic.h``); there is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _hip
from .critic_ops import OPS, rank_matrix, resolve_critic
from .mi_critics import _batch_codes, _CriticFn, _f32_inputs, study_id_codes

__all__ = ["retrieval_ranks", "matrix_retrieval_ranks", "retrieval_metrics"]

_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def retrieval_ranks(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic,
                    precision: str = "f32") -> Tuple[torch.Tensor, torch.Tensor]:
    """(rank_i2t, rank_t2i), int32 [B] each, of the batch under ``critic``.

    ``critic`` and ``precision`` are those of ``fused_mi_bound``: a ``BilinearCritic`` or ``SeparableCritic`` runs the
    forward half of the GEMM chain with a counting epilogue (``mi_rank_bilinear`` / ``mi_rank_separable``) and never
    holds a [B, B] matrix -- precisions "f32" (bf16x3 on the bilinear critic where every size is a multiple of 8, exact
    fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8", "f16" and "f16x3" raise ValueError.  A ``make_mlp``
    critic has no GEMM form: its scores exist only in its fused forward, so this path runs that forward for the scores
    and HOLDS THE [B, B] fp32 SCORE MATRIX (4 B^2 bytes) before counting (``mi_rank_matrix``).

    Evaluation only: the inputs are detached and nothing here takes part in autograd."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    with torch.no_grad():
        x, y = embedding_img.detach().float(), embedding_txt.detach().float()
        sid = _batch_codes(x, y, study_id)
        kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
        params = [p.detach() for p in params]
        if kind == "concat_mlp":
            scores = _CriticFn.apply(kind, sid, _hip.MI_DV, prec, True, x, y, *params)[2]
            return rank_matrix(scores, sid)
        if prec not in _CHAIN_PRECISIONS:
            raise ValueError(f'precision="{precision}" is not available for the retrieval ranks of the {kind} critic '
                             '(use "f32", "f32_exact", "bf16" or "bf16x3")')
        x, y, params = _f32_inputs(x, y, params)
        return OPS[kind]().rank_step(x, y, params, sid, prec)


def matrix_retrieval_ranks(scores: torch.Tensor, study_id) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rank_i2t, rank_t2i), int32 [B] each, of a [B, B] score matrix you computed: S[i, j] = critic(img_i, txt_j)."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B, B]")
    sid = study_id_codes(study_id, scores.device)
    if sid.numel() != scores.shape[0]:
        raise ValueError("study_id length must equal B")
    return rank_matrix(_hip.f32c(scores.detach(), "scores"), sid)


def retrieval_metrics(ranks: torch.Tensor, ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """Summary of 0-based ranks [B] (any integer dtype, any device): ``recall@K`` = mean(rank < K) for each K,
    ``median_rank`` (1-based; the mean of the two middle values for an even B) and ``mrr`` = mean(1 / (rank + 1)).
    Plain torch in fp64 on the host, so equal ranks give equal figures wherever they were counted."""
    r = torch.as_tensor(ranks).detach().reshape(-1).cpu().to(torch.float64)
    if r.numel() == 0:
        raise ValueError("ranks is empty")
    out = {f"recall@{int(k)}": float((r < int(k)).to(torch.float64).mean()) for k in ks}
    s = torch.sort(r).values
    n = s.numel()
    out["median_rank"] = float((s[(n - 1) // 2] + s[n // 2]) / 2) + 1.0
    out["mrr"] = float((1.0 / (r + 1.0)).mean())
    return out
