"""Image-report retrieval: where does each image's own report rank among all reports, and each report's image among all
images (ConVIRT, CLIP and the chest X-ray retrieval literature); recall@K, median rank and MRR summarise it.

With ``S[i, j] = critic(img_i, txt_j)`` over a batch of B pairs, positives ``(i, i)``, and the package's masking -- a
pair ``i != j`` with equal study ids is dropped, neither a hit nor a miss:

    rank_i2t[i] = #{ j : sid_j != sid_i and S[i, j] > S[i, i] }        image  -> report
    rank_t2i[j] = #{ i : sid_i != sid_j and S[i, j] > S[j, j] }        report -> image

0-based int32; strictly greater, so a tie counts for the true pair.  The counts are taken by HIP kernels through the C
ABI (``mi_rank_*`` in ``include/mi_critic.h``); there is no CPU path: CPU tensors raise.

The ranks say where the true pair stands inside one square batch.  ``retrieval_topk`` says WHICH items were retrieved,
over a gallery: N query images against M != N candidate reports and the other way round, without an [N, M] matrix
(``mi_topk_*``).  The result of a query is its first k candidates in the total order "score
descending, then candidate index ascending"; relevance is defined by the ids, not by position (``gallery_recall``).
Called with the ids, equal-id candidates are left out: the lists are then the hard negatives of a contrastive trainer.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _hip
from .critic_ops import OPS, rank_matrix, resolve_critic, topk_matrix
from .mi_critics import _batch_codes, _CriticFn, _f32_inputs, study_id_codes

__all__ = ["retrieval_ranks", "matrix_retrieval_ranks", "retrieval_metrics", "retrieval_topk", "matrix_topk",
           "gallery_recall"]

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


# ------------------------------------------------------------------------------------------------ top-k over a gallery
_DIRECTIONS = ("i2t", "t2i")


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= _hip.MI_TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {_hip.MI_TOPK_MAX_K}] (got {k})")
    return k


def _id_codes(ids_a, ids_b, n_a: int, n_b: int, names, device):
    """The two id code tensors of a top-k call (both None: nothing excluded)."""
    if (ids_a is None) != (ids_b is None):
        raise ValueError(f"pass {names[0]} and {names[1]}, or neither")
    if ids_a is None:
        return None, None
    a, b = study_id_codes(ids_a, device), study_id_codes(ids_b, device)
    if a.numel() != n_a or b.numel() != n_b:
        raise ValueError(f"{names[0]} / {names[1]} must have one id per row: {n_a} and {n_b}")
    return a, b


def retrieval_topk(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, critic, k: int, precision: str = "f32",
                   img_ids=None, txt_ids=None, directions: Sequence[str] = _DIRECTIONS) -> Dict[str, tuple]:
    """``{"i2t": (idx, val), "t2i": (idx, val)}`` (the directions asked for): for every image the ``k`` best reports
    (idx int32 [n_img, k] into ``embedding_txt``, val float32 the kernel's score of each), for every report the ``k`` best
    images ([n_txt, k] into ``embedding_img``).  Best = score descending, ties by the lower index.  ``n_img != n_txt`` is
    fine: one image set against a gallery of reports.  Where fewer than ``k`` candidates remain the tail is idx = -1,
    val = -inf.  ``k`` is at most 32.

    With ``img_ids`` and ``txt_ids`` (study ids, as everywhere in the package) a candidate whose id equals the query's is
    left out -- the true pair included -- so the lists are the HARD NEGATIVES of each query: what a contrastive trainer
    mines.  Without ids nothing is left out: the retrieval evaluation (``gallery_recall`` of the result).

    ``critic`` and ``precision`` resolve as in ``retrieval_ranks``: a ``BilinearCritic`` or ``SeparableCritic`` runs the
    forward half of the GEMM chain with an inserting epilogue (``mi_topk_bilinear`` / ``mi_topk_separable``) and holds
    no [n_img, n_txt] matrix; "f32" is bf16x3 on the bilinear critic where both counts and both widths are multiples of
    8.  A ``make_mlp`` critic works for ``n_img == n_txt`` only: its scores exist only in its fused forward, which is
    square, so this path HOLDS THE [B, B] fp32 SCORES and selects with ``mi_topk_matrix``; for a rectangular gallery
    compute the scores yourself and call ``matrix_topk``.  Evaluation only: inputs are detached, no autograd."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a make_mlp critic, a BilinearCritic or a SeparableCritic")
    k = _check_k(k)
    directions = tuple(directions)
    if not directions or any(d not in _DIRECTIONS for d in directions):
        raise ValueError(f'directions must name "i2t", "t2i" or both (got {directions!r})')
    if embedding_img.dim() != 2 or embedding_txt.dim() != 2:
        raise ValueError("embedding_img / embedding_txt must be [n_img, d_img] / [n_txt, d_txt]")
    i2t, t2i = "i2t" in directions, "t2i" in directions
    with torch.no_grad():
        x, y = embedding_img.detach().float(), embedding_txt.detach().float()
        (n_img, dx), (n_txt, dy) = x.shape, y.shape
        sid_img, sid_txt = _id_codes(img_ids, txt_ids, n_img, n_txt, ("img_ids", "txt_ids"), x.device)
        kind, params, prec = resolve_critic(critic, precision, n_img, dx, dy)
        params = [p.detach() for p in params]
        out = {}
        if kind == "concat_mlp":
            if n_img != n_txt:
                raise ValueError("a make_mlp critic scores square batches only (n_img == n_txt): for a rectangular gallery "
                                 "compute the [n_img, n_txt] scores yourself and call matrix_topk")
            sid = sid_img if sid_img is not None else torch.arange(n_img, dtype=torch.int64, device=x.device)
            scores = _CriticFn.apply(kind, sid, _hip.MI_DV, prec, True, x, y, *params)[2]
            if i2t:
                out["i2t"] = topk_matrix(scores, k, 0, sid_img, sid_txt)
            if t2i:
                out["t2i"] = topk_matrix(scores, k, 1, sid_img, sid_txt)
            return out
        # "f32" on a rectangular call: both counts take part in the multiple-of-8 rule
        prec = _hip.resolve_precision(precision, kind == "bilinear" and bool(params), (n_img, n_txt, dx, dy))
        if prec not in _CHAIN_PRECISIONS:
            raise ValueError(f'precision="{precision}" is not available for the top-k retrieval of the {kind} critic '
                             '(use "f32", "f32_exact", "bf16" or "bf16x3")')
        x, y, params = _f32_inputs(x, y, params)
        out_i, out_t = OPS[kind]().topk_step(x, y, params, sid_img, sid_txt, prec, k, i2t, t2i)
        if i2t:
            out["i2t"] = out_i
        if t2i:
            out["t2i"] = out_t
        return out


def matrix_topk(scores: torch.Tensor, k: int, axis: int = 0, row_ids=None, col_ids=None):
    """(idx int32, val float32) of a [n_rows, n_cols] score matrix you computed: ``axis`` 0 gives each row's ``k`` best
    columns ([n_rows, k]), ``axis`` 1 each column's ``k`` best rows ([n_cols, k]); order, tail and ``row_ids`` /
    ``col_ids`` (equal-id candidates left out) as in ``retrieval_topk``."""
    _hip.require_device(scores, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be [n_rows, n_cols]")
    if axis not in (0, 1):
        raise ValueError("axis must be 0 (each row's best columns) or 1 (each column's best rows)")
    k = _check_k(k)
    sid_rows, sid_cols = _id_codes(row_ids, col_ids, scores.shape[0], scores.shape[1], ("row_ids", "col_ids"), scores.device)
    return topk_matrix(_hip.f32c(scores.detach(), "scores"), k, axis, sid_rows, sid_cols)


def gallery_recall(idx: torch.Tensor, query_ids, gallery_ids, ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """Summary of retrieved indices [n_q, k] (one direction of ``retrieval_topk`` run WITHOUT ids) under id relevance: a
    retrieved entry hits when its gallery id equals the query's id, so a study with several images or reports has
    several right answers; -1 entries never hit.  ``recall@K`` is the share of queries with a hit among their first K
    entries (K > k raises ValueError) and ``mrr`` the mean of 1 / (1-based place of the first hit), 0 where none of the
    k entries hits.  Plain torch in fp64 on the host."""
    i = torch.as_tensor(idx).detach().cpu().long()
    if i.dim() != 2 or i.shape[0] == 0:
        raise ValueError("idx must be [n_q, k] with at least one query")
    q, g = study_id_codes(query_ids, "cpu"), study_id_codes(gallery_ids, "cpu")
    if q.numel() != i.shape[0]:
        raise ValueError("query_ids must have one id per row of idx")
    if int(i.max()) >= g.numel():
        raise ValueError("idx points outside gallery_ids")
    k = i.shape[1]
    hit = (i >= 0) & (g[i.clamp(min=0)] == q[:, None])
    out = {}
    for kk in ks:
        if not 1 <= int(kk) <= k:
            raise ValueError(f"recall@{int(kk)} needs at least {int(kk)} retrieved entries per query (idx has {k})")
        out[f"recall@{int(kk)}"] = float(hit[:, :int(kk)].any(dim=1).to(torch.float64).mean())
    first = torch.where(hit.any(dim=1), hit.to(torch.int64).argmax(dim=1), torch.full((i.shape[0],), -1))
    out["mrr"] = float(torch.where(first >= 0, 1.0 / (first.to(torch.float64) + 1.0),
                                   torch.zeros(i.shape[0], dtype=torch.float64)).mean())
    return out
