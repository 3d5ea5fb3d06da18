"""Per-sample InfoNCE against a memory bank of past embeddings.

With unique study ids and ``n`` candidates per query the per-sample InfoNCE cannot rise above ``log n``, and in
``fused_mi_bound`` ``n`` is the batch size.  A memory bank (a MoCo-style queue) keeps the detached embeddings of the last
``M`` samples and scores every image of the batch against the batch's reports and the bank's -- in the symmetric form also
every report against the batch's and the bank's images.  Only the batch and the critic's parameters get gradients.  With
``S[i, j] = critic(img_i, txt_j)`` under the CURRENT critic, index ``B + m`` denoting bank entry ``m`` on either side, and
the package's masking extended to the bank (an entry of the query's own study is never a candidate):

    C_i = {i} u {j < B : sid_j != sid_i} u {B + m : bank_sid_m != sid_i}        r_i = log sum_{j in C_i} exp S[i, j]
    R_j = {j} u {i < B : sid_i != sid_j} u {B + m : bank_sid_m != sid_j}        c_j = log sum_{i in R_j} exp S[i, j]
    row-wise:  L = mean_i (r_i - S[i, i])          symmetric:  L = 1/2 mean_i (r_i - S[i, i]) + 1/2 mean_j (c_j - S[j, j])

Bank entries get no row or column terms of their own, and there is no bank x bank block: the work is ``B (B + M)`` scores
(plus ``M B`` in the symmetric mode), never ``M^2``.  A row or column whose only candidate is its positive contributes
exactly 0.

THE CEILING IS log(B + M).  With unique ids and bank entries that are draws from the marginal, ``log(B + M) - L_rowwise``
is the InfoNCE bound with ``B + M`` candidates: exact with frozen encoders.  STALENESS CAVEAT: the embeddings in a
training queue were produced by earlier encoder weights (encoder drift), so during training this is a training loss with
that ceiling, not a bound on the current encoders' mutual information.

Scores, loss and every gradient are HIP kernels behind the C ABI (``mi_banknce_*`` in ``include/mi_critic.h``): no
``[B, B + M]`` fp32 score or gradient matrix is ever held, no float atomics, identical bits from call to call.  It runs
eagerly on one GPU: there is no graphed and no sharded form, and no matrix entry for ``make_mlp`` scores.  There is no CPU
path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _hip
from .critic_ops import OPS, resolve_critic
from .mi_critics import _batch_codes, _critic_kind, _f32_inputs, fused_mi_bound, study_id_codes

__all__ = ["EmbeddingQueue", "memory_bank_infonce", "check_capacity"]

_CHAIN_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def check_capacity(capacity) -> int:
    """``capacity`` as an int >= 1; ValueError otherwise."""
    if isinstance(capacity, bool) or not isinstance(capacity, (int, float)) or int(capacity) != capacity or capacity < 1:
        raise ValueError(f"the memory bank's capacity must be an integer >= 1 (got {capacity!r})")
    return int(capacity)


class EmbeddingQueue:
    """A FIFO ring of ``(img, txt, study-id code)`` triples: the memory bank of ``memory_bank_infonce``.

    ``push(img, txt, study_id)`` stores detached fp32 copies and overwrites the oldest entries on wrap; a push of more
    than ``capacity`` rows keeps the last ``capacity``.  ``len(q)`` is the number of valid entries, ``q.img`` /
    ``q.txt`` / ``q.ids`` are the valid entries ([len, d_img], [len, d_txt], int64 [len]; slot order, which the loss does
    not depend on), ``clear()`` empties it.  Plain torch indexing: this is not the hot path.

    The entries are as stale as the encoder weights that produced them (module docstring).  The queue is not part of any
    checkpoint: after a resume it is empty and refills."""

    def __init__(self, capacity: int, d_img: int, d_txt: int, device="cpu"):
        self.capacity = check_capacity(capacity)
        self.device = torch.device(device)
        self._img = torch.zeros(self.capacity, int(d_img), dtype=torch.float32, device=self.device)
        self._txt = torch.zeros(self.capacity, int(d_txt), dtype=torch.float32, device=self.device)
        self._ids = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self._next = 0
        self._len = 0

    def __len__(self) -> int:
        return self._len

    @property
    def img(self) -> torch.Tensor:
        return self._img[:self._len]

    @property
    def txt(self) -> torch.Tensor:
        return self._txt[:self._len]

    @property
    def ids(self) -> torch.Tensor:
        return self._ids[:self._len]

    def clear(self) -> None:
        self._next = 0
        self._len = 0

    @torch.no_grad()
    def push(self, img: torch.Tensor, txt: torch.Tensor, study_id) -> None:
        if img.dim() != 2 or txt.dim() != 2 or img.shape[0] != txt.shape[0]:
            raise ValueError("img / txt must be [n, d_img] / [n, d_txt]")
        if img.shape[1] != self._img.shape[1] or txt.shape[1] != self._txt.shape[1]:
            raise ValueError(f"this queue holds widths {self._img.shape[1]} / {self._txt.shape[1]} "
                             f"(got {img.shape[1]} / {txt.shape[1]})")
        ids = study_id_codes(study_id, self.device)
        n = img.shape[0]
        if ids.numel() != n:
            raise ValueError("study_id length must equal the number of rows")
        img = img.detach().to(device=self.device, dtype=torch.float32)
        txt = txt.detach().to(device=self.device, dtype=torch.float32)
        if n > self.capacity:  # only the last `capacity` rows survive
            img, txt, ids, n = img[-self.capacity:], txt[-self.capacity:], ids[-self.capacity:], self.capacity
        if n == 0:
            return
        slots = (self._next + torch.arange(n, device=self.device)) % self.capacity
        self._img[slots] = img
        self._txt[slots] = txt
        self._ids[slots] = ids
        self._next = (self._next + n) % self.capacity
        self._len = min(self.capacity, self._len + n)


class _BankNceFn(torch.autograd.Function):
    """The memory-bank InfoNCE of the bilinear or separable critic in one library call (``ops.banknce_step``), as
    ``hard_negatives._HardNceFn``: with ``need_grad`` the call also writes every gradient for dL/dloss = 1 and the backward
    only scales them.  The bank tensors are constants.  Returns (loss [1], lse_rows, lse_cols or None)."""

    @staticmethod
    def forward(ctx, kind: str, sid, bank_x, bank_y, bank_sid, mode: int, precision: int, need_grad: bool, x, y, *params):
        x, y, params = _f32_inputs(x, y, params)
        loss, r, c, grads = OPS[kind]().banknce_step(x, y, params, sid, bank_x, bank_y, bank_sid, mode, precision,
                                                     need_grad)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(*[t for t in (r, c) if t is not None])
        return loss, r, c

    @staticmethod
    def backward(ctx, grad_loss, *_):
        saved = ctx.saved_tensors
        if not saved:
            raise RuntimeError("_BankNceFn: the forward ran without gradients (need_grad=False)")
        go = grad_loss.reshape(-1)[:1].to(torch.float32)
        return (None,) * 8 + tuple(g * go for g in saved)


def _bank_tensors(bank, device):
    """(bank_img or None, bank_txt, bank_ids int64 codes, m) of an ``EmbeddingQueue`` or a triple."""
    if isinstance(bank, EmbeddingQueue):
        if len(bank) == 0:
            return None, None, None, 0
        return bank.img, bank.txt, bank.ids, len(bank)
    try:
        bimg, btxt, bids = bank
    except (TypeError, ValueError):
        raise TypeError("bank must be an EmbeddingQueue or a (bank_img, bank_txt, bank_ids) triple") from None
    if btxt is None:
        raise ValueError("bank_txt is required (bank_img may be None when symmetric=False)")
    for name, t in (("bank_img", bimg), ("bank_txt", btxt)):
        if t is not None and torch.is_tensor(t) and t.requires_grad:
            raise ValueError(f"{name} requires grad, but the memory bank is a constant of this loss: its gradient would "
                             "silently vanish.  Pass detached tensors")
    m = btxt.shape[0]
    if m == 0:
        return None, None, None, 0
    ids = study_id_codes(bids, device)
    if ids.numel() != m or (bimg is not None and bimg.shape[0] != m):
        raise ValueError("bank_img, bank_txt and bank_ids must have the same number of entries")
    return bimg, btxt, ids, m


def memory_bank_infonce(embedding_img: torch.Tensor, embedding_txt: torch.Tensor, study_id, critic, bank,
                        symmetric: bool = True, precision: str = "f32", return_stats: bool = False):
    """The per-sample InfoNCE of the batch against the batch and a memory bank (module docstring), a 0-d tensor carrying
    autograd to the embeddings and the critic's parameters; the bank gets none.

    The candidates per query are the batch and the bank, so the ceiling is log(B + M): with unique ids and bank entries
    drawn from the marginal ``log(B + M) - loss`` (row-wise) is the InfoNCE bound with B + M candidates -- exact with
    frozen encoders.  Staleness: entries queued during training came from earlier encoder weights, so then this is a
    training loss with that ceiling, not a bound.

    ``critic``: a ``BilinearCritic`` or a ``SeparableCritic``; a ``make_mlp`` critic raises ValueError (there is no
    matrix entry for this loss).  ``bank``: an ``EmbeddingQueue`` or a ``(bank_img, bank_txt, bank_ids)`` triple of
    detached tensors (a bank tensor with ``requires_grad`` raises ValueError); ``bank_img`` may be None when
    ``symmetric=False``, which reads the bank's reports only.  An empty bank returns
    ``fused_mi_bound(..., "infonce_rowwise" | "infonce_symmetric")`` itself.

    One library call runs the operand preparation of batch and bank, T = X W (and U = bank_img W), the score GEMMs of the
    top block [B, B + M] and -- symmetric -- the left block [M, B] with the record epilogues, the merge and the loss and,
    when an input needs a gradient, the G GEMMs and the backward products; the backward pass only scales the saved
    gradients.  ``precision`` as for ``hard_negative_infonce``: "f32" (bf16x3 on the bilinear critic where every size is
    a multiple of 8, exact fp32 products otherwise), "f32_exact", "bf16", "bf16x3"; "fp8", "f16" and "f16x3" raise
    ValueError.  ``return_stats=True``: ``(loss, (lse_rows, lse_cols))``, lse_cols None in the row-wise mode."""
    _hip.require_device(embedding_img, "embedding_img")
    _hip.require_device(embedding_txt, "embedding_txt")
    if critic is None:
        raise TypeError("critic must be a BilinearCritic or a SeparableCritic")
    if _critic_kind(critic) == "concat_mlp":
        raise ValueError("memory_bank_infonce is implemented for the bilinear and separable critics only (a make_mlp "
                         "critic has no GEMM form, and there is no matrix entry for this loss)")
    bimg, btxt, bids, m = _bank_tensors(bank, embedding_img.device)
    est = "infonce_symmetric" if symmetric else "infonce_rowwise"
    if m == 0:
        return fused_mi_bound(embedding_img, embedding_txt, study_id, critic, est, precision=precision,
                              return_stats=return_stats)
    if symmetric and bimg is None:
        raise ValueError("the symmetric form scores the bank's images too: bank_img is required")
    x = embedding_img.float() if embedding_img.dtype == torch.float64 else embedding_img
    y = embedding_txt.float() if embedding_txt.dtype == torch.float64 else embedding_txt
    sid = _batch_codes(x, y, study_id)
    bx = _hip.f32c(bimg.detach(), "bank_img") if (bimg is not None and symmetric) else None
    by = _hip.f32c(btxt.detach(), "bank_txt")
    if by.dim() != 2 or by.shape[1] != y.shape[1] or (bx is not None and (bx.dim() != 2 or bx.shape[1] != x.shape[1])):
        raise ValueError("bank_img / bank_txt must be [M, d_img] / [M, d_txt] of the batch's widths")
    kind, params, prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1])
    if prec not in _CHAIN_PRECISIONS:
        raise ValueError(f'precision="{precision}" is not available for the memory-bank InfoNCE of the {kind} critic '
                         '(use "f32", "f32_exact", "bf16" or "bf16x3")')
    mode = _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, *params))
    loss, r, c = _BankNceFn.apply(kind, sid, bx, by, bids.contiguous(), mode, prec, need_grad, x, y, *params)
    loss = loss.reshape(())
    return (loss, (r, c)) if return_stats else loss
