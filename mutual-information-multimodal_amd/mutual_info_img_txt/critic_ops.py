"""The one binding of the critic entry points of the C ABI (mi_bilinear_*, mi_separable_*, mi_concat_mlp_*, mi_nce_*,
mi_fdiv_*, mi_rank_*, mi_topk_*, mi_estimates_*, mi_hardnce_*, mi_banknce_*, mi_posnce_*, mi_softnce_*), shared by ``mi_critics`` (eager autograd), ``graphed`` (hipGraph step) and ``distributed`` (sharded step).

An ops object scores the row block ``x`` [b_rows, d_img] (starting at ``row_offset``) against all of ``y_all``
[b, d_txt]; a whole batch is ``b_rows == b``, ``row_offset == 0``.  Each ``*_call`` method writes one entry point's
argument list and returns the launch bound to the given tensors (a ``functools.partial`` of ``_hip.call``, which looks
up the current stream per call): eager callers issue it at once, ``GraphedMiStep`` binds its static buffers once.
"""
from __future__ import annotations

import ctypes
from functools import partial

import torch

from . import _hip
from ._hip import PRECISIONS, ptr as _p


def _precision_code(precision: str) -> int:
    if precision not in PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}: expected one of {sorted(PRECISIONS)}")
    return PRECISIONS[precision]


NOT_MAKE_MLP = ("the fused concat-MLP path supports make_mlp(input_dim, [h1, h2]) critics "
                "(Linear-ReLU-Linear-ReLU-Linear(->1)); use create_mi_pairs + the critic module otherwise")


def _concat_params(critic):
    """(W1,b1,W2,b2,W3,b3) of an nn.Sequential built by make_mlp(input_dim,[h1,h2]) (reference model.py:18-32)."""
    mods = list(critic)
    lin = [m for m in mods if isinstance(m, torch.nn.Linear)]
    act = [m for m in mods if not isinstance(m, torch.nn.Linear)]
    if len(lin) != 3 or len(mods) != 5 or not all(isinstance(a, torch.nn.ReLU) for a in act) or lin[2].out_features != 1:
        raise ValueError(NOT_MAKE_MLP)
    return lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias


def resolve_critic(critic, precision: str, b: int, d_img: int, d_txt: int, params=None):
    """(kind, params, precision code) of a critic: a ``BilinearCritic``, a ``SeparableCritic``, the reference's make_mlp
    critic, None (S = X Y^T), or -- for the sharded path -- a kind name with its ``params``.

    "f32" means fp32-grade results (``_hip.resolve_precision``): the bf16x3 scheme on the bilinear critic with a weight
    where b, d_img and d_txt are multiples of 8, the f16x3 scheme on make_mlp critics of the fused hidden sizes, exact
    fp32 products otherwise.  ``params`` of a make_mlp critic are the module's own tensors (W3 is [1, h2])."""
    from . import model as _model  # local import: model.py imports nothing from here
    weighted = False
    if isinstance(critic, str):
        kind, params, weighted = critic, list(params or ()), critic == "bilinear"
    elif isinstance(critic, _model.BilinearCritic):
        kind, params, weighted = "bilinear", [critic.weight], True
    elif isinstance(critic, _model.SeparableCritic):
        kind, params = "separable", [critic.wg, critic.wh]
        if critic.wg.shape[0] != d_img or tuple(critic.wh.shape) != (d_txt, critic.wg.shape[1]):
            raise ValueError("projection shapes must be [d_img, d_proj] and [d_txt, d_proj]")
    elif critic is None:
        # GraphedMiStep's weightless form; unlike BilinearCritic, "f32" stays exact fp32 here (no bf16x3)
        if d_img != d_txt:
            raise ValueError("critic=None is the separable form S = X Y^T: widths must agree")
        kind, params = "bilinear", []
    else:
        kind, params = "concat_mlp", list(_concat_params(critic))
        if params[0].shape[1] != d_img + d_txt:
            raise ValueError(f"critic expects {params[0].shape[1]} inputs, embeddings give {d_img} + {d_txt}")
    hidden = (params[0].shape[0], params[2].shape[0]) if kind == "concat_mlp" and len(params) == 6 else None
    return kind, params, _hip.resolve_precision(precision, weighted, (b, d_img, d_txt), concat_hidden=hidden)


def fwd_outputs(device, scores=None):
    """(loss [1], statistics, partial record, scores) -- the outputs of one forward call."""
    return (torch.empty(1, dtype=torch.float32, device=device), _hip.new_stats(device),
            torch.empty(_hip.RECORD_FLOATS, dtype=torch.float32, device=device), scores)


def _call(name, device, *args):
    return partial(_hip.call, name, device, *args)


def rank_matrix(scores, sid, i2t=True, t2i=True):
    """Retrieval ranks of a float32 [B, B] score matrix (mi_rank_matrix): (rank_i2t, rank_t2i) int32 [B]; a direction
    not asked for is None."""
    b, dev = scores.shape[0], scores.device
    ri = torch.empty(b, dtype=torch.int32, device=dev) if i2t else None
    rt = torch.empty(b, dtype=torch.int32, device=dev) if t2i else None
    _hip.call("mi_rank_matrix", dev, scores.data_ptr(), sid.data_ptr(), b, _p(ri), _p(rt))
    return ri, rt


def estimates_taus(taus):
    """The clips of an estimates call as the C array the entry points read (a host pointer, copied during the call)."""
    return (ctypes.c_float * max(len(taus), 1))(*taus)


def estimates_matrix(scores, sid, taus):
    """MI estimates of a float32 [B, B] score matrix (mi_estimates_matrix): float32 [MI_EST_FLOATS] on the device."""
    b, dev = scores.shape[0], scores.device
    ws = _hip.workspace(_hip.load().mi_estimates_matrix_workspace_bytes(b), dev)
    est = torch.empty(_hip.MI_EST_FLOATS, dtype=torch.float32, device=dev)
    _hip.call("mi_estimates_matrix", dev, scores.data_ptr(), sid.data_ptr(), b, estimates_taus(taus), len(taus),
              est.data_ptr(), ws.data_ptr(), ws.numel())
    return est


def topk_outputs(n_q, k, device):
    """(idx int32 [n_q, k], val float32 [n_q, k]) of one top-k direction."""
    return (torch.empty(n_q, k, dtype=torch.int32, device=device), torch.empty(n_q, k, dtype=torch.float32, device=device))


def topk_matrix(scores, k, axis=0, sid_rows=None, sid_cols=None):
    """Top-k of a float32 [n_rows, n_cols] score matrix (mi_topk_matrix): (idx, val) [n_rows, k] of each row's best
    columns (``axis`` 0) or [n_cols, k] of each column's best rows (``axis`` 1); with the two id code tensors a candidate
    whose code equals the query's is left out."""
    (n_rows, n_cols), dev = scores.shape, scores.device
    ws = _hip.workspace(_hip.load().mi_topk_matrix_workspace_bytes(n_rows, n_cols, k, axis), dev)
    idx, val = topk_outputs(n_rows if axis == 0 else n_cols, k, dev)
    _hip.call("mi_topk_matrix", dev, scores.data_ptr(), n_rows, n_cols, _p(sid_rows), _p(sid_cols), k, axis,
              idx.data_ptr(), val.data_ptr(), ws.data_ptr(), ws.numel())
    return idx, val


def hardnce_matrix_fwd(scores, sid, mode, k):
    """Hard-negative InfoNCE of a float32 [B, B] score matrix (mi_matrix_hardnce_fwd): (loss [1], lse_rows, lse_cols,
    idx_rows, idx_cols); the column side is None in the row-wise mode."""
    b, dev = scores.shape[0], scores.device
    sym = mode == _hip.MI_NCE_SYMMETRIC
    ws = _hip.workspace(_hip.load().mi_matrix_hardnce_workspace_bytes(b, k), dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    r, ir = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, k, dtype=torch.int32, device=dev)
    c, ic = (torch.empty_like(r), torch.empty_like(ir)) if sym else (None, None)
    _hip.call("mi_matrix_hardnce_fwd", dev, scores.data_ptr(), sid.data_ptr(), b, mode, k, loss.data_ptr(), r.data_ptr(),
              _p(c), ir.data_ptr(), _p(ic), ws.data_ptr(), ws.numel())
    return loss, r, c, ir, ic


def hardnce_matrix_bwd(scores, mode, k, r, c, idx_rows, idx_cols, grad_out):
    """grad_scores [B, B] of grad_out[0] * loss (mi_matrix_hardnce_bwd) from the forward's lists and LSEs."""
    g = torch.empty_like(scores)
    _hip.call("mi_matrix_hardnce_bwd", scores.device, scores.data_ptr(), scores.shape[0], mode, k, idx_rows.data_ptr(),
              _p(idx_cols), r.data_ptr(), _p(c), _p(grad_out), g.data_ptr())
    return g


def posnce_matrix_fwd(scores, sid, mode):
    """Study-positive InfoNCE of a float32 [B, B] score matrix (mi_matrix_posnce_fwd): (loss [1], lse_rows [B], lse_cols
    [B], n_pos int32 [B]); both LSEs in either mode."""
    b, dev = scores.shape[0], scores.device
    ws = _hip.workspace(_hip.load().mi_matrix_posnce_workspace_bytes(b), dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    r, c = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
    n_pos = torch.empty(b, dtype=torch.int32, device=dev)
    _hip.call("mi_matrix_posnce_fwd", dev, scores.data_ptr(), sid.data_ptr(), b, mode, loss.data_ptr(), r.data_ptr(),
              c.data_ptr(), n_pos.data_ptr(), ws.data_ptr(), ws.numel())
    return loss, r, c, n_pos


def posnce_matrix_bwd(scores, sid, mode, r, c, n_pos, grad_out):
    """grad_scores [B, B] of grad_out[0] * loss (mi_matrix_posnce_bwd) from the forward's LSEs and positive counts."""
    g = torch.empty_like(scores)
    _hip.call("mi_matrix_posnce_bwd", scores.device, scores.data_ptr(), sid.data_ptr(), scores.shape[0], mode,
              r.data_ptr(), _p(c), n_pos.data_ptr(), _p(grad_out), g.data_ptr())
    return g


def softnce_matrix_fwd(scores, lab, mode, tau, mix):
    """Soft-target InfoNCE of a float32 [B, B] score matrix (mi_matrix_softnce_fwd): (loss [1], lse_rows [B], lse_cols
    [B], target_norm [B]); both LSEs in either mode."""
    b, dev = scores.shape[0], scores.device
    ws = _hip.workspace(_hip.load().mi_matrix_softnce_workspace_bytes(b), dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    r, c, z = (torch.empty(b, dtype=torch.float32, device=dev) for _ in range(3))
    _hip.call("mi_matrix_softnce_fwd", dev, scores.data_ptr(), lab.data_ptr(), b, mode, tau, mix, loss.data_ptr(),
              r.data_ptr(), c.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel())
    return loss, r, c, z


def softnce_matrix_bwd(scores, lab, mode, tau, mix, r, c, z, grad_out):
    """grad_scores [B, B] of grad_out[0] * loss (mi_matrix_softnce_bwd) from the forward's LSEs and target norms."""
    g = torch.empty_like(scores)
    _hip.call("mi_matrix_softnce_bwd", scores.device, scores.data_ptr(), lab.data_ptr(), scores.shape[0], mode, tau, mix,
              r.data_ptr(), _p(c), z.data_ptr(), _p(grad_out), g.data_ptr())
    return g


class _HipOps:
    """The ops protocol of ``distributed.GlobalBatchCriticFn`` (forward / merge / backward) on the C ABI.  ``saved`` is
    (x, y_all, params, sid_rows, sid_all, row_offset, precision, scores, ws) for every critic."""

    def _scores(self, x, y_all):
        return None

    def _workspace(self, x, y_all, params, precision, flags):
        """(workspace, extra need_grad bits) of a forward without a caller-provided workspace."""
        nbytes = self.workspace_bytes(x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], params, precision, flags)
        return _hip.workspace(nbytes, x.device), 0

    def forward(self, x, y_all, params, sid_rows, sid_all, row_offset, estimator, precision, need_grad, out=None, ws=None):
        """Partial record of the row block -> (record, saved).  ``out`` = preallocated ``fwd_outputs``; ``ws`` = a
        workspace sized by ``workspace_bytes``."""
        flags = int(bool(need_grad))
        if ws is None:
            ws, bits = self._workspace(x, y_all, params, precision, flags)
            flags |= bits
        if out is None:
            out = fwd_outputs(x.device, self._scores(x, y_all))
        self.fwd_call(x, y_all, params, sid_rows, sid_all, row_offset, estimator, precision, flags, out, ws)()
        return out[2], (x, y_all, list(params), sid_rows, sid_all, row_offset, precision, out[3], ws)

    def backward(self, saved, stats, grad_out, out=None):
        """``out`` = (grad_x, grad_y_partial, [grad_params...]) preallocated buffers (e.g. views of one flat all-reduce
        buffer); allocated here when None."""
        x, y_all, params = saved[:3]
        if out is None:
            out = (torch.empty_like(x), torch.empty_like(y_all), [torch.empty_like(p) for p in params])
        self.bwd_call(saved, stats, grad_out, out)()
        return out

    def merge(self, records, n_pos, estimator):
        dev = records.device
        loss, stats = torch.empty(1, dtype=torch.float32, device=dev), _hip.new_stats(dev)
        _hip.call("mi_merge_partials", dev, records.data_ptr(), records.shape[0], n_pos, estimator, loss.data_ptr(),
                  stats.data_ptr())
        return loss, stats

    def chain_step(self, entry, x, y, params, sid, mode, precision, need_grad):
        """The whole batch in one call of ``{entry}_<critic>_step`` (bilinear and separable critics), with the gradients of
        1 * loss when ``need_grad``: (loss [1], a, b, [grad_x, grad_y, grad_params...] or []).  ``entry`` "mi_nce"
        (per-sample InfoNCE): a, b = lse_rows [B], lse_cols [B]; "mi_fdiv" (Jensen-Shannon / NWJ): a = terms [2], b = None."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.chain_workspace_bytes(entry, b, x.shape[1], y.shape[1], params, precision), dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        if entry == "mi_nce":
            r, c = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
        else:
            r, c = torch.empty(2, dtype=torch.float32, device=dev), None
        grads = [torch.empty_like(t) for t in (x, y, *params)] if need_grad else []
        self.chain_call(entry, x, y, params, sid, mode, precision, loss, r, c, grads, ws)()
        return loss, r, c, grads

    def nce_step(self, x, y, params, sid, mode, precision, need_grad):
        """``chain_step("mi_nce", ...)``: the one-call reference the row-block protocol below is checked against."""
        return self.chain_step("mi_nce", x, y, params, sid, mode, precision, need_grad)

    def rank_step(self, x, y, params, sid, precision, want_diag=False):
        """Retrieval ranks of the whole batch in one call of ``mi_rank_<critic>`` (bilinear and separable critics):
        (rank_i2t, rank_t2i) int32 [B], and the diagonal scores S[i, i] when ``want_diag``."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.rank_workspace_bytes(b, x.shape[1], y.shape[1], params, precision), dev)
        ri, rt = (torch.empty(b, dtype=torch.int32, device=dev) for _ in range(2))
        diag = torch.empty(b, dtype=torch.float32, device=dev) if want_diag else None
        self.rank_call(x, y, params, sid, precision, ri, rt, diag, ws)()
        return (ri, rt, diag) if want_diag else (ri, rt)

    def estimates_step(self, x, y, params, sid, precision, taus):
        """MI estimates of the whole batch in one call of ``mi_estimates_<critic>`` (bilinear and separable critics):
        float32 [MI_EST_FLOATS] on the device (the slots ``_hip.MI_EST_*``)."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.estimates_workspace_bytes(b, x.shape[1], y.shape[1], params, precision), dev)
        est = torch.empty(_hip.MI_EST_FLOATS, dtype=torch.float32, device=dev)
        self.estimates_call(x, y, params, sid, precision, taus, est, ws)()
        return est

    def topk_step(self, x, y, params, sid_img, sid_txt, precision, k, i2t=True, t2i=True):
        """Top-k retrieval of x [n_img, d_img] against y [n_txt, d_txt] in one call of ``mi_topk_<critic>`` (bilinear and
        separable critics): ((idx, val) of image -> report or None, (idx, val) of report -> image or None)."""
        (n_img, dx), (n_txt, dy), dev = x.shape, y.shape, x.device
        ws = _hip.workspace(self.topk_workspace_bytes(n_img, n_txt, dx, dy, params, precision, k), dev)
        out_i = topk_outputs(n_img, k, dev) if i2t else None
        out_t = topk_outputs(n_txt, k, dev) if t2i else None
        self.topk_call(x, y, params, sid_img, sid_txt, precision, k, out_i, out_t, ws)()
        return out_i, out_t

    def hardnce_step(self, x, y, params, sid, mode, precision, k, need_grad):
        """The hard-negative InfoNCE of the whole batch in one call of ``mi_hardnce_<critic>_step`` (bilinear and separable
        critics), with the gradients of 1 * loss when ``need_grad``: (loss [1], lse_rows [B], lse_cols [B] or None,
        idx_rows int32 [B, k], idx_cols or None, [grad_x, grad_y, grad_params...] or []).  The column side exists in
        the symmetric mode only."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.hardnce_workspace_bytes(b, x.shape[1], y.shape[1], params, precision, k, need_grad), dev)
        sym = mode == _hip.MI_NCE_SYMMETRIC
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        r, ir = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, k, dtype=torch.int32, device=dev)
        c, ic = (torch.empty_like(r), torch.empty_like(ir)) if sym else (None, None)
        grads = [torch.empty_like(t) for t in (x, y, *params)] if need_grad else []
        self.hardnce_call(x, y, params, sid, mode, precision, k, loss, r, c, ir, ic, grads, ws)()
        return loss, r, c, ir, ic, grads

    def banknce_step(self, x, y, params, sid, bank_x, bank_y, bank_sid, mode, precision, need_grad):
        """The per-sample InfoNCE of the batch against the batch and a memory bank in one call of
        ``mi_banknce_<critic>_step`` (bilinear and separable critics), with the gradients of 1 * loss when ``need_grad``:
        (loss [1], lse_rows [B], lse_cols [B] or None, [grad_x, grad_y, grad_params...] or []).  ``bank_x`` may be None in
        the row-wise mode; the bank gets no gradient."""
        b, m, dev = x.shape[0], bank_y.shape[0], x.device
        ws = _hip.workspace(self.banknce_workspace_bytes(b, m, x.shape[1], y.shape[1], params, mode, precision, need_grad),
                            dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        r = torch.empty(b, dtype=torch.float32, device=dev)
        c = torch.empty_like(r) if mode == _hip.MI_NCE_SYMMETRIC else None
        grads = [torch.empty_like(t) for t in (x, y, *params)] if need_grad else []
        self.banknce_call(x, y, params, sid, bank_x, bank_y, bank_sid, mode, precision, loss, r, c, grads, ws)()
        return loss, r, c, grads

    def posnce_step(self, x, y, params, sid, mode, precision, need_grad):
        """The study-positive InfoNCE of the whole batch in one call of ``mi_posnce_<critic>_step`` (bilinear and separable
        critics), with the gradients of 1 * loss when ``need_grad``: (loss [1], lse_rows [B], lse_cols [B], n_pos int32
        [B], [grad_x, grad_y, grad_params...] or [])."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.posnce_workspace_bytes(b, x.shape[1], y.shape[1], params, precision, need_grad), dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        r, c = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
        n_pos = torch.empty(b, dtype=torch.int32, device=dev)
        grads = [torch.empty_like(t) for t in (x, y, *params)] if need_grad else []
        self.posnce_call(x, y, params, sid, mode, precision, loss, r, c, n_pos, grads, ws)()
        return loss, r, c, n_pos, grads

    def softnce_step(self, x, y, params, lab, mode, precision, tau, mix, need_grad):
        """The soft-target InfoNCE of the whole batch in one call of ``mi_softnce_<critic>_step`` (bilinear and separable
        critics), with the gradients of 1 * loss when ``need_grad``: (loss [1], lse_rows [B], lse_cols [B], target_norm
        [B], [grad_x, grad_y, grad_params...] or [])."""
        b, dev = x.shape[0], x.device
        ws = _hip.workspace(self.softnce_workspace_bytes(b, x.shape[1], y.shape[1], params, precision, need_grad), dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        r, c, z = (torch.empty(b, dtype=torch.float32, device=dev) for _ in range(3))
        grads = [torch.empty_like(t) for t in (x, y, *params)] if need_grad else []
        self.softnce_call(x, y, params, lab, mode, precision, tau, mix, loss, r, c, z, grads, ws)()
        return loss, r, c, z, grads

    # ---------------------------------------------- per-sample InfoNCE on a row block (distributed.GlobalBatchNceFn)
    def nce_forward(self, x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, need_grad=True):
        """The row block's part (``mi_nce_part_floats`` floats, gathered in rank order by the caller) and its row LSEs:
        (part, lse_rows [b_rows], saved).  ``saved`` holds the workspace the backward goes on with."""
        br, b, dev = x.shape[0], y_all.shape[0], x.device
        ws = _hip.workspace(self.nce_shard_workspace_bytes(br, b, x.shape[1], y_all.shape[1], params, precision), dev)
        part = torch.empty(_hip.load().mi_nce_part_floats(br, b), dtype=torch.float32, device=dev)
        r = torch.empty(br, dtype=torch.float32, device=dev)
        self.nce_fwd_call(x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, part, r, ws)()
        return part, r, (x, y_all, list(params), sid_rows, sid_all, row_offset, mode, precision, ws)

    @staticmethod
    def nce_merge(parts, b_rows, mode):
        """parts [n_ranks, P] in rank order -> (loss [1], lse_cols [b]); identical bits on every rank."""
        dev, b = parts.device, parts.shape[0] * b_rows
        loss, c = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
        ws = _hip.workspace(_hip.load().mi_nce_merge_workspace_bytes(b), dev)
        _hip.call("mi_nce_merge_parts", dev, parts.data_ptr(), parts.shape[0], b_rows, b, mode, loss.data_ptr(),
                  c.data_ptr(), ws.data_ptr(), ws.numel())
        return loss, c

    def nce_backward(self, saved, lse_cols, grad_out, out=None):
        """(grad_x, grad_y partial over this row block, [grad_params...] partial) of grad_out[0] * loss."""
        x, y_all, params = saved[:3]
        if out is None:
            out = (torch.empty_like(x), torch.empty_like(y_all), [torch.empty_like(p) for p in params])
        self.nce_bwd_call(saved, lse_cols, grad_out, out)()
        return out

    # ---------------------------------------------- study-positive InfoNCE on a row block (distributed.GlobalBatchPosNceFn)
    def posnce_forward(self, x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, need_grad=True):
        """The row block's part (``mi_posnce_part_floats`` floats, gathered in rank order by the caller), its row LSEs and
        positive counts: (part, lse_rows [b_rows], n_pos int32 [b_rows], saved).  ``saved`` holds the workspace the
        backward goes on with."""
        br, b, dev = x.shape[0], y_all.shape[0], x.device
        ws = _hip.workspace(self.posnce_shard_workspace_bytes(br, b, x.shape[1], y_all.shape[1], params, precision), dev)
        part = torch.empty(_hip.load().mi_posnce_part_floats(br, b), dtype=torch.float32, device=dev)
        r = torch.empty(br, dtype=torch.float32, device=dev)
        n_pos = torch.empty(br, dtype=torch.int32, device=dev)
        self.posnce_fwd_call(x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, part, r, n_pos, ws)()
        return part, r, n_pos, (x, y_all, list(params), sid_rows, sid_all, row_offset, mode, precision, ws)

    @staticmethod
    def _merge_parts(entry, parts, b_rows, mode):
        dev, b = parts.device, parts.shape[0] * b_rows
        loss, c = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
        ws = _hip.workspace(getattr(_hip.load(), f"{entry}_merge_workspace_bytes")(b), dev)
        _hip.call(f"{entry}_merge_parts", dev, parts.data_ptr(), parts.shape[0], b_rows, b, mode, loss.data_ptr(),
                  c.data_ptr(), ws.data_ptr(), ws.numel())
        return loss, c

    @classmethod
    def posnce_merge(cls, parts, b_rows, mode):
        """parts [n_ranks, P] in rank order -> (loss [1], lse_cols [b]); identical bits on every rank."""
        return cls._merge_parts("mi_posnce", parts, b_rows, mode)

    def posnce_backward(self, saved, lse_cols, grad_out, out=None):
        """(grad_x, grad_y partial over this row block, [grad_params...] partial) of grad_out[0] * loss."""
        x, y_all, params = saved[:3]
        if out is None:
            out = (torch.empty_like(x), torch.empty_like(y_all), [torch.empty_like(p) for p in params])
        self.posnce_bwd_call(saved, lse_cols, grad_out, out)()
        return out

    # ---------------------------------------------- soft-target InfoNCE on a row block (distributed_label_targets.GlobalBatchSoftNceFn)
    def softnce_forward(self, x, y_all, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, need_grad=True):
        """The row block's part (``mi_softnce_part_floats`` floats, gathered in rank order by the caller), its row LSEs and
        target norms: (part, lse_rows [b_rows], target_norm [b_rows], saved).  ``saved`` holds the workspace the backward
        goes on with."""
        br, b, dev = x.shape[0], y_all.shape[0], x.device
        ws = _hip.workspace(self.softnce_shard_workspace_bytes(br, b, x.shape[1], y_all.shape[1], params, precision), dev)
        part = torch.empty(_hip.load().mi_softnce_part_floats(br, b), dtype=torch.float32, device=dev)
        r, z = torch.empty(br, dtype=torch.float32, device=dev), torch.empty(br, dtype=torch.float32, device=dev)
        self.softnce_fwd_call(x, y_all, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, part, r, z, ws)()
        return part, r, z, (x, y_all, list(params), lab_rows, lab_all, row_offset, mode, precision, tau, mix, ws)

    @classmethod
    def softnce_merge(cls, parts, b_rows, mode):
        """parts [n_ranks, P] in rank order -> (loss [1], lse_cols [b]); identical bits on every rank."""
        return cls._merge_parts("mi_softnce", parts, b_rows, mode)

    def softnce_backward(self, saved, lse_cols, grad_out, out=None):
        """(grad_x, grad_y partial over this row block, [grad_params...] partial) of grad_out[0] * loss."""
        x, y_all, params = saved[:3]
        if out is None:
            out = (torch.empty_like(x), torch.empty_like(y_all), [torch.empty_like(p) for p in params])
        self.softnce_bwd_call(saved, lse_cols, grad_out, out)()
        return out


class HipBilinearOps(_HipOps):
    """S = (X W) Y^T row block; params = [W] ([] on one GPU: S = X Y^T)."""

    def __init__(self):
        self._fp8_ws = None    # workspace of a staged fp8 preparation, handed on to forward()
        self._local_ws = None  # workspace in which prep_local() prepared the rank's own part, handed on to forward()
        self._local_key = None

    @staticmethod
    def workspace_bytes(br, b, dx, dy, params, precision, need_grad=1):
        return _hip.load().mi_bilinear_workspace_bytes(br, b, dx, dy, precision)

    def fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, estimator, precision, flags, out, ws):
        loss, stats, record, scores = out
        w = params[0] if params else None
        return _call("mi_bilinear_fwd", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid_rows.data_ptr(),
                     sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1], estimator, precision,
                     flags, _p(loss), stats.data_ptr(), _p(record), _p(scores), ws.data_ptr(), ws.numel())

    def bwd_call(self, saved, stats, grad_out, out):
        x, y, params, sid_rows, sid_all, row_offset, precision, _, ws = saved
        gx, gy, gp = out
        return _call("mi_bilinear_bwd", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     precision, stats.data_ptr(), grad_out.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                     _p(gp[0] if gp else None), ws.data_ptr(), ws.numel(), 1)

    def step_call(self, x, y, params, sid, estimator, precision, grad_out, out, grads, ws):
        """Forward + backward of the whole batch in one call: mi_bilinear_step, or mi_bilinear_step_bf16 for bfloat16
        embeddings (and gradients)."""
        loss, stats, record, _ = out
        gx, gy, gp = grads
        w, gw = (params[0], gp[0]) if params else (None, None)
        b, dx, dy = x.shape[0], x.shape[1], y.shape[1]
        if x.dtype == torch.bfloat16:
            return _call("mi_bilinear_step_bf16", x.device, x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b,
                         dx, dy, estimator, grad_out.data_ptr(), loss.data_ptr(), stats.data_ptr(), record.data_ptr(),
                         gx.data_ptr(), gy.data_ptr(), int(gx.dtype == torch.bfloat16), gw.data_ptr(), ws.data_ptr(),
                         ws.numel())
        return _call("mi_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid.data_ptr(), b, dx, dy,
                     estimator, precision, grad_out.data_ptr(), loss.data_ptr(), stats.data_ptr(), record.data_ptr(),
                     gx.data_ptr(), gy.data_ptr(), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def chain_workspace_bytes(entry, b, dx, dy, params, precision):
        return getattr(_hip.load(), f"{entry}_bilinear_workspace_bytes")(b, dx, dy, precision)

    def chain_call(self, entry, x, y, params, sid, mode, precision, loss, r, c, grads, ws):
        w = params[0] if params else None
        gx, gy, gw = (grads + [None] * 3)[:3]
        return _call(f"{entry}_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid.data_ptr(), x.shape[0],
                     x.shape[1], y.shape[1], mode, precision, None, loss.data_ptr(), r.data_ptr(), _p(c), _p(gx),
                     _p(gy), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def rank_workspace_bytes(b, dx, dy, params, precision):
        return _hip.load().mi_rank_bilinear_workspace_bytes(b, dx, dy, precision)

    def rank_call(self, x, y, params, sid, precision, rank_i2t, rank_t2i, diag, ws):
        """Retrieval ranks of the whole batch (mi_rank_bilinear); ``rank_i2t`` / ``rank_t2i`` int32 [B] (either may be
        None), ``diag`` float32 [B] or None."""
        return _call("mi_rank_bilinear", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], precision, _p(rank_i2t), _p(rank_t2i), _p(diag),
                     ws.data_ptr(), ws.numel())

    @staticmethod
    def estimates_workspace_bytes(b, dx, dy, params, precision):
        return _hip.load().mi_estimates_bilinear_workspace_bytes(b, dx, dy, precision)

    def estimates_call(self, x, y, params, sid, precision, taus, est, ws):
        """MI estimates of the whole batch (mi_estimates_bilinear); ``taus`` a sequence of at most MI_EST_MAX_TAUS clips,
        ``est`` float32 [MI_EST_FLOATS]."""
        return _call("mi_estimates_bilinear", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], precision, estimates_taus(taus), len(taus),
                     est.data_ptr(), ws.data_ptr(), ws.numel())

    @staticmethod
    def topk_workspace_bytes(n_img, n_txt, dx, dy, params, precision, k):
        return _hip.load().mi_topk_bilinear_workspace_bytes(n_img, n_txt, dx, dy, precision, k)

    def topk_call(self, x, y, params, sid_img, sid_txt, precision, k, out_i2t, out_t2i, ws):
        """Top-k retrieval over a gallery (mi_topk_bilinear); ``out_i2t`` / ``out_t2i`` are (idx int32, val float32)
        pairs [n_img, k] / [n_txt, k] (either may be None), ``sid_img`` / ``sid_txt`` id codes or both None."""
        (ii, vi), (it, vt) = out_i2t or (None, None), out_t2i or (None, None)
        return _call("mi_topk_bilinear", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     _p(sid_img), _p(sid_txt), x.shape[0], y.shape[0], x.shape[1], y.shape[1], precision, k, _p(ii), _p(vi),
                     _p(it), _p(vt), ws.data_ptr(), ws.numel())

    @staticmethod
    def hardnce_workspace_bytes(b, dx, dy, params, precision, k, need_grad):
        return _hip.load().mi_hardnce_bilinear_workspace_bytes(b, dx, dy, precision, k, int(bool(need_grad)))

    def hardnce_call(self, x, y, params, sid, mode, precision, k, loss, r, c, idx_rows, idx_cols, grads, ws):
        """Hard-negative InfoNCE step (mi_hardnce_bilinear_step); ``c`` / ``idx_cols`` None in the row-wise mode,
        ``grads`` [] for the forward launches alone."""
        w = params[0] if params else None
        gx, gy, gw = (grads + [None] * 3)[:3]
        return _call("mi_hardnce_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid.data_ptr(), x.shape[0],
                     x.shape[1], y.shape[1], mode, precision, k, None, loss.data_ptr(), _p(r), _p(c), _p(idx_rows),
                     _p(idx_cols), _p(gx), _p(gy), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def banknce_workspace_bytes(b, m, dx, dy, params, mode, precision, need_grad):
        return _hip.load().mi_banknce_bilinear_workspace_bytes(b, m, dx, dy, mode, precision, int(bool(need_grad)))

    def banknce_call(self, x, y, params, sid, bank_x, bank_y, bank_sid, mode, precision, loss, r, c, grads, ws):
        """Memory-bank InfoNCE step (mi_banknce_bilinear_step); ``c`` None in the row-wise mode, ``grads`` [] for the
        forward launches alone."""
        w = params[0] if params else None
        gx, gy, gw = (grads + [None] * 3)[:3]
        return _call("mi_banknce_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid.data_ptr(), _p(bank_x),
                     bank_y.data_ptr(), bank_sid.data_ptr(), x.shape[0], bank_y.shape[0], x.shape[1], y.shape[1], mode,
                     precision, None, loss.data_ptr(), _p(r), _p(c), _p(gx), _p(gy), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def posnce_workspace_bytes(b, dx, dy, params, precision, need_grad):
        return _hip.load().mi_posnce_bilinear_workspace_bytes(b, dx, dy, precision, int(bool(need_grad)))

    def posnce_call(self, x, y, params, sid, mode, precision, loss, r, c, n_pos, grads, ws):
        """Study-positive InfoNCE step (mi_posnce_bilinear_step); ``r`` / ``c`` / ``n_pos`` may be None, ``grads`` [] for
        the forward launches alone."""
        w = params[0] if params else None
        gx, gy, gw = (grads + [None] * 3)[:3]
        return _call("mi_posnce_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), sid.data_ptr(), x.shape[0],
                     x.shape[1], y.shape[1], mode, precision, None, loss.data_ptr(), _p(r), _p(c), _p(n_pos), _p(gx),
                     _p(gy), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def softnce_workspace_bytes(b, dx, dy, params, precision, need_grad):
        return _hip.load().mi_softnce_bilinear_workspace_bytes(b, dx, dy, precision, int(bool(need_grad)))

    def softnce_call(self, x, y, params, lab, mode, precision, tau, mix, loss, r, c, z, grads, ws):
        """Soft-target InfoNCE step (mi_softnce_bilinear_step); ``r`` / ``c`` / ``z`` may be None, ``grads`` [] for the
        forward launches alone."""
        w = params[0] if params else None
        gx, gy, gw = (grads + [None] * 3)[:3]
        return _call("mi_softnce_bilinear_step", x.device, x.data_ptr(), y.data_ptr(), _p(w), lab.data_ptr(), x.shape[0],
                     x.shape[1], y.shape[1], mode, precision, tau, mix, None, loss.data_ptr(), _p(r), _p(c), _p(z), _p(gx),
                     _p(gy), _p(gw), ws.data_ptr(), ws.numel())

    @staticmethod
    def nce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_nce_bilinear_shard_workspace_bytes(br, b, dx, dy, precision)

    def nce_fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, mode, precision, part, r, ws):
        return _call("mi_nce_bilinear_shard_fwd", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     mode, precision, part.data_ptr(), _p(r), ws.data_ptr(), ws.numel())

    def nce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, params, sid_rows, sid_all, row_offset, mode, precision, ws = saved
        gx, gy, gp = out
        return _call("mi_nce_bilinear_shard_bwd", x.device, x.data_ptr(), y.data_ptr(), _p(params[0] if params else None),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     mode, precision, lse_cols.data_ptr(), grad_out.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                     _p(gp[0] if gp else None), ws.data_ptr(), ws.numel())

    @staticmethod
    def posnce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_posnce_bilinear_shard_workspace_bytes(br, b, dx, dy, precision)

    def posnce_fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, mode, precision, part, r, n_pos, ws):
        return _call("mi_posnce_bilinear_shard_fwd", x.device, x.data_ptr(), y.data_ptr(),
                     _p(params[0] if params else None), sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0],
                     row_offset, x.shape[1], y.shape[1], mode, precision, part.data_ptr(), _p(r), _p(n_pos), ws.data_ptr(),
                     ws.numel())

    def posnce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, params, sid_rows, sid_all, row_offset, mode, precision, ws = saved
        gx, gy, gp = out
        return _call("mi_posnce_bilinear_shard_bwd", x.device, x.data_ptr(), y.data_ptr(),
                     _p(params[0] if params else None), sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0],
                     row_offset, x.shape[1], y.shape[1], mode, precision, _p(lse_cols), _p(grad_out), gx.data_ptr(),
                     gy.data_ptr(), _p(gp[0] if gp else None), ws.data_ptr(), ws.numel())

    @staticmethod
    def softnce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_softnce_bilinear_shard_workspace_bytes(br, b, dx, dy, precision)

    def softnce_fwd_call(self, x, y, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, part, r, z, ws):
        return _call("mi_softnce_bilinear_shard_fwd", x.device, x.data_ptr(), y.data_ptr(),
                     _p(params[0] if params else None), lab_rows.data_ptr(), lab_all.data_ptr(), x.shape[0], y.shape[0],
                     row_offset, x.shape[1], y.shape[1], mode, precision, tau, mix, part.data_ptr(), _p(r), _p(z),
                     ws.data_ptr(), ws.numel())

    def softnce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, ws = saved
        gx, gy, gp = out
        return _call("mi_softnce_bilinear_shard_bwd", x.device, x.data_ptr(), y.data_ptr(),
                     _p(params[0] if params else None), lab_rows.data_ptr(), lab_all.data_ptr(), x.shape[0], y.shape[0],
                     row_offset, x.shape[1], y.shape[1], mode, precision, tau, mix, _p(lse_cols), _p(grad_out),
                     gx.data_ptr(), gy.data_ptr(), _p(gp[0] if gp else None), ws.data_ptr(), ws.numel())

    # ------------------------------------------------------------------------------------------ sharded extras
    def prep_local(self, x, params, b, precision) -> bool:
        """The part of the forward that needs neither the gathered text embeddings nor the gathered ids -- bf16 copies of
        X and W, T = X W (mi_bilinear_prep_local) -- issued while the all-gather is in flight.  False where the shape or
        precision does not take the fused kernels (forward() then does everything, as before)."""
        lib = _hip.load()
        (w,) = params
        br, dx = x.shape
        dy = w.shape[1]
        if precision == _hip.MI_PREC_FP8:
            return False
        ws = _hip.workspace(lib.mi_bilinear_workspace_bytes(br, b, dx, dy, precision), x.device)
        with torch.cuda.device(x.device):
            rc = lib.mi_bilinear_prep_local(x.data_ptr(), w.data_ptr(), br, b, dx, dy, precision, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(x.device).cuda_stream)
        if rc == _hip.MI_ESHAPE:
            return False
        _hip.check(rc, "mi_bilinear_prep_local")
        self._local_ws = ws
        self._local_key = (x.data_ptr(), w.data_ptr(), br, b, dx, dy, precision)
        return True

    def _take_local_ws(self, x, w, br, b, dx, dy, precision):
        """The workspace prep_local() filled -- only for the call it was made for (same tensors, shapes, precision)."""
        ws, self._local_ws = self._local_ws, None
        if ws is not None and self._local_key != (x.data_ptr(), w.data_ptr(), br, b, dx, dy, precision):
            return None  # a prep_local() whose forward never came: not this call's
        return ws

    def _workspace(self, x, y_all, params, precision, flags):
        if precision == _hip.MI_PREC_FP8 and self._fp8_ws is not None:
            ws, self._fp8_ws = self._fp8_ws, None
            return ws, 2  # bit 1: the fp8 operands are staged in this workspace
        if params:
            ws = self._take_local_ws(x, params[0], x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], precision)
            if ws is not None:
                return ws, 4  # bit 2: prep_local() already ran in this workspace
        return super()._workspace(x, y_all, params, precision, flags)

    def fp8_stage(self, stage, x, y_all, params, amax):
        """One stage of the fp8 mode's preparation (mi_bilinear_fp8_stage): ``amax`` (4 floats on the device: x, y, W, T)
        is MAX-all-reduced by the caller between the stages, so that every rank quantises with the whole batch's scales."""
        (w,) = params
        br, dx = x.shape
        b, dy = y_all.shape
        if stage == 0:
            self._fp8_ws = _hip.workspace(self.workspace_bytes(br, b, dx, dy, params, _hip.MI_PREC_FP8), x.device)
        ws = self._fp8_ws
        _hip.call("mi_bilinear_fp8_stage", x.device, x.data_ptr(), y_all.data_ptr(), w.data_ptr(), br, b, dx, dy, int(stage),
                  amax.data_ptr(), ws.data_ptr(), ws.numel())

    def forward_raw(self, x, y_all, params, sid_rows, sid_all, row_offset, estimator, precision):
        """Forward WITHOUT the finalize launch (mi_bilinear_fwd, need_grad bit 3): returns the fused kernel's per-wave
        records ([n, 4] float32, a view of the workspace) for the caller to all-gather, or None where the shape does not take
        that path.  `merge_backward` then merges the gathered records inside the backward's first launch."""
        off = ctypes.c_size_t(0)
        n = _hip.load().mi_bilinear_raw_records(x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], precision,
                                                ctypes.byref(off))
        if n == 0:
            return None
        ws, bits = self._workspace(x, y_all, params, precision, 1)
        stats = _hip.new_stats(x.device)  # (untouched by this call; the C ABI wants a valid pointer)
        self.fwd_call(x, y_all, params, sid_rows, sid_all, row_offset, estimator, precision, 1 | 8 | bits,
                      (None, stats, None, None), ws)()
        records = ws[off.value:off.value + 16 * n].view(torch.float32).view(n, 4)
        return records, (x, y_all, list(params), sid_rows, sid_all, row_offset, precision, None, ws)

    def merge_backward(self, saved, records_all, n_pos, estimator, grad_out, out=None, dw=True):
        """mi_bilinear_bwd_records: merge of the gathered raw records (rank order), loss, statistics and all gradients in
        the backward's two launches -> (loss, stats, grad_x, grad_y, [grad_w]).  ``dw=False``: the first launch only."""
        x, y, params, sid_rows, sid_all, row_offset, precision, _, ws = saved
        dev = x.device
        gx, gy, gp = out if out is not None else (torch.empty_like(x), torch.empty_like(y), [torch.empty_like(params[0])])
        loss, stats = torch.empty(1, dtype=torch.float32, device=dev), _hip.new_stats(dev)
        _hip.call("mi_bilinear_bwd_records", dev, x.data_ptr(), y.data_ptr(), params[0].data_ptr(), sid_rows.data_ptr(),
                  sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1], precision, estimator,
                  records_all.data_ptr(), records_all.shape[0], n_pos, grad_out.data_ptr(), loss.data_ptr(),
                  stats.data_ptr(), gx.data_ptr(), gy.data_ptr(), gp[0].data_ptr() if dw else None, ws.data_ptr(),
                  ws.numel())
        return loss, stats, gx, gy, gp

    def merge_backward_tail(self, saved, records_all, n_pos, estimator, grad_out, out=None):
        """The first launch of merge_backward only (mi_bilinear_bwd_records with grad_w = NULL): statistics, loss, grad_x and
        the partial grad_y.  The caller starts the reduce-scatter of grad_y and then calls ``backward_dw``."""
        if out is None:
            out = (torch.empty_like(saved[0]), torch.empty_like(saved[1]), [None])
        return self.merge_backward(saved, records_all, n_pos, estimator, grad_out, out, dw=False)[:4]

    def backward_dw(self, saved, out=None):
        """dW = X^T dT (mi_bilinear_bwd_dw) from the workspace merge_backward_tail left."""
        x, y_all, params, _sr, _sa, _ro, precision, _, ws = saved
        gw = torch.empty_like(params[0]) if out is None else out[2][0]
        _hip.call("mi_bilinear_bwd_dw", x.device, x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], precision,
                  gw.data_ptr(), ws.data_ptr(), ws.numel())
        return [gw]


class HipSeparableOps(_HipOps):
    """S = (X Wg)(Y Wh)^T row block (BASELINE.json configs[1]); params = [Wg, Wh].  Every rank projects ALL text rows
    (B d k flops, small beside the B^2 stage); d(Wh) and dY are partials over the row block like the bilinear dY."""

    @staticmethod
    def workspace_bytes(br, b, dx, dy, params, precision, need_grad=1):
        return _hip.load().mi_separable_workspace_bytes(br, b, dx, dy, params[0].shape[1], precision)

    def fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, estimator, precision, flags, out, ws):
        (wg, wh), (loss, stats, record, _) = params, out
        return _call("mi_separable_fwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], estimator, precision, flags, loss.data_ptr(), stats.data_ptr(), record.data_ptr(),
                     ws.data_ptr(), ws.numel())

    def bwd_call(self, saved, stats, grad_out, out):
        x, y, (wg, wh), sid_rows, sid_all, row_offset, precision, _, ws = saved
        gx, gy, (gg, gh) = out
        return _call("mi_separable_bwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], precision, stats.data_ptr(), grad_out.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                     gg.data_ptr(), gh.data_ptr(), ws.data_ptr(), ws.numel(), 1)

    def step_call(self, x, y, params, sid, estimator, precision, grad_out, out, grads, ws):
        """Forward + backward of the whole batch in one call (mi_separable_step)."""
        (wg, wh), (loss, stats, record, _), (gx, gy, (gg, gh)) = params, out, grads
        return _call("mi_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], estimator, precision,
                     grad_out.data_ptr(), loss.data_ptr(), stats.data_ptr(), record.data_ptr(), gx.data_ptr(),
                     gy.data_ptr(), gg.data_ptr(), gh.data_ptr(), ws.data_ptr(), ws.numel())

    @staticmethod
    def chain_workspace_bytes(entry, b, dx, dy, params, precision):
        return getattr(_hip.load(), f"{entry}_separable_workspace_bytes")(b, dx, dy, params[0].shape[1], precision)

    def chain_call(self, entry, x, y, params, sid, mode, precision, loss, r, c, grads, ws):
        wg, wh = params
        return _call(f"{entry}_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], mode, precision, None,
                     loss.data_ptr(), r.data_ptr(), _p(c), *[_p(g) for g in grads or [None] * 4], ws.data_ptr(),
                     ws.numel())

    @staticmethod
    def rank_workspace_bytes(b, dx, dy, params, precision):
        return _hip.load().mi_rank_separable_workspace_bytes(b, dx, dy, params[0].shape[1], precision)

    def rank_call(self, x, y, params, sid, precision, rank_i2t, rank_t2i, diag, ws):
        """Retrieval ranks of the whole batch (mi_rank_separable), as ``HipBilinearOps.rank_call``."""
        wg, wh = params
        return _call("mi_rank_separable", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], precision, _p(rank_i2t),
                     _p(rank_t2i), _p(diag), ws.data_ptr(), ws.numel())

    @staticmethod
    def estimates_workspace_bytes(b, dx, dy, params, precision):
        return _hip.load().mi_estimates_separable_workspace_bytes(b, dx, dy, params[0].shape[1], precision)

    def estimates_call(self, x, y, params, sid, precision, taus, est, ws):
        """MI estimates of the whole batch (mi_estimates_separable), as ``HipBilinearOps.estimates_call``."""
        wg, wh = params
        return _call("mi_estimates_separable", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], precision, estimates_taus(taus),
                     len(taus), est.data_ptr(), ws.data_ptr(), ws.numel())

    @staticmethod
    def topk_workspace_bytes(n_img, n_txt, dx, dy, params, precision, k):
        return _hip.load().mi_topk_separable_workspace_bytes(n_img, n_txt, dx, dy, params[0].shape[1], precision, k)

    def topk_call(self, x, y, params, sid_img, sid_txt, precision, k, out_i2t, out_t2i, ws):
        """Top-k retrieval over a gallery (mi_topk_separable), as ``HipBilinearOps.topk_call``."""
        wg, wh = params
        (ii, vi), (it, vt) = out_i2t or (None, None), out_t2i or (None, None)
        return _call("mi_topk_separable", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(), _p(sid_img),
                     _p(sid_txt), x.shape[0], y.shape[0], x.shape[1], y.shape[1], wg.shape[1], precision, k, _p(ii), _p(vi),
                     _p(it), _p(vt), ws.data_ptr(), ws.numel())

    @staticmethod
    def hardnce_workspace_bytes(b, dx, dy, params, precision, k, need_grad):
        return _hip.load().mi_hardnce_separable_workspace_bytes(b, dx, dy, params[0].shape[1], precision, k,
                                                                int(bool(need_grad)))

    def hardnce_call(self, x, y, params, sid, mode, precision, k, loss, r, c, idx_rows, idx_cols, grads, ws):
        """Hard-negative InfoNCE step (mi_hardnce_separable_step), as ``HipBilinearOps.hardnce_call``."""
        wg, wh = params
        return _call("mi_hardnce_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], mode, precision, k, None,
                     loss.data_ptr(), _p(r), _p(c), _p(idx_rows), _p(idx_cols), *[_p(g) for g in grads or [None] * 4],
                     ws.data_ptr(), ws.numel())

    @staticmethod
    def banknce_workspace_bytes(b, m, dx, dy, params, mode, precision, need_grad):
        return _hip.load().mi_banknce_separable_workspace_bytes(b, m, dx, dy, params[0].shape[1], mode, precision,
                                                                int(bool(need_grad)))

    def banknce_call(self, x, y, params, sid, bank_x, bank_y, bank_sid, mode, precision, loss, r, c, grads, ws):
        """Memory-bank InfoNCE step (mi_banknce_separable_step), as ``HipBilinearOps.banknce_call``."""
        wg, wh = params
        return _call("mi_banknce_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), _p(bank_x), bank_y.data_ptr(), bank_sid.data_ptr(), x.shape[0], bank_y.shape[0],
                     x.shape[1], y.shape[1], wg.shape[1], mode, precision, None, loss.data_ptr(), _p(r), _p(c),
                     *[_p(g) for g in grads or [None] * 4], ws.data_ptr(), ws.numel())

    @staticmethod
    def posnce_workspace_bytes(b, dx, dy, params, precision, need_grad):
        return _hip.load().mi_posnce_separable_workspace_bytes(b, dx, dy, params[0].shape[1], precision,
                                                               int(bool(need_grad)))

    def posnce_call(self, x, y, params, sid, mode, precision, loss, r, c, n_pos, grads, ws):
        """Study-positive InfoNCE step (mi_posnce_separable_step), as ``HipBilinearOps.posnce_call``."""
        wg, wh = params
        return _call("mi_posnce_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], mode, precision, None,
                     loss.data_ptr(), _p(r), _p(c), _p(n_pos), *[_p(g) for g in grads or [None] * 4], ws.data_ptr(),
                     ws.numel())

    @staticmethod
    def softnce_workspace_bytes(b, dx, dy, params, precision, need_grad):
        return _hip.load().mi_softnce_separable_workspace_bytes(b, dx, dy, params[0].shape[1], precision,
                                                                int(bool(need_grad)))

    def softnce_call(self, x, y, params, lab, mode, precision, tau, mix, loss, r, c, z, grads, ws):
        """Soft-target InfoNCE step (mi_softnce_separable_step), as ``HipBilinearOps.softnce_call``."""
        wg, wh = params
        return _call("mi_softnce_separable_step", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     lab.data_ptr(), x.shape[0], x.shape[1], y.shape[1], wg.shape[1], mode, precision, tau, mix, None,
                     loss.data_ptr(), _p(r), _p(c), _p(z), *[_p(g) for g in grads or [None] * 4], ws.data_ptr(),
                     ws.numel())

    @staticmethod
    def nce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_nce_separable_shard_workspace_bytes(br, b, dx, dy, params[0].shape[1], precision)

    def nce_fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, mode, precision, part, r, ws):
        wg, wh = params
        return _call("mi_nce_separable_shard_fwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, part.data_ptr(), _p(r), ws.data_ptr(), ws.numel())

    def nce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, (wg, wh), sid_rows, sid_all, row_offset, mode, precision, ws = saved
        gx, gy, (gg, gh) = out
        return _call("mi_nce_separable_shard_bwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, lse_cols.data_ptr(), grad_out.data_ptr(), gx.data_ptr(),
                     gy.data_ptr(), gg.data_ptr(), gh.data_ptr(), ws.data_ptr(), ws.numel())

    @staticmethod
    def posnce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_posnce_separable_shard_workspace_bytes(br, b, dx, dy, params[0].shape[1], precision)

    def posnce_fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, mode, precision, part, r, n_pos, ws):
        wg, wh = params
        return _call("mi_posnce_separable_shard_fwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, part.data_ptr(), _p(r), _p(n_pos), ws.data_ptr(), ws.numel())

    def posnce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, (wg, wh), sid_rows, sid_all, row_offset, mode, precision, ws = saved
        gx, gy, (gg, gh) = out
        return _call("mi_posnce_separable_shard_bwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, _p(lse_cols), _p(grad_out), gx.data_ptr(), gy.data_ptr(),
                     gg.data_ptr(), gh.data_ptr(), ws.data_ptr(), ws.numel())

    @staticmethod
    def softnce_shard_workspace_bytes(br, b, dx, dy, params, precision):
        return _hip.load().mi_softnce_separable_shard_workspace_bytes(br, b, dx, dy, params[0].shape[1], precision)

    def softnce_fwd_call(self, x, y, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, part, r, z, ws):
        wg, wh = params
        return _call("mi_softnce_separable_shard_fwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     lab_rows.data_ptr(), lab_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, tau, mix, part.data_ptr(), _p(r), _p(z), ws.data_ptr(), ws.numel())

    def softnce_bwd_call(self, saved, lse_cols, grad_out, out):
        x, y, (wg, wh), lab_rows, lab_all, row_offset, mode, precision, tau, mix, ws = saved
        gx, gy, (gg, gh) = out
        return _call("mi_softnce_separable_shard_bwd", x.device, x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(),
                     lab_rows.data_ptr(), lab_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     wg.shape[1], mode, precision, tau, mix, _p(lse_cols), _p(grad_out), gx.data_ptr(), gy.data_ptr(),
                     gg.data_ptr(), gh.data_ptr(), ws.data_ptr(), ws.numel())


class HipConcatMlpOps(_HipOps):
    """S[i,j] = MLP([x_i ; y_j]) row block; params = [W1, b1, W2, b2, w3, b3] (w3 flat or [1, h2])."""

    def _scores(self, x, y_all):
        return torch.empty(x.shape[0], y_all.shape[0], dtype=torch.float32, device=x.device)

    @staticmethod
    def workspace_bytes(br, b, dx, dy, params, precision, need_grad=1):
        return _hip.load().mi_concat_mlp_workspace_bytes(br, b, dx, dy, params[0].shape[0], params[2].shape[0],
                                                         precision, int(need_grad))

    def fwd_call(self, x, y, params, sid_rows, sid_all, row_offset, estimator, precision, flags, out, ws):
        loss, stats, record, scores = out
        return _call("mi_concat_mlp_fwd", x.device, x.data_ptr(), y.data_ptr(), *[p.data_ptr() for p in params],
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     params[0].shape[0], params[2].shape[0], estimator, precision, flags, loss.data_ptr(),
                     stats.data_ptr(), record.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel())

    def bwd_call(self, saved, stats, grad_out, out):
        x, y, params, sid_rows, sid_all, row_offset, precision, scores, ws = saved
        gx, gy, gp = out
        return _call("mi_concat_mlp_bwd", x.device, x.data_ptr(), y.data_ptr(), *[p.data_ptr() for p in params],
                     sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                     params[0].shape[0], params[2].shape[0], precision, stats.data_ptr(), grad_out.data_ptr(),
                     scores.data_ptr(), gx.data_ptr(), gy.data_ptr(), *[g.data_ptr() for g in gp], ws.data_ptr(),
                     ws.numel())

    # ---------------------------------------------- Jensen-Shannon / NWJ bounds (mi_fdiv_concat_mlp_*)
    def fdiv_forward(self, x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, need_grad):
        """(loss [1], terms [2], saved) of the row block; ``saved`` = (..., mode, precision, scores, stats, ws) for
        ``fdiv_backward``."""
        dev = x.device
        ws = _hip.workspace(self.workspace_bytes(x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], params,
                                                 precision, int(bool(need_grad))), dev)
        loss, terms = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
        stats, scores = _hip.new_stats(dev), self._scores(x, y_all)
        _hip.call("mi_fdiv_concat_mlp_fwd", dev, x.data_ptr(), y_all.data_ptr(), *[p.data_ptr() for p in params],
                  sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y_all.shape[0], row_offset, x.shape[1],
                  y_all.shape[1], params[0].shape[0], params[2].shape[0], mode, precision, int(bool(need_grad)),
                  loss.data_ptr(), terms.data_ptr(), stats.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel())
        return loss, terms, (x, y_all, list(params), sid_rows, sid_all, row_offset, mode, precision, scores, stats, ws)

    def fdiv_backward(self, saved, grad_out):
        """(grad_x, grad_y, [grad_params...]) of grad_out[0] * loss from the forward's scores, statistics and workspace."""
        x, y, params, sid_rows, sid_all, row_offset, mode, precision, scores, stats, ws = saved
        gx, gy, gp = torch.empty_like(x), torch.empty_like(y), [torch.empty_like(p) for p in params]
        _hip.call("mi_fdiv_concat_mlp_bwd", x.device, x.data_ptr(), y.data_ptr(), *[p.data_ptr() for p in params],
                  sid_rows.data_ptr(), sid_all.data_ptr(), x.shape[0], y.shape[0], row_offset, x.shape[1], y.shape[1],
                  params[0].shape[0], params[2].shape[0], mode, precision, stats.data_ptr(), grad_out.data_ptr(),
                  scores.data_ptr(), gx.data_ptr(), gy.data_ptr(), *[g.data_ptr() for g in gp], ws.data_ptr(), ws.numel())
        return gx, gy, gp

    # ---------------------------------------------- the critic as a differentiable score matrix (fused_scores.py)
    def scores_forward(self, x, y_all, params, precision, need_grad):
        """(scores [b_rows, b], saved) of the rows ``x`` against all of ``y_all`` (mi_concat_mlp_scores_fwd: the score
        kernels alone, no study ids and no loss); ``saved`` = (x, y_all, params, precision, ws) for ``scores_backward``,
        which needs ``need_grad``."""
        flags = int(bool(need_grad))
        ws = _hip.workspace(self.workspace_bytes(x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], params, precision,
                                                 flags), x.device)
        scores = self._scores(x, y_all)
        _hip.call("mi_concat_mlp_scores_fwd", x.device, x.data_ptr(), y_all.data_ptr(), *[p.data_ptr() for p in params],
                  x.shape[0], y_all.shape[0], x.shape[1], y_all.shape[1], params[0].shape[0], params[2].shape[0], precision,
                  flags, scores.data_ptr(), ws.data_ptr(), ws.numel())
        return scores, (x, y_all, list(params), precision, ws)

    def scores_backward(self, saved, grad_scores):
        """(grad_x, grad_y, [grad_params...]) of sum(grad_scores * scores) for a contiguous float32 ``grad_scores``
        [b_rows, b] (mi_concat_mlp_bwd_from_g).  The workspace is read, not consumed: the call can be repeated."""
        x, y, params, precision, ws = saved
        gx, gy, gp = torch.empty_like(x), torch.empty_like(y), [torch.empty_like(p) for p in params]
        stats = _hip.new_stats(x.device)  # scratch of the call: max|grad_scores| and the kernels' grad_out = 1
        _hip.call("mi_concat_mlp_bwd_from_g", x.device, x.data_ptr(), y.data_ptr(), *[p.data_ptr() for p in params],
                  x.shape[0], y.shape[0], x.shape[1], y.shape[1], params[0].shape[0], params[2].shape[0], precision,
                  grad_scores.data_ptr(), stats.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                  *[g.data_ptr() for g in gp], ws.data_ptr(), ws.numel())
        return gx, gy, gp


OPS ={"bilinear": HipBilinearOps, "separable": HipSeparableOps, "concat_mlp": HipConcatMlpOps}
