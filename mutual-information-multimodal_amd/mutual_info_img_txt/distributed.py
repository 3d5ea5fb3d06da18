"""Global-batch negatives across the GPUs of one node (one process per GPU, torch.distributed over RCCL/xGMI).

The reference is single-process; "global batch" is defined as the reference loss at B = B_global
(SURVEY.md 8e).  The B x B score matrix is sharded by row blocks: rank g owns samples [g*B/G, (g+1)*B/G).

forward : all-gather the text embeddings and study ids (the only bulk exchange: B/G x d floats per rank), score the
          local row block against all columns with the fused kernel, all-gather one 32-byte partial record per rank
          (max, rescaled sum, positive sum, negative count) and merge the records IN RANK ORDER on every rank, so all
          ranks hold bit-identical statistics and loss.
backward: local kernel -> dX of the row block is complete; dY is a partial over this row block for ALL columns ->
          reduce-scatter; critic-parameter gradients -> all-reduce (sum: the loss is one global scalar).

The local compute is an ``ops`` object.  The product default runs the HIP kernels through the C ABI; the CPU tests
(gloo, world_size 2) inject an oracle-backed ops object to check the exchange logic without a GPU.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from . import _hip
# the product's local ops (through the C ABI); re-exported under their historical home
from .critic_ops import OPS, HipBilinearOps, HipConcatMlpOps, HipSeparableOps, resolve_critic  # noqa: F401


# ----------------------------------------------------------------------------------------------------------
# collectives (RCCL on GPUs; gloo in the CPU tests)
# ----------------------------------------------------------------------------------------------------------
def _all_gather_rows(t: torch.Tensor, group, async_op: bool = False):
    world = dist.get_world_size(group)
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    work = dist.all_gather_into_tensor(out, t.contiguous(), group=group, async_op=async_op)
    return (out, work) if async_op else out


def gather_under_local_work(ops, x, params, b, precision, gathers):
    """Overlap: ``gathers`` = callables that START the all-gathers of the text
    embeddings and ids (async: on RCCL's stream) and return their work handles; the part of the forward that depends on
    this rank's own rows only (``ops.prep_local``: conversions of X and W, T = X W) is then issued on the compute stream,
    and only after that the compute stream is made to wait for the gathers.  Ops objects without ``prep_local`` (the
    concat-MLP critic, whose first layer's text half needs the gathered rows) just wait."""
    works = [g() for g in gathers]
    if hasattr(ops, "prep_local"):
        ops.prep_local(x, params, b, precision)
    for w in works:
        if w is not None:
            w.wait()


def _reduce_scatter_rows(t: torch.Tensor, group) -> torch.Tensor:
    """Sum over ranks of t [G*r, ...], return this rank's block [r, ...]."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    rows = t.shape[0] // world
    if dist.get_backend(group) == "gloo":  # gloo has no reduce_scatter: all-reduce and slice (CPU tests only)
        t = t.contiguous()
        dist.all_reduce(t, group=group)
        return t[rank * rows:(rank + 1) * rows].clone()
    out = torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.reduce_scatter_tensor(out, t.contiguous(), group=group)
    return out


def _reduce_scatter_rows_start(t: torch.Tensor, group):
    """Start the reduce-scatter of t [G*r, ...] (async: on the backend's own stream); returns a function that waits for it
    and returns this rank's block.  What the caller launches in between runs beside the collective."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    rows = t.shape[0] // world
    t = t.contiguous()
    if dist.get_backend(group) == "gloo":  # gloo has no reduce_scatter: all-reduce and slice (CPU tests only)
        work = dist.all_reduce(t, group=group, async_op=True)

        def finish():
            work.wait()
            return t[rank * rows:(rank + 1) * rows].clone()
        return finish
    out = torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    work = dist.reduce_scatter_tensor(out, t, group=group, async_op=True)

    def finish():
        work.wait()
        return out
    return finish


def fp8_global_scales(ops, x, y_all, params, group) -> None:
    """fp8 mode (BASELINE configs[4]) on a sharded batch: per-tensor scales absmax / 448 of the WHOLE batch.  The local
    image rows (and the local rows of T = x W) differ between ranks, so the four absmax values are MAX-all-reduced
    between the stages of the preparation; the text embeddings are already all-gathered and W is replicated (their
    maxima are equal everywhere -- reducing them too keeps it one 16-byte collective).  Two collectives, forward only."""
    amax = torch.zeros(4, dtype=torch.float32, device=x.device)
    ops.fp8_stage(0, x, y_all, params, amax)
    dist.all_reduce(amax, op=dist.ReduceOp.MAX, group=group)
    ops.fp8_stage(1, x, y_all, params, amax)
    dist.all_reduce(amax, op=dist.ReduceOp.MAX, group=group)
    ops.fp8_stage(2, x, y_all, params, amax)


def flat_views(like: Sequence[torch.Tensor]):
    """One contiguous buffer and per-tensor views into it: the parameter gradients of a step travel in ONE all-reduce
    (six separate latency-bound collectives for the concat-MLP critic otherwise)."""
    if not like:
        return None, []
    flat = torch.empty(sum(t.numel() for t in like), dtype=like[0].dtype, device=like[0].device)
    views, off = [], 0
    for t in like:
        views.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    return flat, views


def _supports_out(ops) -> bool:
    import inspect
    try:
        return "out" in inspect.signature(ops.backward).parameters
    except (TypeError, ValueError):
        return False


class GlobalBatchCriticFn(torch.autograd.Function):
    """loss over the GLOBAL batch from this rank's row block.  Returns (loss[1], stats)."""

    @staticmethod
    def forward(ctx, ops, group, estimator: int, precision: int, sid_rows, x, y, *params):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        br = x.shape[0]
        need_grad = any(t.requires_grad for t in (x, y) + tuple(params))
        x = x.contiguous()
        params_c = [p.contiguous() for p in params]
        got = {}

        def start(name, t):
            def go():
                got[name], work = _all_gather_rows(t, group, async_op=True)
                return work
            return go
        gather_under_local_work(ops, x, params_c, world * br, precision, [start("y", y), start("sid", sid_rows)])
        y_all, sid_all = got["y"], got["sid"]
        if precision == _hip.MI_PREC_FP8:
            if not hasattr(ops, "fp8_stage"):
                raise ValueError('precision="fp8" on a sharded batch needs an ops object with fp8_stage (bilinear critic)')
            fp8_global_scales(ops, x, y_all, params_c, group)
        record, saved = ops.forward(x, y_all, params_c, sid_rows.contiguous(), sid_all, rank * br, estimator, precision,
                                    need_grad)
        records = _all_gather_rows(record.reshape(1, -1), group)  # [G, 8], rank order
        loss, stats = ops.merge(records, world * br, estimator)
        ctx.ops, ctx.group, ctx.saved = ops, group, saved
        ctx.param_like = [p.detach() for p in params]
        ctx.y_all_like, ctx.x_shape = y_all, tuple(x.shape)
        ctx.save_for_backward(stats)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, _gstats):
        (stats,) = ctx.saved_tensors
        go = grad_loss.reshape(-1)[:1].to(torch.float32).contiguous()
        params = ctx.param_like
        flat, views = flat_views(params)
        if flat is not None and _supports_out(ctx.ops):
            y_all_like = ctx.y_all_like
            gx = torch.empty(ctx.x_shape, dtype=y_all_like.dtype, device=y_all_like.device)
            gy_partial = torch.empty_like(y_all_like)
            ctx.ops.backward(ctx.saved, stats, go, out=(gx, gy_partial, views))
            gparams = views
        else:  # ops objects without preallocated outputs (the oracle-backed ones of the CPU tests)
            gx, gy_partial, gparams = ctx.ops.backward(ctx.saved, stats, go)
            if flat is not None:
                for v, g in zip(views, gparams):
                    v.copy_(g)
                gparams = views
        gy = _reduce_scatter_rows(gy_partial, ctx.group)
        if flat is not None:
            dist.all_reduce(flat, group=ctx.group)  # one collective for all parameter gradients
        return (None, None, None, None, None, gx, gy, *gparams)


class GlobalBatchNceFn(torch.autograd.Function):
    """Per-sample InfoNCE over the GLOBAL batch from this rank's row block.
    Returns (loss [1], lse_rows [b_rows], lse_cols [B]).

    forward : all-gather Y and the ids; the rank's scores -> one flat part (column partials, row terms, its diagonal
              scores); all-gather the parts; merge them in rank order -> c, loss (identical bits on every rank).
    backward: the rank's gradients from its r and the merged c -> dX complete, dY partial (reduce-scatter), parameter
              gradients partial (one flat all-reduce).  Five collectives per step, as GlobalBatchCriticFn's."""

    @staticmethod
    def forward(ctx, ops, group, mode: int, precision: int, sid_rows, x, y, *params):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        br = x.shape[0]
        x = x.contiguous()
        params_c = [p.contiguous() for p in params]
        y_all, work_y = _all_gather_rows(y, group, async_op=True)
        sid_all, work_sid = _all_gather_rows(sid_rows, group, async_op=True)
        work_y.wait()
        work_sid.wait()
        part, lse_rows, saved = ops.nce_forward(x, y_all, params_c, sid_rows.contiguous(), sid_all, rank * br, mode,
                                                precision)
        parts = _all_gather_rows(part.reshape(1, -1), group)  # [G, P], rank order
        loss, lse_cols = ops.nce_merge(parts, br, mode)
        ctx.ops, ctx.group, ctx.saved = ops, group, saved
        ctx.param_like = [p.detach() for p in params]
        ctx.save_for_backward(lse_cols)
        ctx.mark_non_differentiable(lse_rows, lse_cols)
        return loss, lse_rows, lse_cols

    @staticmethod
    def backward(ctx, grad_loss, _glr, _glc):
        (lse_cols,) = ctx.saved_tensors
        go = grad_loss.reshape(-1)[:1].to(lse_cols.dtype).contiguous()
        flat, views = flat_views(ctx.param_like)
        gx, gy_partial, gparams = ctx.ops.nce_backward(ctx.saved, lse_cols, go)
        if flat is not None:
            for v, g in zip(views, gparams):
                v.copy_(g)
            gparams = views
        gy = _reduce_scatter_rows(gy_partial, ctx.group)
        if flat is not None:
            dist.all_reduce(flat, group=ctx.group)  # one collective for all parameter gradients
        return (None, None, None, None, None, gx, gy, *gparams)


def global_batch_mi_bound(embedding_img, embedding_txt, study_id_codes, critic_params: Sequence[torch.Tensor],
                          estimator: str = "infonce", precision: str = "bf16", critic: str = "bilinear", group=None,
                          ops=None, return_stats: bool = False):
    """Reference loss at B = world_size * local_batch with this rank's [B/G, d] embeddings.
    ``study_id_codes``: int64 tensor [B/G] (codes must be consistent across ranks, e.g. the integer study ids).
    Every rank returns the same loss; ``.backward()`` leaves the gradient of the global loss w.r.t. the local
    embeddings and the (all-reduced) gradient w.r.t. the critic parameters.

    ``estimator`` = "infonce_rowwise" / "infonce_symmetric" (critic "bilinear" or "separable"): the per-sample InfoNCE
    normalised over the global batch (GlobalBatchNceFn), loss of shape []; ``return_stats=True`` then gives
    ``(loss, (lse_rows [B/G], lse_cols [B]))``."""
    est = _hip.check_estimator(estimator, critic, "sharded")
    if ops is None:
        ops = OPS[critic]()
    # the same name -> code resolution as on one GPU, except that the bf16x3 condition looks at this rank's row count
    # rather than at the global batch (kept as it is; tests/test_critic_resolution.py pins it)
    prec = resolve_critic(critic, precision, embedding_img.shape[0], embedding_img.shape[1], embedding_txt.shape[1],
                          critic_params)[2]
    fn = GlobalBatchNceFn if est.family == "nce" else GlobalBatchCriticFn
    loss, *stats = fn.apply(ops, group, est.code, prec, study_id_codes, embedding_img, embedding_txt, *critic_params)
    loss = est.shape_loss(loss)
    # stats: GlobalBatchCriticFn's statistics block, or GlobalBatchNceFn's (lse_rows, lse_cols)
    return (loss, stats[0] if len(stats) == 1 else tuple(stats)) if return_stats else loss


def _gather_block_inputs(group, y, codes):
    """The two input all-gathers of a row-block step, both in flight at once: (y_all [B, d_txt], codes_all [B])."""
    y_all, work_y = _all_gather_rows(y, group, async_op=True)
    codes_all, work_c = _all_gather_rows(codes, group, async_op=True)
    work_y.wait()
    work_c.wait()
    return y_all, codes_all


def _exchange_block_gradients(group, param_like, gx, gy_partial, gparams):
    """dY partial -> reduce-scatter, the parameter gradients -> ONE flat all-reduce: (gx, gy, *gparams)."""
    flat, views = flat_views(param_like)
    if flat is not None:
        for v, g in zip(views, gparams):
            v.copy_(g)
        gparams = views
    gy = _reduce_scatter_rows(gy_partial, group)
    if flat is not None:
        dist.all_reduce(flat, group=group)
    return (gx, gy, *gparams)


class GlobalBatchPosNceFn(torch.autograd.Function):
    """Study-positive InfoNCE over the GLOBAL batch from this rank's row block (DESIGN.md section
    5); the label-weighted InfoNCE of section 16 has the same protocol in ``distributed_label_targets``.  Returns (loss [1], lse_rows [b_rows], lse_cols [B], n_pos int32 [b_rows]).

    forward : all-gather Y and the ids; the rank's scores -> one flat part (column LSE partials, column positive-score
              partials, row terms, row counts); all-gather the parts; merge them in rank order -> c, loss (identical bits
              on every rank).
    backward: the rank's gradients from its r, 1/n and the merged c -> dX complete, dY partial (reduce-scatter),
              parameter gradients partial (one flat all-reduce).  Five collectives per step, as GlobalBatchNceFn's."""

    @staticmethod
    def forward(ctx, ops, group, mode: int, precision: int, sid_rows, x, y, *params):
        rank = dist.get_rank(group)
        br = x.shape[0]
        x = x.contiguous()
        params_c = [p.contiguous() for p in params]
        y_all, sid_all = _gather_block_inputs(group, y, sid_rows)
        part, lse_rows, n_pos, saved = ops.posnce_forward(x, y_all, params_c, sid_rows.contiguous(), sid_all, rank * br,
                                                          mode, precision)
        parts = _all_gather_rows(part.reshape(1, -1), group)  # [G, P], rank order
        loss, lse_cols = ops.posnce_merge(parts, br, mode)
        ctx.ops, ctx.group, ctx.saved = ops, group, saved
        ctx.param_like = [p.detach() for p in params]
        ctx.save_for_backward(lse_cols)
        ctx.mark_non_differentiable(lse_rows, lse_cols, n_pos)
        return loss, lse_rows, lse_cols, n_pos

    @staticmethod
    def backward(ctx, grad_loss, *_):
        (lse_cols,) = ctx.saved_tensors
        go = grad_loss.reshape(-1)[:1].to(lse_cols.dtype).contiguous()
        gx, gy_partial, gparams = ctx.ops.posnce_backward(ctx.saved, lse_cols, go)
        return (None,) * 5 + _exchange_block_gradients(ctx.group, ctx.param_like, gx, gy_partial, gparams)


_BLOCK_LOSS_PRECISIONS = (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3)


def _block_loss_setup(what: str, embedding_img, embedding_txt, codes, critic_params, precision: str, critic: str, ops):
    """(ops, precision code) of a training loss on a sharded batch: bilinear and separable critics, the precisions of the
    one-GPU losses; ``codes`` is this rank's int64 [B/G] id or mask tensor."""
    if critic not in ("bilinear", "separable"):
        raise ValueError(f"{what} is implemented for the bilinear and separable critics only (got {critic!r})")
    if embedding_img.dim() != 2 or embedding_txt.dim() != 2 or embedding_img.shape[0] != embedding_txt.shape[0]:
        raise ValueError("embedding_img / embedding_txt must be [B/G, d_img] / [B/G, d_txt]")
    if codes.dtype != torch.int64 or codes.dim() != 1 or codes.shape[0] != embedding_img.shape[0]:
        raise ValueError("the id codes / label masks of a rank must be an int64 tensor [B/G]")
    prec = resolve_critic(critic, precision, embedding_img.shape[0], embedding_img.shape[1], embedding_txt.shape[1],
                          critic_params)[2]  # (as global_batch_mi_bound: bf16x3 looks at this rank's row count)
    if prec not in _BLOCK_LOSS_PRECISIONS:
        raise ValueError(f'precision="{precision}" is not available for {what} of the {critic} critic '
                         '(use "f32", "f32_exact", "bf16" or "bf16x3")')
    return (ops if ops is not None else OPS[critic]()), prec


def global_batch_study_positive_infonce(embedding_img, embedding_txt, study_id_codes,
                                        critic_params: Sequence[torch.Tensor], symmetric: bool = True,
                                        precision: str = "f32", critic: str = "bilinear", group=None, ops=None,
                                        return_stats: bool = False):
    """``study_positives.study_positive_infonce`` at B = world_size * local_batch with this rank's [B/G, d] embeddings:
    every same-study pair of the GLOBAL batch is a positive, wherever its two members sit (GlobalBatchPosNceFn).
    ``study_id_codes``: int64 tensor [B/G] (codes must be consistent across ranks, e.g. the integer study ids);
    ``critic`` "bilinear" (``critic_params`` = [W]) or "separable" ([Wg, Wh]).  Every rank returns the same 0-d loss;
    ``.backward()`` leaves the gradient of the global loss w.r.t. the local embeddings and the (all-reduced) gradient
    w.r.t. the critic parameters.  A training loss, not an MI bound, and not an estimator name.

    ``return_stats=True``: ``(loss, {"lse_rows": r [B/G], "lse_cols": c [B], "n_pos": n int32 [B/G]})``."""
    ops, prec = _block_loss_setup("the study-positive InfoNCE", embedding_img, embedding_txt, study_id_codes,
                                  critic_params, precision, critic, ops)
    mode = _hip.MI_NCE_SYMMETRIC if symmetric else _hip.MI_NCE_ROWWISE
    loss, r, c, n_pos = GlobalBatchPosNceFn.apply(ops, group, mode, prec, study_id_codes, embedding_img, embedding_txt,
                                                  *critic_params)
    loss = loss.reshape(())
    return (loss, {"lse_rows": r, "lse_cols": c, "n_pos": n_pos}) if return_stats else loss


class GlobalBatchGraphStep:
    """Forward + backward of the global-batch bound for FIXED shapes and storage, with the two compute sections of a
    step replayed from hipGraphs and the collectives issued eagerly between them:

        all-gather Y, ids (graph 0 under them: bf16 X, W and T = X W of the rank's own rows) |
        graph 1: rest of the local forward -> partial record | all-gather records |
        graph 2: rank-ordered merge + local backward | reduce-scatter dY, all-reduce d(params)

    Bilinear critic on the fused kernels ("raw-record mode"): graph 1 ends with the fused B x B kernel (no finalize
    launch), the all-gather moves every rank's per-wave records (16 bytes each, a few KB per rank) and the first launch
    of graph 2 merges ALL of them in the gathered order on every workgroup -- no merge launch either.

    Why: at global batch 4096 a rank's kernels take tens of microseconds, and launching them one by one from Python
    (plus an autograd graph) costs several times that.  The graphs hold exactly the C-ABI calls of
    ``GlobalBatchCriticFn``; no collective is captured (RCCL calls stay ordinary stream work between two replays).

    ``x``, ``y`` [B/G, d], ``sid`` int64 [B/G] and ``params`` are read in place on every ``step()``: update their
    contents (``copy_``), not the objects.  ``step()`` returns the loss ([1]); gradients are in ``grad_x``, ``grad_y``,
    ``grad_params`` (overwritten by every step)."""

    def __init__(self, x, y, sid, params: Sequence[torch.Tensor], estimator: str = "infonce", precision: str = "bf16",
                 critic: str = "bilinear", group=None, ops=None, capture: bool = True, overlap_reduce_scatter=None):
        self.est = _hip.check_estimator(estimator, critic, "sharded graphed").code
        self.group = group
        # step_eager(): start the reduce-scatter of dY between the backward's two launches (it then runs beside dW).  OFF by
        # default: with direct calls the step is bound by the HOST (one-rank RCCL rehearsal, B = 4096: 0.196 ms per step
        # for 0.12 ms of kernels), and the extra C call + async handle cost 13 us there (0.208 ms) -- a GPU-side overlap
        # buys nothing until the host keeps ahead.  MI_DIST_RS_OVERLAP=1 or the argument turn it on.
        self.overlap_reduce_scatter = (bool(os.environ.get("MI_DIST_RS_OVERLAP")) if overlap_reduce_scatter is None
                                       else bool(overlap_reduce_scatter))
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.ops = ops if ops is not None else OPS[critic]()
        self.prec = resolve_critic(critic, precision, x.shape[0], x.shape[1], y.shape[1], params)[2]  # as above
        self.x, self.y, self.sid = x.detach(), y.detach(), sid
        self.params = [p.detach() for p in params]
        for t in (self.x, self.y, self.sid, *self.params):
            if not t.is_contiguous():
                raise ValueError("GlobalBatchGraphStep needs contiguous tensors (they are read in place)")
        br = x.shape[0]
        dev = x.device
        on_gpu = dev.type == "cuda"
        self.y_all = torch.empty((self.world * br,) + tuple(y.shape[1:]), dtype=y.dtype, device=dev)
        self.sid_all = torch.empty(self.world * br, dtype=sid.dtype, device=dev)
        self.records = torch.empty(self.world, _hip.RECORD_FLOATS, dtype=x.dtype if not on_gpu else torch.float32, device=dev)
        self.grad_out = torch.ones(1, dtype=x.dtype if not on_gpu else torch.float32, device=dev)
        # the parameter gradients of a step live in one flat buffer: ONE all-reduce per step
        self.grad_flat, self.grad_params = flat_views(self.params)
        self._out = None
        if _supports_out(self.ops):
            self.grad_x = torch.empty_like(self.x)
            self.grad_y_partial = torch.empty_like(self.y_all)
            self._out = (self.grad_x, self.grad_y_partial, self.grad_params)
        self.graph_fwd = self.graph_bwd = self.graph_local = self.graph_full = None
        # raw-record mode (ops.forward_raw / merge_backward): the per-wave records of every rank are gathered and merged
        # inside the backward's first launch -- no finalize and no merge launch.  MI_DIST_NO_RAW=1: A/B switch.
        self._raw = (hasattr(self.ops, "forward_raw") and self.prec != _hip.MI_PREC_FP8
                     and not os.environ.get("MI_DIST_NO_RAW"))
        self.records_raw = None
        # MI_DIST_NO_OVERLAP=1: A/B switch of the measurements in profiles/README.md (the local part then runs inside forward)
        self._has_local = hasattr(self.ops, "prep_local") and not os.environ.get("MI_DIST_NO_OVERLAP")
        self._gather_inputs(local=False)
        if self.prec == _hip.MI_PREC_FP8:
            if not hasattr(self.ops, "fp8_stage"):
                raise ValueError('precision="fp8" on a sharded batch needs the bilinear critic')
            capture = False  # the fp8 preparation holds collectives (global scales): issued eagerly
        if not (capture and on_gpu):
            return  # eager: the same calls issued one by one (the gloo tests on the CPU, `bench.py --graph off`)
        torch.cuda.synchronize()
        # warm-up on a side stream (module loading, attribute calls), then capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._prep_local()
            self._forward()
            self._gather_records()
            self._merge_backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if capture == "full":
            # ONE graph for the whole step, the five RCCL collectives captured with the kernels (RCCL calls are
            # capturable stream work): the host issues a single launch per step instead of ~12 calls.  Opt-in: the
            # capture of collectives could only be rehearsed with one rank on this project's one-GPU boxes.
            self._reduce_scatter_out = torch.empty_like(self.y) if dist.get_backend(group) != "gloo" else None
            with torch.cuda.stream(side):   # one eager pass of exactly the captured sequence (RCCL channel set-up)
                self._whole_step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            dist.barrier(group=self.group)
            self.graph_full = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_full):
                self._whole_step()
            self._remember_captured()
            self._captured["grad_y"] = self.grad_y
            return
        pool = torch.cuda.graph_pool_handle()
        if self._has_local:
            # the rank-local part as its own graph, replayed while the input all-gathers are in flight; its workspace is
            # the one the forward graph goes on with (both captured from one pool, the tensor kept in self.saved)
            local = torch.cuda.CUDAGraph()
            with torch.cuda.graph(local, pool=pool):
                self._prep_local()
            if getattr(self.ops, "_local_ws", None) is not None:
                self.graph_local = local
        self.graph_fwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_fwd, pool=pool):
            self._forward()
        # the record gathered from every rank must exist before the second capture reads it
        self._gather_records()
        self.graph_bwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_bwd, pool=pool):
            self._merge_backward()
        self._remember_captured()

    _CAPTURED_ATTRS = ("record", "saved", "loss", "stats", "grad_x", "grad_y_partial")

    def _remember_captured(self):
        """The tensors the graphs read and write.  step_eager() on this object rebinds record / saved / loss ... to a
        fresh eager workspace; a later replay must gather and return the CAPTURED ones again (in raw-record
        mode the backward graph otherwise merged the records of an older forward)."""
        self._captured = {k: getattr(self, k) for k in self._CAPTURED_ATTRS if hasattr(self, k)}

    def _restore_captured(self):
        for k, v in getattr(self, "_captured", {}).items():
            setattr(self, k, v)

    def _prep_local(self):
        if self._has_local:
            self.ops.prep_local(self.x, self.params, self.y_all.shape[0], self.prec)

    def _gather_inputs(self, local: bool = True):
        """The two input all-gathers, with the rank-local part of the forward issued while they are in flight.  Not
        captured: in the graphed mode the local part is its own small graph (graph_local) replayed at the same place."""
        works = [dist.all_gather_into_tensor(self.y_all, self.y, group=self.group, async_op=True),
                 dist.all_gather_into_tensor(self.sid_all, self.sid, group=self.group, async_op=True)]
        if local and self.graph_local is not None:
            self.graph_local.replay()
        elif local:
            self._prep_local()
        for w in works:
            w.wait()

    def _forward(self):
        if self._raw:
            got = self.ops.forward_raw(self.x, self.y_all, self.params, self.sid, self.sid_all,
                                       self.rank * self.x.shape[0], self.est, self.prec)
            if got is not None:
                self.record, self.saved = got  # [n, 4]: gathered as it is
                if self.records_raw is None:
                    self.records_raw = torch.empty((self.world * self.record.shape[0], 4), dtype=self.record.dtype,
                                                   device=self.record.device)
                return
            self._raw = False  # the shape does not take that path: the record protocol below, from now on
        if self.prec == _hip.MI_PREC_FP8:  # (two tiny MAX all-reduces inside: this section is never captured in that mode)
            fp8_global_scales(self.ops, self.x, self.y_all, self.params, self.group)
        self.record, self.saved = self.ops.forward(self.x, self.y_all, self.params, self.sid, self.sid_all,
                                                   self.rank * self.x.shape[0], self.est, self.prec, True)

    def _gather_records(self):
        if self._raw:
            dist.all_gather_into_tensor(self.records_raw, self.record, group=self.group)
        else:
            dist.all_gather_into_tensor(self.records, self.record.reshape(1, -1).to(self.records.dtype), group=self.group)

    def _merge_backward(self):
        if self._raw:
            self.loss, self.stats, gx, gy, gp = self.ops.merge_backward(
                self.saved, self.records_raw, self.world * self.x.shape[0], self.est, self.grad_out, out=self._out)
            if self._out is None:
                self.grad_x, self.grad_y_partial = gx, gy
                for v, g in zip(self.grad_params, gp):
                    v.copy_(g)
            return
        self.loss, self.stats = self.ops.merge(self.records, self.world * self.x.shape[0], self.est)
        if self._out is not None:
            self.ops.backward(self.saved, self.stats, self.grad_out, out=self._out)
        else:
            self.grad_x, self.grad_y_partial, gp = self.ops.backward(self.saved, self.stats, self.grad_out)
            for v, g in zip(self.grad_params, gp):
                v.copy_(g)

    def _exchange_gradients(self):
        self.grad_y = _reduce_scatter_rows(self.grad_y_partial, self.group)
        if self.grad_flat is not None:
            dist.all_reduce(self.grad_flat, group=self.group)

    def _whole_step(self):
        self._gather_inputs()
        self._forward()
        self._gather_records()
        self._merge_backward()
        if self._reduce_scatter_out is not None:
            dist.reduce_scatter_tensor(self._reduce_scatter_out, self.grad_y_partial, group=self.group)
            self.grad_y = self._reduce_scatter_out
        else:
            self.grad_y = _reduce_scatter_rows(self.grad_y_partial, self.group)
        if self.grad_flat is not None:
            dist.all_reduce(self.grad_flat, group=self.group)

    def step(self):
        """all-gather Y, ids | local forward | all-gather records | merge + local backward | reduce-scatter dY, ONE
        all-reduce of the flat parameter-gradient buffer.  Five collectives per step, in this order on every rank."""
        if self.graph_full is not None:
            self._restore_captured()
            self.graph_full.replay()
            return self.loss
        if self.graph_fwd is None:
            return self.step_eager()
        self._restore_captured()
        self._gather_inputs()
        self.graph_fwd.replay()
        self._gather_records()
        self.graph_bwd.replay()
        self._exchange_gradients()
        return self.loss

    def step_eager(self):
        self._gather_inputs()
        self._forward()
        self._gather_records()
        if self._raw and hasattr(self.ops, "merge_backward_tail") and self.overlap_reduce_scatter:
            # the reduce-scatter of dY needs the backward's FIRST launch only: started (on the backend's stream) before the
            # dW launch, it runs beside it; the parameter all-reduce follows dW.  Same five collectives, same order on
            # every rank.
            got = self.ops.merge_backward_tail(self.saved, self.records_raw, self.world * self.x.shape[0], self.est,
                                               self.grad_out, out=self._out)
            self.loss, self.stats = got[0], got[1]
            if self._out is None:
                self.grad_x, self.grad_y_partial = got[2], got[3]
            finish = _reduce_scatter_rows_start(self.grad_y_partial, self.group)
            gp = self.ops.backward_dw(self.saved, out=self._out)
            if self._out is None:
                for v, g in zip(self.grad_params, gp):
                    v.copy_(g)
            if self.grad_flat is not None:
                dist.all_reduce(self.grad_flat, group=self.group)
            self.grad_y = finish()
            return self.loss
        self._merge_backward()
        self._exchange_gradients()
        return self.loss
