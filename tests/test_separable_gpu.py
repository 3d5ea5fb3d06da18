"""The separable critic's DV / InfoNCE step, S = (X Wg)(Y Wh)^T, on every kernel path of plan_separable
(csrc/mi_bilinear.hip) at the shapes where those paths have edges, through the C ABI (mi_separable_step / _fwd / _bwd),
against the fp64 restatement of tests/separable_reference.py.  The case table lives there; tests/test_separable_cpu.py
checks that every case lands on the path its row names.

Tolerances (the project's own):
  f32 (generic kernels, exact fp32 products) against the exact reference, as test_separable_f32_vs_oracle: loss rtol 1e-5 /
    atol 5e-5; gradients rtol 2e-3 / atol 5e-4 max|ref|.  The entry points have no score output: the score bound of that
    test, 5e-5 max(|S|max, 1), is applied to the two statistics that are plain functions of the scores, lse and pos_mean.
  bf16 against the reference that rounds where the path rounds ("fused16" / "generic16"), as test_config1_separable_bf16 and
    test_separable_one_call_step: loss 2e-3 max(|S|max, 1); gradients 1.5e-2 max|ref|;
  bf16 also against the exact reference at the band of test_bilinear_bf16_vs_rounded_oracle, gradients 6e-2 max|ref|: the
    rounded reference did not drift along with the kernels.
  One call against two calls, as test_separable_one_call_step: loss 1e-5 max(|S|max, 1), gradients 2e-3 max|ref|.
Every comparison prints "SEPFIG <what> <error / tolerance>" before it asserts (python -m pytest -s shows them).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math
import os

import numpy as np
import pytest
import torch

import separable_reference as ref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu
GO = ref.GRAD_OUT
EST_CODES = {"dv": 0, "infonce": 1}


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    assert not any(os.environ.get(k) for k in ("MI_NO_TAIL", "MI_NO_FLASH", "MI_SEP_NO_FUSED_PREP", "MI_FLASH_SLAB_F32"))
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ references (computed once)
@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return ref.inputs(shape)


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, mode, row_block=None, offsets=()):
    """Shared between the tests and never written to."""
    return ref.step(*_inputs(shape), ref.ids(shape[0], kind, offsets), mode, row_block=row_block, grad_out=GO)


# ------------------------------------------------------------------------------------------------ the C ABI
class _Call:
    """One problem on the device: inputs, NaN-poisoned outputs and workspace, and the three entry points."""

    def __init__(self, dev, tensors, sid, prec, rows=None):
        from mutual_info_img_txt import _hip, mi_critics
        self.hip, self.lib, self.dev = _hip, _hip.load(), dev
        x, y, wg, wh = (t.float().contiguous() for t in tensors)
        self.b, self.dx, self.dy, self.k = x.shape[0], x.shape[1], y.shape[1], wg.shape[1]
        self.r0, self.br = (0, self.b) if rows is None else rows
        codes = mi_critics.study_id_codes(sid, dev)
        self.sid, self.sid_rows = codes, codes[self.r0:self.r0 + self.br].contiguous()
        self.x, self.y, self.wg, self.wh = (t.to(dev) for t in (x[self.r0:self.r0 + self.br].contiguous(), y, wg, wh))
        self.prec = _hip.PRECISIONS[prec]
        self.go = torch.full((1,), GO, device=dev)
        self.ws = torch.empty(max(int(self.lib.mi_separable_workspace_bytes(self.br, self.b, self.dx, self.dy, self.k,
                                                                            self.prec)), 256), dtype=torch.uint8, device=dev)
        self.poison()

    def poison(self, outputs=True, workspace=True):
        nan = lambda *s: torch.full(s, float("nan"), device=self.dev)  # noqa: E731
        if outputs:
            self.loss, self.record = nan(1), nan(self.hip.RECORD_FLOATS)
            self.stats = torch.full((self.hip.STATS_BYTES,), 0xFF, dtype=torch.uint8, device=self.dev)
            self.gx, self.gy = nan(self.br, self.dx), nan(self.b, self.dy)
            self.gwg, self.gwh = nan(self.dx, self.k), nan(self.dy, self.k)
        if workspace:
            self.ws.fill_(0xFF)   # NaN as fp32, bf16 and fp16

    def _run(self, name, *args):
        self.hip.call(name, self.dev, *args)
        torch.cuda.synchronize()

    def step(self, est):
        assert (self.r0, self.br) == (0, self.b)
        p = lambda t: t.data_ptr()  # noqa: E731
        self._run("mi_separable_step", p(self.x), p(self.y), p(self.wg), p(self.wh), p(self.sid), self.b, self.dx, self.dy,
                  self.k, EST_CODES[est], self.prec, p(self.go), p(self.loss), p(self.stats), p(self.record), p(self.gx),
                  p(self.gy), p(self.gwg), p(self.gwh), p(self.ws), self.ws.numel())
        return self

    def fwd(self, est, need_grad=1):
        p = lambda t: t.data_ptr()  # noqa: E731
        self._run("mi_separable_fwd", p(self.x), p(self.y), p(self.wg), p(self.wh), p(self.sid_rows), p(self.sid), self.br,
                  self.b, self.r0, self.dx, self.dy, self.k, EST_CODES[est], self.prec, need_grad, p(self.loss),
                  p(self.stats), p(self.record), p(self.ws), self.ws.numel())
        return self

    def bwd(self, from_forward, stats=None):
        p = lambda t: t.data_ptr()  # noqa: E731
        self._run("mi_separable_bwd", p(self.x), p(self.y), p(self.wg), p(self.wh), p(self.sid_rows), p(self.sid), self.br,
                  self.b, self.r0, self.dx, self.dy, self.k, self.prec, p(self.stats if stats is None else stats),
                  p(self.go), p(self.gx), p(self.gy), p(self.gwg), p(self.gwh), p(self.ws), self.ws.numel(), from_forward)
        return self

    def grads(self):
        return {"dx": self.gx.cpu().double(), "dy": self.gy.cpu().double(), "dwg": self.gwg.cpu().double(),
                "dwh": self.gwh.cpu().double()}

    def outputs(self):
        """Every output buffer, for bit comparisons."""
        return {"loss": self.loss.cpu(), "stats": self.stats.cpu()[:24].clone(), "stats_counts": self.stats.cpu()[32:48].clone(),
                "record": self.record.cpu(), **{k: v.float() for k, v in self.grads().items()}}

    def stats_dict(self):
        return self.hip.stats_dict(self.stats)

    def record_terms(self):
        m, s, pos, lo, hi = (float(v) for v in self.record.cpu()[:5])
        return (m + math.log(s) if s > 0 else -math.inf), pos, int(lo) + (int(hi) << 24)


def _merge(call, records, est):
    """mi_merge_partials over per-block records in block order, as the sharded step does: (loss [1], statistics)."""
    rec = torch.stack(records).contiguous()
    loss, stats = torch.empty(1, device=call.dev), call.hip.new_stats(call.dev)
    call.hip.call("mi_merge_partials", call.dev, rec.data_ptr(), rec.shape[0], call.b, EST_CODES[est], loss.data_ptr(),
                  stats.data_ptr())
    torch.cuda.synchronize()
    return loss, stats


# ------------------------------------------------------------------------------------------------ comparisons
def _figure(what, err, tol):
    print(f"SEPFIG {what} {err / tol if tol > 0 else (0.0 if err == 0 else math.inf):.3f}")


def _cls(v):
    """The class of a loss value: logsumexp of no negatives is -inf, and the DV form then subtracts log 0."""
    v = float(v)
    return "nan" if math.isnan(v) else ("finite" if math.isfinite(v) else ("+inf" if v > 0 else "-inf"))


def _check_loss(what, prec, est, loss, st, r_round, r_exact):
    """loss_out, and the statistics block: n_neg exactly, lse / pos_mean / both loss forms within the loss tolerance."""
    assert st["n_neg"] == r_round["n_neg"] and st["n_pos"] == r_round["scores"].shape[0], (what, st)
    want = {"loss": r_round[f"loss_{est}"], "loss_dv": r_round["loss_dv"], "loss_infonce": r_round["loss_infonce"],
            "lse": r_round["lse"], "pos_mean": r_round["pos_mean"]}
    got = {"loss": float(loss), **{k: st[k] for k in ("loss_dv", "loss_infonce", "lse", "pos_mean")}}
    if r_round["n_neg"] == 0:
        for k in want:
            assert _cls(got[k]) == _cls(want[k]), (what, k, got[k], float(want[k]))
        return
    sc = max(float(r_exact["scores"].abs().max()), 1.0)
    for k, w in want.items():
        w = float(w)
        if prec == "f32":
            tol = 5e-5 * sc if k in ("lse", "pos_mean") else 5e-5 + 1e-5 * abs(w)
        else:
            tol = 2e-3 * sc
        _figure(f"{what} {k}", abs(got[k] - w), tol)
        assert abs(got[k] - w) < tol, (what, k, got[k], w, tol)


def _check_grads(what, prec, got, r_round, r_exact, names=ref.GRADS):
    for name in names:
        g, rr, re = got[name], r_round[name], r_exact[name]
        assert bool(torch.isfinite(g).all()), (what, name)
        if prec == "f32":
            tol = 5e-4 * float(re.abs().max()) + 2e-3 * re.abs()
            ratio = float(((g - re).abs() / tol.clamp_min(1e-300)).max()) if float(re.abs().max()) > 0 else 0.0
            print(f"SEPFIG {what} {name} {ratio:.3f}")
            np.testing.assert_allclose(g.numpy(), re.numpy(), rtol=2e-3, atol=5e-4 * float(re.abs().max()), err_msg=f"{what} {name}")
            continue
        for tag, want, band in (("rounded", rr, 1.5e-2), ("exact", re, 6e-2)):
            err, tol = float((g - want).abs().max()), band * float(want.abs().max())
            _figure(f"{what} {name} vs-{tag}", err, tol)
            assert err < tol or err == tol == 0.0, (what, name, tag, err, tol)


def _check_cross(what, one, two, r_round, r_exact):
    """The one-call step against the two calls, at the bound of test_separable_one_call_step."""
    sc = max(float(r_exact["scores"].abs().max()), 1.0)
    if r_round["n_neg"] == 0:
        assert _cls(one[0]) == _cls(two[0])
    else:
        _figure(f"{what} loss one-vs-two", abs(float(one[0]) - float(two[0])), 1e-5 * sc)
        assert abs(float(one[0]) - float(two[0])) < 1e-5 * sc, what
    for name in ref.GRADS:
        err, tol = float((one[1][name] - two[1][name]).abs().max()), 2e-3 * float(r_round[name].abs().max())
        _figure(f"{what} {name} one-vs-two", err, tol)
        assert err < tol or err == tol == 0.0, (what, name, err, tol)


CASE_PARAMS = pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
ONE_PER_PATH = [c for c in ref.CASES if (c[0], c[1]) in (((96, 72, 200, 128), "bf16"), ((128, 32, 96, 128), "bf16"),
                                                          ((130, 20, 12, 10), "bf16"), ((130, 20, 12, 10), "f32"))]
assert [c[2] for c in ONE_PER_PATH] == [ref.FUSED, ref.FUSED_TAIL, ref.GENERIC, ref.GENERIC]


# ------------------------------------------------------------------------------------------------ tests
@CASE_PARAMS
@pytest.mark.parametrize("kind", ["unique", "dup"])
@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_step_vs_reference(dev, case, kind, est):
    """mi_separable_step: loss, statistics (n_neg exactly) and all four gradients of 0.37 * loss."""
    shape, prec, _, mode = case
    what = f"step {ref.case_id(case)} {kind} {est}"
    r_round, r_exact = _reference(shape, kind, mode), _reference(shape, kind, "exact")
    assert r_round["n_neg"] == int(orc.negative_mask(ref.ids(shape[0], kind)).sum())
    c = _Call(dev, _inputs(shape), ref.ids(shape[0], kind), prec).step(est)
    _check_loss(what, prec, est, c.loss.cpu(), c.stats_dict(), r_round, r_exact)
    _check_grads(what, prec, c.grads(), r_round, r_exact)


@CASE_PARAMS
@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_two_calls_vs_reference(dev, case, est):
    """mi_separable_fwd then mi_separable_bwd: on the forward's workspace (workspace_from_forward = 1) and on a workspace
    that holds nothing but NaN (0: the backward recomputes what it needs), both against the reference and against the
    one-call step."""
    shape, prec, _, mode = case
    kind = "dup"
    sid = ref.ids(shape[0], kind)
    r_round, r_exact = _reference(shape, kind, mode), _reference(shape, kind, "exact")
    one = _Call(dev, _inputs(shape), sid, prec).step(est)
    one = (one.loss.cpu(), one.grads())
    for wff in (1, 0):
        what = f"two-calls wff={wff} {ref.case_id(case)} {est}"
        c = _Call(dev, _inputs(shape), sid, prec).fwd(est)
        if not wff:
            c.poison(outputs=False)
        c.bwd(wff)
        _check_loss(what, prec, est, c.loss.cpu(), c.stats_dict(), r_round, r_exact)
        _check_grads(what, prec, c.grads(), r_round, r_exact)
        _check_cross(what, one, (c.loss.cpu(), c.grads()), r_round, r_exact)


@pytest.mark.parametrize("rbc", ref.ROW_BLOCK_CASES, ids=lambda c: ref.case_id(c) + f"-{len(c[4])}blocks")
@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_row_blocks(dev, rbc, est):
    """Row blocks through the C ABI: per-block forward records merged in block order (mi_merge_partials, as
    test_separable_row_blocks_equal_full_batch) give the full batch's loss and statistics; every block's record and
    grad_x are the reference's for its rows; the blocks' grad_y / grad_wg / grad_wh add up to the full batch's."""
    shape, prec, _, mode, blocks = rbc
    kind, offs = "dup", tuple(rb[0] for rb in blocks if rb[0])   # repeated ids at the blocks' own offsets as well
    sid = ref.ids(shape[0], kind, offs)
    what = f"row-blocks {ref.case_id(rbc)} {est}"
    r_round, r_exact = _reference(shape, kind, mode, None, offs), _reference(shape, kind, "exact", None, offs)
    calls = [_Call(dev, _inputs(shape), sid, prec, rows=rb).fwd(est) for rb in blocks]
    sc = max(float(r_exact["scores"].abs().max()), 1.0)
    for rb, c in zip(blocks, calls):
        rr = _reference(shape, kind, mode, rb, offs)
        lse, pos, n = c.record_terms()
        assert n == rr["block_n_neg"], (what, rb)
        tol = 5e-5 * sc if prec == "f32" else 2e-3 * sc
        assert abs(lse - float(rr["block_lse"])) < tol and abs(pos - float(rr["block_pos_sum"])) < tol * rb[1], (what, rb)
    loss, stats = _merge(calls[0], [c.record for c in calls], est)
    _check_loss(what, prec, est, loss.cpu(), calls[0].hip.stats_dict(stats), r_round, r_exact)
    total = {name: 0.0 for name in ref.GRADS[1:]}
    for rb, c in zip(blocks, calls):
        g = c.bwd(1, stats=stats).grads()
        _check_grads(f"{what} block {rb}", prec, g, _reference(shape, kind, mode, rb, offs),
                     _reference(shape, kind, "exact", rb, offs), names=("dx",))
        for name in total:
            total[name] = total[name] + g[name]
    _check_grads(f"{what} summed", prec, total, r_round, r_exact, names=ref.GRADS[1:])


@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_row_block_at_unaligned_offset(dev, est):
    """Rows [40, 72) of 96: an offset that is no multiple of 32, so the diagonal of the pair matrix cuts through the
    32 x 32 tiles (the separable twin of test_flash_unaligned_row_offset_and_flag_values).  The block's record, its grad_x
    and its parts of grad_y / grad_wg / grad_wh against the reference's terms of those rows, under the statistics of the
    whole batch."""
    shape, prec, _, mode, rb = ref.UNALIGNED_BLOCK
    kind, offs = "dup", (rb[0],)
    sid = ref.ids(shape[0], kind, offs)
    what = f"unaligned-block {rb} {est}"
    full = _Call(dev, _inputs(shape), sid, prec).fwd(est, need_grad=0)
    c = _Call(dev, _inputs(shape), sid, prec, rows=rb).fwd(est)
    rr, re = _reference(shape, kind, mode, rb, offs), _reference(shape, kind, "exact", rb, offs)
    sc = max(float(re["scores"].abs().max()), 1.0)
    lse, pos, n = c.record_terms()
    assert n == rr["block_n_neg"] == int(orc.negative_mask(sid)[rb[0]:rb[0] + rb[1]].sum())
    assert abs(lse - float(rr["block_lse"])) < 2e-3 * sc and abs(pos - float(rr["block_pos_sum"])) < 2e-3 * sc * rb[1]
    _check_loss(what, prec, est, full.loss.cpu(), full.stats_dict(), rr, re)
    _check_grads(what, prec, c.bwd(1, stats=full.stats).grads(), rr, re)


@pytest.mark.parametrize("shape", ref.FUSED_CASES + ref.TAIL_CASES[:1], ids=lambda s: "-".join(map(str, s)))
def test_structure_exact(dev, shape):
    """The separable twin of test_flash_structure_exact.  Operands from {-1, 0, 1}; Wg is zero in the second half of its
    columns and Wh in the first, so S == 0 exactly, every exponential is 1 and A, C are small integers, exact in bf16, with
    pairwise distinct rows (ref.structure_inputs).  Then dA_i = 0.37 ((sum_{j in neg(i)} C_j) / n_neg - C_i / b) with integer
    sums, likewise dC: operand maps, mask, diagonal, slab layout and the dW launches are pinned without any rounding but
    that of dA / dC in the way.  The one-call step and the two calls."""
    x, y, wg, wh, sid = ref.structure_inputs(shape)
    s = ref.structure_reference(x, y, wg, wh, sid, GO)
    # on the CPU first: one wrong row in either sum moves the reference by more than the bound asserted below
    assert ref.structure_row_swap_shows(x, y, wg, wh, sid, GO)
    for route in ("step", "two-calls"):
        what = f"structure {'-'.join(map(str, shape))} {route}"
        c = _Call(dev, (x, y, wg, wh), sid, "bf16")
        c = c.step("infonce") if route == "step" else c.fwd("infonce").bwd(1)
        assert c.stats_dict()["n_neg"] == s["n_neg"]
        assert abs(float(c.loss.cpu()) - math.log(s["n_neg"])) < 1e-5
        g = c.grads()
        # dX = dA Wg^T: dA lives in the columns where Wg is zero (dY likewise): exact zeros, not small numbers
        assert float(g["dx"].abs().max()) == 0.0 and float(g["dy"].abs().max()) == 0.0, what
        # the bound, derived in ref.structure_reference: every dA / dC element carries ONE bf16 rounding, half an ulp of its
        # exact value (2^-9 .. 2^-8 of it) plus the fp32 arithmetic that forms it (2^-18 of either of its two terms);
        # dWg[a, c] = sum_i X[i, a] dA[i, c] adds these up over the non-zero X[i, a] (integers), in fp32 (2^-19 of the
        # absolute sum), so  |dWg - ref| <= |X|^T (ulp_bf16(dA) / 2 + 2^-18 (|sum term| + |diagonal term|)) + 2^-19 |X|^T |dA|
        for name in ("dwg", "dwh"):
            want, bound = s[name]
            err = (g[name] - want).abs()
            ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max())
            print(f"SEPFIG {what} {name} {ratio:.3f}")
            assert bool((err <= bound).all()), (what, name, ratio, float(err[bound == 0].max()) if bool((bound == 0).any()) else 0.0)


@pytest.mark.parametrize("case", ONE_PER_PATH, ids=ref.case_id)
def test_hygiene(dev, case):
    """Outputs and workspace NaN-poisoned before every call: two calls give identical bits for every output, every output
    element is finite (so every element was written), and a forward-only call (need_grad = 0) returns the same
    statistics -- n_neg exactly, the loss to the 1e-4 max(|loss|, 1) of test_flash_small_batches_d512 (the forward-only
    kernel keeps reference points of its own: the sums differ in fp32 rounding)."""
    shape, prec, _, _ = case
    sid = ref.ids(shape[0], "dup")
    for route in ("step", "two-calls"):
        outs = []
        for _ in range(2):
            c = _Call(dev, _inputs(shape), sid, prec)
            c = c.step("dv") if route == "step" else c.fwd("dv").bwd(1)
            outs.append(c.outputs())
        for name, t in outs[0].items():
            if t.dtype.is_floating_point:
                assert bool(torch.isfinite(t).all()), (route, name)
            assert torch.equal(t.view(torch.uint8), outs[1][name].view(torch.uint8)), (route, name)
    f = _Call(dev, _inputs(shape), sid, prec).fwd("dv", need_grad=0)
    sf, sg, loss = f.stats_dict(), c.stats_dict(), float(c.loss.cpu())
    assert sf["n_neg"] == sg["n_neg"] and sf["n_pos"] == sg["n_pos"]
    assert abs(float(f.loss.cpu()) - loss) < 1e-4 * max(abs(loss), 1.0)
    for k in ("lse", "pos_mean", "loss_dv", "loss_infonce"):
        assert abs(sf[k] - sg[k]) < 1e-4 * max(abs(sg[k]), 1.0), k
    assert bool(torch.isfinite(f.record.cpu()).all())


@pytest.mark.parametrize("case", [c for c in ref.CASES if (c[0], c[1]) in (((32, 8, 16, 128), "bf16"), ((128, 32, 96, 128), "bf16"),
                                                                             ((64, 64, 64, 48), "bf16"), ((64, 64, 64, 48), "f32"),
                                                                             ((1, 8, 8, 4), "bf16"), ((1, 8, 8, 4), "f32"))],
                         ids=ref.case_id)
@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_no_negatives(dev, case, est):
    """All ids equal: no negative pair at all -> the same non-finite loss class as the reference gives (logsumexp of
    nothing), as test_flash_no_negatives_and_single_block asserts for the bilinear critic; a batch of one is the same
    case.  The gradients are those of the positive term alone, and finite."""
    shape, prec, _, mode = case
    r_round, r_exact = _reference(shape, "equal", mode), _reference(shape, "equal", "exact")
    assert r_round["n_neg"] == 0
    want = orc.bound_from_matrix(r_exact["scores"], ref.ids(shape[0], "equal"), est)
    assert not math.isfinite(float(want.sum())) and _cls(want.sum()) == _cls(r_round[f"loss_{est}"])
    what = f"no-negatives {ref.case_id(case)} {est}"
    for route in ("step", "two-calls"):
        c = _Call(dev, _inputs(shape), ref.ids(shape[0], "equal"), prec)
        c = c.step(est) if route == "step" else c.fwd(est).bwd(1)
        assert _cls(c.loss.cpu()) == _cls(want.sum()), (what, route, float(c.loss.cpu()))
        _check_loss(f"{what} {route}", prec, est, c.loss.cpu(), c.stats_dict(), r_round, r_exact)
        _check_grads(f"{what} {route}", prec, c.grads(), r_round, r_exact)


@pytest.mark.parametrize("case", ONE_PER_PATH, ids=ref.case_id)
@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_python_route(dev, case, est):
    """mi_critics.fused_mi_bound(SeparableCritic) under autograd, with 0.37 as the incoming gradient."""
    from mutual_info_img_txt import _hip, mi_critics
    from mutual_info_img_txt.model import SeparableCritic
    shape, prec, _, mode = case
    kind = "dup"
    x, y, wg, wh = _inputs(shape)
    sid = ref.ids(shape[0], kind)
    critic = SeparableCritic(shape[1], shape[2], shape[3])
    with torch.no_grad():
        critic.wg.copy_(wg)
        critic.wh.copy_(wh)
    critic.to(dev)
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, stats = mi_critics.fused_mi_bound(xl, yl, sid, critic, est, precision="f32_exact" if prec == "f32" else prec,
                                            return_stats=True)
    assert tuple(loss.shape) == ((1,) if est == "dv" else ())
    (loss.sum() * GO).backward()
    torch.cuda.synchronize()
    r_round, r_exact = _reference(shape, kind, mode), _reference(shape, kind, "exact")
    what = f"python {ref.case_id(case)} {est}"
    _check_loss(what, prec, est, loss.detach().cpu().sum(), _hip.stats_dict(stats), r_round, r_exact)
    got = {"dx": xl.grad, "dy": yl.grad, "dwg": critic.wg.grad, "dwh": critic.wh.grad}
    _check_grads(what, prec, {k: v.cpu().double() for k, v in got.items()}, r_round, r_exact)


@pytest.mark.parametrize("est", ["dv", "infonce"])
def test_graphed_step_eager_off_the_tail(dev, est):
    """GraphedMiStep.step_eager() on a FUSED shape: the one-call step has no tail kernels there and runs the two calls."""
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.graphed import GraphedMiStep
    from mutual_info_img_txt.model import SeparableCritic
    shape, kind = (96, 72, 200, 128), "dup"
    x, y, wg, wh = _inputs(shape)
    sid = ref.ids(shape[0], kind)
    critic = SeparableCritic(shape[1], shape[2], shape[3])
    with torch.no_grad():
        critic.wg.copy_(wg)
        critic.wh.copy_(wh)
    critic.to(dev)
    step = GraphedMiStep(critic, shape[0], shape[1], shape[2], est, "bf16", dev, capture=False)
    assert step.path == _hip.MI_PATH_FUSED
    step.set_inputs(x.to(dev), y.to(dev), sid)
    step.grad_out.fill_(GO)
    for t in (step.grad_x, step.grad_y, *step.grad_params):
        t.fill_(float("nan"))
    loss = step.step_eager().clone()
    torch.cuda.synchronize()
    r_round, r_exact = _reference(shape, kind, "fused16"), _reference(shape, kind, "exact")
    what = f"graphed-eager {est}"
    _check_loss(what, "bf16", est, loss.cpu().sum(), _hip.stats_dict(step.stats), r_round, r_exact)
    got = {"dx": step.grad_x, "dy": step.grad_y, "dwg": step.grad_params[0], "dwh": step.grad_params[1]}
    _check_grads(what, "bf16", {k: v.cpu().double() for k, v in got.items()}, r_round, r_exact)
