"""Every loss family on every kernel of the 16-bit GEMM launcher (DESIGN.md sections 10 - 17; the shape table and what it
reaches: tests/gemm_variant_cases.py).

The families added after the per-sample InfoNCE -- study-positive, soft-target, hard-negative, memory-bank, JSD / NWJ, the
MI estimates, retrieval ranks and top-k -- run their B x B sweep through one launcher that picks one of six kernels from
the shape alone, each a separate instantiation per epilogue with its own tile map, epilogue call form, staging area and
ragged-edge handling.  The family files hold B <= 520, where only one kernel ever runs; here each family runs at the
smallest ragged shape that reaches each other kernel.  Every case asserts its kernel through mi_gemm16_variant before it
launches, so a threshold change fails here and does not quietly lose the coverage.

Two kinds of case, both through the family files' own inputs, references and ``_check`` helpers, WITH THEIR TOLERANCES
UNCHANGED (no figure is stated in this file that is not stated in the family's):
  * statistics on exact data: operands from {-1, 0, 1} scaled by a power of two (gemm_variant_cases.exact_case, which
    asserts on the host that T and S are exact in bf16 and bf16x3).  Loss, LSEs, n_pos / target norm, the 12 estimates
    are held to each family's fp32 figure -- the control row's -- whatever the kernel; ranks, lists and list values are
    compared exactly.  Forward-only calls: the statistics epilogue's instantiation.
  * gradients on Gaussian data (the families with a backward): everything against the family's restatement (rounded at
    the chain's rounding points in bf16, plain fp64 in bf16x3), which runs the gradient epilogue's instantiation with its
    G / G^T stores.  JSD / NWJ has no rounded restatement: its own ``_check_step`` holds bf16 to the unrounded one.
Ids and label masks put their special cases on the kernels' seams (gemm_variant_cases.seam_ids).  Both modes run on every
row.
Every comparison prints "<family>-err <what> <error / tolerance>" before it asserts (pytest -s shows the figures).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math

import numpy as np
import pytest
import torch

import gemm_variant_cases as cases
import hardnce_reference as hardref
import banknce_reference as bankref
import fdiv_reference as fdref
import posnce_reference as posref
import retrieval_reference as rankref
import softnce_reference as softref
import topk_reference as topkref
import test_banknce_gpu as bank
import test_fdiv_gpu as fd
import test_hardnce_gpu as hard
import test_mi_estimates_gpu as est
import test_nce_gpu as nce
import test_posnce_gpu as pos
import test_retrieval_gpu as rank
import test_softnce_gpu as soft
import test_topk_gpu as topk

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("row", cases.NEW_ROWS, ids=[r.name for r in cases.NEW_ROWS])
EXTRA, D_IMG = cases.EXTRA, cases.D_IMG
TAU, MIX = 0.5, 0.3      # the soft targets of test_softnce_gpu's hygiene and exact-operand tests
K_HARD = 5               # as test_hardnce_gpu
K_TOP = 32               # MI_TOPK_MAX_K: the longest lists


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _printing(close, tag):
    """A family's ``_close`` that prints error / tolerance first, for the families whose own does not."""
    def wrapped(got, want, atol, rtol=0.0, what=""):
        g, w = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
        ratio = float(np.max(np.abs(g - w) / np.maximum(atol + rtol * np.abs(w), 1e-300))) if g.size else 0.0
        print(f"{tag}-err {what} {ratio:.3f}")
        return close(got, want, atol, rtol=rtol, what=what)
    return wrapped


@pytest.fixture(autouse=True)
def _print_ratios(monkeypatch):
    for mod, tag in ((hard, "hardnce"), (bank, "banknce"), (fd, "fdiv"), (nce, "nce")):
        monkeypatch.setattr(mod, "_close", _printing(mod._close, tag))


def _exact(row):
    """x, y (the batch's reports), w, the fp64 scores [b, b] and the whole case, after the kernel check."""
    cases.check_row(row)
    c = cases.exact_case(row.name)
    return c["x"], c["y_all"][:row.b].contiguous(), c["w"], c["s_all"][:row.b, :row.b], c


@functools.lru_cache(maxsize=None)
def _gauss_case(name):
    """The family files' Gaussian inputs (their common ``_inputs``) at b + EXTRA samples, the reports scaled so that the
    scores keep the spread they have at d_txt = 64 there (std 0.3 sqrt(64) = 2.4): x, bank_x, y_all, w."""
    row = cases.by_name(name)
    x_all, y_all, w = pos._inputs(row.b + EXTRA, D_IMG, row.d_txt, row.b + row.d_txt)
    y_all = y_all * min(1.0, math.sqrt(64.0 / row.d_txt))
    return x_all[:row.b].contiguous(), x_all[row.b:].contiguous(), y_all, w


def _gauss(row):
    cases.check_row(row)
    x, bank_x, y_all, w = _gauss_case(row.name)
    return x, y_all[:row.b].contiguous(), w, bank_x, y_all


def _sid(row):
    return cases.strings(cases.seam_ids(row.b))


def _masks(row):
    return cases.seam_masks(row.b, soft._masks(row.b, "random14"))


# ------------------------------------------------------------------------------------------------ study positives
@ROWS
def test_posnce_statistics_on_exact_data(dev, row):
    x, y, w, _, _ = _exact(row)
    sid = _sid(row)
    for e in posref.MODES:
        got = pos._raw(dev, x, y, w, sid, e, row.precision, grads=False, poison=True)
        o = posref.bilinear_case(x, y, w, sid, e)
        pos._check(got, o, [], row.precision, f"exact {row.name} {e}", fp32_tolerance=True)


@ROWS
def test_posnce_gradients(dev, row):
    x, y, w, _, _ = _gauss(row)
    sid = _sid(row)
    for e in posref.MODES:
        got = pos._raw(dev, x, y, w, sid, e, row.precision, poison=True)
        o = posref.bilinear_case(x, y, w, sid, e, rounded=row.precision == "bf16")
        pos._check(got, o, ["dx", "dy", "dw"], row.precision, f"gauss {row.name} {e}")


@ROWS
def test_hygiene_once_per_kernel(dev, row):
    """Outputs NaN-poisoned and the workspace filled with 0xFF before each call (as test_separable_gpu.test_hygiene): two
    calls give identical bits for every output, and every output element is finite (so every element was written)."""
    x, y, w, _, _ = _gauss(row)
    sid = _sid(row)
    one = pos._raw(dev, x, y, w, sid, "infonce_symmetric", row.precision, poison=True)
    two = pos._raw(dev, x, y, w, sid, "infonce_symmetric", row.precision, poison=True)
    for n in ("loss", "lse_rows", "lse_cols", "n_pos", "dx", "dy", "dw"):
        assert torch.equal(one[n].reshape(-1).view(torch.uint8), two[n].reshape(-1).view(torch.uint8)), (row.name, n)
        if one[n].dtype.is_floating_point:
            assert bool(torch.isfinite(one[n]).all()), (row.name, n)
    assert int(one["n_pos"].min()) >= 1 and int(one["n_pos"].max()) == 5


# ------------------------------------------------------------------------------------------------ soft targets
@ROWS
def test_softnce_statistics_on_exact_data(dev, row):
    x, y, w, _, _ = _exact(row)
    masks = _masks(row)
    try:
        for e in posref.MODES:
            got = soft._raw(dev, x, y, w, masks, e, row.precision, TAU, MIX, grads=False, poison=True)
            o = softref.bilinear_case(x, y, w, masks, e, TAU, MIX)
            soft._check(got, o, [], row.precision, f"exact {row.name} {e}", fp32_tolerance=True)
    finally:
        softref._TARGETS.clear()     # two [B, B] fp64 target matrices per mask set: not worth keeping at B = 3336


@ROWS
def test_softnce_gradients(dev, row):
    x, y, w, _, _ = _gauss(row)
    masks = _masks(row)
    try:
        for e in posref.MODES:
            got = soft._raw(dev, x, y, w, masks, e, row.precision, TAU, MIX, poison=True)
            o = softref.bilinear_case(x, y, w, masks, e, TAU, MIX, rounded=row.precision == "bf16")
            soft._check(got, o, ["dx", "dy", "dw"], row.precision, f"gauss {row.name} {e}")
    finally:
        softref._TARGETS.clear()


# ------------------------------------------------------------------------------------------------ hard negatives
@ROWS
def test_hardnce_statistics_on_exact_data(dev, row):
    """The lists are the fp64 selection with all its ties (the restatement's OWN lists, as
    test_hardnce_gpu.test_tie_order_on_exact_operands); loss and LSEs at that file's fp32 figures."""
    x, y, w, _, _ = _exact(row)
    sid = _sid(row)
    for e in posref.MODES:
        got = hard._ops_step(dev, "bilinear", x, y, [w], sid, e, row.precision, K_HARD, need_grad=False)
        o = hardref.bilinear_case(x, y, w, sid, K_HARD, e)
        assert torch.equal(got["idx_rows"].cpu().long(), o["idx_rows"]), (row.name, e)
        if e == "infonce_symmetric":
            assert torch.equal(got["idx_cols"].cpu().long(), o["idx_cols"]), (row.name, e)
        else:
            o.pop("lse_cols")
        hard._check(got, o, [], "f32", f"exact {row.name} {e}")      # "f32": the fp32 figures, whatever the row's precision


@ROWS
def test_hardnce_gradients(dev, row):
    """With the kernel's own lists, as test_hardnce_gpu.test_bilinear_step_vs_restatement."""
    x, y, w, _, _ = _gauss(row)
    sid = _sid(row)
    for e in posref.MODES:
        got = hard._ops_step(dev, "bilinear", x, y, [w], sid, e, row.precision, K_HARD)
        got["dx"], got["dy"], got["dw"] = got["grads"]
        o = hardref.bilinear_case(x, y, w, sid, K_HARD, e, (got["idx_rows"], got["idx_cols"]),
                                  rounded=row.precision == "bf16")
        if e == "infonce_rowwise":
            o.pop("lse_cols")
        hard._check(got, o, ["dx", "dy", "dw"], row.precision, f"gauss {row.name} {e}")


# ------------------------------------------------------------------------------------------------ memory bank
def _bank_ids(row):
    return _sid(row), cases.strings(cases.extra_ids(row.b))


@ROWS
def test_banknce_statistics_on_exact_data(dev, row):
    x, y, w, _, c = _exact(row)
    sid, bsid = _bank_ids(row)
    bx, by = c["bank_x"], c["y_all"][row.b:].contiguous()
    for e in posref.MODES:
        got = bank._step(dev, "bilinear", x, y, [w], sid, bx, by, bsid, e, row.precision, grads=False)
        o = bankref.case(x, y, [w], sid, bx, by, bsid, e)
        bank._check(got, o, False, f"exact {row.name} {e}", grads=False)


@ROWS
def test_banknce_gradients(dev, row):
    x, y, w, bx, y_all = _gauss(row)
    sid, bsid = _bank_ids(row)
    by = y_all[row.b:].contiguous()
    for e in posref.MODES:
        got = bank._step(dev, "bilinear", x, y, [w], sid, bx, by, bsid, e, row.precision)
        o = bankref.case(x, y, [w], sid, bx, by, bsid, e, rounded=row.precision == "bf16")
        bank._check(got, o, row.precision == "bf16", f"gauss {row.name} {e}")


# ------------------------------------------------------------------------------------------------ JSD / NWJ
@ROWS
def test_fdiv_statistics_on_exact_data(dev, row):
    from mutual_info_img_txt import mi_critics
    x, y, w, s, _ = _exact(row)
    sid = _sid(row)
    critic = fd._bilinear(dev, w)
    for mode in fdref.MODES:
        with torch.no_grad():
            loss = mi_critics.fused_mi_bound(x.to(dev), y.to(dev), sid, critic, mode, precision=row.precision)
        torch.cuda.synchronize()
        want, _ = fdref.matrix_loss(s, sid, mode)
        o = {"loss": want, "smax": float(s.abs().max()), "grads": {}}
        fd._check_step({"loss": loss}, o, "f32", mode, f"exact {row.name} {mode}")   # "f32": the fp32 figures


@ROWS
def test_fdiv_gradients(dev, row):
    """As test_fdiv_gpu.test_bilinear_vs_restatement: the fp64 restatement runs on the device."""
    x, y, w, _, _ = _gauss(row)
    sid = _sid(row)
    critic = fd._bilinear(dev, w)
    for mode in fdref.MODES:
        got = fd._run(dev, x, y, critic, sid, mode, row.precision)
        xd, yd, wd = (t.double().to(dev).requires_grad_(True) for t in (x, y, w))
        s = (xd @ wd) @ yd.t()
        loss, _ = fdref.matrix_loss(s, sid, mode)
        loss.backward()
        o = {"loss": loss.detach(), "smax": float(s.detach().abs().max()),
             "grads": {"dx": xd.grad, "dy": yd.grad, "dp0": wd.grad}}
        if row.precision == "bf16":
            for k, r in o["grads"].items():
                fro, worst = fd._errs(got[k], r)
                print(f"fdiv-err gauss {row.name} {mode} {k} frobenius {fro / 2e-2:.3f} worst {worst / 0.15:.3f}")
        fd._check_step(got, o, row.precision, mode, f"gauss {row.name} {mode}")
        del s, loss, xd, yd, wd, o


# ------------------------------------------------------------------------------------------------ estimates, ranks
def _ops():
    from mutual_info_img_txt.critic_ops import HipBilinearOps
    return HipBilinearOps()


@ROWS
def test_estimates_on_exact_data(row):
    from mutual_info_img_txt import _hip
    x, y, w, s, _ = _exact(row)
    sid = cases.seam_ids(row.b)
    prec = _hip.PRECISIONS[row.precision]
    xd, yd, pd, sidd = x.to(est.DEV), y.to(est.DEV), [w.to(est.DEV)], sid.to(est.DEV)
    got = est._chain_call(_ops(), xd, yd, pd, sidd, prec, est.TAUS)
    est._check(est._host(got), s, sid, est.TAUS, f"estimates-err {row.name}")
    assert not torch.isnan(got).any()
    assert torch.equal(est._bits(est._chain_call(_ops(), xd, yd, pd, sidd, prec, est.TAUS)), est._bits(got))


@ROWS
def test_ranks_on_exact_data(row):
    from mutual_info_img_txt import _hip
    x, y, w, s, _ = _exact(row)
    sid = cases.seam_ids(row.b)
    want_i2t, want_t2i = rankref.ranks(s, sid)
    assert int(((s == torch.diagonal(s)[:, None]).sum(1) - 1).sum()) > 0      # ties off the diagonal do occur
    ri, rt, diag = rank._run_ops(_ops(), x.to(rank.DEV), y.to(rank.DEV), [w.to(rank.DEV)], sid.to(rank.DEV),
                                 _hip.PRECISIONS[row.precision])
    assert torch.equal(diag.cpu().double(), torch.diagonal(s)), float((diag.cpu().double() - torch.diagonal(s)).abs().max())
    assert torch.equal(ri.cpu().long(), want_i2t), int((ri.cpu().long() - want_i2t).abs().max())
    assert torch.equal(rt.cpu().long(), want_t2i), int((rt.cpu().long() - want_t2i).abs().max())


# ------------------------------------------------------------------------------------------------ top-k over a gallery
@ROWS
def test_topk_on_exact_data(row):
    """b images against a gallery of b + EXTRA reports: b x (b + EXTRA) one way, (b + EXTRA) x b the other, both on the
    row's kernel.  Indices and values exactly, ties included."""
    from mutual_info_img_txt import _hip
    x, _, w, _, c = _exact(row)
    y_all, s = c["y_all"], c["s_all"][:row.b]
    img_ids = cases.seam_ids(row.b)
    txt_ids = torch.cat([img_ids, cases.extra_ids(row.b)])
    want = topkref.both_directions(s, K_TOP, img_ids, txt_ids)
    got = topk._run_ops(_ops(), x.to(topk.DEV), y_all.to(topk.DEV), [w.to(topk.DEV)], img_ids.to(topk.DEV),
                        txt_ids.to(topk.DEV), _hip.PRECISIONS[row.precision], K_TOP)
    topk._assert_same(got[0], want["i2t"], (row.name, "i2t"))
    topk._assert_same(got[1], want["t2i"], (row.name, "t2i"))


# ------------------------------------------------------------------------------------------------ per-sample InfoNCE
def test_nce_step_on_the_256x128_kernel(dev):
    """mi_nce_bilinear_step reaches every other kernel through test_nce_gpu.SHAPES; this is the one it does not.  The
    figures are those of test_nce_gpu.test_bilinear_step_vs_restatement for the fp32-grade precisions."""
    row = cases.by_name("pipe256x128")
    x, y, w, _, _ = _gauss(row)
    sid = _sid(row)
    e = "infonce_symmetric"
    got = nce._run_bilinear(dev, x, y, w, sid, e, row.precision)
    o = nce._plain_oracle(x, y, w, sid, e)
    what = f"{row.name} {e}"
    nce._close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=f"{what} loss")
    nce._close(got["lse_rows"], o["lse_rows"], 1e-4 * max(1.0, o["smax"]), what=f"{what} lse_rows")
    nce._close(got["lse_cols"], o["lse_cols"], 1e-4 * max(1.0, o["smax"]), what=f"{what} lse_cols")
    for n in ("dx", "dy", "dw"):
        nce._close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{what} {n}")
