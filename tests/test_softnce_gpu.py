"""Soft-target InfoNCE from finding-label bit masks on the MI355X against the fp64 restatement
(tests/softnce_reference.py): loss, both LSEs, the target norms and every gradient, in both modes, for the bilinear,
w == NULL and separable forms and the matrix entry, in every precision, over mask patterns chosen for the ways an
epilogue can go wrong; then the cross-checks on the device (the study-positive entry points on unique ids, on one bit
per study and on equal masks), B = 1, row sums, bit reproducibility with poisoned buffers and on a side stream,
forward-only calls, grad_out, autograd, the concat composition, the rejections, a training run.

Tolerances are those stated at the head of tests/test_posnce_gpu.py for the same precision and path, unchanged (the added
arithmetic is a weighted sum of at most B scores with weights summing to 1): materialised fp32 scores (exact expf): loss /
LSEs 2e-6 * max(1, |S|max), gradients 2e-5 * max|grad|.  bf16 step: against the restatement rounded at the chain's
rounding points, loss / LSEs 2e-3 * max(1, |S|max), gradients 1e-2 * max|grad|.  "f32" (bf16x3) / "f32_exact" / "bf16x3":
against plain fp64, loss rtol 1e-5 atol 3e-5, LSEs 1e-4 * max(1, |S|max), gradients rtol 2e-3 atol 3e-4 * max|grad|.
target_norm: 1e-5 relative in the fp32-grade modes, 2e-3 relative on the bf16 path.
Every comparison prints "softnce-err <what> <error / tolerance>" before it asserts (pytest -s shows the figures).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import math

import numpy as np
import pytest
import torch

import softnce_reference as ref

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "f32_exact", "bf16", "bf16x3"]
# 16-bit chain: multiples of 8 but not of 64 (a partial last tile, two or three tiles per side); generic kernels: ragged,
# a single sample, three samples
CHAIN16 = [(72, 64, 192), (136, 192, 64)]
GENERIC = [(100, 40, 24), (1, 8, 8), (3, 8, 8)]
SHAPES = CHAIN16 + GENERIC
SHAPE_IDS = [f"{b}x{dx}x{dy}" for b, dx, dy in SHAPES]
PATTERNS = ("random14", "high", "empty", "equal", "far", "group5", "study")
TAU_MIX = ((0.5, 0.3), (0.05, 1.0), (2.0, 1.0))


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def softnce_max_labels():
    from mutual_info_img_txt import _hip
    return _hip.MI_SOFTNCE_MAX_LABELS


def _masks(b, kind):
    """int64 [b] label masks of a pattern; None where the pattern does not fit the batch."""
    gen = torch.Generator().manual_seed(1000 + b)
    rnd = torch.randint(0, 1 << 40, (b,), generator=gen, dtype=torch.int64)
    if kind == "random14":        # the CheXpert table: 14 findings
        return rnd & 0x3fff
    if kind == "high":            # sets that differ only in bits 32 ... 62: catches a 32-bit truncation
        n = torch.arange(b, dtype=torch.int64)
        one = torch.ones(b, dtype=torch.int64)
        return (one * 0x5) | (one << (32 + n % 31)) | (one << (32 + (3 * n + 1) % 31)) | (one << 62) * (n % 2)
    if kind == "empty":
        return torch.zeros(b, dtype=torch.int64)
    if kind == "equal":
        return torch.full((b,), 0x2a51, dtype=torch.int64)
    if kind == "far":             # identical sets at (i, i + 70) only: the heavy off-diagonal weights lie outside the
        if b < 71:                # diagonal tiles
            return None
        m = rnd.clone()           # (b > 140: in pairs of 70-blocks, so that each set still has one partner, 70 away)
        n = torch.arange(b)
        second = (n // 70) % 2 == 1
        m[second] = rnd[n[second] - 70]
        return m
    if kind == "group5":          # identical sets at indices 62 .. 66: straddles a tile edge
        if b < 67:
            return None
        m = rnd.clone()
        m[62:67] = m[62]
        return m
    if kind == "study":           # one bit per group of three samples: fits the 63 label bits up to b = 189
        if b > 3 * softnce_max_labels():
            return None
        return torch.ones(b, dtype=torch.int64) << (torch.arange(b, dtype=torch.int64) // 3)
    raise ValueError(kind)


def _patterns(b):
    return [(k, _masks(b, k)) for k in PATTERNS if _masks(b, k) is not None]


def _close(got, want, atol, rtol=0.0, what=""):
    g, w = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    ratio = float(np.max(np.abs(g - w) / np.maximum(atol + rtol * np.abs(w), 1e-300))) if g.size else 0.0
    print(f"softnce-err {what} {ratio:.3f}")
    np.testing.assert_allclose(g, w, rtol=rtol, atol=atol, err_msg=what)


def _inputs(b, dx, dy, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(b, dx, generator=gen)
    y = torch.randn(b, dy, generator=gen)
    w = torch.randn(dx, dy, generator=gen) * (0.3 / math.sqrt(dx))
    return x, y, w


def _bilinear(dev, w):
    from mutual_info_img_txt.model import BilinearCritic
    critic = BilinearCritic(w.shape[0], w.shape[1])
    with torch.no_grad():
        critic.weight.copy_(w)
    return critic.to(dev)


def _separable(dev, wg, wh):
    from mutual_info_img_txt.model import SeparableCritic
    critic = SeparableCritic(wg.shape[0], wh.shape[0], wg.shape[1])
    with torch.no_grad():
        critic.wg.copy_(wg)
        critic.wh.copy_(wh)
    return critic.to(dev)


def _run(dev, x, y, critic, masks, est, precision, names, tau, mix):
    """The public path: loss, statistics and the gradients of x, y and the critic's parameters (named ``names``)."""
    from mutual_info_img_txt import soft_targets as st
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, stats = st.soft_target_infonce(xl, yl, masks, critic, tau=tau, mix=mix, symmetric=est == "infonce_symmetric",
                                         precision=precision, return_stats=True)
    assert loss.shape == () and stats["target_norm"].dtype == torch.float32 and stats["target_norm"].shape == (x.shape[0],)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "dx": xl.grad, "dy": yl.grad, **stats}
    out.update({n: p.grad for n, p in zip(names, critic.parameters())})
    return out


def _run_pos(dev, x, y, critic, sid, est, precision, names):
    """The same through study_positives.study_positive_infonce: the yardstick of the cross-checks."""
    from mutual_info_img_txt import study_positives as sp
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, stats = sp.study_positive_infonce(xl, yl, sid, critic, symmetric=est == "infonce_symmetric", precision=precision,
                                            return_stats=True)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().double(), "dx": xl.grad.double(), "dy": yl.grad.double(),
           "lse_rows": stats["lse_rows"].double(), "lse_cols": stats["lse_cols"].double(),
           "target_norm": stats["n_pos"].double()}
    out.update({n: p.grad.double() for n, p in zip(names, critic.parameters())})
    return out


def _raw(dev, x, y, w, masks, est, precision, tau, mix, grads=True, go=None, poison=False):
    """mi_softnce_bilinear_step through ctypes (w None: S = X Y^T): everything the entry point writes."""
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import OPS, resolve_critic
    b, dx, dy = x.shape[0], x.shape[1], y.shape[1]
    xd, yd = x.to(dev), y.to(dev)
    wd = None if w is None else w.to(dev)
    params = [] if wd is None else [wd]
    lab = masks.to(dev)
    prec = resolve_critic("bilinear", precision, b, dx, dy, params)[2] if params else _hip.PRECISIONS[precision]
    ws = _hip.workspace(OPS["bilinear"].softnce_workspace_bytes(b, dx, dy, params, prec, grads), dev)
    fill = float("nan") if poison else 0.0
    if poison:
        ws.fill_(0xFF)
    new = lambda *s: torch.full(s, fill, device=dev)
    loss, r, c, z = new(1), new(b), new(b), new(b)
    gl = [new(*t.shape) for t in (xd, yd, *params)] if grads else []
    gx, gy, gw = (gl + [None] * 3)[:3]
    p = _hip.ptr
    _hip.call("mi_softnce_bilinear_step", dev, xd.data_ptr(), yd.data_ptr(), p(wd), lab.data_ptr(), b, dx, dy,
              _hip.NCE_ESTIMATORS[est], prec, tau, mix, p(go), loss.data_ptr(), r.data_ptr(), c.data_ptr(), z.data_ptr(),
              p(gx), p(gy), p(gw), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    out = {"loss": loss[0], "lse_rows": r, "lse_cols": c, "target_norm": z, "grads": gl}
    out.update(dict(zip(("dx", "dy", "dw"), gl)))
    return out


def _check(got, o, names, precision, what, fp32_tolerance=False):
    smax = max(1.0, o["smax"])
    if precision == "bf16" and not fp32_tolerance:
        _close(got["target_norm"], o["target_norm"], 0.0, rtol=2e-3, what=f"{what} target_norm")
        _close(got["loss"], o["loss"], 2e-3 * smax, what=f"{what} loss")
        for n in ("lse_rows", "lse_cols"):
            _close(got[n], o[n], 2e-3 * smax, what=f"{what} {n}")
        for n in names:
            _close(got[n], o[n], 1e-2 * float(o[n].abs().max()), what=f"{what} {n}")
    else:
        _close(got["target_norm"], o["target_norm"], 0.0, rtol=2e-3 if precision == "bf16" else 1e-5,
               what=f"{what} target_norm")
        _close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=f"{what} loss")
        for n in ("lse_rows", "lse_cols"):
            _close(got[n], o[n], 1e-4 * smax, what=f"{what} {n}")
        for n in names:
            _close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{what} {n}")


def _cases(b):
    for kind, masks in _patterns(b):
        for tau, mix in TAU_MIX:
            for est in ref.MODES:
                yield kind, masks, tau, mix, est


# ------------------------------------------------------------------------------------------------ the three forms
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bilinear_step_vs_restatement(dev, shape, precision):
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + dx)
    critic = _bilinear(dev, w)
    for kind, masks, tau, mix, est in _cases(b):
        got = _run(dev, x, y, critic, masks, est, precision, ["dw"], tau, mix)
        o = ref.bilinear_case(x, y, w, masks, est, tau, mix, rounded=precision == "bf16")
        _check(got, o, ["dx", "dy", "dw"], precision, f"bilinear {b} {precision} {kind} {tau} {mix} {est}")


@pytest.mark.parametrize("shape", [(72, 64), (136, 192), (100, 40), (1, 8), (3, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_weightless_step_vs_restatement(dev, shape, precision):
    """w == NULL: S = X Y^T, through the C ABI."""
    b, d = shape
    x, y, _ = _inputs(b, d, d, b + d)
    x, y = x * 0.3, y * 0.3
    for kind, masks, tau, mix, est in _cases(b):
        got = _raw(dev, x, y, None, masks, est, precision, tau, mix)
        o = ref.bilinear_case(x, y, None, masks, est, tau, mix, rounded=precision == "bf16")
        _check(got, o, ["dx", "dy"], precision, f"weightless {b} {precision} {kind} {tau} {mix} {est}")


@pytest.mark.parametrize("shape", [(72, 64, 192, 48), (100, 40, 24, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_separable_step_vs_restatement(dev, shape, precision):
    b, dx, dy, kp = shape
    gen = torch.Generator().manual_seed(b + kp)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    wg = torch.randn(dx, kp, generator=gen) * (0.7 / math.sqrt(dx))
    wh = torch.randn(dy, kp, generator=gen) * (0.7 / math.sqrt(dy))
    critic = _separable(dev, wg, wh)
    for kind, masks, tau, mix, est in _cases(b):
        got = _run(dev, x, y, critic, masks, est, precision, ["dwg", "dwh"], tau, mix)
        o = ref.separable_case(x, y, wg, wh, masks, est, tau, mix, rounded=precision == "bf16")
        _check(got, o, ["dx", "dy", "dwg", "dwh"], precision, f"separable {b} {precision} {kind} {tau} {mix} {est}")


# ------------------------------------------------------------------------------------------------ cross-checks
def _ids_of(values):
    return [str(50000000 + int(v)) for v in values]


@pytest.mark.parametrize("critic_kind", ["bilinear", "separable"])
@pytest.mark.parametrize("shape", [(72, 64, 192), (100, 40, 24)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_study_positive_entry_points(dev, critic_kind, shape, precision):
    """On the device, against mi_posnce_*_step of the same build: mix = 0 is its loss on unique ids, one bit per study
    (tau = 0.02, mix = 1) its loss with those ids, equal masks (mix = 1) its loss with all ids equal."""
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, 33)
    gen = torch.Generator().manual_seed(34)
    wg, wh = torch.randn(dx, 16, generator=gen) * (0.7 / math.sqrt(dx)), torch.randn(dy, 16, generator=gen) * (0.7 / math.sqrt(dy))
    critic = _bilinear(dev, w) if critic_kind == "bilinear" else _separable(dev, wg, wh)
    pnames = ["dw"] if critic_kind == "bilinear" else ["dwg", "dwh"]
    study = torch.arange(b) // 3
    trios = ((_masks(b, "random14"), 0.5, 0.0, _ids_of(range(b)), "mix0"),
             (_masks(b, "study"), 0.02, 1.0, _ids_of(study), "study"),
             (_masks(b, "equal"), 0.5, 1.0, _ids_of([0] * b), "equal"))
    for masks, tau, mix, sid, tag in trios:
        for est in ref.MODES:
            got = _run(dev, x, y, critic, masks, est, precision, pnames, tau, mix)
            want = _run_pos(dev, x, y, critic, sid, est, precision, pnames)
            want["smax"] = float((x @ w @ y.t()).abs().max()) if critic_kind == "bilinear" else \
                float(((x @ wg) @ (y @ wh).t()).abs().max())
            if tag == "mix0":            # the targets play no part in the loss, but z is still that of the masks
                want["target_norm"] = ref.targets(masks, tau, mix)[2]
            _check(got, want, ["dx", "dy"] + pnames, precision, f"vs posnce {critic_kind} {b} {precision} {tag} {est}")


@pytest.mark.parametrize("shape", [(72, 64, 64), (100, 36, 20)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_operands(dev, shape, precision):
    """Operands from {-1, 0, 1} (W scaled by a power of two): T and S are exact in every precision, so every precision
    meets the fp32 tolerance in loss, LSEs and target norms (bf16 keeps its own for target_norm: no operand enters it).
    The gradients of bf16 keep the bf16 tolerance: the chain rounds G to bf16 whatever the operands, and where the fp32
    G of the device and the fp64 G of the restatement fall on either side of a rounding boundary, one element of G moves
    by 2^-9 |G_ij|, which is above the fp32 tolerance of a gradient of 64 such terms."""
    b, dx, dy = shape
    gen = torch.Generator().manual_seed(b)
    x = torch.randint(-1, 2, (b, dx), generator=gen).float()
    y = torch.randint(-1, 2, (b, dy), generator=gen).float()
    w = torch.randint(-1, 2, (dx, dy), generator=gen).float() / 16.0
    critic = _bilinear(dev, w)
    for kind, masks in _patterns(b):
        for est in ref.MODES:
            got = _run(dev, x, y, critic, masks, est, precision, ["dw"], 0.5, 0.3)
            o = ref.bilinear_case(x, y, w, masks, est, 0.5, 0.3, rounded=precision == "bf16")
            what = f"exact {b} {precision} {kind} {est}"
            _check(got, o, [] if precision == "bf16" else ["dx", "dy", "dw"], precision, what, fp32_tolerance=True)
            if precision == "bf16":
                for n in ("dx", "dy", "dw"):
                    _close(got[n], o[n], 1e-2 * float(o[n].abs().max()), what=f"{what} {n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_sample_is_exactly_zero(dev, precision):
    from mutual_info_img_txt import soft_targets as st
    x, y, w = _inputs(1, 8, 8, 1)
    gen = torch.Generator().manual_seed(2)
    wg, wh = torch.randn(8, 4, generator=gen), torch.randn(8, 4, generator=gen)
    for lab in (torch.tensor([0x2a51]), torch.tensor([0])):
        for tau, mix in TAU_MIX:
            for est in ref.MODES:
                got = _run(dev, x, y, _bilinear(dev, w), lab, est, precision, ["dw"], tau, mix)
                sep = _run(dev, x, y, _separable(dev, wg, wh), lab, est, precision, ["dwg", "dwh"], tau, mix)
                raw = _raw(dev, x, y, None, lab, est, precision, tau, mix)
                for o, names in ((got, ["dx", "dy", "dw"]), (sep, ["dx", "dy", "dwg", "dwh"]), (raw, ["dx", "dy"])):
                    assert float(o["loss"]) == 0.0 and o["target_norm"].tolist() == [1.0], (est, tau, mix)
                    for n in names:
                        assert torch.equal(o[n], torch.zeros_like(o[n])), (est, n, tau, mix)
                s = torch.full((1, 1), 3.25, device=dev, requires_grad=True)
                loss = st.matrix_soft_target_infonce(s, lab, tau=tau, mix=mix, symmetric=est == "infonce_symmetric")
                loss.backward()
                assert float(loss.detach()) == 0.0 and torch.equal(s.grad, torch.zeros_like(s.grad))


# ------------------------------------------------------------------------------------------------ matrix entry
def _row_sum_floor(b, smax):
    """What the fp32 r_i alone contributes to a row sum of dL/dS, on top of the elementwise 2e-5 * max|grad|.  The
    backward reads r_i as the fp32 number the forward stored, off the exact log-sum-exp by d_i, so in exact arithmetic
    the row sums to (exp(-d_i) - 1) / B = -d_i / B, not to 0.  d_i is held to 2e-6 * max(1, |S|max) by this test's own
    lse_rows figure (and cannot be below half an ulp of r_i, 4.8e-7 at r = 10), while max|grad| falls like 1 / B^2: at
    B = 1000 no fp32 r_i meets 2e-5 * max|grad| alone (measured there: row sum 1.2e-9 = 1.2e-6 / B, 9.7 x that figure).
    The batches up to 130 meet the elementwise figure without this term and keep it as it was."""
    return 2e-6 * smax / b if b > 130 else 0.0


@pytest.mark.parametrize("b", [1, 3, 64, 130, 1000])
@pytest.mark.parametrize("scale", [3.0, 80.0])
def test_matrix_entry_vs_restatement_and_torch(dev, b, scale):
    from mutual_info_img_txt import _hip, critic_ops, soft_targets as st
    gen = torch.Generator().manual_seed(b + int(scale))
    s = (torch.rand(b, b, generator=gen) * 2.0 - 1.0) * scale  # scale 80: scores of +-80
    sd = s.to(dev)
    smax = max(1.0, float(s.abs().max()))
    for kind, masks in _patterns(b):
        lab = masks.to(dev)
        for tau, mix in TAU_MIX:
            qr, qc, _ = (t.to(dev).float() for t in ref.targets(masks, tau, mix))
            for est, mode in _hip.NCE_ESTIMATORS.items():
                what = f"matrix {b} {scale} {kind} {tau} {mix} {est}"
                o = ref.matrix_case(s, masks, est, tau, mix)
                loss, r, c, z = critic_ops.softnce_matrix_fwd(sd, lab, mode, tau, mix)
                g = critic_ops.softnce_matrix_bwd(sd, lab, mode, tau, mix, r, c, z, None)
                torch.cuda.synchronize()
                _close(z, o["target_norm"], 0.0, rtol=1e-5, what=f"{what} target_norm")
                _close(loss[0], o["loss"], 2e-6 * smax, what=f"{what} loss")
                _close(r, o["lse_rows"], 2e-6 * smax, what=f"{what} lse_rows")
                _close(c, o["lse_cols"], 2e-6 * smax, what=f"{what} lse_cols")
                gmax = max(float(o["grad"].abs().max()), 1e-30)
                _close(g, o["grad"], 2e-5 * gmax, what=f"{what} grad")
                if est == "infonce_rowwise":     # each row's share of dL/dS sums to zero
                    rows = g.double().sum(dim=1).abs().max()
                    row_tol = 2e-5 * float(g.abs().max()) + _row_sum_floor(b, smax)
                    print(f"softnce-err {what} row sums {float(rows) / (row_tol + 1e-300):.3f}")
                    assert float(rows) <= row_tol, what
                # the public autograd path against torch's own logsumexp route on the device
                sl = sd.clone().requires_grad_(True)
                l2, stats = st.matrix_soft_target_infonce(sl, masks, tau=tau, mix=mix, symmetric=est == "infonce_symmetric",
                                                          return_stats=True)
                assert l2.shape == () and torch.equal(l2.detach().reshape(1), loss)
                assert torch.equal(stats["target_norm"], z) and torch.equal(stats["lse_rows"], r)
                l2.backward()
                assert torch.equal(sl.grad, g), what
                st_ = sd.clone().requires_grad_(True)
                row = (torch.logsumexp(st_, dim=1) - (qr * st_).sum(dim=1)).mean()
                lt = row if est == "infonce_rowwise" else 0.5 * row + 0.5 * (torch.logsumexp(st_, dim=0) -
                                                                             (qc * st_).sum(dim=0)).mean()
                lt.backward()
                _close(l2, lt, 2e-6 * smax, what=f"{what} loss vs torch")
                _close(sl.grad, st_.grad, 2e-5 * gmax, what=f"{what} grad vs torch")


# ------------------------------------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("shape", CHAIN16[:1] + GENERIC[:1], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_bit_reproducible_poisoned_streams_forward_only_and_grad_out(dev, shape, precision):
    from mutual_info_img_txt import soft_targets as st
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, 11)
    masks, tau, mix = _masks(b, "far"), 0.5, 0.3
    keys = ("loss", "lse_rows", "lse_cols", "target_norm")
    for est in ref.MODES:
        one = _raw(dev, x, y, w, masks, est, precision, tau, mix)
        # a second call, with every output and the whole workspace poisoned (0xFF bytes / NaN) beforehand
        two = _raw(dev, x, y, w, masks, est, precision, tau, mix, poison=True)
        # ... and on a non-default stream
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            three = _raw(dev, x, y, w, masks, est, precision, tau, mix, poison=True)
        for other in (two, three):
            for n in keys:
                assert torch.equal(one[n], other[n]), (est, n)
            for a, c in zip(one["grads"], other["grads"]):
                assert torch.equal(a, c), est
        # forward only (all gradient pointers NULL, the forward-only workspace): the same loss bits
        fwd = _raw(dev, x, y, w, masks, est, precision, tau, mix, grads=False, poison=True)
        assert fwd["grads"] == []
        for n in keys:
            assert torch.equal(one[n], fwd[n]), (est, n, "forward only")
        # grad_out = 2 doubles every gradient exactly
        dbl = _raw(dev, x, y, w, masks, est, precision, tau, mix, go=torch.full((1,), 2.0, device=dev))
        assert torch.equal(dbl["loss"], one["loss"])
        for a, c in zip(one["grads"], dbl["grads"]):
            assert torch.equal(2.0 * a, c), est
        # the public path: the same bits, and no graph where nothing needs a gradient
        critic = _bilinear(dev, w)
        got = _run(dev, x, y, critic, masks, est, precision, ["dw"], tau, mix)
        assert torch.equal(got["loss"], one["loss"])
        for n in ("dx", "dy", "dw"):
            assert torch.equal(got[n], one[n]), (est, n)
        with torch.no_grad():
            l2 = st.soft_target_infonce(x.to(dev), y.to(dev), masks, critic, tau=tau, mix=mix,
                                        symmetric=est == "infonce_symmetric", precision=precision)
        assert l2.grad_fn is None and torch.equal(l2, one["loss"])
        # bit 63 of a mask is ignored on the device
        flagged = _raw(dev, x, y, w, masks | torch.iinfo(torch.int64).min, est, precision, tau, mix)
        for n in keys + ("dx", "dy", "dw"):
            assert torch.equal(one[n], flagged[n]), (est, n, "bit 63")


@pytest.mark.parametrize("kind", ["bilinear", "separable"])
def test_autograd_through_the_public_function(dev, kind):
    """The loss composes with autograd: d(3 L)/d(input) is three times the step's gradient, through a torch op upstream."""
    from mutual_info_img_txt import soft_targets as st
    b, dx, dy = 72, 64, 192
    x, y, w = _inputs(b, dx, dy, 5)
    gen = torch.Generator().manual_seed(5)
    wg, wh = torch.randn(dx, 48, generator=gen) / math.sqrt(dx), torch.randn(dy, 48, generator=gen) / math.sqrt(dy)
    critic = _bilinear(dev, w) if kind == "bilinear" else _separable(dev, wg, wh)
    names = ["dw"] if kind == "bilinear" else ["dwg", "dwh"]
    masks = _masks(b, "group5")
    base = _run(dev, x, y, critic, masks, "infonce_symmetric", "f32", names, 0.5, 0.3)
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    hot = ((masks[:, None] >> torch.arange(40)) & 1).bool()          # the same labels as a multi-hot [B, 40] tensor
    loss = st.soft_target_infonce(xl * 1.0, yl, hot.to(dev), critic, tau=0.5, mix=0.3, precision="f32") * 3.0
    loss.backward()
    assert torch.equal(loss.detach(), base["loss"] * 3.0)
    assert torch.equal(xl.grad, base["dx"] * 3.0) and torch.equal(yl.grad, base["dy"] * 3.0)
    for n, p in zip(names, critic.parameters()):
        assert torch.equal(p.grad, base[n] * 3.0), n


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_concat_composition_is_the_matrix_function_on_the_fused_scores(dev, precision):
    """fused_scores.concat_soft_target_infonce equals matrix_soft_target_infonce applied to fused_critic_scores, bit for
    bit: loss and gradients."""
    from mutual_info_img_txt import fused_scores, soft_targets as st
    from mutual_info_img_txt.model import make_mlp
    from oracle import mi_oracle as orc
    b = 130
    x, y, _, params = orc.synthetic_case(b, 32, 32, h1=64, h2=512, salt=b, dup=True)
    mlp = make_mlp(64, [64, 512])
    with torch.no_grad():
        for p, v in zip(mlp.parameters(), params):
            p.copy_(v)
    mlp = mlp.to(dev)
    masks = _masks(b, "group5")

    def run(fn):
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        for p in mlp.parameters():
            p.grad = None
        loss = fn(xl, yl)
        loss.backward()
        return loss.detach(), [t.grad.clone() for t in (xl, yl, *mlp.parameters())]

    l1, g1 = run(lambda a, c: fused_scores.concat_soft_target_infonce(a, c, masks, mlp, tau=0.5, mix=0.3, symmetric=False,
                                                                      precision=precision))
    l2, g2 = run(lambda a, c: st.matrix_soft_target_infonce(fused_scores.fused_critic_scores(a, c, mlp, precision), masks,
                                                            tau=0.5, mix=0.3, symmetric=False))
    assert l1.shape == () and math.isfinite(float(l1)) and torch.equal(l1, l2)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c) and torch.isfinite(a).all()
    assert float(g1[0].abs().max()) > 0 and float(g1[4].abs().max()) > 0


def test_rejections(dev):
    from mutual_info_img_txt import soft_targets as st
    from mutual_info_img_txt.model import make_mlp
    x, y, w = _inputs(64, 128, 128, 2)
    masks = _masks(64, "random14")
    xd, yd = x.to(dev), y.to(dev)
    kw = dict(tau=0.5, mix=0.3)
    with pytest.raises(ValueError, match="matrix_soft_target_infonce"):
        st.soft_target_infonce(xd[:8, :16], yd[:8, :16], masks[:8], make_mlp(32, [8, 8]).to(dev), **kw)
    critic = _bilinear(dev, w)
    for prec in ("fp8", "f16", "f16x3"):
        with pytest.raises(ValueError, match="precision"):
            st.soft_target_infonce(xd, yd, masks, critic, precision=prec, **kw)
    with pytest.raises(TypeError):
        st.soft_target_infonce(xd, yd, masks, None, **kw)
    with pytest.raises(TypeError):                          # tau and mix are required keywords
        st.soft_target_infonce(xd, yd, masks, critic)
    with pytest.raises(ValueError, match="labels"):
        st.soft_target_infonce(xd, yd, masks[:5], critic, **kw)
    with pytest.raises(ValueError, match="non-negative"):
        st.soft_target_infonce(xd, yd, masks - (1 << 62) - (1 << 62), critic, **kw)
    with pytest.raises(ValueError, match="at most 63"):
        st.soft_target_infonce(xd, yd, torch.zeros(64, 64, dtype=torch.bool), critic, **kw)
    for bad in (dict(tau=0.0, mix=0.3), dict(tau=float("nan"), mix=0.3), dict(tau=0.5, mix=1.5), dict(tau=0.5, mix=-0.1)):
        with pytest.raises(ValueError, match="tau|mix"):
            st.soft_target_infonce(xd, yd, masks, critic, **bad)
        with pytest.raises(ValueError, match="tau|mix"):
            st.matrix_soft_target_infonce(torch.zeros(64, 64, device=dev), masks, **bad)
    with pytest.raises(ValueError, match="B, B"):
        st.matrix_soft_target_infonce(torch.zeros(8, 7, device=dev), masks[:8], **kw)
    with pytest.raises(ValueError, match="labels"):
        st.matrix_soft_target_infonce(torch.zeros(8, 8, device=dev), masks[:7], **kw)
    # the library itself, on device pointers: rejected with nothing launched and nothing written
    from mutual_info_img_txt import _hip, critic_ops
    s = torch.zeros(8, 8, device=dev)
    lab = masks[:8].to(dev)
    for tau, mix in ((0.0, 0.3), (0.5, 2.0)):
        with pytest.raises(ValueError, match="tau|mix"):
            critic_ops.softnce_matrix_fwd(s, lab, _hip.MI_NCE_SYMMETRIC, tau, mix)
    with pytest.raises(ValueError, match="mode"):
        critic_ops.softnce_matrix_fwd(s, lab, 7, 0.5, 0.3)
    z = torch.ones(8, device=dev)
    with pytest.raises(ValueError, match="symmetric"):
        critic_ops.softnce_matrix_bwd(s, lab, _hip.MI_NCE_SYMMETRIC, 0.5, 0.3, z, None, z, None)
    g = torch.full((8, 8), 7.0, device=dev)
    rc = _hip.load().mi_matrix_softnce_bwd(s.data_ptr(), lab.data_ptr(), 8, _hip.MI_NCE_ROWWISE, 0.5, 0.3, z.data_ptr(), None,
                                           None, None, g.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"target_norm" in _hip.load().mi_last_error() and float(g.min()) == 7.0


def test_training_run_through_the_manager(dev):
    """30 Adam steps through MultiModalManager(soft_targets=...) on synthetic data at B = 64: the loss falls and stays
    above the mean entropy of its targets (a cross-entropy never falls below it)."""
    from mutual_info_img_txt.main_utils import MultiModalManager
    b, d, tau, mix = 64, 32, 0.5, 0.3
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(b, d, generator=gen)
    y = x @ (torch.randn(d, d, generator=gen) / math.sqrt(d)) + 0.1 * torch.randn(b, d, generator=gen)
    masks = _masks(b, "random14")
    sid = [f"s{50000000 + n}" for n in range(b)]
    table = {str(50000000 + n): int(m) for n, m in enumerate(masks.tolist())}
    torch.manual_seed(0)
    m = MultiModalManager(d_img=d, d_txt=d, critic="bilinear", mi_estimator="infonce_symmetric", soft_targets=table,
                          soft_tau=tau, soft_mix=mix)
    critic = m.mi_discriminator.to(dev)
    opt = torch.optim.Adam(critic.parameters(), lr=2e-2)
    xd, yd = x.to(dev), y.to(dev)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = m.mi_step(xd, yd, sid, "infonce_symmetric", precision="f32")
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    floor = ref.mean_target_entropy(masks, tau, mix)
    print(f"softnce-err training first {losses[0]:.4f} last {losses[-1]:.4f} floor {floor:.4f}")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert min(losses) > floor > 0.0
    with pytest.raises(KeyError, match="59999999"):
        m.mi_step(xd, yd, sid[:-1] + ["59999999"], "infonce_symmetric")
