"""The make_mlp critic as a differentiable score matrix on the MI355X (mutual_info_img_txt/fused_scores.py,
mi_concat_mlp_scores_fwd / mi_concat_mlp_bwd_from_g).

Reference of every gradient: fp64 autograd through ``orc.concat_scores_matrix`` as ``(S * G).sum().backward()``, run on the
device.  Shapes: the edge shapes of the concat kernels (``CONCAT_CASES`` of tests/test_gpu_parity.py: partial row and column
tiles, both h2, d_img != d_txt) and one rectangular case, 64 images x 130 reports.  Tolerances:
  * fp32-grade modes ("f32" = the two-part fp16 scheme, "f32_exact"): the DV backward test's rtol 2e-3, atol 3e-4 * max|grad|;
    db3 = sum(G): atol 5e-6 * sum|G| with a floor of 1e-5 (the DV test's 1e-5 for sum|g| = 2);
  * against the existing backward on the same workspace (G = the bound's own dL/dS): one tenth of the tolerance against the
    oracle -- 3e-5 * max|grad| in the fp32-grade modes, one tenth of the DV step's own error against fp64 in bf16 / f16; db3
    (a sum of g that nearly cancels, scale sum|g| <= 2): 1e-6, one tenth of the DV test's 1e-5;
  * bf16 / f16 against fp64: within 4 x the DV step's errors on the same inputs, floors 2e-2 (Frobenius) and 0.1 (worst
    element), the yardstick of tests/test_fdiv_gpu.py.
Every test prints the figures it asserts on.  All tests need an MI355X:  python -m pytest tests -m gpu"""
import math

import numpy as np
import pytest
import torch

import fdiv_reference as fref
import nce_reference as nref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu

# (b, d_img, d_txt, h1, h2, duplicated ids) -- tests/test_gpu_parity.py
CONCAT_CASES = [(40, 24, 40, 64, 256, True), (96, 128, 128, 1024, 512, False), (33, 16, 8, 128, 256, True),
                (130, 32, 32, 64, 512, True)]
RECT = ("rect", 64, 130, 24, 40, 64, 256)  # n_img, n_txt, d_img, d_txt, h1, h2
GRAD_NAMES = ["dx", "dy", "dw1", "db1", "dw2", "db2", "dw3", "db3"]
F32_MODES = ["f32_exact", "f32"]
ALL_MODES = ["f32", "f32_exact", "bf16", "f16"]


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _inputs(case):
    """(x [n_img, d_img], y [n_txt, d_txt], study ids of the reports, params) of a square or the rectangular case."""
    if case[0] == "rect":
        _, n_img, b, dx, dy, h1, h2 = case
        x, y, sid, params = orc.synthetic_case(b, dx, dy, h1=h1, h2=h2, salt=7, dup=True)
        return x[:n_img].contiguous(), y, sid, params
    b, dx, dy, h1, h2, dup = case
    return orc.synthetic_case(b, dx, dy, h1=h1, h2=h2, salt=b, dup=dup)


def _mlp(dev, params):
    from mutual_info_img_txt.model import make_mlp
    mlp = make_mlp(params[0].shape[1], [params[0].shape[0], params[2].shape[0]])
    with torch.no_grad():
        for p, v in zip(mlp.parameters(), params):
            p.copy_(v)
    return mlp.to(dev)


def _general_g(n_img, b, salt):
    """dL/dS of no loss in particular: mixed signs, row magnitudes 2^0 ... 2^-12, about a quarter exact zeros, one all-zero
    row and one all-zero column."""
    g = orc.hash_uniform((n_img, b), 1000 + salt) * 2.0
    g = g * (2.0 ** -(torch.arange(n_img) % 13).float())[:, None]
    g = g * (orc.hash_uniform((n_img, b), 2000 + salt) >= -0.25).float()
    g[n_img // 2] = 0.0
    g[:, b // 3] = 0.0
    return g


def _vjp64(dev, x, y, params, g, block=128):
    """fp64 gradients of sum(S * g) in the order of GRAD_NAMES (row-blocked autograd on the device)."""
    xl, yl = x.to(dev).double().requires_grad_(True), y.to(dev).double().requires_grad_(True)
    pl = [p.to(dev).double().requires_grad_(True) for p in params]
    g = g.to(dev).double()
    for i0 in range(0, x.shape[0], block):
        sb = orc.concat_scores_matrix(xl[i0:i0 + block], yl, pl)
        (sb * g[i0:i0 + block]).sum().backward()
    return [t.grad.cpu() for t in (xl, yl, *pl)]


def _vjp(dev, x, y, mlp, g, precision):
    """(scores, gradients) of sum(S * g) from the fused kernels."""
    from mutual_info_img_txt import fused_scores
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    for p in mlp.parameters():
        p.grad = None
    s = fused_scores.fused_critic_scores(xl, yl, mlp, precision=precision)
    s.backward(g.to(dev))
    torch.cuda.synchronize()
    return s.detach(), [t.grad.cpu() for t in (xl, yl, *mlp.parameters())]


def _check_f32(grads, refs, g, what, atol_grad=3e-4):
    """The fp32-grade tolerances of the module docstring; ``g`` is the dL/dS the gradients belong to."""
    db3_atol = max(5e-6 * float(g.double().abs().sum()), 1e-5)
    for name, got, ref in zip(GRAD_NAMES, grads, refs):
        got, ref = got.double().cpu(), ref.double().cpu().reshape(got.shape)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"{what} {name}: max|d| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}")
        atol = db3_atol if name == "db3" else atol_grad * scale
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-3, atol=atol, err_msg=f"{what} {name}")


_REF_CACHE = {}


def _cached(key, fn):
    if key not in _REF_CACHE:
        _REF_CACHE[key] = fn()
    return _REF_CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("precision", ALL_MODES)
@pytest.mark.parametrize("case", CONCAT_CASES, ids=lambda c: f"b{c[0]}")
def test_forward_bits_equal_the_dv_forward(dev, case, precision):
    from mutual_info_img_txt import fused_scores, mi_critics
    x, y, sid, params = _inputs(case)
    mlp = _mlp(dev, params)
    with torch.no_grad():
        _, want = mi_critics.fused_mi_bound(x.to(dev), y.to(dev), sid, mlp, "dv", precision=precision, return_scores=True)
        plain = fused_scores.fused_critic_scores(x.to(dev), y.to(dev), mlp, precision=precision)
    assert not plain.requires_grad and plain.grad_fn is None
    tracked = fused_scores.fused_critic_scores(x.to(dev).requires_grad_(True), y.to(dev), mlp, precision=precision)
    assert tracked.requires_grad
    assert plain.shape == (case[0], case[0]) and plain.dtype == torch.float32
    assert torch.equal(plain, want)
    assert torch.equal(tracked.detach(), want)


@pytest.mark.parametrize("precision", ALL_MODES)
def test_forward_rectangular(dev, precision):
    """64 images x 130 reports: no_grad and grad-enabled bits agree; the values against fp64."""
    from mutual_info_img_txt import fused_scores
    x, y, _, params = _inputs(RECT)
    mlp = _mlp(dev, params)
    with torch.no_grad():
        plain = fused_scores.fused_critic_scores(x.to(dev), y.to(dev), mlp, precision=precision)
    tracked = fused_scores.fused_critic_scores(x.to(dev), y.to(dev).requires_grad_(True), mlp, precision=precision)
    assert plain.shape == (64, 130) and torch.equal(plain, tracked.detach())
    s64 = orc.concat_scores_matrix(x.double(), y.double(), [p.double() for p in params])
    sc = max(float(s64.abs().max()), 1.0)
    # the forward tests' figures: 2e-5 (fp32-grade), 3e-2 (bf16, unrounded oracle), 4e-3 (f16)
    tol = {"f32": 2e-5, "f32_exact": 2e-5, "bf16": 3e-2, "f16": 4e-3}[precision]
    np.testing.assert_allclose(plain.cpu().numpy(), s64.numpy(), rtol=0, atol=tol * sc)


# ------------------------------------------------------------------------------------------------ 2. VJP, general G
@pytest.mark.parametrize("precision", F32_MODES)
@pytest.mark.parametrize("case", CONCAT_CASES + [RECT], ids=lambda c: "rect" if c[0] == "rect" else f"b{c[0]}")
def test_vjp_general_g_vs_fp64(dev, case, precision):
    x, y, _, params = _inputs(case)
    g = _general_g(x.shape[0], y.shape[0], y.shape[0])
    assert float(g[x.shape[0] // 2].abs().max()) == 0.0 and float(g[:, y.shape[0] // 3].abs().max()) == 0.0
    assert 0.2 < float((g == 0).float().mean()) < 0.35 and float(g.min()) < 0 < float(g.max())
    refs = _cached(("general", case), lambda: _vjp64(dev, x, y, params, g))
    _, grads = _vjp(dev, x, y, _mlp(dev, params), g, precision)
    _check_f32(grads, refs, g, f"general G {precision}")


# ------------------------------------------------------------------------------------------------ 3. existing backward
def _ops_inputs(dev, case, precision):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.critic_ops import resolve_critic
    x, y, sid, params = _inputs(case)
    mlp = _mlp(dev, params)
    prec = resolve_critic(mlp, precision, x.shape[0], x.shape[1], y.shape[1])[2]
    p_dev = [p.detach() for p in mlp.parameters()]
    return x.to(dev), y.to(dev), mi_critics.study_id_codes(sid, dev), p_dev, prec, (x, y, sid, params)


@pytest.mark.parametrize("precision", ALL_MODES)
@pytest.mark.parametrize("case", [CONCAT_CASES[3], CONCAT_CASES[1]], ids=["b130", "b96"])
def test_agrees_with_the_existing_backward(dev, case, precision):
    """G = the DV / JSD bound's own dL/dS (mi_matrix_bound_bwd, mi_fdiv_matrix_bwd on the op's scores); bwd_from_g on the
    workspace of that forward against mi_concat_mlp_bwd / mi_fdiv_concat_mlp_bwd."""
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import HipConcatMlpOps, fwd_outputs
    xd, yd, sidc, p_dev, prec, (x, y, sid, params) = _ops_inputs(dev, case, precision)
    b = x.shape[0]
    ops = HipConcatMlpOps()
    go = torch.ones(1, dtype=torch.float32, device=dev)

    out = fwd_outputs(dev, torch.empty(b, b, dtype=torch.float32, device=dev))
    _, saved = ops.forward(xd, yd, p_dev, sidc, sidc, 0, _hip.MI_DV, prec, True, out=out)
    stats, scores, ws = out[1], out[3], saved[8]
    gx, gy, gp = ops.backward(saved, stats, go)
    dv_old = [gx, gy, *gp]
    g_dv = torch.empty_like(scores)
    _hip.call("mi_matrix_bound_bwd", dev, scores.data_ptr(), sidc.data_ptr(), b, stats.data_ptr(), go.data_ptr(),
              g_dv.data_ptr())
    gx, gy, gp = ops.scores_backward((xd, yd, p_dev, prec, ws), g_dv)
    dv_new = [gx, gy, *gp]

    _, _, fsaved = ops.fdiv_forward(xd, yd, p_dev, sidc, sidc, 0, _hip.MI_FDIV_JSD, prec, True)
    fscores, fstats, fws = fsaved[8:]
    gx, gy, gp = ops.fdiv_backward(fsaved, go)
    jsd_old = [gx, gy, *gp]
    g_jsd = torch.empty_like(fscores)
    _hip.call("mi_fdiv_matrix_bwd", dev, fscores.data_ptr(), sidc.data_ptr(), b, _hip.MI_FDIV_JSD, fstats.data_ptr(),
              go.data_ptr(), g_jsd.data_ptr())
    gx, gy, gp = ops.scores_backward((xd, yd, p_dev, prec, fws), g_jsd)
    jsd_new = [gx, gy, *gp]
    torch.cuda.synchronize()

    if precision in ("bf16", "f16"):  # the DV step's own error against fp64, per gradient, over max|grad|
        o = _cached(("dv64", case), lambda: fref.concat_case(xd, yd, p_dev, sid, "dv"))
        refs = [o["dx"], o["dy"], *o["dparams"]]
        bound = [0.1 * float((a.double() - r.reshape(a.shape)).abs().max()) / max(float(r.abs().max()), 1e-300)
                 for a, r in zip(dv_old, refs)]
    else:
        bound = [3e-5] * 8
    for rule, old, new in (("dv", dv_old, dv_new), ("jsd", jsd_old, jsd_new)):
        for name, a, c, bd in zip(GRAD_NAMES, old, new, bound):
            assert torch.isfinite(c).all()
            dev_abs = float((a.double() - c.double()).abs().max())
            scale = float(a.abs().max())
            if name == "db3":
                print(f"{rule} {precision} db3: |d| = {dev_abs:.3e} (bound 1e-6)")
                assert dev_abs <= 1e-6, (rule, name, dev_abs)
                continue
            print(f"{rule} {precision} {name}: max|d| / max|grad| = {dev_abs / scale:.3e} (bound {bd:.3e})")
            assert dev_abs <= bd * scale, (rule, name, dev_abs / scale, bd)


# ------------------------------------------------------------------------------------------------ 4. scale handling
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_scale_handling(dev, precision):
    case = CONCAT_CASES[3]
    x, y, _, params = _inputs(case)
    mlp = _mlp(dev, params)
    g = _general_g(x.shape[0], y.shape[0], 5)
    _, base = _vjp(dev, x, y, mlp, g, precision)
    _, again = _vjp(dev, x, y, mlp, g, precision)
    for name, a, c in zip(GRAD_NAMES, base, again):
        assert torch.equal(a, c), f"two calls differ in {name}"
    for k in (-20, 10):
        _, scaled = _vjp(dev, x, y, mlp, g * 2.0 ** k, precision)
        for name, a, c in zip(GRAD_NAMES, base, scaled):
            want = a.double() * 2.0 ** k
            rel = float(((c.double() - want).abs() / want.abs().clamp_min(1e-300)).max())
            print(f"{precision} k = {k} {name}: worst relative deviation {rel:.3e}")
            np.testing.assert_allclose(c.double().numpy(), want.numpy(), rtol=1e-6, atol=0, err_msg=f"k={k} {name}")
    _, zero = _vjp(dev, x, y, mlp, torch.zeros_like(g), precision)
    for name, c in zip(GRAD_NAMES, zero):
        assert torch.isfinite(c).all() and float(c.abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------------ 5. 16-bit modes
def _errs(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu().reshape(got.shape)
    return (float((got - want).norm()) / max(float(want.norm()), 1e-30),
            float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30))


def _loose(got, want, yard, what):
    """tests/test_fdiv_gpu.py::_loose: errors within max(floor, 4 x the DV step's errors ``yard`` on the same inputs)."""
    fro, worst = _errs(got, want)
    print(what, f"frobenius {fro:.2e} worst {worst:.2e} (DV: {yard[0]:.2e}, {yard[1]:.2e})")
    assert fro <= max(2e-2, 4 * yard[0]), (what, "frobenius", fro, yard)
    assert worst <= max(0.1, 4 * yard[1]), (what, "worst element", worst, yard)


def _ids(b):
    sid = list(range(b))
    for n in range(b // 8):
        sid[n] = n - (n % 2)
    return [str(50000000 + s) for s in sid]


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("b", [128, 512])
def test_16bit_modes_vs_fp64(dev, b, precision):
    from mutual_info_img_txt import mi_critics
    d = 768
    x, y, _, params = orc.synthetic_case(b, d, d, h1=1024, h2=512, salt=b // 8)
    sid = _ids(b)
    mlp = _mlp(dev, params)
    p_dev = [p.to(dev) for p in params]

    def fp64_side():
        o = fref.concat_case(x.to(dev), y.to(dev), p_dev, sid, "dv")
        g = nref.nce_grad_scores(o["scores"].cpu(), sid, "infonce_symmetric").float()
        return [o["dx"].cpu(), o["dy"].cpu()] + [q.cpu() for q in o["dparams"]], g, _vjp64(dev, x, y, params, g)

    dv_refs, g, refs = _cached(("16bit", b), fp64_side)
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    for p in mlp.parameters():
        p.grad = None
    mi_critics.fused_mi_bound(xl, yl, sid, mlp, "dv", precision=precision).sum().backward()
    yard = [_errs(t.grad, r) for t, r in zip((xl, yl, *mlp.parameters()), dv_refs)]
    _, grads = _vjp(dev, x, y, mlp, g, precision)
    for name, got, ref, yd in zip(GRAD_NAMES, grads, refs, yard):
        if name == "db3":  # the fp32 sum of the given G (true value 0): the bound of the fp32-grade modes
            atol = max(5e-6 * float(g.double().abs().sum()), 1e-5)
            print(f"{precision} B = {b} db3: {float(got):.3e} against {float(ref):.3e} (atol {atol:.1e})")
            assert abs(float(got) - float(ref)) <= atol
            continue
        _loose(got, ref, yd, f"{precision} B = {b} {name}")


# ------------------------------------------------------------------------------------------------ 6. the losses
def _sid(b, ids):
    if ids == "unique":
        return [str(50000000 + n) for n in range(b)]
    return orc.synthetic_case(b, 1, 1, h1=1, h2=1, dup=True)[2]


@pytest.mark.parametrize("precision", F32_MODES)
@pytest.mark.parametrize("estimator", nref.MODES)
@pytest.mark.parametrize("ids", ["unique", "dup"])
@pytest.mark.parametrize("case", [CONCAT_CASES[0], CONCAT_CASES[3]], ids=["b40", "b130"])
def test_concat_infonce_vs_restatement(dev, case, ids, estimator, precision):
    from mutual_info_img_txt import fused_scores
    x, y, _, params = _inputs(case)
    sid = _sid(x.shape[0], ids)

    def fp64_side():
        s64 = orc.concat_scores_matrix(x.double(), y.double(), [p.double() for p in params])
        g64 = nref.nce_grad_scores(s64, sid, estimator)
        return nref.nce_loss(s64, sid, estimator), g64, _vjp64(dev, x, y, params, g64)

    loss64, g64, refs = _cached(("nce", case, ids, estimator), fp64_side)
    mlp = _mlp(dev, params)
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss = fused_scores.concat_infonce(xl, yl, sid, mlp, estimator, precision=precision)
    assert loss.shape == ()
    loss.backward()
    got = float(loss.detach())
    print(f"{estimator} {ids} {precision}: loss {got:.7f} against {float(loss64):.7f}")
    assert abs(got - float(loss64)) <= 3e-5 + 1e-5 * abs(float(loss64))
    _check_f32([t.grad for t in (xl, yl, *mlp.parameters())], refs, g64, f"{estimator} {ids} {precision}")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_hard_negative_and_study_positive_are_compositions(dev, precision):
    """The two conveniences equal their matrix function applied to fused_critic_scores, bit for bit: loss and gradients."""
    from mutual_info_img_txt import fused_scores
    from mutual_info_img_txt.hard_negatives import matrix_hard_negative_infonce
    from mutual_info_img_txt.study_positives import matrix_study_positive_infonce
    x, y, sid, params = _inputs(CONCAT_CASES[3])
    mlp = _mlp(dev, params)

    def run(fn):
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        for p in mlp.parameters():
            p.grad = None
        loss = fn(xl, yl)
        loss.backward()
        return loss.detach(), [t.grad.clone() for t in (xl, yl, *mlp.parameters())]

    pairs = [
        (lambda a, c: fused_scores.concat_hard_negative_infonce(a, c, sid, mlp, 5, precision=precision),
         lambda a, c: matrix_hard_negative_infonce(fused_scores.fused_critic_scores(a, c, mlp, precision), sid, 5)),
        (lambda a, c: fused_scores.concat_study_positive_infonce(a, c, sid, mlp, symmetric=False, precision=precision),
         lambda a, c: matrix_study_positive_infonce(fused_scores.fused_critic_scores(a, c, mlp, precision), sid,
                                                    symmetric=False)),
    ]
    for short, spelled in pairs:
        (l1, g1), (l2, g2) = run(short), run(spelled)
        assert l1.shape == () and math.isfinite(float(l1)) and torch.equal(l1, l2)
        for name, a, c in zip(GRAD_NAMES, g1, g2):
            assert torch.equal(a, c), name
            assert torch.isfinite(a).all()
        assert float(g1[0].abs().max()) > 0 and float(g1[4].abs().max()) > 0


def test_adam_loop_on_symmetric_infonce(dev):
    from mutual_info_img_txt import fused_scores
    from mutual_info_img_txt.model import make_mlp
    b, d = 64, 32
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(b, d, generator=gen)
    y = (x + 0.5 * torch.randn(b, d, generator=gen)).to(dev)
    x = x.to(dev)
    torch.manual_seed(6)
    mlp = make_mlp(2 * d, [64, 256]).to(dev)
    opt = torch.optim.Adam(mlp.parameters(), lr=1e-3)
    sid = _sid(b, "dup")
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = fused_scores.concat_infonce(x, y, sid, mlp, "infonce_symmetric")
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("symmetric InfoNCE over 30 Adam steps:", losses[0], "->", losses[-1])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_backward_twice_and_torch_loss(dev):
    """retain_graph: the workspace lives in ctx; a loss written in plain torch trains the critic."""
    from mutual_info_img_txt import fused_scores
    x, y, _, params = _inputs(CONCAT_CASES[0])
    mlp = _mlp(dev, params)
    xl = x.to(dev).requires_grad_(True)
    s = fused_scores.fused_critic_scores(xl, y.to(dev), mlp)
    loss = torch.nn.functional.cross_entropy(s, torch.arange(s.shape[0], device=dev))
    loss.backward(retain_graph=True)
    first = [xl.grad.clone()] + [p.grad.clone() for p in mlp.parameters()]
    xl.grad = None
    for p in mlp.parameters():
        p.grad = None
    loss.backward()
    for a, c in zip(first, [xl.grad] + [p.grad for p in mlp.parameters()]):
        assert torch.equal(a, c)
    s64 = orc.concat_scores_matrix(x.double(), y.double(), [p.double() for p in params])
    g64 = torch.autograd.functional.jacobian(
        lambda t: torch.nn.functional.cross_entropy(t, torch.arange(t.shape[0])), s64)
    refs = _vjp64(dev, x, y, params, g64)
    _check_f32(first[:1], refs[:1], g64, "cross-entropy in torch")


# ------------------------------------------------------------------------------------------------ 7. row blocks
@pytest.mark.parametrize("precision", F32_MODES)
def test_row_blocks_through_the_ops_object(dev, precision):
    from mutual_info_img_txt.critic_ops import HipConcatMlpOps
    xd, yd, _, p_dev, prec, (x, y, _, _) = _ops_inputs(dev, CONCAT_CASES[3], precision)
    g = _general_g(130, 130, 9).to(dev)
    ops = HipConcatMlpOps()
    s_all, saved = ops.scores_forward(xd, yd, p_dev, prec, True)
    gx, gy, gp = ops.scores_backward(saved, g)
    whole = [gx, gy, *gp]
    parts = []
    for lo, hi in ((0, 64), (64, 130)):
        s_blk, saved = ops.scores_forward(xd[lo:hi].contiguous(), yd, p_dev, prec, True)
        assert s_blk.shape == (hi - lo, 130)
        np.testing.assert_allclose(s_blk.cpu().numpy(), s_all[lo:hi].cpu().numpy(), rtol=0,
                                   atol=2e-5 * max(1.0, float(s_all.abs().max())))
        bx, by, bp = ops.scores_backward(saved, g[lo:hi].contiguous())
        parts.append([bx, by, *bp])
    summed = [torch.cat([parts[0][0], parts[1][0]])] + [a + c for a, c in zip(parts[0][1:], parts[1][1:])]
    _check_f32([t.cpu() for t in summed], [t.cpu() for t in whole], g.cpu(), f"row blocks {precision}")
