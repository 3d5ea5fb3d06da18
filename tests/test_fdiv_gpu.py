"""Jensen-Shannon and NWJ bounds on the MI355X against the fp64 restatement (tests/fdiv_reference.py): the kernels on
logits and on materialised scores, the concat-MLP critic in its four precisions, the bilinear and separable critics, bit
reproducibility, forward-only calls, rejected precisions and the training loop.

Tolerances: materialised fp32 scores: loss 2e-6 * max(1, |S|max), gradients 2e-5 * max|grad|.
"f32" / "f32_exact" critics: the DV tests' figures (loss 3e-5 + 1e-5 rel; gradients rtol 2e-3, atol 3e-4 * max|grad|;
concat critic 2e-3 * max|grad|).  NWJ losses grow like e^s, so their tolerance is relative and scales
with |S|max.  bf16 / f16 modes: against the UNROUNDED fp64 restatement (the rounded oracles of the DV tests are
DV-specific): loss 3e-3 * max(1, |S|max) (relative for NWJ); every gradient's relative Frobenius error and worst element
(over max|grad|) within max(floor, 4 x the error of the DV step on the same inputs and precision against the same kind of
oracle), floors 2e-2 and 0.1.
All tests need an MI355X:  python -m pytest tests -m gpu"""
import math

import numpy as np
import pytest
import torch

import fdiv_reference as ref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _ids(b, kind):
    if kind == "unique":
        return [str(50000000 + n) for n in range(b)]
    if kind == "dup":
        sid = list(range(b))
        for n in range(b // 8):
            sid[n] = n - (n % 2)
        return [str(50000000 + s) for s in sid]
    return ["50000000"] * b


def _close(got, want, atol, rtol=0.0, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy(), rtol=rtol,
                               atol=atol, err_msg=what)


def _errs(got, want):
    """(relative Frobenius error, worst element / max|want|)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu().reshape(got.shape)
    return (float((got - want).norm()) / max(float(want.norm()), 1e-30),
            float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30))


def _loose(got, want, yard, what):
    """16-bit modes: errors within max(floor, 4 x the DV step's errors ``yard`` on the same inputs)."""
    fro, worst = _errs(got, want)
    print(what, f"frobenius {fro:.2e} worst {worst:.2e} (DV: {yard[0]:.2e}, {yard[1]:.2e})")
    assert fro <= max(2e-2, 4 * yard[0]), (what, "frobenius", fro, yard)
    assert worst <= max(0.1, 4 * yard[1]), (what, "worst element", worst, yard)


def _loss_tol(mode, loss, smax, base):
    return base * max(1.0, smax) * (max(1.0, abs(float(loss))) if mode == "nwj" else 1.0)


# ------------------------------------------------------------------------------------------------ logits and matrices
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("n,pos", [(1, 1), (7, 3), (5000, 64), (100000, 317)])
@pytest.mark.parametrize("scale", [3.0, 80.0])
def test_logits_kernels_vs_restatement(dev, mode, n, pos, scale):
    from mutual_info_img_txt import mi_critics
    if mode == "nwj" and scale > 50:
        scale = 10.0  # e^s must stay finite in fp32 (|s| < 88) for a finite NWJ value
    gen = torch.Generator().manual_seed(n + pos)
    logits = (torch.randn(n, 1, generator=gen) * scale)
    fn = mi_critics.jsd_bound_loss if mode == "jsd" else mi_critics.nwj_bound_loss
    x = logits.to(dev).requires_grad_(True)
    loss = fn(x, pos, dev)
    assert loss.shape == ()
    loss.backward()
    o = ref.logits_case(logits, pos, mode)
    if pos == n:  # no negatives
        assert math.isnan(float(loss))
        return
    _close(loss, o["loss"], 2e-6 * max(1.0, abs(float(o["loss"]))), what=mode)
    _close(x.grad, o["grad"], 2e-5 * float(o["grad"].abs().max()), what=mode)


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("b", [1, 3, 64, 1000])
@pytest.mark.parametrize("ids", ["unique", "dup", "equal"])
def test_matrix_kernels_vs_restatement(dev, mode, b, ids):
    from mutual_info_img_txt import mi_critics
    gen = torch.Generator().manual_seed(b)
    s = torch.randn(b, b, generator=gen) * 3
    sid = _ids(b, ids)
    sl = s.to(dev).requires_grad_(True)
    loss = mi_critics.matrix_bound_loss(sl, sid, mode)
    assert loss.shape == ()
    loss.backward()
    o = ref.matrix_case(s, sid, mode)
    if ids == "equal" or b == 1:
        assert math.isnan(float(loss))
        return
    smax = max(1.0, float(s.abs().max()))
    _close(loss, o["loss"], 2e-6 * smax * max(1.0, abs(float(o["loss"]))), what=mode)
    _close(sl.grad, o["grad"], 2e-5 * float(o["grad"].abs().max()), what=mode)


def test_jsd_finite_at_large_scores(dev):
    from mutual_info_img_txt import mi_critics
    s = torch.tensor([[80.0, -80.0, 80.0], [80.0, -80.0, -80.0], [-80.0, 80.0, 80.0]])
    sl = s.to(dev).requires_grad_(True)
    loss = mi_critics.matrix_bound_loss(sl, ["a", "b", "c"], "jsd")
    loss.backward()
    assert math.isfinite(float(loss)) and torch.isfinite(sl.grad).all()
    _close(loss, ref.matrix_case(s, ["a", "b", "c"], "jsd")["loss"], 1e-4)


# ------------------------------------------------------------------------------------------------ concat-MLP critic
def _mlp(dev, params, hidden, d):
    from mutual_info_img_txt.model import make_mlp
    mlp = make_mlp(2 * d, list(hidden))
    with torch.no_grad():
        for p, v in zip(mlp.parameters(), params):
            p.copy_(v)
    return mlp.to(dev)


def _concat_run(dev, x, y, sid, mlp, mode, precision, stats=False):
    from mutual_info_img_txt import mi_critics
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    for p in mlp.parameters():
        p.grad = None
    out = mi_critics.fused_mi_bound(xl, yl, sid, mlp, mode, precision=precision, return_scores=True, return_stats=True)
    loss, scores, stats = out
    tp, tn = stats if mode != "dv" else (loss.reshape(()), torch.zeros((), device=dev))
    assert loss.shape == (() if mode != "dv" else (1,))
    loss.sum().backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "scores": scores, "terms": (tp, tn), "dx": xl.grad, "dy": yl.grad,
            "dparams": [p.grad for p in mlp.parameters()]}


@pytest.mark.parametrize("b", [128, 512])
@pytest.mark.parametrize("hidden", [(1024, 512), (256, 256)], ids=["h1024_512", "h256_256"])
@pytest.mark.parametrize("precision", ["f32", "f32_exact", "bf16", "f16"])
def test_concat_vs_restatement(dev, b, hidden, precision):
    d = 768
    x, y, _, params = orc.synthetic_case(b, d, d, h1=hidden[0], h2=hidden[1], salt=b // 8)
    sid = _ids(b, "dup")
    mlp = _mlp(dev, params, hidden, d)
    p_dev = [p.to(dev) for p in params]

    def run(mode):
        got = _concat_run(dev, x, y, sid, mlp, mode, precision)
        o = ref.concat_case(x.to(dev), y.to(dev), p_dev, sid, mode)
        refs = [("dx", got["dx"], o["dx"]), ("dy", got["dy"], o["dy"])]
        refs += [(f"dparam{n}", g, r) for n, (g, r) in enumerate(zip(got["dparams"], o["dparams"]))]
        return got, o, refs

    yard = {}
    if precision in ("bf16", "f16"):
        _, _, refs = run("dv")
        yard = {name: _errs(g, r) for name, g, r in refs}
    for mode in ref.MODES:
        got, o, refs = run(mode)
        _close(got["terms"][0] + got["terms"][1], got["loss"], 1e-6 * max(1.0, abs(float(got["loss"]))))
        sc = max(float(o["scores"].abs().max()), 1.0)
        if precision in ("f32", "f32_exact"):
            _close(got["loss"], o["loss"], 3e-5 + 1e-5 * abs(float(o["loss"])), what=f"{mode} loss")
            for name, g, r in refs:
                # 2e-3 (DV: 5e-4): measured 8.9e-4 * max|dx| for "jsd" at B = 128 in both fp32-grade modes alike (the two
                # kernels agree; the oracle differs on a few small elements), DESIGN.md section 9
                scale = 1.0 if name == "dparam5" else float(r.abs().max())
                _close(g, r.reshape(g.shape), (1e-5 if name == "dparam5" else 2e-3) * scale, rtol=2e-3,
                       what=f"{mode} {name}")
        else:
            _close(got["loss"], o["loss"], _loss_tol(mode, o["loss"], sc, 3e-3), what=f"{mode} loss")
            for name, g, r in refs:
                if name == "dparam5":
                    # db3 = sum of g, two cancelling terms of size <= 1 (DV's vanishes: no yardstick); it moves with the
                    # 16-bit scores as the loss does
                    _close(g, r.reshape(g.shape), 3e-3 * sc, what=f"{mode} {precision} db3")
                    continue
                _loose(g, r, yard[name], f"{mode} {precision} {name}")


def test_concat_full_size_f16(dev):
    """B = 4096, d = 768, f16: the loss checked on the kernels' own scores, sampled grad_x rows against the fp64 gradient
    of those rows (the whole-batch g from the kernels' scores)."""
    b, d = 4096, 768
    x, y, _, params = orc.synthetic_case(b, d, d, h1=1024, h2=512, salt=3)
    sid = _ids(b, "dup")
    mlp = _mlp(dev, params, (1024, 512), d)
    rows = [0, 1, 7, 1000, 2047, 4095]
    p64 = [p.to(dev).double() for p in params]
    yard = None
    for mode in ("dv",) + ref.MODES:
        got = _concat_run(dev, x, y, sid, mlp, mode, "f16")
        o = ref.matrix_case(got["scores"].double(), sid, mode)
        _close(got["loss"].reshape(()), o["loss"], 1e-5 * max(1.0, abs(float(o["loss"]))),
               what=f"{mode} loss on own scores")
        g = o["grad"]
        xd = x.to(dev).double()[rows].clone().requires_grad_(True)
        sb = orc.concat_scores_matrix(xd, y.to(dev).double(), p64)
        (sb * g[rows]).sum().backward()
        if mode == "dv":
            yard = _errs(got["dx"][rows], xd.grad)
            continue
        _loose(got["dx"][rows], xd.grad, yard, f"{mode} sampled grad_x rows")


# ------------------------------------------------------------------------------------------------ bilinear / separable
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


def _run(dev, x, y, critic, sid, mode, precision):
    from mutual_info_img_txt import mi_critics
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    for p in critic.parameters():
        p.grad = None
    loss, (tp, tn) = mi_critics.fused_mi_bound(xl, yl, sid, critic, mode, precision=precision, return_stats=True)
    assert loss.shape == ()
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "tp": tp, "tn": tn, "dx": xl.grad, "dy": yl.grad,
            **{f"dp{n}": p.grad for n, p in enumerate(critic.parameters())}}


def _check_step(got, o, precision, mode, what):
    if precision == "bf16":
        _close(got["loss"], o["loss"], _loss_tol(mode, o["loss"], o["smax"], 3e-3), what=what)
        for k, r in o["grads"].items():
            fro, worst = _errs(got[k], r)
            assert fro <= 2e-2 and worst <= 0.15, (what, k, fro, worst)
    else:
        _close(got["loss"], o["loss"], 3e-5, rtol=1e-5 if mode == "jsd" else 2e-6 * max(1.0, o["smax"]), what=what)
        for k, r in o["grads"].items():
            _close(got[k], r, 3e-4 * float(r.abs().max()), rtol=2e-3, what=f"{what} {k}")


@pytest.mark.parametrize("shape", [(256, 128, 128), (1000, 72, 40), (512, 512, 512)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", ["f32", "f32_exact", "bf16", "bf16x3"])
def test_bilinear_vs_restatement(dev, shape, precision):
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + dx)
    sid = _ids(b, "dup")
    critic = _bilinear(dev, w)
    for mode in ref.MODES:
        got = _run(dev, x, y, critic, sid, mode, precision)
        xd, yd, wd = (t.double().to(dev).requires_grad_(True) for t in (x, y, w))
        s = (xd @ wd) @ yd.t()
        loss, _ = ref.matrix_loss(s, sid, mode)
        loss.backward()
        o = {"loss": loss.detach(), "smax": float(s.abs().max()), "grads": {"dx": xd.grad, "dy": yd.grad, "dp0": wd.grad}}
        _check_step(got, o, precision, mode, f"{mode} {precision}")
        _close(got["tp"] + got["tn"], got["loss"], 1e-6 * max(1.0, abs(float(got["loss"]))))


@pytest.mark.parametrize("precision", ["f32", "f32_exact", "bf16"])
def test_separable_vs_restatement(dev, precision):
    from mutual_info_img_txt.model import SeparableCritic
    b, dx, dy, k = 384, 96, 64, 48
    torch.manual_seed(4)
    critic = SeparableCritic(dx, dy, k).to(dev)
    x, y = torch.randn(b, dx), torch.randn(b, dy)
    sid = _ids(b, "dup")
    for mode in ref.MODES:
        got = _run(dev, x, y, critic, sid, mode, precision)
        xd, yd = x.double().to(dev).requires_grad_(True), y.double().to(dev).requires_grad_(True)
        wg, wh = (p.detach().double().clone().requires_grad_(True) for p in (critic.wg, critic.wh))
        s = (xd @ wg) @ (yd @ wh).t()
        loss, _ = ref.matrix_loss(s, sid, mode)
        loss.backward()
        o = {"loss": loss.detach(), "smax": float(s.abs().max()),
             "grads": {"dx": xd.grad, "dy": yd.grad, "dp0": wg.grad, "dp1": wh.grad}}
        _check_step(got, o, precision, mode, f"{mode} {precision}")


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_bit_reproducible_and_forward_only(dev, precision):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import make_mlp
    b, d = 512, 256
    x, y, w = _inputs(b, d, d, 11)
    sid = _ids(b, "dup")
    critic = _bilinear(dev, w)
    torch.manual_seed(2)
    mlp = make_mlp(2 * d, [256, 256]).to(dev)
    for mode in ref.MODES:
        for c in (critic, mlp):
            one, two = _run(dev, x, y, c, sid, mode, precision), _run(dev, x, y, c, sid, mode, precision)
            for k in one:
                assert torch.equal(one[k], two[k]), (mode, k)
            with torch.no_grad():
                loss = mi_critics.fused_mi_bound(x.to(dev), y.to(dev), sid, c, mode, precision=precision)
            assert torch.equal(loss, one["loss"]), mode


def test_rejected_precisions(dev):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import make_mlp
    x, y, w = _inputs(64, 128, 128, 2)
    critic = _bilinear(dev, w)
    for mode in ref.MODES:
        for prec in ("fp8", "f16", "f16x3"):
            with pytest.raises(ValueError):
                mi_critics.fused_mi_bound(x.to(dev), y.to(dev), _ids(64, "unique"), critic, mode, precision=prec)
        with pytest.raises(ValueError):
            mi_critics.fused_mi_bound(x.to(dev), y.to(dev), _ids(64, "unique"), make_mlp(256, [64, 256]).to(dev), mode,
                                      precision="bf16x3")


@pytest.mark.parametrize("critic", ["concat_mlp", "bilinear"])
def test_training_run_jsd(dev, tmp_path, critic):
    """train.py --synthetic --mi_estimator jsd: finite, falling loss (the step runs eagerly)."""
    import train
    losses = train.train_MI_models(["--synthetic", "--batch_size", "64", "--num_train_epochs", "3", "--steps_per_epoch",
                                    "15", "--critic", critic, "--embed_dim_img", "32", "--embed_dim_txt", "32",
                                    "--init_lr", "1e-3", "--save_directory", str(tmp_path), "--precision", "f32",
                                    "--mi_estimator", "jsd"])
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
