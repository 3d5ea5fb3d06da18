"""Per-sample InfoNCE on the MI355X against the fp64 restatement (tests/nce_reference.py): the kernels on materialised
scores, the bilinear and separable steps in every precision, and the cross-checks (autograd through torch, bit
reproducibility, forward-only calls, hipGraph replay, the training loop).

Tolerances: materialised fp32 scores (exact expf): loss / LSEs 2e-6 * max(1, |S|max), gradients 2e-5 * max|grad|.
bf16 step: against the oracle rounded at the chain's rounding points, loss 2e-3 * max(1, |S|max), gradients
1e-2 * max|grad| (test_flash_bilinear.py's DV figures).  "f32" (bf16x3) / "f32_exact": against plain fp64, loss rtol 1e-5
atol 3e-5, gradients rtol 2e-3 atol 3e-4 * max|grad| (test_parity_configs.py's DV figures).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nce_reference as ref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _dup_ids(b):
    """SURVEY.md 8d duplicates: sid_i = i - (i mod 2) for i < B / 8."""
    sid = list(range(b))
    for n in range(b // 8):
        sid[n] = n - (n % 2)
    return [str(50000000 + s) for s in sid]


def _ids(b, kind):
    if kind == "unique":
        return [str(50000000 + n) for n in range(b)]
    if kind == "dup":
        return _dup_ids(b)
    return ["50000000"] * b  # all equal: no negatives at all


def _close(got, want, atol, rtol=0.0, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy(), rtol=rtol,
                               atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------------ materialised scores
@pytest.mark.parametrize("b", [1, 3, 64, 1000, 4096])
@pytest.mark.parametrize("ids", ["unique", "dup", "equal"])
@pytest.mark.parametrize("scale", [3.0, 80.0])
def test_matrix_kernels_vs_restatement(dev, b, ids, scale):
    from mutual_info_img_txt import _hip, mi_critics
    gen = torch.Generator().manual_seed(b + int(scale))
    s = (torch.rand(b, b, generator=gen) * 2.0 - 1.0) * scale  # scale 80: scores of +-80
    sid = _ids(b, ids)
    lib = _hip.load()
    codes = mi_critics.study_id_codes(sid, dev)
    sd = s.to(dev)
    for est, mode in _hip.NCE_ESTIMATORS.items():
        o = ref.matrix_case(s, sid, est)
        smax = max(1.0, float(s.abs().max()))
        # through the C ABI: LSE outputs and the backward
        ws = _hip.workspace(lib.mi_matrix_nce_workspace_bytes(b), dev)
        loss = torch.empty(1, device=dev)
        r = torch.empty(b, device=dev)
        c = torch.empty(b, device=dev)
        _hip.call("mi_matrix_nce_fwd", dev, sd.data_ptr(), codes.data_ptr(), b, mode, loss.data_ptr(), r.data_ptr(),
                  c.data_ptr(), ws.data_ptr(), ws.numel())
        g = torch.empty_like(sd)
        _hip.call("mi_matrix_nce_bwd", dev, sd.data_ptr(), codes.data_ptr(), b, mode, r.data_ptr(), c.data_ptr(), None,
                  g.data_ptr())
        torch.cuda.synchronize()
        if ids == "equal":
            assert float(loss) == 0.0 and float(g.abs().max()) == 0.0, est  # no negatives: exactly 0 (DV: NaN)
        _close(loss[0], o["loss"], 2e-6 * smax, what=est)
        _close(r, o["lse_rows"], 2e-6 * smax, what=est)
        _close(c, o["lse_cols"], 2e-6 * smax, what=est)
        _close(g, o["grad"], 2e-5 * max(float(o["grad"].abs().max()), 1e-30), what=est)
        # the public autograd path
        sl = sd.clone().requires_grad_(True)
        l2 = mi_critics.matrix_bound_loss(sl, sid, est)
        assert l2.shape == ()
        (l2 * 2.0).backward()
        assert torch.equal(l2.detach().reshape(1), loss)
        # grad_out = 2 enters as a factor of the kernel's weights: equal up to rounding (and denormals, at scale 80)
        _close(sl.grad, 2.0 * g, 1e-6 * float(g.abs().max()), rtol=1e-6, what=est)


# ------------------------------------------------------------------------------------------------ bilinear step
SHAPES = [(64, 128, 128), (256, 256, 256), (1024, 512, 512), (4096, 512, 512), (1024, 768, 768), (1000, 520, 520),
          (37, 20, 12)]


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


def _run_bilinear(dev, x, y, w, sid, est, precision):
    from mutual_info_img_txt import mi_critics
    critic = _bilinear(dev, w)
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, (r, c) = mi_critics.fused_mi_bound(xl, yl, sid, critic, est, precision=precision, return_stats=True)
    assert loss.shape == ()
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "lse_rows": r, "lse_cols": c, "dx": xl.grad, "dy": yl.grad, "dw": critic.weight.grad}


def _plain_oracle(x, y, w, sid, est):
    """fp64, closed-form gradients: G = dL/dS, dT = G y, dY = G^T T, dX = dT W^T, dW = x^T dT."""
    x, y, w = x.double(), y.double(), w.double()
    t = x @ w
    s = t @ y.t()
    o = ref.matrix_case(s, sid, est)
    g = o["grad"]
    dt = g @ y
    o.update({"dx": dt @ w.t(), "dy": g.t() @ t, "dw": x.t() @ dt, "smax": float(s.abs().max())})
    return o


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{b}x{dx}x{dy}" for b, dx, dy in SHAPES])
@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_bilinear_step_vs_restatement(dev, shape, dup, precision):
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + dx)
    sid = _ids(b, "dup" if dup else "unique")
    for est in ref.MODES:
        got = _run_bilinear(dev, x, y, w, sid, est, precision)
        if precision == "bf16":
            o = ref.bilinear_step_rounded(x, y, w, sid, est)
            smax = max(1.0, float((orc.round_bf16(orc.round_bf16(x.double()) @ orc.round_bf16(w.double())) @
                                   orc.round_bf16(y.double()).t()).abs().max()))
            _close(got["loss"], o["loss"], 2e-3 * smax, what=est)
            _close(got["lse_rows"], o["lse_rows"], 2e-3 * smax, what=est)
            _close(got["lse_cols"], o["lse_cols"], 2e-3 * smax, what=est)
            for n in ("dx", "dy", "dw"):
                _close(got[n], o[n], 1e-2 * float(o[n].abs().max()), what=f"{est} {n}")
        else:
            o = _plain_oracle(x, y, w, sid, est)
            _close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=est)
            _close(got["lse_rows"], o["lse_rows"], 1e-4 * max(1.0, o["smax"]), what=est)
            _close(got["lse_cols"], o["lse_cols"], 1e-4 * max(1.0, o["smax"]), what=est)
            for n in ("dx", "dy", "dw"):
                _close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{est} {n}")


# ------------------------------------------------------------------------------------------------ separable step
def _separable_oracle(x, y, wg, wh, sid, est, rounded):
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y, wg, wh = x.double(), y.double(), wg.double(), wh.double()
    a = rb(rb(x) @ rb(wg))
    c = rb(rb(y) @ rb(wh))
    s = a @ c.t()
    o = ref.matrix_case(s, sid, est)
    g = rb(o["grad"])
    da, dc = rb(g @ c), rb(g.t() @ a)
    o.update({"dx": da @ rb(wg).t(), "dwg": rb(x).t() @ da, "dy": dc @ rb(wh).t(), "dwh": rb(y).t() @ dc,
              "smax": float(s.abs().max())})
    return o


@pytest.mark.parametrize("shape", [(256, 256, 256, 256), (37, 20, 12, 10)], ids=["configs1", "ragged"])
@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_separable_step_vs_restatement(dev, shape, precision):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import SeparableCritic
    b, dx, dy, k = shape
    gen = torch.Generator().manual_seed(b + k)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    wg = torch.randn(dx, k, generator=gen) * (0.7 / math.sqrt(dx))
    wh = torch.randn(dy, k, generator=gen) * (0.7 / math.sqrt(dy))
    sid = _dup_ids(b)
    critic = SeparableCritic(dx, dy, k)
    with torch.no_grad():
        critic.wg.copy_(wg)
        critic.wh.copy_(wh)
    critic.to(dev)
    for est in ref.MODES:
        for p in critic.parameters():
            p.grad = None
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        loss, (r, c) = mi_critics.fused_mi_bound(xl, yl, sid, critic, est, precision=precision, return_stats=True)
        loss.backward()
        torch.cuda.synchronize()
        got = {"dx": xl.grad, "dy": yl.grad, "dwg": critic.wg.grad, "dwh": critic.wh.grad}
        o = _separable_oracle(x, y, wg, wh, sid, est, precision == "bf16")
        if precision == "bf16":
            lt, gt, grt = 2e-3 * max(1.0, o["smax"]), 1.5e-2, 0.0
        else:
            lt, gt, grt = 3e-5, 3e-4, 2e-3
        _close(loss, o["loss"], lt, rtol=1e-5, what=est)
        _close(r, o["lse_rows"], max(lt, 1e-4 * max(1.0, o["smax"])), what=est)
        _close(c, o["lse_cols"], max(lt, 1e-4 * max(1.0, o["smax"])), what=est)
        for n in ("dx", "dy", "dwg", "dwh"):
            _close(got[n], o[n], gt * float(o[n].abs().max()), rtol=grt, what=f"{est} {n}")


# ------------------------------------------------------------------------------------------------ cross-checks
def test_step_equals_matrix_loss_on_own_scores(dev):
    """The fused step against matrix_bound_loss on the critic's own scores, autograd through torch in fp32."""
    from mutual_info_img_txt import mi_critics
    b, d = 64, 128
    x, y, w = _inputs(b, d, d, 5)
    sid = _dup_ids(b)
    for est in ref.MODES:
        got = _run_bilinear(dev, x, y, w, sid, est, "f32_exact")
        critic = _bilinear(dev, w)
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        loss = mi_critics.matrix_bound_loss(critic(xl, yl), sid, est)
        loss.backward()
        _close(got["loss"], loss, 1e-5, rtol=1e-5, what=est)
        for n, g in (("dx", xl.grad), ("dy", yl.grad), ("dw", critic.weight.grad)):
            _close(got[n], g, 1e-4 * float(g.abs().max()), rtol=1e-4, what=f"{est} {n}")


@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_bit_reproducible_and_forward_only(dev, precision):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import SeparableCritic
    b, d = (1024, 512) if precision != "f32_exact" else (256, 256)
    x, y, w = _inputs(b, d, d, 11)
    sid = _dup_ids(b)
    for est in ref.MODES:
        one = _run_bilinear(dev, x, y, w, sid, est, precision)
        two = _run_bilinear(dev, x, y, w, sid, est, precision)
        for k in one:
            assert torch.equal(one[k], two[k]), (est, k)
        critic = _bilinear(dev, w)
        with torch.no_grad():
            loss, (r, c) = mi_critics.fused_mi_bound(x.to(dev), y.to(dev), sid, critic, est, precision=precision,
                                                     return_stats=True)
        assert torch.equal(loss, one["loss"]) and torch.equal(r, one["lse_rows"]) and torch.equal(c, one["lse_cols"])
        # inputs that need no gradient: the forward-only call as well
        loss2 = mi_critics.fused_mi_bound(x.to(dev), y.to(dev), sid, critic.requires_grad_(False), est, precision=precision)
        assert loss2.grad_fn is None and torch.equal(loss2, one["loss"])
    sep = SeparableCritic(64, 48, 32).to(dev)
    xs, ys = torch.randn(96, 64, device=dev), torch.randn(96, 48, device=dev)
    full = mi_critics.fused_mi_bound(xs, ys, _dup_ids(96), sep, "infonce_symmetric", precision=precision)
    full.backward()
    with torch.no_grad():
        fwd = mi_critics.fused_mi_bound(xs, ys, _dup_ids(96), sep, "infonce_symmetric", precision=precision)
    assert torch.equal(full.detach(), fwd)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_graph_capture_replay(precision):
    r = subprocess.run([sys.executable, os.path.join(HERE, "nce_capture_worker.py"), precision], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "capture ok" in r.stdout


def test_concat_critic_rejected(dev):
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import make_mlp
    x, y = torch.randn(8, 16, device=dev), torch.randn(8, 16, device=dev)
    for est in ref.MODES:
        with pytest.raises(ValueError, match="matrix_bound_loss"):
            mi_critics.fused_mi_bound(x, y, [str(n) for n in range(8)], make_mlp(32, [8, 8]).to(dev), est)


def test_precisions_outside_the_loss_rejected(dev):
    from mutual_info_img_txt import mi_critics
    x, y, w = _inputs(64, 128, 128, 2)
    critic = _bilinear(dev, w)
    for prec in ("fp8", "f16", "f16x3"):
        with pytest.raises(ValueError):
            mi_critics.fused_mi_bound(x.to(dev), y.to(dev), [str(n) for n in range(64)], critic, "infonce_rowwise",
                                      precision=prec)


@pytest.mark.parametrize("critic", ["bilinear", "separable"])
def test_training_run_symmetric(dev, tmp_path, critic):
    """train.py --synthetic with --mi_estimator infonce_symmetric: finite, falling loss (the step runs eagerly)."""
    import train
    losses = train.train_MI_models(["--synthetic", "--batch_size", "64", "--num_train_epochs", "3", "--steps_per_epoch",
                                    "15", "--critic", critic, "--embed_dim_img", "32", "--embed_dim_txt", "32",
                                    "--init_lr", "1e-3", "--save_directory", str(tmp_path), "--precision", "f32",
                                    "--mi_estimator", "infonce_symmetric"])
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
