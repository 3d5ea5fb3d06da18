"""Study-positive InfoNCE on the MI355X against the fp64 restatement (tests/posnce_reference.py):
loss, both LSEs, the positive counts (exact integers) and every gradient, in both modes, for the bilinear, w == NULL and
separable forms and the matrix entry, in every precision; then the cross-checks (the per-sample InfoNCE on unique ids,
exact operands, B = 1, bit reproducibility with poisoned buffers and on a side stream, forward-only calls, grad_out,
autograd, the rejections, the training loop).

Tolerances are those of tests/test_nce_gpu.py for the same precision and path (the arithmetic is the same chain plus one
fp32 sum of at most B scores per row): materialised fp32 scores (exact expf): loss / LSEs 2e-6 * max(1, |S|max),
gradients 2e-5 * max|grad|.  bf16 step: against the restatement rounded at the chain's rounding points, loss / LSEs
2e-3 * max(1, |S|max), gradients 1e-2 * max|grad|.  "f32" (bf16x3) / "f32_exact" / "bf16x3": against plain fp64, loss
rtol 1e-5 atol 3e-5, LSEs 1e-4 * max(1, |S|max), gradients rtol 2e-3 atol 3e-4 * max|grad|.
Every comparison prints "posnce-err <what> <error / tolerance>" before it asserts (pytest -s shows the figures).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import posnce_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = ["f32", "f32_exact", "bf16", "bf16x3"]
# 16-bit chain: multiples of 8 but not of 64 (a partial last tile, two or three tiles per side); generic kernels: ragged,
# a single sample, three samples
CHAIN16 = [(72, 64, 192), (136, 192, 64)]
GENERIC = [(100, 40, 24), (1, 8, 8), (3, 8, 8)]
SHAPES = CHAIN16 + GENERIC
SHAPE_IDS = [f"{b}x{dx}x{dy}" for b, dx, dy in SHAPES]
PATTERNS = ("unique", "dup", "group5", "far", "equal")


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _dup_ids(b):
    """SURVEY.md 8d duplicates (as tests/test_nce_gpu.py): sid_i = i - (i mod 2) for i < B / 8."""
    sid = list(range(b))
    for n in range(b // 8):
        sid[n] = n - (n % 2)
    return [str(50000000 + s) for s in sid]


def _ids(b, kind):
    """None where the pattern does not fit the batch."""
    sid = list(range(b))
    if kind == "dup":
        return _dup_ids(b)
    if kind == "group5":          # a group of five at indices 62 .. 66: straddles a tile edge
        if b < 67:
            return None
        for n in range(62, 67):
            sid[n] = 62
    elif kind == "far":           # pairs (i, i + 70): the positives beside the diagonal lie in off-diagonal tiles only
        if b < 71:
            return None
        for n in range(b - 70):
            sid[n + 70] = n
    elif kind == "equal":
        sid = [0] * b
    return [str(50000000 + s) for s in sid]


def _patterns(b):
    return [(k, _ids(b, k)) for k in PATTERNS if _ids(b, k) is not None]


def _close(got, want, atol, rtol=0.0, what=""):
    g, w = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    ratio = float(np.max(np.abs(g - w) / np.maximum(atol + rtol * np.abs(w), 1e-300))) if g.size else 0.0
    print(f"posnce-err {what} {ratio:.3f}")
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


def _run(dev, x, y, critic, sid, est, precision, names):
    """The public path: loss, statistics and the gradients of x, y and the critic's parameters (named ``names``)."""
    from mutual_info_img_txt import study_positives as sp
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, st = sp.study_positive_infonce(xl, yl, sid, critic, symmetric=est == "infonce_symmetric", precision=precision,
                                         return_stats=True)
    assert loss.shape == () and st["n_pos"].dtype == torch.int32 and st["n_pos"].shape == (x.shape[0],)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "dx": xl.grad, "dy": yl.grad, **st}
    out.update({n: p.grad for n, p in zip(names, critic.parameters())})
    return out


def _raw(dev, x, y, w, sid, est, precision, grads=True, go=None, poison=False):
    """mi_posnce_bilinear_step through ctypes (w None: S = X Y^T): everything the entry point writes."""
    from mutual_info_img_txt import _hip, mi_critics
    from mutual_info_img_txt.critic_ops import OPS, resolve_critic
    b, dx, dy = x.shape[0], x.shape[1], y.shape[1]
    xd, yd = x.to(dev), y.to(dev)
    wd = None if w is None else w.to(dev)
    params = [] if wd is None else [wd]
    codes = mi_critics.study_id_codes(sid, dev)
    prec = resolve_critic("bilinear", precision, b, dx, dy, params)[2] if params else _hip.PRECISIONS[precision]
    ws = _hip.workspace(OPS["bilinear"].posnce_workspace_bytes(b, dx, dy, params, prec, grads), dev)
    fill = float("nan") if poison else 0.0
    if poison:
        ws.fill_(0xFF)
    new = lambda *s: torch.full(s, fill, device=dev)
    loss, r, c = new(1), new(b), new(b)
    n_pos = torch.full((b,), -7, dtype=torch.int32, device=dev)
    gl = [new(*t.shape) for t in (xd, yd, *params)] if grads else []
    gx, gy, gw = (gl + [None] * 3)[:3]
    p = _hip.ptr
    _hip.call("mi_posnce_bilinear_step", dev, xd.data_ptr(), yd.data_ptr(), p(wd), codes.data_ptr(), b, dx, dy,
              _hip.NCE_ESTIMATORS[est], prec, p(go), loss.data_ptr(), r.data_ptr(), c.data_ptr(), n_pos.data_ptr(), p(gx),
              p(gy), p(gw), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    out = {"loss": loss[0], "lse_rows": r, "lse_cols": c, "n_pos": n_pos, "grads": gl}
    out.update(dict(zip(("dx", "dy", "dw"), gl)))
    return out


def _check(got, o, names, precision, what, fp32_tolerance=False):
    smax = max(1.0, o["smax"])
    assert torch.equal(got["n_pos"].cpu(), o["n_pos"]), what           # exact integers
    if precision == "bf16" and not fp32_tolerance:
        _close(got["loss"], o["loss"], 2e-3 * smax, what=f"{what} loss")
        for n in ("lse_rows", "lse_cols"):
            _close(got[n], o[n], 2e-3 * smax, what=f"{what} {n}")
        for n in names:
            _close(got[n], o[n], 1e-2 * float(o[n].abs().max()), what=f"{what} {n}")
    else:
        _close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=f"{what} loss")
        for n in ("lse_rows", "lse_cols"):
            _close(got[n], o[n], 1e-4 * smax, what=f"{what} {n}")
        for n in names:
            _close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{what} {n}")


# ------------------------------------------------------------------------------------------------ the three forms
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bilinear_step_vs_restatement(dev, shape, precision):
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + dx)
    critic = _bilinear(dev, w)
    for kind, sid in _patterns(b):
        for est in ref.MODES:
            got = _run(dev, x, y, critic, sid, est, precision, ["dw"])
            o = ref.bilinear_case(x, y, w, sid, est, rounded=precision == "bf16")
            _check(got, o, ["dx", "dy", "dw"], precision, f"bilinear {b} {precision} {kind} {est}")


@pytest.mark.parametrize("shape", [(72, 64), (136, 192), (100, 40), (1, 8), (3, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_weightless_step_vs_restatement(dev, shape, precision):
    """w == NULL: S = X Y^T, through the C ABI."""
    b, d = shape
    x, y, _ = _inputs(b, d, d, b + d)
    x, y = x * 0.3, y * 0.3
    for kind, sid in _patterns(b):
        for est in ref.MODES:
            got = _raw(dev, x, y, None, sid, est, precision)
            o = ref.bilinear_case(x, y, None, sid, est, rounded=precision == "bf16")
            _check(got, o, ["dx", "dy"], precision, f"weightless {b} {precision} {kind} {est}")


@pytest.mark.parametrize("shape", [(72, 64, 192, 48), (136, 192, 64, 48), (100, 40, 24, 10), (1, 8, 8, 4), (3, 8, 8, 4)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_separable_step_vs_restatement(dev, shape, precision):
    b, dx, dy, kp = shape
    gen = torch.Generator().manual_seed(b + kp)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    wg = torch.randn(dx, kp, generator=gen) * (0.7 / math.sqrt(dx))
    wh = torch.randn(dy, kp, generator=gen) * (0.7 / math.sqrt(dy))
    critic = _separable(dev, wg, wh)
    for kind, sid in _patterns(b):
        for est in ref.MODES:
            got = _run(dev, x, y, critic, sid, est, precision, ["dwg", "dwh"])
            o = ref.separable_case(x, y, wg, wh, sid, est, rounded=precision == "bf16")
            _check(got, o, ["dx", "dy", "dwg", "dwh"], precision, f"separable {b} {precision} {kind} {est}")


# ------------------------------------------------------------------------------------------------ cross-checks
@pytest.mark.parametrize("shape", [(72, 64, 192), (100, 40, 24)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_unique_ids_give_the_per_sample_infonce(dev, shape, precision):
    from mutual_info_img_txt import mi_critics
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, 33)
    sid = _ids(b, "unique")
    critic = _bilinear(dev, w)
    for est in ref.MODES:
        got = _run(dev, x, y, critic, sid, est, precision, ["dw"])
        critic.weight.grad = None
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        full, (r, c) = mi_critics.fused_mi_bound(xl, yl, sid, critic, est, precision=precision, return_stats=True)
        full.backward()
        assert torch.allclose(got["loss"], full.detach(), rtol=1e-5, atol=3e-5), est
        assert torch.allclose(got["lse_rows"], r, rtol=1e-5, atol=3e-5) and torch.allclose(got["lse_cols"], c, rtol=1e-5, atol=3e-5)
        assert int(got["n_pos"].min()) == 1 and int(got["n_pos"].max()) == 1
        for n, g in (("dx", xl.grad), ("dy", yl.grad), ("dw", critic.weight.grad)):
            assert torch.allclose(got[n], g, rtol=2e-3, atol=3e-4 * float(g.abs().max())), (est, n)


@pytest.mark.parametrize("shape", [(72, 64, 64), (100, 36, 20)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_operands(dev, shape, precision):
    """Operands from {-1, 0, 1} (W scaled by a power of two): T and S are exact in every precision, so every precision
    meets the fp32 tolerance."""
    b, dx, dy = shape
    gen = torch.Generator().manual_seed(b)
    x = torch.randint(-1, 2, (b, dx), generator=gen).float()
    y = torch.randint(-1, 2, (b, dy), generator=gen).float()
    w = torch.randint(-1, 2, (dx, dy), generator=gen).float() / 16.0
    critic = _bilinear(dev, w)
    for kind, sid in _patterns(b):
        for est in ref.MODES:
            got = _run(dev, x, y, critic, sid, est, precision, ["dw"])
            o = ref.bilinear_case(x, y, w, sid, est, rounded=precision == "bf16")
            _check(got, o, ["dx", "dy", "dw"], precision, f"exact {b} {precision} {kind} {est}", fp32_tolerance=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_sample_is_exactly_zero(dev, precision):
    from mutual_info_img_txt import study_positives as sp
    x, y, w = _inputs(1, 8, 8, 1)
    gen = torch.Generator().manual_seed(2)
    wg, wh = torch.randn(8, 4, generator=gen), torch.randn(8, 4, generator=gen)
    for est in ref.MODES:
        got = _run(dev, x, y, _bilinear(dev, w), ["7"], est, precision, ["dw"])
        sep = _run(dev, x, y, _separable(dev, wg, wh), ["7"], est, precision, ["dwg", "dwh"])
        raw = _raw(dev, x, y, None, ["7"], est, precision)
        for o, names in ((got, ["dx", "dy", "dw"]), (sep, ["dx", "dy", "dwg", "dwh"]), (raw, ["dx", "dy"])):
            assert float(o["loss"]) == 0.0 and o["n_pos"].tolist() == [1], est
            for n in names:
                assert torch.equal(o[n], torch.zeros_like(o[n])), (est, n)
        s = torch.full((1, 1), 3.25, device=dev, requires_grad=True)
        loss = sp.matrix_study_positive_infonce(s, ["7"], symmetric=est == "infonce_symmetric")
        loss.backward()
        assert float(loss.detach()) == 0.0 and torch.equal(s.grad, torch.zeros_like(s.grad))


# ------------------------------------------------------------------------------------------------ matrix entry
@pytest.mark.parametrize("b", [1, 3, 64, 130, 1000])
@pytest.mark.parametrize("scale", [3.0, 80.0])
def test_matrix_entry_vs_restatement_and_torch(dev, b, scale):
    from mutual_info_img_txt import _hip, critic_ops, mi_critics, study_positives as sp
    gen = torch.Generator().manual_seed(b + int(scale))
    s = (torch.rand(b, b, generator=gen) * 2.0 - 1.0) * scale  # scale 80: scores of +-80
    sd = s.to(dev)
    smax = max(1.0, float(s.abs().max()))
    for kind, sid in _patterns(b):
        codes = mi_critics.study_id_codes(sid, dev)
        pos = ref.positives(sid).to(dev)
        n = pos.sum(dim=1).float()
        for est, mode in _hip.NCE_ESTIMATORS.items():
            what = f"matrix {b} {scale} {kind} {est}"
            o = ref.matrix_case(s, sid, est)
            loss, r, c, n_pos = critic_ops.posnce_matrix_fwd(sd, codes, mode)
            g = critic_ops.posnce_matrix_bwd(sd, codes, mode, r, c, n_pos, None)
            torch.cuda.synchronize()
            assert torch.equal(n_pos.cpu(), o["n_pos"]), what
            _close(loss[0], o["loss"], 2e-6 * smax, what=f"{what} loss")
            _close(r, o["lse_rows"], 2e-6 * smax, what=f"{what} lse_rows")
            _close(c, o["lse_cols"], 2e-6 * smax, what=f"{what} lse_cols")
            gmax = max(float(o["grad"].abs().max()), 1e-30)
            _close(g, o["grad"], 2e-5 * gmax, what=f"{what} grad")
            # the public autograd path against torch's own logsumexp route on the device
            sl = sd.clone().requires_grad_(True)
            l2, st = sp.matrix_study_positive_infonce(sl, sid, symmetric=est == "infonce_symmetric", return_stats=True)
            assert l2.shape == () and torch.equal(l2.detach().reshape(1), loss) and torch.equal(st["n_pos"], n_pos)
            l2.backward()
            assert torch.equal(sl.grad, g), what
            st_ = sd.clone().requires_grad_(True)
            row = (torch.logsumexp(st_, dim=1) - (pos * st_).sum(dim=1) / n).mean()
            lt = row if est == "infonce_rowwise" else 0.5 * row + 0.5 * (torch.logsumexp(st_, dim=0) -
                                                                         (pos * st_).sum(dim=0) / n).mean()
            lt.backward()
            _close(l2, lt, 2e-6 * smax, what=f"{what} loss vs torch")
            _close(sl.grad, st_.grad, 2e-5 * gmax, what=f"{what} grad vs torch")


# ------------------------------------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("shape", CHAIN16[:1] + GENERIC[:1], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_bit_reproducible_poisoned_streams_forward_only_and_grad_out(dev, shape, precision):
    from mutual_info_img_txt import study_positives as sp
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, 11)
    sid = _ids(b, "far")
    keys = ("loss", "lse_rows", "lse_cols", "n_pos")
    for est in ref.MODES:
        one = _raw(dev, x, y, w, sid, est, precision)
        # a second call, with every output and the whole workspace NaN-poisoned beforehand
        two = _raw(dev, x, y, w, sid, est, precision, poison=True)
        # ... and on a non-default stream
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            three = _raw(dev, x, y, w, sid, est, precision, poison=True)
        for other in (two, three):
            for n in keys:
                assert torch.equal(one[n], other[n]), (est, n)
            for a, c in zip(one["grads"], other["grads"]):
                assert torch.equal(a, c), est
        # forward only (all gradient pointers NULL, the forward-only workspace): the same loss bits
        fwd = _raw(dev, x, y, w, sid, est, precision, grads=False, poison=True)
        assert fwd["grads"] == []
        for n in keys:
            assert torch.equal(one[n], fwd[n]), (est, n, "forward only")
        # grad_out = 2 doubles every gradient exactly
        dbl = _raw(dev, x, y, w, sid, est, precision, go=torch.full((1,), 2.0, device=dev))
        assert torch.equal(dbl["loss"], one["loss"])
        for a, c in zip(one["grads"], dbl["grads"]):
            assert torch.equal(2.0 * a, c), est
        # the public path: the same bits, and no graph where nothing needs a gradient
        critic = _bilinear(dev, w)
        got = _run(dev, x, y, critic, sid, est, precision, ["dw"])
        assert torch.equal(got["loss"], one["loss"])
        for n in ("dx", "dy", "dw"):
            assert torch.equal(got[n], one[n]), (est, n)
        with torch.no_grad():
            l2 = sp.study_positive_infonce(x.to(dev), y.to(dev), sid, critic, est == "infonce_symmetric", precision)
        assert l2.grad_fn is None and torch.equal(l2, one["loss"])


@pytest.mark.parametrize("kind", ["bilinear", "separable"])
def test_autograd_through_the_public_function(dev, kind):
    """The loss composes with autograd: d(3 L)/d(input) is three times the step's gradient, through a torch op upstream."""
    from mutual_info_img_txt import study_positives as sp
    b, dx, dy = 72, 64, 192
    x, y, w = _inputs(b, dx, dy, 5)
    gen = torch.Generator().manual_seed(5)
    wg, wh = torch.randn(dx, 48, generator=gen) / math.sqrt(dx), torch.randn(dy, 48, generator=gen) / math.sqrt(dy)
    critic = _bilinear(dev, w) if kind == "bilinear" else _separable(dev, wg, wh)
    names = ["dw"] if kind == "bilinear" else ["dwg", "dwh"]
    sid = _ids(b, "group5")
    base = _run(dev, x, y, critic, sid, "infonce_symmetric", "f32", names)
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss = sp.study_positive_infonce(xl * 1.0, yl, sid, critic, precision="f32") * 3.0
    loss.backward()
    assert torch.equal(loss.detach(), base["loss"] * 3.0)
    assert torch.equal(xl.grad, base["dx"] * 3.0) and torch.equal(yl.grad, base["dy"] * 3.0)
    for n, p in zip(names, critic.parameters()):
        assert torch.equal(p.grad, base[n] * 3.0), n


def test_rejections(dev):
    from mutual_info_img_txt import study_positives as sp
    from mutual_info_img_txt.model import make_mlp
    x, y, w = _inputs(64, 128, 128, 2)
    sid = _ids(64, "unique")
    xd, yd = x.to(dev), y.to(dev)
    with pytest.raises(ValueError, match="matrix_study_positive_infonce"):
        sp.study_positive_infonce(xd[:8, :16], yd[:8, :16], sid[:8], make_mlp(32, [8, 8]).to(dev))
    critic = _bilinear(dev, w)
    for prec in ("fp8", "f16", "f16x3"):
        with pytest.raises(ValueError, match="precision"):
            sp.study_positive_infonce(xd, yd, sid, critic, precision=prec)
    with pytest.raises(TypeError):
        sp.study_positive_infonce(xd, yd, sid, None)
    with pytest.raises(ValueError):
        sp.study_positive_infonce(xd, yd, sid[:5], critic)
    with pytest.raises(ValueError, match="B, B"):
        sp.matrix_study_positive_infonce(torch.zeros(8, 7, device=dev), sid[:8])
    with pytest.raises(ValueError, match="study_id"):
        sp.matrix_study_positive_infonce(torch.zeros(8, 8, device=dev), sid[:7])


def test_training_run_study_positives(tmp_path):
    """train.py --synthetic --critic bilinear --mi_estimator infonce_symmetric --study_positives as a child process:
    finite, falling loss."""
    script = os.path.join(os.path.dirname(HERE), "mutual-information-multimodal_amd", "train.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--batch_size", "64", "--num_train_epochs", "3",
                        "--steps_per_epoch", "15", "--critic", "bilinear", "--embed_dim_img", "32", "--embed_dim_txt", "32",
                        "--init_lr", "1e-3", "--save_directory", str(tmp_path), "--precision", "f32", "--mi_estimator",
                        "infonce_symmetric", "--study_positives"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    losses = [float(v) for v in re.findall(r"Epoch loss: (\S+)", r.stdout)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), r.stdout
    assert losses[-1] < losses[0]
