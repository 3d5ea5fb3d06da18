"""Hard-negative InfoNCE on the MI355X: the lists against retrieval_topk, loss and every gradient
against the fp64 restatement (tests/hardnce_reference.py) evaluated WITH THE KERNEL'S OWN LISTS (selection tolerance is
top-k's business, tests/test_topk_gpu.py), the exact support of G, tie order, the reduction to the full per-sample
InfoNCE, bit reproducibility, poisoned buffers, forward-only calls and the training loop.

Tolerances are those of tests/test_nce_gpu.py for the same precision and path (the arithmetic is the same chain):
materialised fp32 scores: loss / LSEs 2e-6 * max(1, |S|max), gradients 2e-5 * max|grad|.  bf16 step: against the
restatement rounded at the chain's rounding points, loss / LSEs 2e-3 * max(1, |S|max), gradients 1e-2 * max|grad| (1.5e-2
on the separable critic).  "f32" (bf16x3) / "f32_exact" / "bf16x3": against plain fp64, loss rtol 1e-5 atol 3e-5, LSEs
1e-4 * max(1, |S|max), gradients rtol 2e-3 atol 3e-4 * max|grad|.
All tests need an MI355X:  python -m pytest tests -m gpu"""
import math

import numpy as np
import pytest
import torch

import hardnce_reference as ref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "f32_exact", "bf16", "bf16x3"]


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _ids(b, kind):
    if kind == "unique":
        return [str(50000000 + n) for n in range(b)]
    if kind == "dup":  # SURVEY.md 8d duplicates: sid_i = i - (i mod 2) for i < B / 8, and two far-apart equal ids
        sid = list(range(b))
        for n in range(b // 8):
            sid[n] = n - (n % 2)
        if b > 40:
            sid[b - 1] = sid[b // 2]
        return [str(50000000 + s) for s in sid]
    return ["50000000"] * b  # all equal: no negatives at all


def _close(got, want, atol, rtol=0.0, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy(), rtol=rtol,
                               atol=atol, err_msg=what)


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


def _run(dev, x, y, critic, sid, k, est, precision, names):
    """The public path: loss, the lists and the gradients of x, y and the critic's parameters (named ``names``)."""
    from mutual_info_img_txt import hard_negatives as hn
    for p in critic.parameters():
        p.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss, lists = hn.hard_negative_infonce(xl, yl, sid, critic, k, symmetric=est == "infonce_symmetric",
                                           precision=precision, return_lists=True)
    assert loss.shape == () and lists["i2t"].dtype == torch.int32 and lists["i2t"].shape == (x.shape[0], k)
    assert (lists["t2i"] is None) == (est == "infonce_rowwise")
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "idx_rows": lists["i2t"], "idx_cols": lists["t2i"], "dx": xl.grad, "dy": yl.grad}
    out.update({n: p.grad for n, p in zip(names, critic.parameters())})
    return out


def _ops_step(dev, kind, x, y, params, sid, est, precision, k, need_grad=True):
    """The ops layer (also the w == NULL form, params == []): everything the entry point writes."""
    from mutual_info_img_txt import _hip, mi_critics
    from mutual_info_img_txt.critic_ops import OPS, resolve_critic
    codes = mi_critics.study_id_codes(sid, dev)
    prec = resolve_critic(kind, precision, x.shape[0], x.shape[1], y.shape[1], params)[2] if params else \
        _hip.PRECISIONS[precision]
    loss, r, c, ir, ic, grads = OPS[kind]().hardnce_step(x.to(dev), y.to(dev), [p.to(dev) for p in params], codes,
                                                         _hip.NCE_ESTIMATORS[est], prec, k, need_grad)
    torch.cuda.synchronize()
    return {"loss": loss[0], "lse_rows": r, "lse_cols": c, "idx_rows": ir, "idx_cols": ic, "grads": grads}


def _check(got, o, names, precision, est, sep=False):
    smax = max(1.0, o["smax"])
    if precision == "bf16":
        _close(got["loss"], o["loss"], 2e-3 * smax, what=est)
        for n in ("lse_rows", "lse_cols"):
            if got.get(n) is not None:
                _close(got[n], o[n], 2e-3 * smax, what=f"{est} {n}")
        for n in names:
            _close(got[n], o[n], (1.5e-2 if sep else 1e-2) * float(o[n].abs().max()), what=f"{est} {n}")
    else:
        _close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=est)
        for n in ("lse_rows", "lse_cols"):
            if got.get(n) is not None:
                _close(got[n], o[n], 1e-4 * smax, what=f"{est} {n}")
        for n in names:
            _close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{est} {n}")


def _separable_case(x, y, wg, wh, sid, k, est, lists, rounded):
    """As test_nce_gpu._separable_oracle: the w == NULL chain on the projections, then the back-projection."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    xd, yd, wgd, whd = x.double(), y.double(), wg.double(), wh.double()
    a, c = rb(rb(xd) @ rb(wgd)), rb(rb(yd) @ rb(whd))
    s = a @ c.t()
    o = ref.matrix_case(s, sid, k, est, lists)
    g = rb(o["grad"])
    da, dc = rb(g @ c), rb(g.t() @ a)
    o.update({"dx": da @ rb(wgd).t(), "dwg": rb(xd).t() @ da, "dy": dc @ rb(whd).t(), "dwh": rb(yd).t() @ dc,
              "smax": float(s.abs().max())})
    return o


# ------------------------------------------------------------------------------------------------ exact lists
@pytest.mark.parametrize("ids", ["unique", "dup", "equal"])
@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("shape", [(72, 64, 192), (100, 77, 40)], ids=["chain16", "generic"])
def test_lists_equal_retrieval_topk(dev, shape, k, ids):
    from mutual_info_img_txt import hard_negatives as hn, retrieval
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + k)
    gen = torch.Generator().manual_seed(k)
    kp = 48 if b % 8 == 0 else 10
    wg, wh = torch.randn(dx, kp, generator=gen) / math.sqrt(dx), torch.randn(dy, kp, generator=gen) / math.sqrt(dy)
    sid = _ids(b, ids)
    xd, yd = x.to(dev), y.to(dev)
    for critic in (_bilinear(dev, w), _separable(dev, wg, wh)):
        for precision in PRECISIONS:
            top = retrieval.retrieval_topk(xd, yd, critic, k, precision, img_ids=sid, txt_ids=sid)
            with torch.no_grad():
                _, sym = hn.hard_negative_infonce(xd, yd, sid, critic, k, True, precision, return_lists=True)
                _, row = hn.hard_negative_infonce(xd, yd, sid, critic, k, False, precision, return_lists=True)
            what = (type(critic).__name__, precision)
            assert torch.equal(sym["i2t"], top["i2t"][0]) and torch.equal(sym["t2i"], top["t2i"][0]), what
            assert torch.equal(row["i2t"], top["i2t"][0]) and row["t2i"] is None, what
            if ids == "equal":
                assert int(sym["i2t"].max()) == -1 and int(sym["t2i"].max()) == -1


# ------------------------------------------------------------------------------------------------ loss and gradients
# 16-bit chain: ragged 64-tiles (72, 136), more than one 256-tile and ragged (520); generic kernels: (100, 77, 40)
SHAPES = [(72, 64, 192), (136, 64, 192), (520, 64, 192), (100, 77, 40)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{b}x{dx}x{dy}" for b, dx, dy in SHAPES])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bilinear_step_vs_restatement(dev, shape, precision):
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, b + dx)
    sid = _ids(b, "dup")
    critic = _bilinear(dev, w)
    for est in ref.MODES:
        got = _run(dev, x, y, critic, sid, 5, est, precision, ["dw"])
        o = ref.bilinear_case(x, y, w, sid, 5, est, (got["idx_rows"], got["idx_cols"]), rounded=precision == "bf16")
        _check(got, o, ["dx", "dy", "dw"], precision, est)
        # the LSE outputs of the entry point
        raw = _ops_step(dev, "bilinear", x, y, [w], sid, est, precision, 5)
        assert torch.equal(raw["loss"], got["loss"]) and torch.equal(raw["idx_rows"], got["idx_rows"])
        if est == "infonce_rowwise":
            o.pop("lse_cols")
        _check(raw, o, [], precision, est)


@pytest.mark.parametrize("shape", [(72, 64), (136, 192), (520, 64), (100, 77)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_weightless_step_vs_restatement(dev, shape, precision):
    """w == NULL: S = X Y^T, through the ops layer."""
    b, d = shape
    x, y, _ = _inputs(b, d, d, b + d)
    x, y = x * 0.3, y * 0.3
    sid = _ids(b, "dup")
    for est in ref.MODES:
        got = _ops_step(dev, "bilinear", x, y, [], sid, est, precision, 5)
        got["dx"], got["dy"] = got["grads"]
        o = ref.bilinear_case(x, y, None, sid, 5, est, (got["idx_rows"], got["idx_cols"]), rounded=precision == "bf16")
        if est == "infonce_rowwise":
            o.pop("lse_cols")
        _check(got, o, ["dx", "dy"], precision, est)


@pytest.mark.parametrize("shape", [(72, 64, 192, 48), (136, 64, 192, 48), (520, 64, 192, 48), (100, 77, 40, 10)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_separable_step_vs_restatement(dev, shape, precision):
    b, dx, dy, kp = shape
    gen = torch.Generator().manual_seed(b + kp)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    wg = torch.randn(dx, kp, generator=gen) * (0.7 / math.sqrt(dx))
    wh = torch.randn(dy, kp, generator=gen) * (0.7 / math.sqrt(dy))
    sid = _ids(b, "dup")
    critic = _separable(dev, wg, wh)
    for est in ref.MODES:
        got = _run(dev, x, y, critic, sid, 5, est, precision, ["dwg", "dwh"])
        o = _separable_case(x, y, wg, wh, sid, 5, est, (got["idx_rows"], got["idx_cols"]), precision == "bf16")
        _check(got, o, ["dx", "dy", "dwg", "dwh"], precision, est, sep=True)


def test_f32_exact_randn_k5_is_the_support_test(dev):
    """One wrong entry of G moves a row of grad_x by a few percent of max|grad|: the fp32 tolerance sees it.  The lists of
    this precision are also the fp64 selection wherever no two fp64 scores of a query lie within fp32 rounding."""
    b, dx, dy = 136, 64, 192
    x, y, w = _inputs(b, dx, dy, 99)
    sid = _ids(b, "dup")
    critic = _bilinear(dev, w)
    for est in ref.MODES:
        got = _run(dev, x, y, critic, sid, 5, est, "f32_exact", ["dw"])
        o = ref.bilinear_case(x, y, w, sid, 5, est, (got["idx_rows"], got["idx_cols"]))
        _check(got, o, ["dx", "dy", "dw"], "f32_exact", est)
        own = ref.select(o["scores"], sid, 5)
        assert float((own[0] == got["idx_rows"].cpu()).double().mean()) > 0.99


# ------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("case", [(1, "unique"), (2, "equal"), (72, "equal"), (100, "equal")], ids=lambda c: f"{c[0]}{c[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_negatives_is_exactly_zero(dev, case, precision):
    b, ids = case
    d = 64 if b % 8 == 0 else 20
    x, y, w = _inputs(b, d, d, b)
    sid = _ids(b, ids)
    for est in ref.MODES:
        got = _run(dev, x, y, _bilinear(dev, w), sid, 5, est, precision, ["dw"])
        assert float(got["loss"]) == 0.0, est
        for n in ("dx", "dy", "dw"):
            assert float(got[n].abs().max()) == 0.0, (est, n)
        assert int(got["idx_rows"].max()) == -1 and (got["idx_cols"] is None or int(got["idx_cols"].max()) == -1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_samples(dev, precision):
    """B = 2 with different ids: one negative each, lists [other, -1, ...]."""
    x, y, w = _inputs(2, 16, 16, 2)
    sid = _ids(2, "unique")
    for est in ref.MODES:
        got = _run(dev, x, y, _bilinear(dev, w), sid, 3, est, precision, ["dw"])
        assert got["idx_rows"].tolist() == [[1, -1, -1], [0, -1, -1]]
        o = ref.bilinear_case(x, y, w, sid, 3, est, (got["idx_rows"], got["idx_cols"]), rounded=precision == "bf16")
        _check(got, o, ["dx", "dy", "dw"], precision, est)


# ------------------------------------------------------------------------------------------------ matrix entry
@pytest.mark.parametrize("b", [1, 33, 65, 200, 1000])
@pytest.mark.parametrize("ids", ["unique", "dup"])
def test_matrix_entry_support_and_values(dev, b, ids):
    from mutual_info_img_txt import hard_negatives as hn
    gen = torch.Generator().manual_seed(b)
    s = torch.round(torch.randn(b, b, generator=gen) * 20.0) / 10.0   # one decimal: many exact ties
    sid = _ids(b, ids)
    sd = s.to(dev)
    k = 5
    smax = max(1.0, float(s.abs().max()))
    for est in ref.MODES:
        sl = sd.clone().requires_grad_(True)
        loss, lists = hn.matrix_hard_negative_infonce(sl, sid, k, symmetric=est == "infonce_symmetric", return_lists=True)
        assert loss.shape == ()
        loss.backward()
        torch.cuda.synchronize()
        o = ref.matrix_case(s, sid, k, est)     # fp32 inputs are exact in fp64: the same order, the same ties
        assert torch.equal(lists["i2t"].cpu().long(), o["idx_rows"]), est
        if est == "infonce_symmetric":
            assert torch.equal(lists["t2i"].cpu().long(), o["idx_cols"]), est
        # the support: the lists plus the diagonal, nothing else and nothing missing
        want = ref.support(o["idx_rows"])
        if est == "infonce_symmetric":
            want = want | ref.support(o["idx_cols"]).t()
        if b == 1:
            want = torch.zeros(1, 1, dtype=torch.bool)   # no negatives: the diagonal term is exactly 0 as well
        assert torch.equal(sl.grad.cpu() != 0, want), est
        assert torch.equal(o["grad"] != 0, want), est
        _close(loss, o["loss"], 2e-6 * smax, what=est)
        _close(sl.grad, o["grad"], 2e-5 * max(float(o["grad"].abs().max()), 1e-30), what=est)
        # grad_out enters as a factor of the kernel's weights
        s2 = sd.clone().requires_grad_(True)
        (hn.matrix_hard_negative_infonce(s2, sid, k, symmetric=est == "infonce_symmetric") * 2.0).backward()
        _close(s2.grad, 2.0 * sl.grad, 1e-6 * float(sl.grad.abs().max()), rtol=1e-6, what=est)


def test_matrix_entry_lse_outputs(dev):
    from mutual_info_img_txt import _hip, critic_ops, mi_critics
    b, k = 65, 7
    s = torch.round(torch.randn(b, b, generator=torch.Generator().manual_seed(3)) * 20.0) / 10.0
    sid = _ids(b, "dup")
    codes = mi_critics.study_id_codes(sid, dev)
    for est, mode in _hip.NCE_ESTIMATORS.items():
        loss, r, c, ir, ic = critic_ops.hardnce_matrix_fwd(s.to(dev), codes, mode, k)
        o = ref.matrix_case(s, sid, k, est)
        smax = max(1.0, float(s.abs().max()))
        _close(r, o["lse_rows"], 2e-6 * smax, what=est)
        if est == "infonce_symmetric":
            _close(c, o["lse_cols"], 2e-6 * smax, what=est)
        else:
            assert c is None and ic is None


# ------------------------------------------------------------------------------------------------ tie order on the chains
@pytest.mark.parametrize("shape", [(72, 64, 64), (100, 36, 20)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tie_order_on_exact_operands(dev, shape, precision):
    """Operands from {-1, 0, 1} (W scaled by a power of two): T and S are exact in every precision, so the lists are the
    fp64 selection with all its ties, in every precision."""
    b, dx, dy = shape
    gen = torch.Generator().manual_seed(b)
    x = torch.randint(-1, 2, (b, dx), generator=gen).float()
    y = torch.randint(-1, 2, (b, dy), generator=gen).float()
    w = torch.randint(-1, 2, (dx, dy), generator=gen).float() / 16.0
    sid = _ids(b, "dup")
    critic = _bilinear(dev, w)
    for est in ref.MODES:
        got = _run(dev, x, y, critic, sid, 5, est, precision, ["dw"])
        o = ref.bilinear_case(x, y, w, sid, 5, est, rounded=precision == "bf16")   # the reference's OWN lists
        assert torch.equal(got["idx_rows"].cpu().long(), o["idx_rows"]), est
        if est == "infonce_symmetric":
            assert torch.equal(got["idx_cols"].cpu().long(), o["idx_cols"]), est
        _close(got["loss"], o["loss"], 3e-5, rtol=1e-5, what=est)
        for n in ("dx", "dy", "dw"):
            _close(got[n], o[n], 3e-4 * float(o[n].abs().max()), rtol=2e-3, what=f"{est} {n}")


# ------------------------------------------------------------------------------------------------ reduction to the full loss
@pytest.mark.parametrize("est", ref.MODES)
def test_reduces_to_the_full_loss(dev, est):
    from mutual_info_img_txt import mi_critics
    b, d = 33, 24
    x, y, w = _inputs(b, d, d, 33)
    sid = _ids(b, "unique")
    critic = _bilinear(dev, w)
    got = _run(dev, x, y, critic, sid, 32, est, "f32", ["dw"])
    critic.weight.grad = None
    xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    full = mi_critics.fused_mi_bound(xl, yl, sid, critic, estimator=est, precision="f32")
    full.backward()
    _close(got["loss"], full, 3e-5, rtol=1e-5, what=est)
    for n, g in (("dx", xl.grad), ("dy", yl.grad), ("dw", critic.weight.grad)):
        _close(got[n], g, 3e-4 * float(g.abs().max()), rtol=2e-3, what=f"{est} {n}")


# ------------------------------------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("shape", [(520, 64, 192), (100, 77, 40)], ids=["chain16", "generic"])
@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_bit_reproducible_poisoned_and_forward_only(dev, shape, precision):
    from mutual_info_img_txt import _hip, hard_negatives as hn, mi_critics
    from mutual_info_img_txt.critic_ops import OPS, resolve_critic
    b, dx, dy = shape
    x, y, w = _inputs(b, dx, dy, 11)
    sid = _ids(b, "dup")
    k = 10
    for est in ref.MODES:
        one = _ops_step(dev, "bilinear", x, y, [w], sid, est, precision, k)
        two = _ops_step(dev, "bilinear", x, y, [w], sid, est, precision, k)
        keys = [n for n in ("loss", "lse_rows", "lse_cols", "idx_rows", "idx_cols") if one[n] is not None]
        for n in keys:
            assert torch.equal(one[n], two[n]), (est, n)
        for a, c in zip(one["grads"], two["grads"]):
            assert torch.equal(a, c), est
        # every output and the whole workspace poisoned
        ops = OPS["bilinear"]()
        xd, yd, wd = x.to(dev), y.to(dev), w.to(dev)
        codes = mi_critics.study_id_codes(sid, dev)
        prec = resolve_critic("bilinear", precision, b, dx, dy, [wd])[2]
        mode = _hip.NCE_ESTIMATORS[est]
        sym = est == "infonce_symmetric"
        ws = _hip.workspace(ops.hardnce_workspace_bytes(b, dx, dy, [wd], prec, k, True), dev).fill_(0xFF)
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        loss, r, c = nan(1), nan(b), nan(b) if sym else None
        ir = torch.full((b, k), -7, dtype=torch.int32, device=dev)
        ic = ir.clone() if sym else None
        grads = [nan(*t.shape) for t in (xd, yd, wd)]
        ops.hardnce_call(xd, yd, [wd], codes, mode, prec, k, loss, r, c, ir, ic, grads, ws)()
        torch.cuda.synchronize()
        for n, t in zip(("loss", "lse_rows", "lse_cols", "idx_rows", "idx_cols"), (loss[0], r, c, ir, ic)):
            if t is not None:
                assert torch.equal(one[n], t), (est, n, "poisoned")
        for a, c2 in zip(one["grads"], grads):
            assert torch.equal(a, c2), (est, "poisoned")
        # forward only (no gradient pointers, the forward-only workspace): the training forward's bits
        fwd = _ops_step(dev, "bilinear", x, y, [w], sid, est, precision, k, need_grad=False)
        assert fwd["grads"] == []
        for n in keys:
            assert torch.equal(one[n], fwd[n]), (est, n, "forward only")
        critic = _bilinear(dev, w)
        with torch.no_grad():
            l2 = hn.hard_negative_infonce(xd, yd, sid, critic, k, sym, precision)
        assert l2.grad_fn is None and torch.equal(l2, one["loss"])
        l3 = hn.hard_negative_infonce(xd, yd, sid, critic.requires_grad_(False), k, sym, precision)
        assert l3.grad_fn is None and torch.equal(l3, one["loss"])


def test_rejections(dev):
    from mutual_info_img_txt import hard_negatives as hn
    from mutual_info_img_txt.model import make_mlp
    x, y, w = _inputs(64, 128, 128, 2)
    sid = _ids(64, "unique")
    xd, yd = x.to(dev), y.to(dev)
    with pytest.raises(ValueError, match="matrix_hard_negative_infonce"):
        hn.hard_negative_infonce(xd[:8, :16], yd[:8, :16], sid[:8], make_mlp(32, [8, 8]).to(dev), 3)
    critic = _bilinear(dev, w)
    for prec in ("fp8", "f16", "f16x3"):
        with pytest.raises(ValueError, match="precision"):
            hn.hard_negative_infonce(xd, yd, sid, critic, 3, precision=prec)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k must be"):
            hn.hard_negative_infonce(xd, yd, sid, critic, k)
        with pytest.raises(ValueError, match="k must be"):
            hn.matrix_hard_negative_infonce(torch.zeros(8, 8, device=dev), sid[:8], k)
    with pytest.raises(TypeError):
        hn.hard_negative_infonce(xd, yd, sid, None, 3)


@pytest.mark.parametrize("critic", ["bilinear", "separable"])
def test_training_run_hard_negatives(dev, tmp_path, critic):
    """train.py --synthetic --mi_estimator infonce_symmetric --hard_negatives 8: finite, falling loss."""
    import train
    losses = train.train_MI_models(["--synthetic", "--batch_size", "64", "--num_train_epochs", "3", "--steps_per_epoch",
                                    "15", "--critic", critic, "--embed_dim_img", "32", "--embed_dim_txt", "32",
                                    "--init_lr", "1e-3", "--save_directory", str(tmp_path), "--precision", "f32",
                                    "--mi_estimator", "infonce_symmetric", "--hard_negatives", "8"])
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
