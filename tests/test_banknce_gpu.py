"""Per-sample InfoNCE against a memory bank on the MI355X: loss, lse_rows, lse_cols and every
gradient against the fp64 restatement (tests/banknce_reference.py) in both modes for the bilinear, w == NULL and separable
forms; id cases, exact scores, the cross-check against the row-block kernels, bank permutation, hygiene (bit
reproducibility, poisoned buffers, forward-only calls, grad_out, a non-default stream) and the Python layer.

Tolerances are those stated at the top of tests/test_nce_gpu.py for the same precision and path.  bf16: against the
restatement rounded at this step's own rounding points (banknce_reference.case(rounded=True)), loss / LSEs
2e-3 * max(1, |S|max), gradients 1e-2 * max|grad|.  "f32" (bf16x3 where every size is a multiple of 8) / "f32_exact" /
"bf16x3": against plain fp64, loss rtol 1e-5 atol 3e-5, LSEs 1e-4 * max(1, |S|max), gradients rtol 2e-3 atol
3e-4 * max|grad|.
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math
import numpy as np
import pytest
import torch

import banknce_reference as ref

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "f32_exact", "bf16", "bf16x3"]
# (B, M, d_img, d_txt).  16-bit chain: ragged 64-tiles with B + M = 272 across a 256 tile; rows across 128, several 256
# tiles of columns and several row tiles of the left block; M < B, the smallest chain bank.  Generic kernels: odd sizes,
# the smallest and a near-smallest case.
SHAPES = [(72, 200, 64, 192), (136, 520, 192, 64), (136, 8, 64, 64), (100, 77, 40, 24), (1, 1, 8, 8), (2, 3, 8, 8)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
FORMS = ["bilinear", "xyT", "separable"]


@pytest.fixture(scope="module")
def dev():
    from mutual_info_img_txt import _hip
    _hip.load()
    return torch.device("cuda:0")


def _ids(b, m, kind):
    """(sid, bank_sid).  unique; dup: duplicates inside the batch; third: a third of the bank shares ids with the batch;
    mixed: both; equal: every id equal on both sides."""
    if kind == "equal":
        return ["50000000"] * b, ["50000000"] * m
    sid = list(range(b))
    if kind in ("dup", "mixed"):
        for n in range(max(b // 4, min(b, 2))):
            sid[n] = n - (n % 2)
        if b > 40:
            sid[b - 1] = sid[b // 2]
    bank = [10 ** 6 + n for n in range(m)]
    if kind in ("third", "mixed"):
        for n in range(0, m, 3):
            bank[n] = sid[(7 * n) % b]
    return [str(50000000 + s) for s in sid], [str(50000000 + s) for s in bank]


@functools.lru_cache(maxsize=None)
def _inputs(shape, form, seed=0):
    b, m, dx, dy = shape
    gen = torch.Generator().manual_seed(1000 * b + m + seed)
    if form == "xyT":
        dx = dy
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    bx, by = torch.randn(m, dx, generator=gen), torch.randn(m, dy, generator=gen)
    if form == "bilinear":
        params = [torch.randn(dx, dy, generator=gen) * (0.3 / math.sqrt(dx))]
    elif form == "separable":
        kp = 48 if all(v % 8 == 0 for v in shape) else 10
        params = [torch.randn(dx, kp, generator=gen) * (0.7 / math.sqrt(dx)),
                  torch.randn(dy, kp, generator=gen) * (0.7 / math.sqrt(dy))]
    else:
        params = []
        x, bx = x * 0.3, bx * 0.3
    return x, y, params, bx, by


@functools.lru_cache(maxsize=None)
def _oracle(shape, form, ids, est, rounded):
    x, y, params, bx, by = _inputs(shape, form)
    sid, bsid = _ids(shape[0], shape[1], ids)
    return ref.case(x, y, params, sid, bx, by, bsid, est, kind="separable" if form == "separable" else "bilinear",
                    rounded=rounded)


def _prec_code(form, precision, x, y, params):
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import resolve_critic
    if form == "xyT":
        return _hip.PRECISIONS[precision]
    return resolve_critic("separable" if form == "separable" else "bilinear", precision, x.shape[0], x.shape[1],
                          y.shape[1], params)[2]


def _poisoned(n, dev, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype, device=dev)


def _step(dev, form, x, y, params, sid, bx, by, bsid, est, precision, grads=True, grad_out=None):
    """One raw C-ABI call on NaN-poisoned outputs and workspace: everything the entry point writes."""
    from mutual_info_img_txt import _hip, mi_critics
    lib = _hip.load()
    mode = _hip.NCE_ESTIMATORS[est]
    sym = est == "infonce_symmetric"
    b, m, dx, dy = x.shape[0], by.shape[0], x.shape[1], y.shape[1]
    prec = _prec_code(form, precision, x, y, params)
    xd, yd, byd = x.to(dev).contiguous(), y.to(dev).contiguous(), by.to(dev).contiguous()
    bxd = bx.to(dev).contiguous() if (bx is not None and sym) else None
    pd = [p.to(dev).contiguous() for p in params]
    codes, bcodes = mi_critics.study_id_codes(sid, dev), mi_critics.study_id_codes(bsid, dev)
    loss, r = _poisoned(1, dev), _poisoned(b, dev)
    c = _poisoned(b, dev) if sym else None
    gs = [torch.full_like(t, float("nan")) for t in (xd, yd, *pd)] if grads else []
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=dev)
    p = _hip.ptr
    if form == "separable":
        nbytes = lib.mi_banknce_separable_workspace_bytes(b, m, dx, dy, pd[0].shape[1], mode, prec, int(grads))
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        _hip.call("mi_banknce_separable_step", dev, p(xd), p(yd), p(pd[0]), p(pd[1]), p(codes), p(bxd), p(byd), p(bcodes),
                  b, m, dx, dy, pd[0].shape[1], mode, prec, p(go), p(loss), p(r), p(c),
                  *[p(g) for g in (gs or [None] * 4)], p(ws), ws.numel())
    else:
        nbytes = lib.mi_banknce_bilinear_workspace_bytes(b, m, dx, dy, mode, prec, int(grads))
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        w = pd[0] if pd else None
        g3 = (gs + [None] * 3)[:3]
        _hip.call("mi_banknce_bilinear_step", dev, p(xd), p(yd), p(w), p(codes), p(bxd), p(byd), p(bcodes), b, m, dx, dy,
                  mode, prec, p(go), p(loss), p(r), p(c), p(g3[0]), p(g3[1]), p(g3[2]), p(ws), ws.numel())
    torch.cuda.synchronize()
    return {"loss": loss[0], "lse_rows": r, "lse_cols": c, "grads": gs}


def _close(got, want, atol, rtol=0.0, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy(), rtol=rtol,
                               atol=atol, err_msg=str(what))


def _check(got, o, bf16, what, grads=True):
    smax = max(1.0, o["smax"])
    if bf16:
        lt, lrt, st, gt, grt = 2e-3 * smax, 0.0, 2e-3 * smax, 1e-2, 0.0
    else:
        lt, lrt, st, gt, grt = 3e-5, 1e-5, 1e-4 * smax, 3e-4, 2e-3
    assert bool(torch.isfinite(got["loss"])), what
    _close(got["loss"], o["loss"], lt, rtol=lrt, what=what)
    _close(got["lse_rows"], o["lse_rows"], st, what=(what, "lse_rows"))
    if o["lse_cols"] is not None:
        _close(got["lse_cols"], o["lse_cols"], st, what=(what, "lse_cols"))
    else:
        assert got["lse_cols"] is None
    if grads:
        for n, (g, w) in enumerate(zip(got["grads"], o["grads"])):
            print(f"{what} grad {n}: max err {float((g.double().cpu() - w).abs().max()):.3e} of max {float(w.abs().max()):.3e}")
            _close(g, w, gt * max(float(w.abs().max()), 1e-30), rtol=grt, what=(what, "grad", n))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_step_vs_restatement(dev, shape, precision):
    """Loss, LSEs and every gradient, both modes, the three forms; ids with duplicates in the batch and a third of the
    bank sharing ids with the batch."""
    sid, bsid = _ids(shape[0], shape[1], "mixed")
    for form in FORMS:
        x, y, params, bx, by = _inputs(shape, form)
        for est in ref.MODES:
            got = _step(dev, form, x, y, params, sid, bx, by, bsid, est, precision)
            _check(got, _oracle(shape, form, "mixed", est, precision == "bf16"), precision == "bf16",
                   (form, est, precision))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("ids", ["unique", "dup", "third", "equal"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["chain16", "generic"])
def test_id_cases(dev, shape, ids, precision):
    sid, bsid = _ids(shape[0], shape[1], ids)
    x, y, params, bx, by = _inputs(shape, "bilinear")
    for est in ref.MODES:
        got = _step(dev, "bilinear", x, y, params, sid, bx, by, bsid, est, precision)
        o = _oracle(shape, "bilinear", ids, est, precision == "bf16")
        _check(got, o, precision == "bf16", (ids, est, precision))
        if ids == "equal":  # no row or column has a negative: exactly 0, exact zero gradients, LSEs = the diagonal
            assert float(got["loss"]) == 0.0
            for g in got["grads"]:
                assert torch.equal(g, torch.zeros_like(g))
            if got["lse_cols"] is not None:
                assert torch.equal(got["lse_rows"], got["lse_cols"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(72, 200, 64, 64), (100, 77, 40, 24)], ids=["chain16", "generic"])
def test_exact_scores(dev, shape, precision):
    """Operands from {-1, 0, 1}: T and the scores are small integers, exact in every precision, so loss and gradients are
    held to the fp32 tolerance in all four precisions (bf16: against the restatement at this step's rounding points,
    which with exact scores are those of G and dT / dU alone)."""
    b, m, dx, dy = shape
    gen = torch.Generator().manual_seed(5)

    def tern(*size):
        return (torch.randint(0, 16, size, generator=gen) == 0).float() * (torch.randint(0, 2, size, generator=gen) * 2 - 1)

    x, y, w, bx, by = tern(b, dx), tern(b, dy), tern(dx, dy), tern(m, dx), tern(m, dy)
    assert float((x @ w).abs().max()) < 128 and float(((x @ w) @ y.t()).abs().max()) < 64
    sid, bsid = _ids(b, m, "mixed")
    for est in ref.MODES:
        got = _step(dev, "bilinear", x, y, [w], sid, bx, by, bsid, est, precision)
        o = ref.case(x, y, [w], sid, bx, by, bsid, est, rounded=precision == "bf16")
        _check(got, o, False, ("exact", est, precision))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["chain16", "generic"])
def test_rowwise_equals_row_block_kernels(dev, shape):
    """B * L (row-wise) == the sum of the row terms that mi_nce_bilinear_shard_fwd writes for the row block b_rows = B,
    b = B + M, row_offset = 0 on the concatenated reports and ids (floats [2b, 2b + b_rows) of its part)."""
    from mutual_info_img_txt import _hip, mi_critics
    lib = _hip.load()
    b, m, dx, dy = shape
    n = b + m
    x, y, params, bx, by = _inputs(shape, "bilinear")
    sid, bsid = _ids(b, m, "mixed")
    for precision in ("f32", "bf16"):
        prec = _prec_code("bilinear", precision, x, y, params)
        got = _step(dev, "bilinear", x, y, params, sid, None, by, bsid, "infonce_rowwise", precision, grads=False)
        xd, w = x.to(dev), params[0].to(dev)
        yall = torch.cat([y, by]).to(dev).contiguous()
        call = mi_critics.study_id_codes(sid + bsid, dev)
        part = torch.empty(lib.mi_nce_part_floats(b, n), device=dev)
        r = torch.empty(b, device=dev)
        ws = _hip.workspace(lib.mi_nce_bilinear_shard_workspace_bytes(b, n, dx, dy, prec), dev)
        _hip.call("mi_nce_bilinear_shard_fwd", dev, xd.data_ptr(), yall.data_ptr(), w.data_ptr(), call.data_ptr(),
                  call.data_ptr(), b, n, 0, dx, dy, _hip.MI_NCE_ROWWISE, prec, part.data_ptr(), r.data_ptr(), ws.data_ptr(),
                  ws.numel())
        torch.cuda.synchronize()
        terms = part[2 * n:2 * n + b].double().sum()
        _close(got["loss"].double() * b, terms, 3e-5 * b, rtol=1e-5, what=precision)
        _close(got["lse_rows"], r, 1e-4 * max(1.0, float(r.abs().max())), what=precision)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["chain16", "generic"])
def test_bank_permutation(dev, shape):
    """The loss does not depend on the order of the bank's entries (beyond the order of the float sums)."""
    b, m, dx, dy = shape
    x, y, params, bx, by = _inputs(shape, "bilinear")
    sid, bsid = _ids(b, m, "mixed")
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(3))
    for est in ref.MODES:
        one = _step(dev, "bilinear", x, y, params, sid, bx, by, bsid, est, "f32")
        two = _step(dev, "bilinear", x, y, params, sid, bx[perm], by[perm], [bsid[int(k)] for k in perm], est, "f32")
        _close(two["loss"], one["loss"], 3e-5, rtol=1e-5, what=est)
        for g, h in zip(one["grads"], two["grads"]):
            _close(h, g, 3e-4 * float(g.abs().max()), rtol=2e-3, what=est)


# ------------------------------------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["chain16", "generic"])
def test_hygiene(dev, shape, form):
    """On NaN-poisoned outputs and workspace: a second call gives identical bits for every output; a forward-only call
    writes the same loss and LSE bits; grad_out = 2 scales the gradients; a non-default stream gives the same bits."""
    b, m = shape[0], shape[1]
    x, y, params, bx, by = _inputs(shape, form)
    sid, bsid = _ids(b, m, "mixed")
    for precision in ("bf16", "f32"):
        for est in ref.MODES:
            args = (dev, form, x, y, params, sid, bx, by, bsid, est, precision)
            one, two = _step(*args), _step(*args)
            fwd = _step(*args, grads=False)
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                side = _step(*args)
            twice = _step(*args, grad_out=2.0)
            for other in (two, side):
                for k in ("loss", "lse_rows", "lse_cols"):
                    assert one[k] is None or torch.equal(one[k], other[k]), (k, est, precision)
                for g, h in zip(one["grads"], other["grads"]):
                    assert torch.equal(g, h) and bool(torch.isfinite(g).all()), (est, precision)
            for k in ("loss", "lse_rows", "lse_cols"):
                assert one[k] is None or torch.equal(one[k], fwd[k]), (k, est, precision)
            assert torch.equal(twice["loss"], one["loss"])
            gt, grt = (1e-2, 0.0) if precision == "bf16" else (3e-4, 2e-3)
            for g, h in zip(one["grads"], twice["grads"]):
                _close(h, 2.0 * g, gt * float(g.abs().max()) * 2.0, rtol=grt, what=(est, precision, "grad_out"))


# ------------------------------------------------------------------------------------------------ Python layer
def _critic(dev, form, params):
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    if form == "bilinear":
        critic = BilinearCritic(*params[0].shape)
        with torch.no_grad():
            critic.weight.copy_(params[0])
    else:
        critic = SeparableCritic(params[0].shape[0], params[1].shape[0], params[0].shape[1])
        with torch.no_grad():
            critic.wg.copy_(params[0])
            critic.wh.copy_(params[1])
    return critic.to(dev)


@pytest.mark.parametrize("form", ["bilinear", "separable"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["chain16", "generic"])
def test_autograd_through_memory_bank_infonce(dev, shape, form):
    from mutual_info_img_txt.memory_bank import memory_bank_infonce
    b, m = shape[0], shape[1]
    x, y, params, bx, by = _inputs(shape, form)
    sid, bsid = _ids(b, m, "mixed")
    critic = _critic(dev, form, params)
    for est in ref.MODES:
        sym = est == "infonce_symmetric"
        for p in critic.parameters():
            p.grad = None
        xl, yl = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        bank = (bx.to(dev) if sym else None, by.to(dev), bsid)
        loss, (r, c) = memory_bank_infonce(xl, yl, sid, critic, bank, symmetric=sym, precision="f32", return_stats=True)
        assert loss.shape == ()
        (loss * 2.0).backward()
        torch.cuda.synchronize()
        o = _oracle(shape, form, "mixed", est, False)
        got = {"loss": loss.detach(), "lse_rows": r, "lse_cols": c,
               "grads": [0.5 * g for g in (xl.grad, yl.grad, *[p.grad for p in critic.parameters()])]}
        _check(got, o, False, (form, est, "autograd"))


def test_queue_feeds_the_loss(dev):
    """An empty queue is fused_mi_bound itself (torch.equal); a queue filled by three pushes, with wrap, against the
    restatement on q.img / q.txt / q.ids."""
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.memory_bank import EmbeddingQueue, memory_bank_infonce
    shape = (72, 200, 64, 192)
    b, _, dx, dy = shape
    x, y, params, bx, by = _inputs(shape, "bilinear")
    sid, bsid = _ids(b, 200, "mixed")
    critic = _critic(dev, "bilinear", params)
    xd, yd = x.to(dev), y.to(dev)
    q = EmbeddingQueue(160, dx, dy, dev)
    for sym, est in ((False, "infonce_rowwise"), (True, "infonce_symmetric")):
        with torch.no_grad():
            assert torch.equal(memory_bank_infonce(xd, yd, sid, critic, q, symmetric=sym),
                               mi_critics.fused_mi_bound(xd, yd, sid, critic, est))
    for lo, hi in ((0, 72), (72, 136), (136, 200)):  # 200 rows into 160 slots: the third push wraps
        q.push(bx[lo:hi].to(dev), by[lo:hi].to(dev), bsid[lo:hi])
    assert len(q) == 160
    codes = mi_critics.study_id_codes(sid, dev)
    for sym, est in ((False, "infonce_rowwise"), (True, "infonce_symmetric")):
        xl = xd.clone().requires_grad_(True)
        loss = memory_bank_infonce(xl, yd, sid, critic, q, symmetric=sym, precision="f32")
        loss.backward()
        o = ref.case(x, y, params, codes.cpu(), q.img.cpu(), q.txt.cpu(), q.ids.cpu(), est)
        _close(loss, o["loss"], 3e-5, rtol=1e-5, what=est)
        _close(xl.grad, o["grads"][0], 3e-4 * float(o["grads"][0].abs().max()), rtol=2e-3, what=est)


def test_python_layer_rejections(dev):
    from mutual_info_img_txt.memory_bank import memory_bank_infonce
    from mutual_info_img_txt.model import make_mlp
    shape = (72, 200, 64, 192)
    x, y, params, bx, by = _inputs(shape, "bilinear")
    sid, bsid = _ids(72, 200, "unique")
    critic = _critic(dev, "bilinear", params)
    xd, yd, bxd, byd = (t.to(dev) for t in (x, y, bx, by))
    with pytest.raises(ValueError, match="requires grad"):
        memory_bank_infonce(xd, yd, sid, critic, (bxd, byd.clone().requires_grad_(True), bsid))
    with pytest.raises(ValueError, match="requires grad"):
        memory_bank_infonce(xd, yd, sid, critic, (bxd.clone().requires_grad_(True), byd, bsid))
    with pytest.raises(ValueError, match="bilinear and separable"):
        memory_bank_infonce(xd, yd, sid, make_mlp(64 + 192, [32, 16]).to(dev), (bxd, byd, bsid))
    with pytest.raises(ValueError, match="bank_img"):
        memory_bank_infonce(xd, yd, sid, critic, (None, byd, bsid), symmetric=True)
    with pytest.raises(ValueError):
        memory_bank_infonce(xd, yd, sid, critic, (bxd, byd, bsid), precision="fp8")
    with pytest.raises(Exception):
        memory_bank_infonce(x, y, sid, critic, (bxd, byd, bsid))  # CPU tensors


@pytest.mark.parametrize("critic", ["bilinear", "separable"])
def test_train_py_with_memory_bank(dev, tmp_path, critic):
    """train.py --synthetic --memory_bank 64: two steps per epoch, finite epoch losses (the second batch already scores
    against the queued first one)."""
    import train
    losses = train.train_MI_models(["--synthetic", "--batch_size", "32", "--num_train_epochs", "2", "--steps_per_epoch",
                                    "2", "--critic", critic, "--embed_dim_img", "32", "--embed_dim_txt", "32",
                                    "--init_lr", "1e-3", "--save_directory", str(tmp_path), "--precision", "f32",
                                    "--mi_estimator", "infonce_symmetric", "--memory_bank", "64"])
    print("epoch losses:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert len(train.train_mutual_information.last_manager.bank) == 64
