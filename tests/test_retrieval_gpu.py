"""Retrieval ranks on the GPU, against the fp64 restatement in tests/retrieval_reference.py.

Ranks are integer counts, so wherever the scores are exact the test is ``torch.equal``:
  * the matrix entry point compares the caller's own fp32 values: exact, ties included;
  * the chains on operands drawn from {-1, 0, 1}: every product and every partial sum is a small integer (|T| <= 33 at
    these shapes, |S| in the hundreds), exact in bf16 operands with fp32 accumulation, so every precision must give the
    fp64 ranks, ties included, and diag_out must equal diag(S).
On realistic (randn) inputs the kernel's scores differ from the fp64 ones by rounding, so a rank may move where a
negative lies within that error of the diagonal.  With |S' - S| <= tau elementwise, S'_ij > S'_ii implies
S_ij > S_ii - 2 tau, and S_ij > S_ii + 2 tau implies S'_ij > S'_ii: the kernel's rank lies in [lo, hi] of
``rank_band``.  tau is the project's figure for score-level quantities (tests/nce_shard_gpu_worker.py): 1e-4 max(1,
|S|max) against plain fp64 for "f32" / "f32_exact" / "bf16x3", 2e-3 max(1, |S|max) against fp64 scores of bf16-rounded
X, W, Y and T for "bf16".  So that the band cannot hide a failure its mean width is capped: 4 in bf16, 0.5 in the
fp32-grade modes (the reference alone gives at most 2.68 and 0.16 on the bilinear inputs, against mean ranks of 94 - 120).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math

import pytest
import torch

import retrieval_reference as ref
from oracle import mi_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ids(pattern, b):
    sid = torch.arange(b, dtype=torch.int64)
    if pattern == "dup":
        if b > 3:
            sid[3] = sid[2]
        sid[b - 1] = sid[0]
    elif pattern == "majority":
        sid[: (3 * b) // 4] = 7
    elif pattern == "all_equal":
        sid[:] = 5
    else:
        assert pattern == "unique"
    return sid


# ------------------------------------------------------------------------------------------------ 1. matrix entry
@pytest.mark.parametrize("pattern", ["unique", "dup", "majority", "all_equal"])
@pytest.mark.parametrize("b", [1, 7, 64, 200, 257])
def test_matrix_ranks_exact(b, pattern):
    from mutual_info_img_txt import critic_ops
    from mutual_info_img_txt.retrieval import matrix_retrieval_ranks
    gen = torch.Generator().manual_seed(100 + b)
    s = (torch.round(torch.randn(b, b, generator=gen) * 10.0) / 10.0).float()  # one decimal: ties occur
    sid = _ids(pattern, b)
    want_i2t, want_t2i = ref.ranks(s, sid)
    sd, sidd = s.to(DEV), sid.to(DEV)
    i2t, t2i = matrix_retrieval_ranks(sd, sidd)
    assert i2t.dtype == torch.int32 and t2i.dtype == torch.int32 and i2t.shape == (b,) and t2i.shape == (b,)
    assert torch.equal(i2t.cpu().long(), want_i2t)
    assert torch.equal(t2i.cpu().long(), want_t2i)
    if pattern == "all_equal":
        assert int(i2t.abs().sum()) == 0 and int(t2i.abs().sum()) == 0
    # each direction alone
    only_i, none_t = critic_ops.rank_matrix(sd, sidd, t2i=False)
    none_i, only_t = critic_ops.rank_matrix(sd, sidd, i2t=False)
    assert none_t is None and none_i is None
    assert torch.equal(only_i, i2t) and torch.equal(only_t, t2i)


# ------------------------------------------------------------------------------------------------ 2. chain, integer data
# (critic, precision, b, d); "bilinear_xy": S = X Y^T (no weight)
INT_CASES = [("bilinear", "bf16", 72, 64), ("bilinear", "bf16", 192, 64), ("bilinear", "bf16x3", 256, 128),
             ("bilinear", "f32_exact", 128, 64), ("bilinear", "bf16", 200, 60), ("bilinear_xy", "bf16", 256, 128),
             ("separable", "bf16", 256, 128), ("separable", "f32", 96, 40)]
K_PROJ = 48


def _ops_and_params(kind, d, draw):
    from mutual_info_img_txt.critic_ops import HipBilinearOps, HipSeparableOps
    if kind == "separable":
        return HipSeparableOps(), [draw(d, K_PROJ), draw(d, K_PROJ)]
    return HipBilinearOps(), ([] if kind == "bilinear_xy" else [draw(d, d)])


def _scores64(kind, x, y, params, rb=lambda t: t):
    """fp64 scores; ``rb`` rounds at the 16-bit chain's rounding points (the operands and T, or the projections)."""
    x, y, params = rb(x.double()), rb(y.double()), [rb(p.double()) for p in params]
    if kind == "separable":
        return rb(x @ params[0]) @ rb(y @ params[1]).t()
    return (rb(x @ params[0]) if params else x) @ y.t()


def _run_ops(ops, x, y, params, sid, prec, i2t=True, t2i=True):
    """One mi_rank_* call into poisoned outputs (the call has to zero them itself)."""
    from mutual_info_img_txt import _hip
    b = x.shape[0]
    ws = _hip.workspace(ops.rank_workspace_bytes(b, x.shape[1], y.shape[1], params, prec), x.device)
    ws.fill_(0xA5)
    ri = torch.full((b,), 12345, dtype=torch.int32, device=x.device) if i2t else None
    rt = torch.full((b,), -777, dtype=torch.int32, device=x.device) if t2i else None
    diag = torch.full((b,), float("nan"), device=x.device)
    ops.rank_call(x, y, params, sid, prec, ri, rt, diag, ws)()
    torch.cuda.synchronize()
    return ri, rt, diag


@pytest.mark.parametrize("pattern", ["dup", "all_equal"])
@pytest.mark.parametrize("case", INT_CASES, ids=[f"{c}-{p}-{b}x{d}" for c, p, b, d in INT_CASES])
def test_chain_ranks_exact_on_integer_data(case, pattern):
    from mutual_info_img_txt import _hip
    kind, precision, b, d = case
    gen = torch.Generator().manual_seed(b * 7 + d)

    def draw(r, c):
        return torch.randint(-1, 2, (r, c), generator=gen).float()

    x, y = draw(b, d), draw(b, d)
    ops, params = _ops_and_params(kind, d, draw)
    sid = _ids(pattern, b)
    s = _scores64(kind, x, y, params)
    # integers throughout: T (or A, C) exact in bf16 (8 significant bits), every partial sum exact in fp32
    inner = [x.double() @ params[0].double()] if params else []
    inner += [y.double() @ params[1].double()] if kind == "separable" else []
    assert all(float(t.abs().max()) <= 256.0 for t in inner) and float(s.abs().max()) < 2.0 ** 24
    want_i2t, want_t2i = ref.ranks(s, sid)
    if pattern == "dup":
        assert int(((s == torch.diagonal(s)[:, None]).sum(1) - 1).sum()) > 0  # ties off the diagonal do occur
    prec = _hip.PRECISIONS[precision]
    xd, yd, pd, sidd = x.to(DEV), y.to(DEV), [p.to(DEV) for p in params], sid.to(DEV)
    ri, rt, diag = _run_ops(ops, xd, yd, pd, sidd, prec)
    assert torch.equal(diag.cpu().double(), torch.diagonal(s)), float((diag.cpu().double() - torch.diagonal(s)).abs().max())
    assert torch.equal(ri.cpu().long(), want_i2t), int((ri.cpu().long() - want_i2t).abs().max())
    assert torch.equal(rt.cpu().long(), want_t2i), int((rt.cpu().long() - want_t2i).abs().max())
    if pattern == "all_equal":
        assert int(ri.abs().sum()) == 0 and int(rt.abs().sum()) == 0
    # a second call gives identical bits; each direction alone gives the same ranks
    ri2, rt2, diag2 = _run_ops(ops, xd, yd, pd, sidd, prec)
    assert torch.equal(ri2, ri) and torch.equal(rt2, rt) and torch.equal(diag2, diag)
    only_i, none_t, _ = _run_ops(ops, xd, yd, pd, sidd, prec, t2i=False)
    none_i, only_t, _ = _run_ops(ops, xd, yd, pd, sidd, prec, i2t=False)
    assert none_t is None and none_i is None and torch.equal(only_i, ri) and torch.equal(only_t, rt)
    # the convenience form of the ops objects
    a, c = ops.rank_step(xd, yd, pd, sidd, prec)
    assert torch.equal(a, ri) and torch.equal(c, rt)


# ------------------------------------------------------------------------------------------------ 3. chain, realistic data
# (critic, precision, b, d, planted)
BAND_CASES = [("bilinear", p, b, d, False) for b, d in ((256, 128), (192, 64), (200, 60)) for p in ("bf16", "f32")]
BAND_CASES += [("separable", "bf16", 256, 128, False), ("bilinear", "bf16", 192, 64, True), ("bilinear", "f32", 192, 64, True)]


@functools.lru_cache(maxsize=None)
def _band_inputs(kind, b, d, planted):
    """The inputs of tests/test_nce_shard_gpu.py: randn, W 0.3 / sqrt(d) (projections 0.7 / sqrt(d)), seed 3 b + d."""
    gen = torch.Generator().manual_seed(b * 3 + d)
    x = torch.randn(b, d, generator=gen)
    y = torch.randn(b, d, generator=gen)
    if kind == "separable":
        params = [torch.randn(d, K_PROJ, generator=gen) * (0.7 / math.sqrt(d)) for _ in range(2)]
    else:
        params = [torch.randn(d, d, generator=gen) * (0.3 / math.sqrt(d))]
    if planted:  # every report moved towards its own image's T row: the true pair ranks near the top
        t = x @ params[0]
        y = y + 0.5 * math.sqrt(d) * t / t.norm(dim=1, keepdim=True)
    return x, y, params, _ids("dup", b)


@functools.lru_cache(maxsize=None)
def _band_reference(kind, rounded, b, d, planted):
    x, y, params, sid = _band_inputs(kind, b, d, planted)
    s = _scores64(kind, x, y, params, orc.round_bf16 if rounded else (lambda t: t))
    tau = (2e-3 if rounded else 1e-4) * max(1.0, float(s.abs().max()))
    return ref.rank_band(s, sid, tau) + (ref.ranks(s, sid),)


def _critic(kind, params):
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    d = params[0].shape[0]
    critic = BilinearCritic(d, d) if kind == "bilinear" else SeparableCritic(d, d, params[0].shape[1])
    with torch.no_grad():
        for p, v in zip(critic.parameters(), params):
            p.copy_(v)
    return critic.to(DEV)


@pytest.mark.parametrize("case", BAND_CASES,
                         ids=[f"{c}-{p}-{b}x{d}{'-planted' if pl else ''}" for c, p, b, d, pl in BAND_CASES])
def test_chain_ranks_within_band_on_realistic_data(case):
    from mutual_info_img_txt.retrieval import retrieval_metrics, retrieval_ranks
    kind, precision, b, d, planted = case
    x, y, params, sid = _band_inputs(kind, b, d, planted)
    rounded = precision == "bf16"
    lo, hi, exact = _band_reference(kind, rounded, b, d, planted)
    got = retrieval_ranks(x.to(DEV), y.to(DEV), sid.to(DEV), _critic(kind, params), precision)
    torch.cuda.synchronize()
    cap = 4.0 if rounded else 0.5
    for name, g, l, h, e in zip(("i2t", "t2i"), got, lo, hi, exact):
        g = g.cpu().long()
        width = float((h - l).double().mean())
        moved = int((g != e).sum())
        print(f"{case} {name}: mean rank {float(e.double().mean()):.2f} (kernel {float(g.double().mean()):.2f}), "
              f"band width {width:.3f}, ranks off the fp64 ones {moved} of {b}")
        assert width <= cap, (name, width)  # the reference's own property: a wider band could hide a failure
        assert bool((l <= g).all()) and bool((g <= h).all()), (name, int((l - g).max()), int((g - h).max()))
        mg, ml, mh = retrieval_metrics(g), retrieval_metrics(l), retrieval_metrics(h)
        for key in mg:
            a, c = (ml[key], mh[key]) if key == "median_rank" else (mh[key], ml[key])
            assert a <= mg[key] <= c, (name, key, a, mg[key], c)
    if planted:
        assert float(exact[0].double().mean()) < 3.0  # the plant works: a misaligned diagonal would rank ~b / 2


# ------------------------------------------------------------------------------------------------ 4. concat-MLP critic
def test_concat_mlp_ranks_equal_reference_of_its_own_scores():
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.model import make_mlp
    from mutual_info_img_txt.retrieval import retrieval_metrics, retrieval_ranks
    b, d = 64, 32
    torch.manual_seed(17)
    critic = make_mlp(2 * d, [64, 256]).to(DEV)
    gen = torch.Generator().manual_seed(18)
    x, y = torch.randn(b, d, generator=gen).to(DEV), torch.randn(b, d, generator=gen).to(DEV)
    sid = _ids("dup", b).to(DEV)
    _, scores = mi_critics.fused_mi_bound(x, y, sid, critic, return_scores=True)
    want = ref.ranks(scores, sid)
    got = retrieval_ranks(x, y, sid, critic)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and torch.equal(g.cpu().long(), w)
    assert float(want[0].double().mean()) > 1.0  # an untrained critic: the ranks are not trivially zero
    mgr = MultiModalManager(d_img=d, d_txt=d, critic="concat_mlp", hidden_dims=(64, 256))
    mgr.mi_discriminator = critic
    ev = mgr.retrieval_eval(x, y, sid, ks=(1, 5))
    assert ev == {"i2t": retrieval_metrics(want[0], (1, 5)), "t2i": retrieval_metrics(want[1], (1, 5))}


# ------------------------------------------------------------------------------------------------ 5. Python layer
def test_python_layer_detaches_and_rejects_precisions():
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    from mutual_info_img_txt.retrieval import retrieval_metrics, retrieval_ranks
    b, d = 64, 64
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(b, d, generator=gen).to(DEV).requires_grad_(True)
    y = torch.randn(b, d, generator=gen).to(DEV).requires_grad_(True)
    sid = [str(n) for n in range(b)]
    for critic in (BilinearCritic(d, d).to(DEV), SeparableCritic(d, d, 32).to(DEV)):
        i2t, t2i = retrieval_ranks(x, y, sid, critic)
        for r in (i2t, t2i):
            assert r.dtype == torch.int32 and r.shape == (b,) and not r.requires_grad and r.is_cuda
            assert int(r.min()) >= 0 and int(r.max()) < b
        for precision in ("fp8", "f16", "f16x3"):
            with pytest.raises(ValueError):
                retrieval_ranks(x, y, sid, critic, precision)
    assert x.grad is None and y.grad is None
    mgr = MultiModalManager(d_img=d, d_txt=d, critic="bilinear")
    mgr.mi_discriminator.to(DEV)
    ev = mgr.retrieval_eval(x, y, sid, ks=(1, 10), precision="bf16")
    i2t, t2i = retrieval_ranks(x, y, sid, mgr.mi_discriminator, "bf16")
    assert ev == {"i2t": retrieval_metrics(i2t, (1, 10)), "t2i": retrieval_metrics(t2i, (1, 10))}
    assert set(ev["i2t"]) == {"recall@1", "recall@10", "median_rank", "mrr"}
