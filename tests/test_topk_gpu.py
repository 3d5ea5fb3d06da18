"""Top-k retrieval over a gallery on the GPU, against the fp64 restatement in
tests/topk_reference.py.

The order "score descending, then candidate index ascending" is total, so wherever the scores are exact the test is
``torch.equal`` on idx AND val:
  * the matrix entry point selects among the caller's own fp32 values (rounded to one decimal: ties occur);
  * the chains on operands drawn from {-1, 0, 1}: every product and every partial sum is a small integer (|T| <= 64,
    |S| <= 4096 at these shapes), exact in bf16 operands with fp32 accumulation, so every precision must give the fp64
    lists, ties included;
  * the contention case: scores ascending in the candidate index, so every later tile beats every threshold and all
    waves of a query keep cascading into one list.
On realistic (randn) inputs the kernel's scores S' differ from the fp64 ones by rounding, |S' - S| <= tau.  With t_k the
reference's k-th score of a query: a candidate with S > t_k + 2 tau has S' > t_k + tau, while at most k - 1 candidates
have S > t_k and every other one has S' <= t_k + tau, so it must be returned; and at least k candidates have
S' >= t_k - tau, so every returned one has S' >= t_k - tau, hence S >= t_k - 2 tau.  tau is the project's figure for
score-level quantities: 1e-4 max(1, |S|max) against plain fp64 for "f32" / "f32_exact" / "bf16x3", 2e-3 max(1, |S|max)
against fp64 scores of bf16-rounded X, W, Y and T for "bf16".  So that the band cannot hide a failure, the mean number
of candidates within 2 tau of t_k (the k-th itself not counted) is capped: 0.5 in the fp32-grade modes, 4 in bf16 (on
these inputs the references alone, computed on the host, give at most 0.094 and 1.41).
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math

import pytest
import torch

import topk_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")


def _ids(pattern, n_q, n_g):
    """(query ids, candidate ids) int64, or (None, None)."""
    if pattern == "none":
        return None, None
    q, g = torch.arange(n_q, dtype=torch.int64), torch.arange(n_g, dtype=torch.int64)
    if pattern == "dup":
        q, g = q // 2, g // 3
    elif pattern == "all_equal":
        q[:], g[:] = 5, 5
    else:
        assert pattern == "unique"  # query i loses candidate i
    return q, g


def _dev(t):
    return None if t is None else t.to(DEV)


def _assert_same(got, want, what):
    idx, val = got
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == want[0].shape == val.shape, what
    assert torch.equal(idx.cpu().long(), want[0]), what
    assert torch.equal(val.cpu().double(), want[1]), what


# ------------------------------------------------------------------------------------------------ 1. matrix entry
@pytest.mark.parametrize("pattern", ["none", "unique", "dup", "all_equal"])
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 64), (200, 257), (257, 200), (65, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrix_topk_exact(shape, pattern):
    from mutual_info_img_txt.retrieval import matrix_topk
    n_rows, n_cols = shape
    gen = torch.Generator().manual_seed(100 + n_rows + 3 * n_cols)
    s = (torch.round(torch.randn(n_rows, n_cols, generator=gen) * 10.0) / 10.0).float()  # one decimal: ties occur
    if n_rows > 1:
        s[1, 0] = -0.0
    row_ids, col_ids = _ids(pattern, n_rows, n_cols)
    sd = s.to(DEV)
    for k in (1, 5, 32):  # 32 > n_cols on the small shapes: the tail
        for axis in (0, 1):
            want = ref.topk(s, k, row_ids, col_ids) if axis == 0 else ref.topk(s.t(), k, col_ids, row_ids)
            got = matrix_topk(sd, k, axis, _dev(row_ids), _dev(col_ids))
            _assert_same(got, want, (shape, pattern, k, axis))
            if pattern == "all_equal":
                assert int((got[0] != -1).sum()) == 0 and bool(torch.isinf(got[1]).all())
            again = matrix_topk(sd, k, axis, _dev(row_ids), _dev(col_ids))
            assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


# ------------------------------------------------------------------------------------------------ 2. chains, integer data
K_PROJ = 48
SHAPES_16BIT = [(128, 192, 64), (72, 520, 64)]  # the second spans several 256-wide tiles
SHAPE_GENERIC = (100, 77, 40)


def _ops_and_params(kind, d, draw):
    from mutual_info_img_txt.critic_ops import HipBilinearOps, HipSeparableOps
    if kind == "separable":
        return HipSeparableOps(), [draw(d, K_PROJ), draw(d, K_PROJ)]
    return HipBilinearOps(), ([] if kind == "bilinear_xy" else [draw(d, d)])


def _scores64(kind, x, y, params, rb=lambda t: t):
    """fp64 scores [n_img, n_txt]; ``rb`` rounds at the 16-bit chain's rounding points."""
    x, y, params = rb(x.double()), rb(y.double()), [rb(p.double()) for p in params]
    if kind == "separable":
        return rb(x @ params[0]) @ rb(y @ params[1]).t()
    return (rb(x @ params[0]) if params else x) @ y.t()


def _run_ops(ops, x, y, params, sid_img, sid_txt, prec, k, i2t=True, t2i=True):
    """One mi_topk_* call into poisoned outputs and a poisoned workspace (the call has to empty its lists itself)."""
    from mutual_info_img_txt import _hip
    n_img, n_txt = x.shape[0], y.shape[0]
    ws = _hip.workspace(ops.topk_workspace_bytes(n_img, n_txt, x.shape[1], y.shape[1], params, prec, k), x.device)
    ws.fill_(0xA5)

    def poisoned(n):
        return (torch.full((n, k), 12345, dtype=torch.int32, device=x.device),
                torch.full((n, k), float("nan"), dtype=torch.float32, device=x.device))

    out_i, out_t = poisoned(n_img) if i2t else None, poisoned(n_txt) if t2i else None
    ops.topk_call(x, y, params, sid_img, sid_txt, prec, k, out_i, out_t, ws)()
    torch.cuda.synchronize()
    return out_i, out_t


@pytest.mark.parametrize("precision", ["f32_exact", "bf16", "bf16x3"])
@pytest.mark.parametrize("kind", ["bilinear", "bilinear_xy", "separable"])
@pytest.mark.parametrize("shape", SHAPES_16BIT + [SHAPE_GENERIC], ids=lambda s: "x".join(map(str, s)))
def test_chain_topk_exact_on_integer_data(shape, kind, precision):
    from mutual_info_img_txt import _hip
    n_img, n_txt, d = shape
    gen = torch.Generator().manual_seed(n_img * 7 + n_txt + d)

    def draw(r, c):
        return torch.randint(-1, 2, (r, c), generator=gen).float()

    x, y = draw(n_img, d), draw(n_txt, d)
    ops, params = _ops_and_params(kind, d, draw)
    s = _scores64(kind, x, y, params)
    assert float(s.abs().max()) <= 4096 and bool((s == s.round()).all())  # integers: exact in every precision
    prec = _hip.PRECISIONS[precision]
    xd, yd, pd = x.to(DEV), y.to(DEV), [p.to(DEV) for p in params]
    for pattern, k in (("none", 32), ("dup", 7)):
        img_ids, txt_ids = _ids(pattern, n_img, n_txt)
        want = ref.both_directions(s, k, img_ids, txt_ids)
        si, st = _dev(img_ids), _dev(txt_ids)
        both = _run_ops(ops, xd, yd, pd, si, st, prec, k)
        _assert_same(both[0], want["i2t"], (shape, kind, precision, pattern, "i2t"))
        _assert_same(both[1], want["t2i"], (shape, kind, precision, pattern, "t2i"))
        # each direction alone, and the bits of a second call
        only_i, none_t = _run_ops(ops, xd, yd, pd, si, st, prec, k, t2i=False)
        none_i, only_t = _run_ops(ops, xd, yd, pd, si, st, prec, k, i2t=False)
        assert none_t is None and none_i is None
        again = _run_ops(ops, xd, yd, pd, si, st, prec, k)
        for a, b in ((only_i, both[0]), (only_t, both[1]), (again[0], both[0]), (again[1], both[1])):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 3. contention
@pytest.mark.parametrize("precision", ["bf16", "f32_exact"])
def test_ascending_scores_keep_every_wave_cascading(precision):
    """S[i, j] = j for every image: y_j = (j // 64, j % 64), x = (64, 1), W = I (padded to width 8 with zeros).  Every
    later candidate tile beats the threshold its query shows, so the list of a query takes inserts from all 64 row tiles
    at once -- the case that catches a cascade that loses or duplicates a key."""
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import HipBilinearOps
    n_img, n_txt, d, k = 64, 4096, 8, 32
    j = torch.arange(n_txt)
    y = torch.zeros(n_txt, d)
    y[:, 0], y[:, 1] = (j // 64).float(), (j % 64).float()
    x = torch.zeros(n_img, d)
    x[:, 0], x[:, 1] = 64.0, 1.0
    w = torch.eye(d)
    s = _scores64("bilinear", x, y, [w])
    assert torch.equal(s[0], j.double()) and torch.equal(s[-1], j.double())
    want = ref.both_directions(s, k)
    assert want["i2t"][0][5].tolist() == list(range(n_txt - 1, n_txt - 1 - k, -1))
    assert want["t2i"][0][77].tolist() == list(range(k))  # every image ties: the lower index first
    got = _run_ops(HipBilinearOps(), x.to(DEV), y.to(DEV), [w.to(DEV)], None, None, _hip.PRECISIONS[precision], k)
    _assert_same(got[0], want["i2t"], (precision, "i2t"))
    _assert_same(got[1], want["t2i"], (precision, "t2i"))


# ------------------------------------------------------------------------------------------------ 4. Python layer
def _int_critic(cls, *shape_args):
    critic = cls(*shape_args)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in critic.parameters():
            p.copy_(torch.randint(-1, 2, tuple(p.shape), generator=gen).float())
    return critic


def _critic_scores64(critic, x, y):
    from mutual_info_img_txt.model import BilinearCritic
    if isinstance(critic, BilinearCritic):
        return _scores64("bilinear", x, y, [critic.weight.detach().cpu()])
    return _scores64("separable", x, y, [critic.wg.detach().cpu(), critic.wh.detach().cpu()])


@pytest.mark.parametrize("shape", [(64, 64), (40, 104), (104, 40), (33, 50)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["bilinear", "separable"])
def test_retrieval_topk_bilinear_and_separable(kind, shape):
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    from mutual_info_img_txt.retrieval import retrieval_topk
    (n_img, n_txt), d, k = shape, 32, 6
    critic = _int_critic(BilinearCritic, d, d) if kind == "bilinear" else _int_critic(SeparableCritic, d, d, 16)
    gen = torch.Generator().manual_seed(n_img + n_txt)
    x = torch.randint(-1, 2, (n_img, d), generator=gen).float()
    y = torch.randint(-1, 2, (n_txt, d), generator=gen).float()
    s = _critic_scores64(critic, x, y)
    critic = critic.to(DEV)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    img_ids, txt_ids = [f"s{n // 2}" for n in range(n_img)], [f"s{n // 3}" for n in range(n_txt)]
    codes = _ids("dup", n_img, n_txt)
    for ids, want in (((None, None), ref.both_directions(s, k)), ((img_ids, txt_ids), ref.both_directions(s, k, *codes))):
        for precision in ("f32", "f32_exact", "bf16", "bf16x3"):
            got = retrieval_topk(xd, yd, critic, k, precision, *ids)
            assert set(got) == {"i2t", "t2i"}
            for d_ in ("i2t", "t2i"):
                _assert_same(got[d_], want[d_], (kind, shape, precision, d_))
                assert not got[d_][1].requires_grad
        one = retrieval_topk(xd, yd, critic, k, "bf16", *ids, directions=("t2i",))
        assert set(one) == {"t2i"}
        _assert_same(one["t2i"], want["t2i"], (kind, shape, "t2i alone"))
    assert xd.grad is None and yd.grad is None
    for precision in ("fp8", "f16", "f16x3"):
        with pytest.raises(ValueError):
            retrieval_topk(xd, yd, critic, k, precision)
    for bad_k in (0, 33):
        with pytest.raises(ValueError):
            retrieval_topk(xd, yd, critic, bad_k)
    with pytest.raises(ValueError):
        retrieval_topk(xd, yd, critic, k, img_ids=img_ids)  # ids: both or neither
    with pytest.raises(ValueError):
        retrieval_topk(xd, yd, critic, k, directions=("t2t",))


def test_retrieval_topk_make_mlp_square_and_rectangular_raises():
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import make_mlp
    from mutual_info_img_txt.retrieval import retrieval_topk
    b, d, k = 64, 32, 5
    torch.manual_seed(17)
    critic = make_mlp(2 * d, [64, 256]).to(DEV)
    gen = torch.Generator().manual_seed(18)
    x, y = torch.randn(b, d, generator=gen).to(DEV), torch.randn(b, d, generator=gen).to(DEV)
    sid = torch.arange(b, dtype=torch.int64) // 2
    _, scores = mi_critics.fused_mi_bound(x, y, sid.to(DEV), critic, return_scores=True)  # the kernel's own scores
    got = retrieval_topk(x, y, critic, k)
    want = ref.both_directions(scores.cpu(), k)
    for d_ in ("i2t", "t2i"):
        _assert_same(got[d_], want[d_], d_)
    got = retrieval_topk(x, y, critic, k, img_ids=sid, txt_ids=sid)  # the hard negatives
    want = ref.both_directions(scores.cpu(), k, sid, sid)
    for d_ in ("i2t", "t2i"):
        _assert_same(got[d_], want[d_], d_)
        assert bool((sid[got[d_][0].cpu().long()] != sid[:, None]).all())
    with pytest.raises(ValueError, match="matrix_topk"):
        retrieval_topk(x, y[:48], make_mlp(2 * d, [64, 256]).to(DEV), k)


def test_gallery_eval_runs():
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.retrieval import gallery_recall, retrieval_topk
    n_img, n_txt, d = 96, 64, 32
    gen = torch.Generator().manual_seed(9)
    y = torch.nn.functional.normalize(torch.randn(n_txt, d, generator=gen), dim=1)
    txt_ids = [f"study{n}" for n in range(n_txt)]
    img_ids = [f"study{n % n_txt}" for n in range(n_img)]          # studies 0 .. 31 have two images
    x = y[[n % n_txt for n in range(n_img)]] + 0.01 * torch.randn(n_img, d, generator=gen)
    mgr = MultiModalManager(d_img=d, d_txt=d, critic="bilinear")
    with torch.no_grad():
        mgr.mi_discriminator.weight.copy_(torch.eye(d))
    mgr.mi_discriminator.to(DEV)
    ev = mgr.gallery_eval(x.to(DEV), img_ids, y.to(DEV), txt_ids, ks=(1, 5), precision="f32_exact")
    assert set(ev) == {"i2t", "t2i"} and set(ev["i2t"]) == {"recall@1", "recall@5", "mrr"}
    top = retrieval_topk(x.to(DEV), y.to(DEV), mgr.mi_discriminator, 5, "f32_exact")
    assert ev == {"i2t": gallery_recall(top["i2t"][0], img_ids, txt_ids, (1, 5)),
                  "t2i": gallery_recall(top["t2i"][0], txt_ids, img_ids, (1, 5))}
    # S = <x, y> with x a noisy copy of its report: each image finds its report, each report one of its images
    assert ev["i2t"]["recall@1"] == 1.0 and ev["t2i"]["recall@1"] == 1.0 and ev["i2t"]["mrr"] == 1.0


# ------------------------------------------------------------------------------------------------ 5. rounded scores
RANDN_SHAPES = [(200, 257, 64), (96, 1000, 128), (512, 512, 256)]  # generic path, 16-bit chain, 16-bit chain
RANDN_KS = (1, 10, 16)
F32_GRADE = ("f32", "f32_exact", "bf16x3")


def _bf16_round(t):
    return t.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def _randn_case(n_img, n_txt, d):
    """Inputs, ids and the two fp64 references (plain; bf16-rounded X, W, Y, T), computed once and left unchanged."""
    gen = torch.Generator().manual_seed(n_img + n_txt + d)
    x, y = torch.randn(n_img, d, generator=gen), torch.randn(n_txt, d, generator=gen)
    w = torch.randn(d, d, generator=gen) / math.sqrt(d)
    img_ids = torch.arange(n_img, dtype=torch.int64) // 2
    txt_ids = torch.arange(n_txt, dtype=torch.int64) % (n_img // 2 + 3)
    plain = _scores64("bilinear", x, y, [w])
    rounded = _scores64("bilinear", x, y, [w], _bf16_round)
    return x, y, w, img_ids, txt_ids, plain, rounded


def _tau(s_ref, precision):
    return (2e-3 if precision == "bf16" else 1e-4) * max(1.0, float(s_ref.abs().max()))


def band_mean(s_ref, q_ids, g_ids, k, tau):
    """Mean over the queries (rows of s_ref) of the number of candidates within 2 tau of the k-th score, the k-th itself
    not counted."""
    s = s_ref.masked_fill(q_ids[:, None] == g_ids[None, :], NEG_INF)
    t_k = torch.sort(s, dim=1, descending=True).values[:, k - 1:k]
    return float((((s - t_k).abs() <= 2 * tau).sum(dim=1) - 1).double().mean())


def _check_direction(got, s_ref, q_ids, g_ids, k, tau, cap, what):
    idx, val = got[0].cpu().long(), got[1].cpu().double()
    n_q, n_g = s_ref.shape
    assert idx.shape == (n_q, k) and val.shape == (n_q, k), what
    excl = q_ids[:, None] == g_ids[None, :]
    assert int((~excl).sum(dim=1).min()) >= k  # (these ids leave every query at least k candidates: no tail)
    s = s_ref.masked_fill(excl, NEG_INF)
    t_k = torch.sort(s, dim=1, descending=True).values[:, k - 1:k]
    band = float((((s - t_k).abs() <= 2 * tau).sum(dim=1) - 1).double().mean())
    print(f"{what}: tau {tau:.3e}, mean band {band:.4f} (cap {cap})")
    assert band <= cap, (what, band)
    # indices in range, distinct, not excluded
    assert int(idx.min()) >= 0 and int(idx.max()) < n_g, what
    present = torch.zeros(n_q, n_g, dtype=torch.int64).scatter_add_(1, idx, torch.ones_like(idx))
    assert int(present.max()) == 1, what
    assert not bool(excl.gather(1, idx).any()), what
    # val non-increasing, and the score of idx within tau
    assert bool((val[:, 1:] <= val[:, :-1]).all()), what
    s_at = s_ref.gather(1, idx)
    err = float((val - s_at).abs().max())
    print(f"{what}: max |val - S_ref[idx]| {err:.3e}")
    assert err <= tau, (what, err, tau)
    # everything clearly above the k-th score is there; nothing clearly below it is
    must = s > t_k + 2 * tau
    assert bool((present[must] == 1).all()), what
    assert bool((s_at >= t_k - 2 * tau).all()), what


@pytest.mark.parametrize("precision", ["f32", "f32_exact", "bf16x3", "bf16"])
@pytest.mark.parametrize("shape", RANDN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_topk_on_randn_within_the_score_band(shape, precision):
    from mutual_info_img_txt.model import BilinearCritic
    from mutual_info_img_txt.retrieval import retrieval_topk
    x, y, w, img_ids, txt_ids, plain, rounded = _randn_case(*shape)
    s_ref = rounded if precision == "bf16" else plain
    tau, cap = _tau(s_ref, precision), (4.0 if precision == "bf16" else 0.5)
    critic = BilinearCritic(shape[2], shape[2])
    with torch.no_grad():
        critic.weight.copy_(w)
    critic = critic.to(DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    for k in RANDN_KS:
        got = retrieval_topk(xd, yd, critic, k, precision, img_ids, txt_ids)
        _check_direction(got["i2t"], s_ref, img_ids, txt_ids, k, tau, cap, (shape, precision, k, "i2t"))
        _check_direction(got["t2i"], s_ref.t().contiguous(), txt_ids, img_ids, k, tau, cap, (shape, precision, k, "t2i"))
