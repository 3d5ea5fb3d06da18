"""MI estimates on the GPU, against the fp64 restatement in tests/mi_estimates_reference.py.

Tolerances are the project's figures for kernels that see exact fp32 scores (tests/test_fdiv_gpu.py, tests/test_nce_gpu.py):
2e-6 on O(1) values -- scaled by max(1, |S|max) for the log-sum-exp quantities (dv, smile, nce_*) and the score means, by
max(1, |value|) for jsd and log_n_neg -- and RELATIVE 2e-6 max(1, |S|max) for nwj, which grows like e^s.  The chain calls
run on integer-valued operands scaled by a power of two, so T and every score are exact in every precision (checked on
the CPU in the test) and the same figures apply to bf16, bf16x3 and exact fp32 alike.  The comparisons with the existing
steps of the same precision on the same inputs (the accumulators are the same bits, only the order of the sums differs)
take the same figures.
All tests need an MI355X:  python -m pytest tests -m gpu"""
import functools
import math

import pytest
import torch

import mi_estimates_reference as ref
from test_retrieval_gpu import INT_CASES, _ops_and_params, _scores64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAUS = (0.5, 1.0, 5.0, 40.0)
TOL = 2e-6


def _ids(pattern, b):
    """"dup": the pattern of tests/test_posnce_softnce_shard_gpu.py -- a pair inside one tile, a pair in the two far corner
    tiles, a group of five (placed where b allows)."""
    sid = torch.arange(b, dtype=torch.int64) + 100
    if pattern == "dup":
        if b > 3:
            sid[3] = sid[2]
        sid[b - 1] = sid[0]
        if b >= 75:
            sid[70:75] = sid[70]
        elif b >= 9:
            sid[4:9] = sid[4]
    elif pattern == "all_equal":
        sid[:] = 5
    else:
        assert pattern == "unique"
    return sid


def _host(est):
    return est.detach().cpu().double().tolist()


def _check(got, s, sid, taus, what=""):
    """The 12 floats ``got`` (host list) against the fp64 reference of the scores ``s``; prints each error first."""
    from mutual_info_img_txt import _hip
    want = ref.estimates(s, sid, taus)
    smax = max(1.0, float(s.abs().max()))
    rows = [(n, got[slot], want[n]) for slot, n in enumerate(ref.NAMES)]
    rows += [(f"smile[{k}]", got[_hip.MI_EST_SMILE + k], want["smile"][k]) for k in range(len(taus))]
    for name, g, w in rows:
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) if math.isnan(w) else g == w), (what, name, g, w)
            continue
        if name == "nwj":
            tol = TOL * smax * max(1.0, abs(w))
        elif name in ("jsd", "log_n_neg"):
            tol = TOL * max(1.0, abs(w))
        else:
            tol = TOL * smax
        print(f"{what} {name}: got {g:.9g} want {w:.9g} err {abs(g - w):.3g} tol {tol:.3g}")
        assert abs(g - w) <= tol, (what, name, g, w, abs(g - w), tol)
    for k in range(len(taus), _hip.MI_EST_MAX_TAUS):
        assert math.isnan(got[_hip.MI_EST_SMILE + k]), (what, k)
    if int(ref.masks(sid)[1].sum()) == 0:
        assert got[_hip.MI_EST_NCE_I2T] == 0.0 and got[_hip.MI_EST_NCE_T2I] == 0.0, what  # exactly 0
    return want


def _bits(t):
    return t.detach().cpu().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. matrix entry
def _matrix_call(s, sid, taus, fill=float("nan")):
    """mi_estimates_matrix into a pre-filled output and a poisoned workspace."""
    from mutual_info_img_txt import _hip, critic_ops
    b = s.shape[0]
    ws = _hip.workspace(_hip.load().mi_estimates_matrix_workspace_bytes(b), s.device)
    ws.fill_(0xA5)
    est = torch.full((_hip.MI_EST_FLOATS,), fill, dtype=torch.float32, device=s.device)
    _hip.call("mi_estimates_matrix", s.device, s.data_ptr(), sid.data_ptr(), b, critic_ops.estimates_taus(taus), len(taus),
              est.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    return est


@pytest.mark.parametrize("pattern", ["unique", "dup", "all_equal"])
@pytest.mark.parametrize("b", [1, 9, 72, 200, 256, 1100])
def test_matrix_estimates(b, pattern):
    from mutual_info_img_txt.mi_estimates import ESTIMATE_NAMES, matrix_mi_estimates
    gen = torch.Generator().manual_seed(500 + b)
    s = (torch.randn(b, b, generator=gen) * 2.0).float()
    sid = _ids(pattern, b)
    sd, sidd = s.to(DEV), sid.to(DEV)
    est = _matrix_call(sd, sidd, TAUS)
    want = _check(_host(est), s, sid, TAUS, f"matrix b={b} {pattern}")
    if int(ref.masks(sid)[1].sum()) > 0:
        assert not torch.isnan(est).any()  # pre-filled with NaN: every one of the 12 floats was written
        assert abs(_host(est)[11] - want["dv"]) <= TOL * max(1.0, float(s.abs().max()))  # tau = 40 >= max|s|: SMILE is DV
    assert torch.equal(_bits(_matrix_call(sd, sidd, TAUS)), _bits(est))  # identical bits from call to call
    # the Python form: views of one tensor, the same bits
    out = matrix_mi_estimates(sd, sidd, TAUS)
    assert set(out) == set(ESTIMATE_NAMES) | {"smile"}
    for name, slot in ESTIMATE_NAMES.items():
        assert out[name].shape == () and out[name].is_cuda and torch.equal(_bits(out[name].reshape(1)), _bits(est[slot:slot + 1]))
    assert out["smile"].shape == (4,) and torch.equal(_bits(out["smile"]), _bits(est[8:]))
    assert out["dv"].untyped_storage().data_ptr() == out["smile"].untyped_storage().data_ptr()


@pytest.mark.parametrize("b", [9, 200, 1100])
def test_matrix_estimates_without_taus(b):
    gen = torch.Generator().manual_seed(600 + b)
    s = (torch.randn(b, b, generator=gen) * 2.0).float()
    sid = _ids("dup", b)
    est = _matrix_call(s.to(DEV), sid.to(DEV), (), fill=777.0)
    got = _host(est)
    _check(got, s, sid, (), f"matrix b={b} n_tau=0")
    assert all(math.isnan(v) for v in got[8:]) and 777.0 not in got  # the unused clip slots are written too: NaN
    one = _host(_matrix_call(s.to(DEV), sid.to(DEV), (5.0,)))
    _check(one, s, sid, (5.0,), f"matrix b={b} n_tau=1")
    assert one[:8] == got[:8]


def test_matrix_estimates_large_scores():
    """Entries at +-30: every clip is active, jsd stays finite, exp(s) is far outside what a plain sum could carry."""
    b = 200
    gen = torch.Generator().manual_seed(77)
    s = (torch.randn(b, b, generator=gen) * 2.0).float()
    hit = torch.rand(b, b, generator=gen) < 0.02
    s[hit] = torch.where(torch.rand(b, b, generator=gen) < 0.5, 30.0, -30.0)[hit]
    s[5, 5], s[6, 6], s[0, b - 1], s[b - 1, 0] = 30.0, -30.0, 30.0, -30.0
    sid = _ids("dup", b)
    got = _host(_matrix_call(s.to(DEV), sid.to(DEV), TAUS))
    want = _check(got, s, sid, TAUS, "matrix +-30")
    assert all(math.isfinite(v) for v in got)
    assert want["smile"][0] > want["smile"][2] > want["dv"] + 1.0  # the clips at 0.5 and 5 are active
    assert abs(got[11] - got[0]) <= TOL * 30.0                       # the clip at 40 is not


# ------------------------------------------------------------------------------------------------ 2. chain, exact data
def _chain_call(ops, x, y, params, sid, prec, taus, fill=float("nan")):
    """One mi_estimates_<critic> call into a pre-filled output and a poisoned workspace."""
    from mutual_info_img_txt import _hip
    ws = _hip.workspace(ops.estimates_workspace_bytes(x.shape[0], x.shape[1], y.shape[1], params, prec), x.device)
    ws.fill_(0xA5)
    est = torch.full((_hip.MI_EST_FLOATS,), fill, dtype=torch.float32, device=x.device)
    ops.estimates_call(x, y, params, sid, prec, taus, est, ws)()
    torch.cuda.synchronize()
    return est


@functools.lru_cache(maxsize=None)
def _int_case(case):
    """Operands from {-1, 0, 1}, X scaled by the power of two that brings |S|max to at most 16: x, y, params, the fp64
    scores.  T (or A, C) and S are integers times that power of two: exact in bf16 operands with fp32 accumulation."""
    kind, _precision, b, d = case
    gen = torch.Generator().manual_seed(b * 7 + d)

    def draw(r, c):
        return torch.randint(-1, 2, (r, c), generator=gen).float()

    x, y = draw(b, d), draw(b, d)
    _ops, params = _ops_and_params(kind, d, draw)
    s_int = _scores64(kind, x, y, params)
    inner = [x.double() @ params[0].double()] if params else []
    inner += [y.double() @ params[1].double()] if kind == "separable" else []
    assert all(float(t.abs().max()) <= 256.0 for t in inner) and float(s_int.abs().max()) < 2.0 ** 24
    scale = 2.0 ** -max(0, math.ceil(math.log2(float(s_int.abs().max()) / 16.0)))
    x = x * scale
    s = _scores64(kind, x, y, params)
    assert torch.equal(s, s_int * scale) and 4.0 < float(s.abs().max()) <= 16.0
    # the fp64 scores of the bf16-rounded operands (and T, or the projections) equal the unrounded ones
    assert torch.equal(_scores64(kind, x, y, params, rb=lambda t: t.bfloat16().double()), s)
    return x, y, params, s


@pytest.mark.parametrize("pattern", ["unique", "dup", "all_equal"])
@pytest.mark.parametrize("case", INT_CASES, ids=[f"{c}-{p}-{b}x{d}" for c, p, b, d in INT_CASES])
def test_chain_estimates_on_exact_data(case, pattern):
    from mutual_info_img_txt import _hip
    kind, precision, b, d = case
    x, y, params, s = _int_case(case)
    ops, _ = _ops_and_params(kind, d, lambda r, c: torch.zeros(r, c))
    sid = _ids(pattern, b)
    prec = _hip.PRECISIONS[precision]
    xd, yd, pd, sidd = x.to(DEV), y.to(DEV), [p.to(DEV) for p in params], sid.to(DEV)
    est = _chain_call(ops, xd, yd, pd, sidd, prec, TAUS)
    _check(_host(est), s, sid, TAUS, f"{kind} {precision} {b}x{d} {pattern}")
    if pattern != "all_equal":
        assert not torch.isnan(est).any()  # pre-filled with NaN: every one of the 12 floats was written
    assert torch.equal(_bits(_chain_call(ops, xd, yd, pd, sidd, prec, TAUS)), _bits(est))
    # no clips: the unused slots are written (NaN), the rest keeps its bits; the convenience form of the ops objects
    none = _chain_call(ops, xd, yd, pd, sidd, prec, (), fill=777.0)
    assert torch.equal(_bits(none[:8]), _bits(est[:8])) and bool(torch.isnan(none[8:]).all())
    assert torch.equal(_bits(ops.estimates_step(xd, yd, pd, sidd, prec, TAUS)), _bits(est))


# ------------------------------------------------------------------------------------------------ 3. chain, realistic data
@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_exact"])
def test_chain_estimates_agree_with_the_existing_steps(precision):
    """One Gaussian case per precision (256 x 128, "f32" is bf16x3 here): nwj / jsd / dv against -loss of the forward-only
    mi_fdiv step and of the DV chain, nce_* against log b - loss of the mi_nce step at unique ids -- the same precision on
    the same inputs."""
    from mutual_info_img_txt import _hip, mi_critics
    from mutual_info_img_txt.critic_ops import HipBilinearOps
    from mutual_info_img_txt.model import BilinearCritic
    b, d = 256, 128
    gen = torch.Generator().manual_seed(41)
    x, y = torch.randn(b, d, generator=gen).to(DEV), torch.randn(b, d, generator=gen).to(DEV)
    critic = BilinearCritic(d, d).to(DEV)
    with torch.no_grad():
        critic.weight.copy_((torch.randn(d, d, generator=gen) * (1.5 / d)).to(DEV))
    w = critic.weight.detach().contiguous()
    ops = HipBilinearOps()
    prec = _hip.resolve_precision(precision, True, (b, d, d))
    assert prec == {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3, "f32_exact": _hip.MI_PREC_F32}[precision]
    smax = max(1.0, float(((x.double() @ w.double()) @ y.double().t()).abs().max()))
    for pattern in ("unique", "dup"):
        sid = _ids(pattern, b).to(DEV)
        got = _host(ops.estimates_step(x, y, [w], sid, prec, TAUS))
        jsd = float(ops.chain_step("mi_fdiv", x, y, [w], sid, _hip.MI_FDIV_JSD, prec, False)[0])
        nwj = float(ops.chain_step("mi_fdiv", x, y, [w], sid, _hip.MI_FDIV_NWJ, prec, False)[0])
        with torch.no_grad():
            dv = float(mi_critics.fused_mi_bound(x, y, sid, critic, "dv", precision=precision))
        rows = [("jsd", got[_hip.MI_EST_JSD], -jsd, TOL * max(1.0, abs(jsd))),
                ("nwj", got[_hip.MI_EST_NWJ], -nwj, TOL * smax * max(1.0, abs(nwj))),
                ("dv", got[_hip.MI_EST_DV], -dv, TOL * smax)]
        if pattern == "unique":
            row = float(ops.nce_step(x, y, [w], sid, _hip.MI_NCE_ROWWISE, prec, False)[0])
            sym = float(ops.nce_step(x, y, [w], sid, _hip.MI_NCE_SYMMETRIC, prec, False)[0])
            logb = math.log(b)
            rows += [("nce_i2t", got[_hip.MI_EST_NCE_I2T], logb - row, TOL * smax),
                     ("nce mean", 0.5 * (got[_hip.MI_EST_NCE_I2T] + got[_hip.MI_EST_NCE_T2I]), logb - sym, TOL * smax)]
        for name, g, want, tol in rows:
            print(f"{precision} {pattern} {name}: estimates {g:.9g} step {want:.9g} diff {abs(g - want):.3g} tol {tol:.3g}")
            assert abs(g - want) <= tol, (precision, pattern, name, g, want, abs(g - want), tol)
        assert got[_hip.MI_EST_NWJ] <= got[_hip.MI_EST_DV] + TOL * smax and got[11] == pytest.approx(got[0], abs=TOL * smax)


# ------------------------------------------------------------------------------------------------ 4. make_mlp critic
@pytest.mark.parametrize("precision", ["f32", "f32_exact", "bf16", "f16"])
def test_make_mlp_route_equals_the_matrix_call_on_its_fused_scores(precision):
    from mutual_info_img_txt.fused_scores import fused_critic_scores
    from mutual_info_img_txt.mi_estimates import matrix_mi_estimates, mi_estimates
    from mutual_info_img_txt.model import make_mlp
    b, d = 128, 32
    torch.manual_seed(23)
    critic = make_mlp(2 * d, [64, 256]).to(DEV)
    gen = torch.Generator().manual_seed(24)
    x, y = torch.randn(b, d, generator=gen).to(DEV), torch.randn(b, d, generator=gen).to(DEV)
    sid = _ids("dup", b).to(DEV)
    got = mi_estimates(x, y, sid, critic, TAUS, precision)
    with torch.no_grad():
        scores = fused_critic_scores(x, y, critic, precision)
    want = matrix_mi_estimates(scores, sid, TAUS)
    for name in want:
        assert torch.equal(_bits(got[name].reshape(-1)), _bits(want[name].reshape(-1))), (precision, name)
    _check(_host(torch.cat([torch.stack([got[n] for n in ref.NAMES]), got["smile"]])), scores.cpu(), sid.cpu(), TAUS,
           f"make_mlp {precision}")


# ------------------------------------------------------------------------------------------------ 5. Python layer
def test_python_layer_and_manager():
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.mi_estimates import ESTIMATE_NAMES, mi_estimates
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    b, d = 64, 64
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(b, d, generator=gen).to(DEV).requires_grad_(True)
    y = torch.randn(b, d, generator=gen).to(DEV).requires_grad_(True)
    sid = [str(n) for n in range(b)]
    for critic in (BilinearCritic(d, d).to(DEV), SeparableCritic(d, d, 32).to(DEV)):
        out = mi_estimates(x, y, sid, critic)
        assert set(out) == set(ESTIMATE_NAMES) | {"smile"} and out["smile"].shape == (2,)
        for name, v in out.items():
            assert v.is_cuda and v.dtype == torch.float32 and not v.requires_grad and bool(torch.isfinite(v).all()), name
        assert float(out["log_n_neg"]) == pytest.approx(math.log(b * (b - 1)), abs=1e-5)
        two = mi_estimates(x, y, sid, critic)
        assert all(torch.equal(_bits(out[n].reshape(-1)), _bits(two[n].reshape(-1))) for n in out)
        for precision in ("fp8", "f16", "f16x3"):
            with pytest.raises(ValueError):
                mi_estimates(x, y, sid, critic, precision=precision)
    assert x.grad is None and y.grad is None
    mgr = MultiModalManager(d_img=d, d_txt=d, critic="bilinear")
    mgr.mi_discriminator.to(DEV)
    ev = mgr.mi_estimates_eval(x, y, sid, taus=(1.0, 5.0, 20.0), precision="bf16")
    out = mi_estimates(x, y, sid, mgr.mi_discriminator, (1.0, 5.0, 20.0), "bf16")
    assert set(ev) == set(out) and isinstance(ev["dv"], float) and len(ev["smile"]) == 3
    for name in ESTIMATE_NAMES:
        assert ev[name] == float(out[name]), name
    assert ev["smile"] == out["smile"].cpu().tolist()
