"""CPU-side checks of the soft-target InfoNCE from finding-label bit masks: the symbols and
signatures of the C ABI, the workspace queries, every MI_EINVAL / MI_EWORKSPACE case through ctypes (all rejected before
a launch), the fp64 restatement (tests/softnce_reference.py) against a brute-force double loop, the closed-form gradient,
the properties of the loss against posnce_reference, the label conversions and the label-table reader, and the argument
validation of the Python layer, the manager and train.py.  No GPU needed."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import posnce_reference as pos
import softnce_reference as ref

NEW_SYMBOLS = ("mi_softnce_bilinear_workspace_bytes", "mi_softnce_bilinear_step", "mi_softnce_separable_workspace_bytes",
               "mi_softnce_separable_step", "mi_matrix_softnce_workspace_bytes", "mi_matrix_softnce_fwd",
               "mi_matrix_softnce_bwd")
F32, BF16, BF16X3, FP8, F16, F16X3 = range(6)
ROWWISE, SYMMETRIC = 0, 1
NAN, INF = float("nan"), float("inf")
# the mask patterns of the B = 7 checks: 14 random findings, sets that differ above bit 31 only, no finding at all, all
# equal, one bit per study (two studies with two samples)
MASKS7 = {"random14": [0x2a51, 0x0003, 0x2a51, 0x1ff0, 0x0000, 0x3001, 0x0810],
          "high": [(1 << 62) | 1, (1 << 40) | 1, (1 << 62) | (1 << 40) | 1, 1, (1 << 33) | 1, (1 << 62) | 1, 1 << 32],
          "empty": [0] * 7, "equal": [0x15] * 7, "study": [1, 2, 1, 4, 8, 2, 16]}
TAU_MIX = ((0.5, 0.3), (0.05, 1.0), (2.0, 1.0))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_signatures(lib):
    from mutual_info_img_txt import _hip
    P, I64, I, SZ, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    sig = _hip.SIGNATURES
    # the step signatures are those of mi_posnce_*_step with (tau, mix) behind the precision; target_norm takes the place
    # of n_pos_out
    posn = sig["mi_posnce_bilinear_step"][1]
    assert sig["mi_softnce_bilinear_step"] == (I, posn[:9] + [F, F] + posn[9:])
    posn = sig["mi_posnce_separable_step"][1]
    assert sig["mi_softnce_separable_step"] == (I, posn[:11] + [F, F] + posn[11:])
    assert sig["mi_softnce_bilinear_workspace_bytes"] == (SZ, [I64, I64, I64, I, I])
    assert sig["mi_softnce_separable_workspace_bytes"] == (SZ, [I64, I64, I64, I64, I, I])
    assert sig["mi_matrix_softnce_workspace_bytes"] == (SZ, [I64])
    assert sig["mi_matrix_softnce_fwd"] == (I, [P, P, I64, I, F, F, P, P, P, P, P, SZ, P])
    assert sig["mi_matrix_softnce_bwd"] == (I, [P, P, I64, I, F, F, P, P, P, P, P, P])
    assert lib.mi_abi_version() == 4
    assert _hip.MI_SOFTNCE_MAX_LABELS == 63
    header = open(inspect.getfile(_hip).replace("_hip.py", "../../include/mi_critic.h")).read()
    assert "#define MI_SOFTNCE_MAX_LABELS 63" in header
    assert "A TRAINING LOSS, NOT AN MI BOUND" in header.split("soft-target InfoNCE", 1)[1]


def test_estimator_table_unchanged_and_no_graphed_or_sharded_form():
    from mutual_info_img_txt import _hip, distributed, graphed
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
    assert sorted(_hip.NCE_ESTIMATORS) == ["infonce_rowwise", "infonce_symmetric"]
    for name in ("soft_target_infonce", "softnce", "infonce_soft", "softclip"):
        with pytest.raises(ValueError, match="unknown mi_estimator"):
            _hip.check_estimator(name)
    for fn in (graphed.GraphedMiStep.__init__, distributed.global_batch_mi_bound, distributed.GlobalBatchGraphStep.__init__):
        for name in ("soft_targets", "soft_tau", "soft_mix", "labels"):
            assert name not in inspect.signature(fn).parameters, (fn, name)
    for mod in (graphed, distributed):
        assert not [n for n in dir(mod) if "soft" in n.lower()], mod


@pytest.mark.parametrize("precision", [F32, BF16, BF16X3])
def test_workspace_queries(lib, precision):
    b, d = 4096, 512
    fwd = lib.mi_softnce_bilinear_workspace_bytes(b, d, d, precision, 0)
    full = lib.mi_softnce_bilinear_workspace_bytes(b, d, d, precision, 1)
    assert 0 < fwd < full
    assert full >= 2 * b * b and full - fwd >= 2 * b * b            # the forward-only query holds no G
    # the records: 2 sides x (8-byte NceRec + 4-byte share) per sample and 64-wide tile; O(b) floats besides
    nce = lib.mi_nce_bilinear_workspace_bytes(b, d, d, precision)
    assert full <= nce + 8 * b * (b // 64) + 64 * b + 4096
    # monotone in b; doubling b at most quadruples either query
    for grads in (0, 1):
        one, two = (lib.mi_softnce_bilinear_workspace_bytes(n, d, d, precision, grads) for n in (b, 2 * b))
        assert one < two <= 4 * one
        one, two = (lib.mi_softnce_separable_workspace_bytes(n, 768, 768, d, precision, grads) for n in (b, 2 * b))
        assert one < two <= 4 * one
    # forward only: linear in b but for the records (24 bytes per sample and 64-wide tile), so far below one b x b slot
    # of 16-bit G where b is large
    for n in (16384, 65536):
        lin = lib.mi_softnce_bilinear_workspace_bytes(n, d, d, precision, 0) - 24 * n * (n // 64)
        assert 0 < lin <= 64 * n * d + (1 << 20) and lin + 24 * n * (n // 64) < 2 * n * n
    one, two = (lib.mi_softnce_bilinear_workspace_bytes(n, d, d, precision, 0) - 24 * n * (n // 64) for n in (b, 2 * b))
    assert two <= 2 * one + 8192
    s0 = lib.mi_softnce_separable_workspace_bytes(b, 768, 768, d, precision, 0)
    s1 = lib.mi_softnce_separable_workspace_bytes(b, 768, 768, d, precision, 1)
    assert 0 < s0 < s1 and s1 > full
    m1, m2 = lib.mi_matrix_softnce_workspace_bytes(b), lib.mi_matrix_softnce_workspace_bytes(2 * b)
    assert 0 < m1 < m2 <= 4 * m1 and m1 <= 24 * b * (b // 64) + 64 * b + 4096
    # bad sizes: 0
    assert lib.mi_softnce_bilinear_workspace_bytes(0, d, d, precision, 1) == 0
    assert lib.mi_softnce_bilinear_workspace_bytes(b, 0, d, precision, 1) == 0
    assert lib.mi_softnce_bilinear_workspace_bytes(b, d, -1, precision, 0) == 0
    assert lib.mi_softnce_separable_workspace_bytes(b, d, d, 0, precision, 1) == 0
    assert lib.mi_softnce_separable_workspace_bytes(-2, d, d, 8, precision, 1) == 0
    assert lib.mi_matrix_softnce_workspace_bytes(0) == 0 and lib.mi_matrix_softnce_workspace_bytes(-1) == 0


def _bil(lib, p, *, b=64, dx=128, dy=128, mode=SYMMETRIC, precision=BF16, tau=0.5, mix=0.5, x=True, y=True, lab=True,
         w=True, loss=True, gx=False, gy=False, gw=False, wsp=True, ws=1 << 30):
    """mi_softnce_bilinear_step with a host address standing in for every pointer asked for: the cases below are all
    rejected before anything touches the device."""
    a = lambda on: p if on else None
    return lib.mi_softnce_bilinear_step(a(x), a(y), a(w), a(lab), b, dx, dy, mode, precision, tau, mix, None, a(loss), None,
                                        None, None, a(gx), a(gy), a(gw), a(wsp), ws, None)


def _sep(lib, p, *, b=64, dx=128, dy=96, kp=32, mode=SYMMETRIC, precision=BF16, tau=0.5, mix=0.5, wg=True, wh=True,
         lab=True, loss=True, grads=(False,) * 4, ws=1 << 30):
    a = lambda on: p if on else None
    return lib.mi_softnce_separable_step(p, p, a(wg), a(wh), a(lab), b, dx, dy, kp, mode, precision, tau, mix, None,
                                         a(loss), None, None, None, *[a(g) for g in grads], p, ws, None)


BAD_TAU = (0.0, -0.5, NAN, INF, -INF)
BAD_MIX = (-0.01, 1.01, NAN, INF)


def test_every_einval_and_eworkspace_case(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    err = lambda: lib.mi_last_error().decode()
    # bilinear step
    for missing in ("x", "y", "lab", "loss", "wsp"):
        assert _bil(lib, p, **{missing: False}) == -1 and "null" in err(), missing
    for prec in (FP8, F16, F16X3, 6, -1):
        assert _bil(lib, p, precision=prec) == -1 and "precision" in err() and "soft-target" in err(), prec
    for mode in (-1, 2):
        assert _bil(lib, p, mode=mode) == -1 and "mode" in err()
    assert _bil(lib, p, b=0) == -1 and _bil(lib, p, dx=0) == -1 and _bil(lib, p, dy=0) == -1
    assert _bil(lib, p, b=-5) == -1 and "sizes" in err()
    assert _bil(lib, p, b=1 << 31) == -1 and "2^31" in err()
    for tau in BAD_TAU:
        assert _bil(lib, p, tau=tau) == -1 and "tau" in err(), tau
    for mix in BAD_MIX:
        assert _bil(lib, p, mix=mix) == -1 and "mix" in err(), mix
    assert _bil(lib, p, w=False, dx=128, dy=64) == -1 and "d_img == d_txt" in err()
    assert _bil(lib, p, gx=True) == -1 and "grad" in err()                      # some gradients, not all
    assert _bil(lib, p, gx=True, gy=True) == -1 and "grad" in err()              # with w: grad_w as well
    assert _bil(lib, p, w=False, gx=True, gy=True, gw=True) == -1 and "grad" in err()   # without w: no grad_w
    assert _bil(lib, p, ws=1024) == -3 and "workspace too small" in err()        # MI_EWORKSPACE, before any launch
    # a forward-only workspace does not carry a call with gradients
    small = lib.mi_softnce_bilinear_workspace_bytes(64, 128, 128, BF16, 0)
    assert _bil(lib, p, gx=True, gy=True, gw=True, ws=small) == -3 and "workspace too small" in err()
    # separable step
    assert _sep(lib, p, wg=False) == -1 and "null" in err()
    assert _sep(lib, p, wh=False) == -1 and _sep(lib, p, loss=False) == -1 and _sep(lib, p, lab=False) == -1
    for prec in (FP8, F16, F16X3):
        assert _sep(lib, p, precision=prec) == -1 and "precision" in err()
    assert _sep(lib, p, mode=2) == -1 and "mode" in err()
    assert _sep(lib, p, kp=0) == -1 and "projection" in err()
    assert _sep(lib, p, b=0) == -1 and _sep(lib, p, b=1 << 31) == -1
    for tau in BAD_TAU:
        assert _sep(lib, p, tau=tau) == -1 and "tau" in err(), tau
    for mix in BAD_MIX:
        assert _sep(lib, p, mix=mix) == -1 and "mix" in err(), mix
    assert _sep(lib, p, grads=(True, True, True, False)) == -1 and "gradients" in err()
    assert _sep(lib, p, ws=1024) == -3 and "workspace too small" in err()
    small = lib.mi_softnce_separable_workspace_bytes(64, 128, 96, 32, BF16, 0)
    assert _sep(lib, p, grads=(True,) * 4, ws=small) == -3
    # matrix entry
    fwd = lambda **kw: lib.mi_matrix_softnce_fwd(kw.get("s", p), kw.get("lab", p), kw.get("b", 8),
                                                 kw.get("mode", SYMMETRIC), kw.get("tau", 0.5), kw.get("mix", 0.5),
                                                 kw.get("loss", p), None, None, None, kw.get("wsp", p),
                                                 kw.get("ws", 1 << 20), None)
    for missing in ("s", "lab", "loss", "wsp"):
        assert fwd(**{missing: None}) == -1 and "null" in err(), missing
    assert fwd(b=0) == -1 and fwd(b=1 << 31) == -1 and fwd(mode=2) == -1 and fwd(mode=-1) == -1
    for tau in BAD_TAU:
        assert fwd(tau=tau) == -1 and "tau" in err(), tau
    for mix in BAD_MIX:
        assert fwd(mix=mix) == -1 and "mix" in err(), mix
    assert fwd(ws=16) == -3 and "workspace too small" in err()
    bwd = lambda **kw: lib.mi_matrix_softnce_bwd(kw.get("s", p), kw.get("lab", p), kw.get("b", 8), kw.get("mode", ROWWISE),
                                                 kw.get("tau", 0.5), kw.get("mix", 0.5), kw.get("r", p), kw.get("c", None),
                                                 kw.get("z", p), None, kw.get("g", p), None)
    for missing in ("s", "lab", "r", "g"):
        assert bwd(**{missing: None}) == -1 and "null" in err(), missing
    assert bwd(z=None) == -1 and "target_norm" in err()                          # the forward's z is required
    assert bwd(b=0) == -1 and bwd(b=1 << 31) == -1 and bwd(mode=3) == -1
    for tau in BAD_TAU:
        assert bwd(tau=tau) == -1 and "tau" in err(), tau
    for mix in BAD_MIX:
        assert bwd(mix=mix) == -1 and "mix" in err(), mix
    assert bwd(mode=SYMMETRIC) == -1 and "symmetric" in err()                   # needs lse_cols


# ------------------------------------------------------------------------------------------------ the restatement
def _brute(s, masks, estimator, tau, mix):
    """The definition of the issue, element by element."""
    b = len(masks)
    s = s.double()
    n = [bin(m).count("1") for m in masks]
    k = [[1.0 if i == j else
          math.exp(((bin(masks[i] & masks[j]).count("1") / math.sqrt(n[i] * n[j]) if n[i] * n[j] else 0.0) - 1.0) / tau)
          for j in range(b)] for i in range(b)]
    z = [sum(k[i]) for i in range(b)]
    qr = [[(1.0 - mix) * (i == j) + mix * k[i][j] / z[i] for j in range(b)] for i in range(b)]
    qc = [[(1.0 - mix) * (i == j) + mix * k[i][j] / z[j] for j in range(b)] for i in range(b)]
    r = [math.log(sum(math.exp(s[i, j]) for j in range(b))) for i in range(b)]
    c = [math.log(sum(math.exp(s[i, j]) for i in range(b))) for j in range(b)]
    t_row = [r[i] - sum(qr[i][j] * float(s[i, j]) for j in range(b)) for i in range(b)]
    t_col = [c[j] - sum(qc[i][j] * float(s[i, j]) for i in range(b)) for j in range(b)]
    wr, wc = (1.0 / b, 0.0) if estimator == "infonce_rowwise" else (0.5 / b, 0.5 / b)
    loss = sum(wr * t_row[i] + wc * t_col[i] for i in range(b))
    g = torch.zeros(b, b, dtype=torch.float64)
    for i in range(b):
        for j in range(b):
            g[i, j] = wr * (math.exp(s[i, j] - r[i]) - qr[i][j]) + wc * (math.exp(s[i, j] - c[j]) - qc[i][j])
    return loss, r, c, z, g, k


@pytest.mark.parametrize("pattern", sorted(MASKS7))
def test_reference_against_brute_force_and_closed_form(pattern):
    b = 7
    s = torch.randn(b, b, generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 2.0
    masks = MASKS7[pattern]
    for tau, mix in TAU_MIX:
        for est in ref.MODES:
            o = ref.matrix_case(s, masks, est, tau, mix)
            loss, r, c, z, g, k = _brute(s, masks, est, tau, mix)
            assert abs(float(o["loss"]) - loss) < 1e-12
            assert torch.allclose(o["lse_rows"], torch.tensor(r, dtype=torch.float64), atol=1e-12, rtol=0)
            assert torch.allclose(o["lse_cols"], torch.tensor(c, dtype=torch.float64), atol=1e-12, rtol=0)
            assert torch.allclose(o["target_norm"], torch.tensor(z, dtype=torch.float64), atol=1e-13, rtol=0)
            assert torch.allclose(ref.kernel(masks, tau), torch.tensor(k, dtype=torch.float64), atol=1e-15, rtol=0)
            assert torch.allclose(o["grad"], g, atol=1e-14, rtol=0)                       # autograd against the loop
            assert torch.allclose(ref.grad_scores_closed(s, masks, est, tau, mix), g, atol=1e-14, rtol=0)  # closed form
        qr, qc, z = ref.targets(masks, tau, mix)
        assert torch.allclose(qr.sum(dim=1), torch.ones(b, dtype=torch.float64), atol=1e-14, rtol=0)
        assert torch.allclose(qc.sum(dim=0), torch.ones(b, dtype=torch.float64), atol=1e-14, rtol=0)
        assert torch.equal(ref.kernel(masks, tau), ref.kernel(masks, tau).t()) and float(z.min()) >= 1.0
        # each row's share of the row-wise gradient sums to zero
        g_row = ref.grad_scores(s, masks, "infonce_rowwise", tau, mix)
        assert float(g_row.sum(dim=1).abs().max()) < 1e-15
        assert float(ref.grad_scores_closed(s, masks, "infonce_rowwise", tau, mix).sum(dim=1).abs().max()) < 1e-15


def test_high_bits_count_and_bit_63_is_ignored():
    # sets that differ only above bit 31: a 32-bit truncation would make them equal
    masks = MASKS7["high"]
    k = ref.kernel(masks, 0.5)
    assert float(k[0, 1]) < 1.0 and float(k[0, 5]) == 1.0            # {62, 0} vs {40, 0}; {62, 0} twice
    assert abs(float(k[0, 1]) - math.exp((1.0 / 2.0 - 1.0) / 0.5)) < 1e-15
    assert abs(float(k[0, 2]) - math.exp((2.0 / math.sqrt(6.0) - 1.0) / 0.5)) < 1e-15
    signed = [m - (1 << 64) if m >> 63 else m for m in [m | (1 << 63) for m in masks]]   # bit 63 set: negative int64
    assert torch.equal(ref.kernel(signed, 0.5), k)


def test_properties_against_the_study_positive_reference():
    b = 12
    s = torch.randn(b, b, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2.0
    unique = [str(n) for n in range(b)]
    masks = MASKS7["random14"] + MASKS7["high"][:5]
    for est in ref.MODES:
        # mix = 0: the study-positive / per-sample InfoNCE on unique ids, whatever the masks and tau.  Difference 0.0
        o, p = ref.matrix_case(s, masks, est, 0.3, 0.0), pos.matrix_case(s, unique, est)
        assert float(o["loss"] - p["loss"]) == 0.0 and torch.equal(o["grad"], p["grad"])
        assert torch.equal(o["lse_rows"], p["lse_rows"]) and torch.equal(o["lse_cols"], p["lse_cols"])
        # every mask equal and mix = 1: all ids equal, t_i = r_i - mean_j S[i, j]
        for tau in (0.05, 2.0):
            o, p = ref.matrix_case(s, [0x15] * b, est, tau, 1.0), pos.matrix_case(s, ["a"] * b, est)
            assert abs(float(o["loss"] - p["loss"])) < 1e-14 and torch.allclose(o["grad"], p["grad"], atol=1e-16, rtol=0)
            assert torch.equal(o["target_norm"], torch.full((b,), float(b), dtype=torch.float64))
        # one distinct bit per study, mix = 1, tau = 0.02 (exp(-50) = 1.9e-22, a normal fp32 number): those study ids
        study = [0, 1, 0, 2, 3, 1, 4, 0, 5, 6, 7, 7]
        o = ref.matrix_case(s, [1 << (5 * v) for v in study], est, 0.02, 1.0)
        p = pos.matrix_case(s, [str(v) for v in study], est)
        assert abs(float(o["loss"] - p["loss"])) < 1e-15 and torch.allclose(o["grad"], p["grad"], atol=1e-18, rtol=0)
        assert torch.allclose(o["target_norm"], p["n_pos"].double(), atol=1e-18, rtol=0)
    assert 1e-22 < math.exp(-1.0 / 0.02) < 2e-22 and math.exp(-1.0 / 0.02) > torch.finfo(torch.float32).tiny
    # all masks zero: uniform smoothing of weight exp(-1 / tau) off the diagonal
    tau, mix = 0.5, 0.3
    qr, qc, z = ref.targets([0] * b, tau, mix)
    e = math.exp(-1.0 / tau)
    assert torch.allclose(z, torch.full((b,), 1.0 + (b - 1) * e, dtype=torch.float64), atol=1e-14, rtol=0)
    off = mix * e / (1.0 + (b - 1) * e)
    want = torch.full((b, b), off, dtype=torch.float64)
    want.fill_diagonal_(1.0 - mix + mix / (1.0 + (b - 1) * e))
    assert torch.allclose(qr, want, atol=1e-15, rtol=0) and torch.allclose(qc, want, atol=1e-15, rtol=0)
    # the loss never falls below the mean entropy of its targets
    for t, m in TAU_MIX:
        assert float(ref.loss(s, masks, "infonce_rowwise", t, m)) >= ref.mean_target_entropy(masks, t, m)


def test_reference_single_sample_and_rounded_variant():
    s = torch.tensor([[3.25]], dtype=torch.float64)
    for est in ref.MODES:
        for tau, mix in TAU_MIX:
            o = ref.matrix_case(s, [5], est, tau, mix)
            assert float(o["loss"]) == 0.0 and float(o["grad"].abs().max()) == 0.0 and o["target_norm"].tolist() == [1.0]
    # rounded=True rounds x, y, W, T, G and dT to bf16: bf16-exact operands leave only T, G and dT to differ
    gen = torch.Generator().manual_seed(3)
    x, y, w = torch.randn(9, 8, generator=gen), torch.randn(9, 6, generator=gen), torch.randn(8, 6, generator=gen) * 0.3
    masks, (tau, mix) = MASKS7["random14"] + [3, 0x2a51], (0.5, 0.7)
    plain = ref.bilinear_case(x, y, w, masks, "infonce_symmetric", tau, mix)
    rnd = ref.bilinear_case(x, y, w, masks, "infonce_symmetric", tau, mix, True)
    assert 0.0 < abs(float(plain["loss"] - rnd["loss"])) < 0.1
    auto = ref.step(lambda a, c, ww: (a @ ww) @ c.t(), [x, y, w], masks, "infonce_symmetric", tau, mix)
    assert abs(float(auto["loss"] - plain["loss"])) < 1e-12
    for got, want in zip(auto["grads"], (plain["dx"], plain["dy"], plain["dw"])):
        assert torch.allclose(got, want, atol=1e-13, rtol=0)
    wg, wh = torch.randn(8, 4, generator=gen), torch.randn(6, 4, generator=gen)
    sep = ref.separable_case(x, y, wg, wh, masks, "infonce_rowwise", tau, mix)
    auto = ref.step(lambda a, c, g, h: (a @ g) @ (c @ h).t(), [x, y, wg, wh], masks, "infonce_rowwise", tau, mix)
    for got, want in zip(auto["grads"], (sep["dx"], sep["dy"], sep["dwg"], sep["dwh"])):
        assert torch.allclose(got, want, atol=1e-13, rtol=0)


# ------------------------------------------------------------------------------------------------ labels
def test_label_masks_conversions_and_rejections():
    from mutual_info_img_txt import soft_targets as st
    hot = torch.tensor([[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    for t in (hot, hot.bool(), hot.float(), hot.numpy(), hot.numpy().astype(bool), hot.tolist(), hot.to(torch.uint8)):
        m = st.label_masks(t)
        assert m.dtype == torch.int64 and m.tolist() == [5, 0, 15]
    wide = torch.zeros(2, 63, dtype=torch.bool)
    wide[0, 62] = wide[0, 0] = wide[1, 32] = True
    assert st.label_masks(wide).tolist() == [(1 << 62) | 1, 1 << 32]
    ready = torch.tensor([0, 7, (1 << 62) | 3], dtype=torch.int64)
    assert torch.equal(st.label_masks(ready), ready)
    assert st.label_masks(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError, match="at most 63"):
        st.label_masks(torch.zeros(2, 64, dtype=torch.bool))
    for bad in (torch.tensor([[0.5, 1.0]]), torch.tensor([[2, 0]]), torch.tensor([[-1, 1]]), np.array([[0.0, NAN]])):
        with pytest.raises(ValueError, match="0 and 1"):
            st.label_masks(bad)
    with pytest.raises(ValueError, match="non-negative"):
        st.label_masks(torch.tensor([3, -1], dtype=torch.int64))
    with pytest.raises(TypeError, match="int64"):
        st.label_masks(torch.tensor([3, 1], dtype=torch.int32))
    with pytest.raises(ValueError):
        st.label_masks(torch.zeros(2, 3, 4))


def test_load_label_table(tmp_path):
    from mutual_info_img_txt import mi_critics, soft_targets as st
    path = tmp_path / "labels.csv"
    path.write_text("subject_id,study_id,Atelectasis,Cardiomegaly,No Finding,Support Devices\n"
                    "10000032,50414267,1.0,,0,-1\n"
                    "10000032,s53189527,,-1.0,1,1.0\n"
                    "10000764,57375967,,,,\n"
                    "\n"
                    "10000898,not-a-number,0.0,1,0.0,-1.0\n")
    t = st.load_label_table(path)
    assert t == {"50414267": 0b0001, "53189527": 0b1100, "57375967": 0, st.label_key("not-a-number"): 0b0010}
    t = st.load_label_table(str(path), uncertain_positive=True)
    assert t["50414267"] == 0b1001 and t["53189527"] == 0b1110 and t[st.label_key("not-a-number")] == 0b1010
    # keys: the normalisation of study_id_codes, so the folder name, the bare string and the integer meet
    assert st.label_key("s50414267") == st.label_key("50414267") == st.label_key(50414267) == "50414267"
    assert st.label_key(torch.tensor(50414267)) == "50414267"
    assert int(st.label_key("s50414267")) == int(mi_critics.study_id_codes(["50414267"], "cpu")[0])
    assert st.label_key("not-a-number") == str(int(mi_critics.study_id_codes(["not-a-number"], "cpu")[0]))
    # more than 63 findings, no study_id column, a cell that is no number
    many = tmp_path / "many.csv"
    many.write_text("study_id," + ",".join(f"f{n}" for n in range(64)) + "\n1," + ",".join(["1"] * 64) + "\n")
    with pytest.raises(ValueError, match="at most 63"):
        st.load_label_table(many)
    ok = tmp_path / "ok.csv"
    ok.write_text("study_id,subject_id," + ",".join(f"f{n}" for n in range(63)) + "\n9,1," + ",".join(["1"] * 63) + "\n")
    assert st.load_label_table(ok) == {"9": (1 << 63) - 1}
    noid = tmp_path / "noid.csv"
    noid.write_text("subject_id,Atelectasis\n1,1\n")
    with pytest.raises(ValueError, match="study_id"):
        st.load_label_table(noid)
    bad = tmp_path / "bad.csv"
    bad.write_text("study_id,Atelectasis\n1,yes\n")
    with pytest.raises(ValueError, match="line 2"):
        st.load_label_table(bad)


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_validation_without_gpu():
    from mutual_info_img_txt import fused_scores, soft_targets as st
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import BilinearCritic
    x, y, lab = torch.zeros(4, 8), torch.zeros(4, 8), torch.tensor([1, 2, 3, 0])
    with pytest.raises(MiCriticError):                     # CPU tensors raise as everywhere else
        st.soft_target_infonce(x, y, lab, BilinearCritic(8, 8), tau=0.5, mix=0.5)
    with pytest.raises(MiCriticError):
        st.matrix_soft_target_infonce(torch.zeros(4, 4), lab, tau=0.5, mix=0.5)
    # tau and mix are required keywords
    for fn in (st.soft_target_infonce, st.matrix_soft_target_infonce, fused_scores.concat_soft_target_infonce):
        params = inspect.signature(fn).parameters
        for name in ("tau", "mix"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is inspect.Parameter.empty
        assert params["symmetric"].default is True and "return_stats" in params
    assert "precision" in inspect.signature(st.soft_target_infonce).parameters
    with pytest.raises(TypeError):
        st.matrix_soft_target_infonce(torch.zeros(4, 4), lab)
    for tau, mix in ((0.0, 0.5), (-1.0, 0.5), (NAN, 0.5), (INF, 0.5), (0.5, -0.1), (0.5, 1.1), (0.5, NAN)):
        with pytest.raises(ValueError, match="tau|mix"):
            st.check_tau_mix(tau, mix)
    assert st.check_tau_mix(2, 1) == (2.0, 1.0)
    for doc in (st.__doc__, st.soft_target_infonce.__doc__, st.matrix_soft_target_infonce.__doc__):
        assert "not a" in " ".join(doc.lower().split()) and "bound" in doc   # the documentation duty of the issue
    assert "NOT A MUTUAL-INFORMATION BOUND" in st.__doc__
    for phrase in ("unique ids", "Every mask equal", "One distinct bit per study", "exactly 0.0", "sums to zero",
                   "uniform smoothing", "thresholds them", "out of scope", "no graphed and no sharded"):
        assert phrase in " ".join(st.__doc__.split()), phrase
    assert "concat_soft_target_infonce" in fused_scores.__all__


def test_ops_layer_has_the_entry_points():
    from mutual_info_img_txt import critic_ops
    for cls in (critic_ops.HipBilinearOps, critic_ops.HipSeparableOps):
        for name in ("softnce_workspace_bytes", "softnce_call", "softnce_step"):
            assert callable(getattr(cls, name)), (cls, name)
    assert "softnce_step" in vars(critic_ops._HipOps)        # the shared step
    assert callable(critic_ops.softnce_matrix_fwd) and callable(critic_ops.softnce_matrix_bwd)


def test_manager_validation(tmp_path):
    from mutual_info_img_txt.main_utils import MultiModalManager
    table = {"s50000001": 3, 50000002: 5, "50000003": 0}
    kw = dict(d_img=8, d_txt=8, soft_targets=table, soft_tau=0.5, soft_mix=0.3)
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            m = MultiModalManager(critic=critic, d_proj=4, mi_estimator=est, **kw)
            assert m.soft_targets == {"50000001": 3, "50000002": 5, "50000003": 0}
            assert (m.soft_tau, m.soft_mix) == (0.5, 0.3)
    assert MultiModalManager(d_img=8, d_txt=8, critic="bilinear").soft_targets is None
    # the table from a CSV path
    path = tmp_path / "labels.csv"
    path.write_text("study_id,A,B\ns50000001,1,-1\n50000002,,1\n")
    m = MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", d_img=8, d_txt=8, soft_targets=str(path),
                          soft_tau=0.5, soft_mix=1.0)
    assert m.soft_targets == {"50000001": 1, "50000002": 2}
    m = MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", d_img=8, d_txt=8, soft_targets=str(path),
                          soft_tau=0.5, soft_mix=1.0, soft_uncertain_positive=True)
    assert m.soft_targets == {"50000001": 3, "50000002": 2}
    # the lookup: ids in any spelling; an id absent from the table raises, naming it
    assert m.label_masks_of(["50000002", "s50000001", 50000001]).tolist() == [2, 3, 3]
    with pytest.raises(KeyError, match="50000009"):
        m.label_masks_of(["50000002", "s50000009"])
    with pytest.raises(KeyError, match="50000009"):
        m.mi_step(torch.zeros(2, 8), torch.zeros(2, 8), ["50000002", "50000009"], "infonce_symmetric")
    for est in (None, "dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="soft_targets"):
            MultiModalManager(critic="bilinear", mi_estimator=est, **kw)
    with pytest.raises(ValueError):                        # the make_mlp critic has no per-sample InfoNCE step
        MultiModalManager(critic="concat_mlp", hidden_dims=(8, 8), mi_estimator="infonce_symmetric", **kw)
    for other in (dict(hard_negatives=4), dict(memory_bank=64), dict(study_positives=True)):
        with pytest.raises(ValueError, match="cannot be combined"):
            MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", **kw, **other)
    for drop in ("soft_tau", "soft_mix"):                  # both floats are required
        with pytest.raises(ValueError, match="soft_tau and soft_mix"):
            MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", **{k: v for k, v in kw.items() if k != drop})
    for bad in (dict(soft_tau=0.0), dict(soft_tau=NAN), dict(soft_mix=1.5), dict(soft_mix=-0.1)):
        with pytest.raises(ValueError, match="tau|mix"):
            MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", **dict(kw, **bad))
    with pytest.raises(ValueError, match="63 bits"):
        MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", **dict(kw, soft_targets={"1": 1 << 63}))
    with pytest.raises(ValueError, match="soft_targets"):  # the floats without a table
        MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", soft_tau=0.5)
    # a manager built for one form does not quietly train another
    m = MultiModalManager(critic="bilinear", mi_estimator="infonce_symmetric", **kw)
    with pytest.raises(ValueError, match="soft-target"):
        m.mi_step(torch.zeros(2, 8), torch.zeros(2, 8), ["50000001", "50000002"], "infonce_rowwise")


def test_train_py_validation():
    import train
    parse = lambda *a: train.check_training_parameters(train.construct_training_parameters(list(a)))
    soft = ("--soft_targets", "labels.csv", "--soft_tau", "0.5", "--soft_mix", "0.3")
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            a = parse("--synthetic", "--critic", critic, "--mi_estimator", est, *soft)
            assert (a.soft_targets, a.soft_tau, a.soft_mix, a.soft_uncertain_positive) == ("labels.csv", 0.5, 0.3, False)
    assert parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", *soft,
                 "--soft_uncertain_positive").soft_uncertain_positive is True
    assert parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric").soft_targets is None
    for est in ("dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="--soft_targets"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", est, *soft)
    with pytest.raises(ValueError):
        parse("--synthetic", "--critic", "concat_mlp", "--mi_estimator", "infonce_symmetric", *soft)
    for other in (("--hard_negatives", "8"), ("--memory_bank", "64"), ("--study_positives",)):
        with pytest.raises(ValueError, match="cannot be combined"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", *soft, *other)
    for drop in (2, 4):                                    # --soft_tau / --soft_mix missing
        with pytest.raises(ValueError, match="--soft_tau and --soft_mix"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", *soft[:drop], *soft[drop + 2:])
    for bad in (("--soft_tau", "0"), ("--soft_tau", "nan"), ("--soft_mix", "1.5"), ("--soft_mix", "-0.5")):
        with pytest.raises(ValueError, match="tau|mix"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", *soft, *bad)
    for lone in (("--soft_tau", "0.5"), ("--soft_mix", "0.5"), ("--soft_uncertain_positive",)):
        with pytest.raises(ValueError, match="need --soft_targets"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", *lone)
