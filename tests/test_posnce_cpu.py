"""CPU-side checks of the study-positive InfoNCE: the symbols and signatures of the C ABI, the
workspace queries, every MI_EINVAL / MI_EWORKSPACE case through ctypes (all rejected before a launch), the fp64
restatement (tests/posnce_reference.py) against a brute-force double loop, the closed-form gradient and nce_reference,
and the argument validation of the Python layer, the manager and train.py.  No GPU needed."""
import ctypes
import inspect
import math

import pytest
import torch

import posnce_reference as ref

NEW_SYMBOLS = ("mi_posnce_bilinear_workspace_bytes", "mi_posnce_bilinear_step", "mi_posnce_separable_workspace_bytes",
               "mi_posnce_separable_step", "mi_matrix_posnce_workspace_bytes", "mi_matrix_posnce_fwd",
               "mi_matrix_posnce_bwd")
F32, BF16, BF16X3, FP8, F16, F16X3 = range(6)
ROWWISE, SYMMETRIC = 0, 1
# the id patterns of the B = 7 checks: unique, one pair, one group of 3 that is not adjacent, all equal
IDS7 = {"unique": list("abcdefg"), "pair": list("abcbdef"), "group3": list("abcadae"), "equal": ["a"] * 7}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_signatures(lib):
    from mutual_info_img_txt import _hip
    P, I64, I, SZ = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    sig = _hip.SIGNATURES
    # the step signatures are those of mi_nce_*_step plus the optional int32 [b] n_pos_out behind lse_cols
    nce = sig["mi_nce_bilinear_step"][1]
    assert sig["mi_posnce_bilinear_step"] == (I, nce[:13] + [P] + nce[13:])
    nce = sig["mi_nce_separable_step"][1]
    assert sig["mi_posnce_separable_step"] == (I, nce[:15] + [P] + nce[15:])
    assert sig["mi_posnce_bilinear_workspace_bytes"] == (SZ, [I64, I64, I64, I, I])
    assert sig["mi_posnce_separable_workspace_bytes"] == (SZ, [I64, I64, I64, I64, I, I])
    assert sig["mi_matrix_posnce_workspace_bytes"] == (SZ, [I64])
    assert sig["mi_matrix_posnce_fwd"] == (I, [P, P, I64, I, P, P, P, P, P, SZ, P])
    assert sig["mi_matrix_posnce_bwd"] == (I, [P, P, I64, I, P, P, P, P, P, P])
    assert lib.mi_abi_version() == 4


def test_estimator_table_unchanged():
    from mutual_info_img_txt import _hip
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
    assert sorted(_hip.NCE_ESTIMATORS) == ["infonce_rowwise", "infonce_symmetric"]


@pytest.mark.parametrize("precision", [F32, BF16, BF16X3])
def test_workspace_queries(lib, precision):
    b, d = 4096, 512
    fwd = lib.mi_posnce_bilinear_workspace_bytes(b, d, d, precision, 0)
    full = lib.mi_posnce_bilinear_workspace_bytes(b, d, d, precision, 1)
    assert 0 < fwd < full
    assert full >= 2 * b * b and full - fwd >= 2 * b * b            # the forward-only query holds no G
    # the records: 2 sides x (8-byte NceRec + 8-byte PosRec) per sample and 64-wide tile; O(b) floats besides
    nce = lib.mi_nce_bilinear_workspace_bytes(b, d, d, precision)
    assert full <= nce + 16 * b * (b // 64) + 64 * b + 4096
    # doubling b at most quadruples either query
    for grads in (0, 1):
        one, two = (lib.mi_posnce_bilinear_workspace_bytes(n, d, d, precision, grads) for n in (b, 2 * b))
        assert one < two <= 4 * one
        one, two = (lib.mi_posnce_separable_workspace_bytes(n, 768, 768, d, precision, grads) for n in (b, 2 * b))
        assert one < two <= 4 * one
    s0 = lib.mi_posnce_separable_workspace_bytes(b, 768, 768, d, precision, 0)
    s1 = lib.mi_posnce_separable_workspace_bytes(b, 768, 768, d, precision, 1)
    assert 0 < s0 < s1 and s1 > full
    m1, m2 = lib.mi_matrix_posnce_workspace_bytes(b), lib.mi_matrix_posnce_workspace_bytes(2 * b)
    assert 0 < m1 < m2 <= 4 * m1 and m1 <= 32 * b * (b // 64) + 64 * b + 4096
    # bad sizes: 0
    assert lib.mi_posnce_bilinear_workspace_bytes(0, d, d, precision, 1) == 0
    assert lib.mi_posnce_bilinear_workspace_bytes(b, 0, d, precision, 1) == 0
    assert lib.mi_posnce_separable_workspace_bytes(b, d, d, 0, precision, 1) == 0
    assert lib.mi_matrix_posnce_workspace_bytes(0) == 0


def _bil(lib, p, *, b=64, dx=128, dy=128, mode=SYMMETRIC, precision=BF16, x=True, y=True, sid=True, w=True, loss=True,
         gx=False, gy=False, gw=False, wsp=True, ws=1 << 30):
    """mi_posnce_bilinear_step with a host address standing in for every pointer asked for: the cases below are all
    rejected before anything touches the device."""
    a = lambda on: p if on else None
    return lib.mi_posnce_bilinear_step(a(x), a(y), a(w), a(sid), b, dx, dy, mode, precision, None, a(loss), None, None,
                                       None, a(gx), a(gy), a(gw), a(wsp), ws, None)


def _sep(lib, p, *, b=64, dx=128, dy=96, kp=32, mode=SYMMETRIC, precision=BF16, wg=True, wh=True, loss=True,
         grads=(False,) * 4, ws=1 << 30):
    a = lambda on: p if on else None
    return lib.mi_posnce_separable_step(p, p, a(wg), a(wh), p, b, dx, dy, kp, mode, precision, None, a(loss), None, None,
                                        None, *[a(g) for g in grads], p, ws, None)


def test_every_einval_and_eworkspace_case(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    err = lambda: lib.mi_last_error().decode()
    # bilinear step
    for missing in ("x", "y", "sid", "loss", "wsp"):
        assert _bil(lib, p, **{missing: False}) == -1 and "null" in err(), missing
    for prec in (FP8, F16, F16X3, 6, -1):
        assert _bil(lib, p, precision=prec) == -1 and "precision" in err() and "study-positive" in err(), prec
    for mode in (-1, 2):
        assert _bil(lib, p, mode=mode) == -1 and "mode" in err()
    assert _bil(lib, p, b=0) == -1 and _bil(lib, p, dx=0) == -1 and _bil(lib, p, dy=0) == -1
    assert _bil(lib, p, b=-5) == -1 and "sizes" in err()
    assert _bil(lib, p, b=1 << 31) == -1 and "2^31" in err()
    assert _bil(lib, p, w=False, dx=128, dy=64) == -1 and "d_img == d_txt" in err()
    assert _bil(lib, p, gx=True) == -1 and "grad" in err()                      # some gradients, not all
    assert _bil(lib, p, gx=True, gy=True) == -1 and "grad" in err()              # with w: grad_w as well
    assert _bil(lib, p, w=False, gx=True, gy=True, gw=True) == -1 and "grad" in err()   # without w: no grad_w
    assert _bil(lib, p, ws=1024) == -3 and "workspace too small" in err()        # MI_EWORKSPACE, before any launch
    # a forward-only workspace does not carry a call with gradients
    small = lib.mi_posnce_bilinear_workspace_bytes(64, 128, 128, BF16, 0)
    assert _bil(lib, p, gx=True, gy=True, gw=True, ws=small) == -3 and "workspace too small" in err()
    # separable step
    assert _sep(lib, p, wg=False) == -1 and "null" in err()
    assert _sep(lib, p, wh=False) == -1 and _sep(lib, p, loss=False) == -1
    for prec in (FP8, F16, F16X3):
        assert _sep(lib, p, precision=prec) == -1 and "precision" in err()
    assert _sep(lib, p, mode=2) == -1 and "mode" in err()
    assert _sep(lib, p, kp=0) == -1 and "projection" in err()
    assert _sep(lib, p, b=0) == -1
    assert _sep(lib, p, grads=(True, True, True, False)) == -1 and "gradients" in err()
    assert _sep(lib, p, ws=1024) == -3 and "workspace too small" in err()
    small = lib.mi_posnce_separable_workspace_bytes(64, 128, 96, 32, BF16, 0)
    assert _sep(lib, p, grads=(True,) * 4, ws=small) == -3
    # matrix entry
    fwd = lambda **kw: lib.mi_matrix_posnce_fwd(kw.get("s", p), kw.get("sid", p), kw.get("b", 8), kw.get("mode", SYMMETRIC),
                                                kw.get("loss", p), None, None, None, kw.get("wsp", p),
                                                kw.get("ws", 1 << 20), None)
    for missing in ("s", "sid", "loss", "wsp"):
        assert fwd(**{missing: None}) == -1 and "null" in err(), missing
    assert fwd(b=0) == -1 and fwd(b=1 << 31) == -1 and fwd(mode=2) == -1 and fwd(mode=-1) == -1
    assert fwd(ws=16) == -3 and "workspace too small" in err()
    bwd = lambda **kw: lib.mi_matrix_posnce_bwd(kw.get("s", p), kw.get("sid", p), kw.get("b", 8), kw.get("mode", ROWWISE),
                                                kw.get("r", p), kw.get("c", None), kw.get("n", p), None, kw.get("g", p),
                                                None)
    for missing in ("s", "sid", "r", "n", "g"):
        assert bwd(**{missing: None}) == -1 and "null" in err(), missing
    assert bwd(b=0) == -1 and bwd(mode=3) == -1
    assert bwd(mode=SYMMETRIC) == -1 and "symmetric" in err()                   # needs lse_cols


# ------------------------------------------------------------------------------------------------ the restatement
def _brute(s, sid, estimator):
    """The definition of the issue, element by element."""
    b = len(sid)
    s = s.double()
    pos = [[j for j in range(b) if sid[j] == sid[i]] for i in range(b)]
    r = [math.log(sum(math.exp(s[i, j]) for j in range(b))) for i in range(b)]
    c = [math.log(sum(math.exp(s[i, j]) for i in range(b))) for j in range(b)]
    t_row = [r[i] - sum(float(s[i, p]) for p in pos[i]) / len(pos[i]) for i in range(b)]
    t_col = [c[j] - sum(float(s[p, j]) for p in pos[j]) / len(pos[j]) for j in range(b)]
    wr, wc = (1.0 / b, 0.0) if estimator == "infonce_rowwise" else (0.5 / b, 0.5 / b)
    loss = sum(wr * t_row[i] + wc * t_col[i] for i in range(b))
    g = torch.zeros(b, b, dtype=torch.float64)
    for i in range(b):
        for j in range(b):
            g[i, j] = wr * math.exp(s[i, j] - r[i]) + wc * math.exp(s[i, j] - c[j])
            if sid[i] == sid[j]:
                g[i, j] -= (wr + wc) / len(pos[i])
    return loss, r, c, [len(q) for q in pos], g, t_row


@pytest.mark.parametrize("ids", sorted(IDS7))
def test_reference_against_brute_force_and_closed_form(ids):
    b = 7
    s = torch.randn(b, b, generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 2.0
    sid = IDS7[ids]
    for est in ref.MODES:
        o = ref.matrix_case(s, sid, est)
        loss, r, c, n, g, t_row = _brute(s, sid, est)
        assert abs(float(o["loss"]) - loss) < 1e-12
        assert torch.allclose(o["lse_rows"], torch.tensor(r, dtype=torch.float64), atol=1e-12, rtol=0)
        assert torch.allclose(o["lse_cols"], torch.tensor(c, dtype=torch.float64), atol=1e-12, rtol=0)
        assert o["n_pos"].tolist() == n and o["n_pos"].dtype == torch.int32
        assert torch.allclose(o["grad"], g, atol=1e-14, rtol=0)                       # autograd against the loop
        assert torch.allclose(ref.grad_scores_closed(s, sid, est), g, atol=1e-14, rtol=0)   # and the closed form
        if ids == "equal":   # t_i = r_i - mean_j S[i, j] >= log B: not zero
            assert all(t >= math.log(b) for t in t_row) and float(o["loss"]) >= math.log(b)
    # each row's share of the row-wise gradient sums to zero
    g_row = ref.grad_scores(s, sid, "infonce_rowwise")
    assert float(g_row.sum(dim=1).abs().max()) < 1e-15
    assert float(ref.grad_scores_closed(s, sid, "infonce_rowwise").sum(dim=1).abs().max()) < 1e-15


def test_reference_equals_nce_reference_on_unique_ids():
    import nce_reference as nce
    b = 12
    s = torch.randn(b, b, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2.0
    sid = [str(n) for n in range(b)]
    for est in ref.MODES:
        o, full = ref.matrix_case(s, sid, est), nce.matrix_case(s, sid, est)
        assert abs(float(o["loss"] - full["loss"])) < 1e-12
        for n in ("lse_rows", "lse_cols", "grad"):
            assert torch.allclose(o[n], full[n], atol=1e-12, rtol=0), (est, n)
    # ... and differs from it once ids repeat (the pairs enter the denominators and share the positive weight)
    sid[5] = sid[2]
    assert abs(float(ref.matrix_case(s, sid, "infonce_symmetric")["loss"] -
                     nce.matrix_case(s, sid, "infonce_symmetric")["loss"])) > 1e-3


def test_reference_single_sample_and_rounded_variant():
    s = torch.tensor([[3.25]], dtype=torch.float64)
    for est in ref.MODES:
        o = ref.matrix_case(s, ["a"], est)
        assert float(o["loss"]) == 0.0 and float(o["grad"].abs().max()) == 0.0 and o["n_pos"].tolist() == [1]
    # rounded=True rounds x, y, W, T, G and dT to bf16: bf16-exact operands leave only T, G and dT to differ
    gen = torch.Generator().manual_seed(3)
    x, y, w = torch.randn(9, 8, generator=gen), torch.randn(9, 6, generator=gen), torch.randn(8, 6, generator=gen) * 0.3
    sid = list("aabcdefgc")
    plain, rnd = ref.bilinear_case(x, y, w, sid, "infonce_symmetric"), ref.bilinear_case(x, y, w, sid, "infonce_symmetric", True)
    assert 0.0 < abs(float(plain["loss"] - rnd["loss"])) < 0.1
    auto = ref.step(lambda a, c, ww: (a @ ww) @ c.t(), [x, y, w], sid, "infonce_symmetric")
    assert abs(float(auto["loss"] - plain["loss"])) < 1e-12
    for got, want in zip(auto["grads"], (plain["dx"], plain["dy"], plain["dw"])):
        assert torch.allclose(got, want, atol=1e-13, rtol=0)


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_validation_without_gpu():
    from mutual_info_img_txt import study_positives as sp
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import BilinearCritic
    x, y, sid = torch.zeros(4, 8), torch.zeros(4, 8), list("abcd")
    with pytest.raises(MiCriticError):                     # CPU tensors raise as everywhere else
        sp.study_positive_infonce(x, y, sid, BilinearCritic(8, 8))
    with pytest.raises(MiCriticError):
        sp.matrix_study_positive_infonce(torch.zeros(4, 4), sid)
    for doc in (sp.__doc__, sp.study_positive_infonce.__doc__, sp.matrix_study_positive_infonce.__doc__):
        assert "not a" in " ".join(doc.lower().split()) and "bound" in doc   # the documentation duty of the issue
    assert "NOT A MUTUAL-INFORMATION BOUND" in sp.__doc__
    for phrase in ("unique ids", "denominators", "share the positive weight", "not zero", "exactly 0.0", "sums to zero",
                   "averaged-outside"):
        assert phrase in " ".join(sp.__doc__.split()), phrase
    for name in ("return_stats", "symmetric", "precision"):
        assert name in inspect.signature(sp.study_positive_infonce).parameters
    assert inspect.signature(sp.study_positive_infonce).parameters["symmetric"].default is True


def test_ops_layer_has_the_entry_points():
    from mutual_info_img_txt import critic_ops
    for cls in (critic_ops.HipBilinearOps, critic_ops.HipSeparableOps):
        for name in ("posnce_workspace_bytes", "posnce_call", "posnce_step"):
            assert callable(getattr(cls, name)), (cls, name)
    assert "posnce_step" in vars(critic_ops._HipOps)        # the shared step
    assert callable(critic_ops.posnce_matrix_fwd) and callable(critic_ops.posnce_matrix_bwd)


def test_not_an_estimator_name_and_no_graphed_or_sharded_form():
    from mutual_info_img_txt import _hip, distributed, graphed
    for name in ("study_positive_infonce", "posnce", "infonce_positives", "supcon"):
        with pytest.raises(ValueError, match="unknown mi_estimator"):
            _hip.check_estimator(name)
    for fn in (graphed.GraphedMiStep.__init__, distributed.global_batch_mi_bound, distributed.GlobalBatchGraphStep.__init__):
        assert "study_positives" not in inspect.signature(fn).parameters, fn


def test_manager_validation():
    from mutual_info_img_txt.main_utils import MultiModalManager
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            m = MultiModalManager(d_img=8, d_txt=8, critic=critic, d_proj=4, mi_estimator=est, study_positives=True)
            assert m.study_positives is True
    assert MultiModalManager(d_img=8, d_txt=8, critic="bilinear").study_positives is False
    assert MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric",
                             hard_negatives=4).study_positives is False
    for est in (None, "dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="study_positives"):
            MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator=est, study_positives=True)
    with pytest.raises(ValueError):                        # the make_mlp critic has no per-sample InfoNCE step
        MultiModalManager(d_img=8, d_txt=8, critic="concat_mlp", hidden_dims=(8, 8), mi_estimator="infonce_symmetric",
                          study_positives=True)
    with pytest.raises(ValueError, match="hard_negatives"):
        MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", study_positives=True,
                          hard_negatives=4)
    with pytest.raises(ValueError, match="memory_bank"):
        MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", study_positives=True,
                          memory_bank=64)
    # a manager built for one form does not quietly train another
    m = MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", study_positives=True)
    with pytest.raises(ValueError, match="study-positive"):
        m.mi_step(torch.zeros(4, 8), torch.zeros(4, 8), list("abcd"), "infonce_rowwise")


def test_train_py_validation():
    import train
    parse = lambda *a: train.check_training_parameters(train.construct_training_parameters(list(a)))
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            assert parse("--synthetic", "--critic", critic, "--mi_estimator", est, "--study_positives").study_positives is True
    assert parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric").study_positives is False
    for est in ("dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="--study_positives"):
            parse("--synthetic", "--critic", "bilinear", "--mi_estimator", est, "--study_positives")
    with pytest.raises(ValueError):
        parse("--synthetic", "--critic", "concat_mlp", "--mi_estimator", "infonce_symmetric", "--study_positives")
    with pytest.raises(ValueError, match="cannot be combined"):
        parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", "--study_positives",
              "--hard_negatives", "8")
    with pytest.raises(ValueError, match="cannot be combined"):
        parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", "--study_positives",
              "--memory_bank", "64")
