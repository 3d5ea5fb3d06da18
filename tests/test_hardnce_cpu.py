"""CPU-side checks of the hard-negative InfoNCE: the symbols and signatures of the C ABI, the
workspace queries, every MI_EINVAL case through ctypes (all rejected before a launch), the fp64 restatement
(tests/hardnce_reference.py) against a brute-force loop, and the argument validation of the Python layer, the manager
and train.py.  No GPU needed."""
import ctypes
import inspect
import math

import pytest
import torch

import hardnce_reference as ref

NEW_SYMBOLS = ("mi_hardnce_bilinear_workspace_bytes", "mi_hardnce_bilinear_step", "mi_hardnce_separable_workspace_bytes",
               "mi_hardnce_separable_step", "mi_matrix_hardnce_workspace_bytes", "mi_matrix_hardnce_fwd",
               "mi_matrix_hardnce_bwd")
F32, BF16, BF16X3, FP8, F16, F16X3 = range(6)
ROWWISE, SYMMETRIC = 0, 1


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
    # the step signatures are those of mi_nce_*_step plus `int k` and the two optional int32 [b, k] list outputs
    nce = sig["mi_nce_bilinear_step"][1]
    assert sig["mi_hardnce_bilinear_step"] == (I, nce[:9] + [I] + nce[9:13] + [P, P] + nce[13:])
    nce = sig["mi_nce_separable_step"][1]
    assert sig["mi_hardnce_separable_step"] == (I, nce[:11] + [I] + nce[11:15] + [P, P] + nce[15:])
    assert sig["mi_hardnce_bilinear_workspace_bytes"] == (SZ, [I64, I64, I64, I, I, I])
    assert sig["mi_hardnce_separable_workspace_bytes"] == (SZ, [I64, I64, I64, I64, I, I, I])
    assert sig["mi_matrix_hardnce_workspace_bytes"] == (SZ, [I64, I])
    assert lib.mi_abi_version() == 4
    assert _hip.MI_TOPK_MAX_K == 32


def test_estimator_table_unchanged():
    from mutual_info_img_txt import _hip
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
    assert sorted(_hip.NCE_ESTIMATORS) == ["infonce_rowwise", "infonce_symmetric"]


@pytest.mark.parametrize("precision", [F32, BF16, BF16X3])
def test_workspace_queries(lib, precision):
    b, d = 8192, 512
    fwd = [lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, precision, k, 0) for k in range(1, 33)]
    full = [lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, precision, k, 1) for k in range(1, 33)]
    assert all(a < c for a, c in zip(fwd, fwd[1:])) and all(a < c for a, c in zip(full, full[1:]))  # monotone in k
    # per unit of k: 8-byte keys, 4-byte idx and 4-byte val of both sides' lists
    assert fwd[1] - fwd[0] == 16 * 2 * b and full[9] - full[8] == 16 * 2 * b
    # forward only: linear in b -- no G, no score matrix: doubling b at most doubles it (a term c b^2 would add 2 c b^2)
    k = 10
    f1, f2 = (lib.mi_hardnce_bilinear_workspace_bytes(n, d, d, precision, k, 0) for n in (b, 2 * b))
    assert f2 <= 2 * f1
    # with gradients: the nce step's G and G^T, nothing of that order on top
    g1 = lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, precision, k, 1)
    nce = lib.mi_nce_bilinear_workspace_bytes(b, d, d, precision)
    assert g1 >= 2 * b * b and g1 <= nce + 16 * 2 * b * k + 16 * b + 4096
    # the separable step: the same plus the projections and their gradients
    s0 = lib.mi_hardnce_separable_workspace_bytes(b, 768, 768, d, precision, k, 0)
    s1 = lib.mi_hardnce_separable_workspace_bytes(b, 768, 768, d, precision, k, 1)
    assert 0 < lib.mi_hardnce_separable_workspace_bytes(2 * b, 768, 768, d, precision, k, 0) <= 2 * s0 and s1 > g1
    # the matrix entry: lists and O(b) floats
    assert lib.mi_matrix_hardnce_workspace_bytes(b, k) <= 16 * 2 * b * k + 16 * b + 4096
    assert lib.mi_matrix_hardnce_workspace_bytes(b, 11) > lib.mi_matrix_hardnce_workspace_bytes(b, 10)
    # bad sizes: 0
    assert lib.mi_hardnce_bilinear_workspace_bytes(0, d, d, precision, k, 1) == 0
    assert lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, precision, 0, 1) == 0
    assert lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, precision, 33, 1) == 0
    assert lib.mi_hardnce_separable_workspace_bytes(b, d, d, 0, precision, k, 1) == 0
    assert lib.mi_matrix_hardnce_workspace_bytes(b, 33) == 0 and lib.mi_matrix_hardnce_workspace_bytes(0, 3) == 0


def _bil(lib, p, *, b=64, dx=128, dy=128, mode=SYMMETRIC, precision=BF16, k=5, x=True, w=True, loss=True, gx=False,
         gy=False, gw=False, ws=1 << 30):
    """mi_hardnce_bilinear_step with a host address standing in for every pointer asked for: the cases below are all
    rejected before anything touches the device."""
    a = lambda on: p if on else None
    return lib.mi_hardnce_bilinear_step(a(x), p, a(w), p, b, dx, dy, mode, precision, k, None, a(loss), None, None, None,
                                        None, a(gx), a(gy), a(gw), p, ws, None)


def _sep(lib, p, *, b=64, dx=128, dy=96, kp=32, mode=SYMMETRIC, precision=BF16, k=5, wg=True, grads=(False,) * 4,
         ws=1 << 30):
    a = lambda on: p if on else None
    return lib.mi_hardnce_separable_step(p, p, a(wg), p, p, b, dx, dy, kp, mode, precision, k, None, p, None, None, None,
                                         None, *[a(g) for g in grads], p, ws, None)


def test_every_einval_case(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    err = lambda: lib.mi_last_error().decode()
    # bilinear step
    assert _bil(lib, p, x=False) == -1 and "null" in err()
    assert _bil(lib, p, loss=False) == -1 and "null" in err()
    for k in (0, -1, 33, 1000):
        assert _bil(lib, p, k=k) == -1 and "k must be in [1, 32]" in err(), k
    for prec in (FP8, F16, F16X3, 6, -1):
        assert _bil(lib, p, precision=prec) == -1 and "precision" in err() and "hard-negative" in err(), prec
    for mode in (-1, 2):
        assert _bil(lib, p, mode=mode) == -1 and "mode" in err()
    assert _bil(lib, p, b=0) == -1 and _bil(lib, p, dx=0) == -1 and _bil(lib, p, dy=0) == -1
    assert _bil(lib, p, w=False, dx=128, dy=64) == -1 and "d_img == d_txt" in err()
    assert _bil(lib, p, gx=True) == -1 and "grad" in err()                      # some gradients, not all
    assert _bil(lib, p, gx=True, gy=True) == -1 and "grad" in err()              # with w: grad_w as well
    assert _bil(lib, p, w=False, gx=True, gy=True, gw=True) == -1 and "grad" in err()   # without w: no grad_w
    assert _bil(lib, p, ws=1024) == -3 and "workspace too small" in err()        # MI_EWORKSPACE, before any launch
    # a forward-only workspace does not carry a call with gradients
    small = lib.mi_hardnce_bilinear_workspace_bytes(64, 128, 128, BF16, 5, 0)
    assert _bil(lib, p, gx=True, gy=True, gw=True, ws=small) == -3
    # separable step
    assert _sep(lib, p, wg=False) == -1 and "null" in err()
    for k in (0, 33):
        assert _sep(lib, p, k=k) == -1 and "k must be in [1, 32]" in err()
    for prec in (FP8, F16, F16X3):
        assert _sep(lib, p, precision=prec) == -1 and "precision" in err()
    assert _sep(lib, p, mode=2) == -1 and _sep(lib, p, kp=0) == -1
    assert _sep(lib, p, grads=(True, True, True, False)) == -1 and "gradients" in err()
    assert _sep(lib, p, ws=1024) == -3
    # matrix entry
    fwd = lambda **kw: lib.mi_matrix_hardnce_fwd(kw.get("s", p), p, kw.get("b", 8), kw.get("mode", SYMMETRIC),
                                                 kw.get("k", 3), p, None, None, None, None, p, kw.get("ws", 1 << 20), None)
    assert fwd(s=None) == -1 and "null" in err()
    assert fwd(b=0) == -1 and fwd(mode=2) == -1
    for k in (0, 33):
        assert fwd(k=k) == -1 and "k must be in [1, 32]" in err()
    assert fwd(ws=16) == -3
    bwd = lambda **kw: lib.mi_matrix_hardnce_bwd(p, kw.get("b", 8), kw.get("mode", ROWWISE), kw.get("k", 3),
                                                 kw.get("ir", p), kw.get("ic", None), kw.get("r", p), kw.get("c", None),
                                                 None, kw.get("g", p), None)
    assert bwd(ir=None) == -1 and "null" in err()
    assert bwd(r=None) == -1 and bwd(g=None) == -1
    assert bwd(b=0) == -1 and bwd(mode=3) == -1 and bwd(k=0) == -1 and bwd(k=33) == -1
    assert bwd(mode=SYMMETRIC) == -1 and "symmetric" in err()                   # needs idx_cols and lse_cols
    assert bwd(mode=SYMMETRIC, ic=p) == -1 and bwd(mode=SYMMETRIC, c=p) == -1


# ------------------------------------------------------------------------------------------------ the restatement
def _brute(s, sid, k, estimator):
    """The definition of the issue, element by element."""
    b = len(sid)
    s = s.double()

    def hard(get, q):
        cand = [j for j in range(b) if sid[j] != sid[q]]
        # score descending, then index ascending; -0.0 as +0.0
        cand.sort(key=lambda j: (-(float(get(q, j)) + 0.0), j))
        return cand[:k]

    rows = [hard(lambda i, j: s[i, j], i) for i in range(b)]
    cols = [hard(lambda j, i: s[i, j], j) for j in range(b)]
    r = [math.log(math.exp(s[i, i]) + sum(math.exp(s[i, j]) for j in rows[i])) for i in range(b)]
    c = [math.log(math.exp(s[j, j]) + sum(math.exp(s[i, j]) for i in cols[j])) for j in range(b)]
    wr, wc = (1.0 / b, 0.0) if estimator == "infonce_rowwise" else (0.5 / b, 0.5 / b)
    loss = sum(wr * (r[i] - float(s[i, i])) + wc * (c[i] - float(s[i, i])) for i in range(b))
    g = torch.zeros(b, b, dtype=torch.float64)
    for i in range(b):
        for j in range(b):
            d = 1.0 if i == j else 0.0
            if j in rows[i] or i == j:
                g[i, j] += wr * (math.exp(s[i, j] - r[i]) - d)
            if wc and (i in cols[j] or i == j):
                g[i, j] += wc * (math.exp(s[i, j] - c[j]) - d)
    return loss, r, c, g, rows, cols


@pytest.mark.parametrize("ids", ["unique", "dup", "equal"])
@pytest.mark.parametrize("k", [1, 3, 32])
def test_reference_against_brute_force(ids, k):
    b = 7
    gen = torch.Generator().manual_seed(7 + k)
    s = torch.round(torch.randn(b, b, generator=gen, dtype=torch.float64) * 4.0) / 4.0  # quarter steps: ties
    s[2, 5] = -0.0
    s[2, 3] = 0.0
    sid = {"unique": list("abcdefg"), "dup": list("aabcdde"), "equal": ["a"] * b}[ids]
    for est in ref.MODES:
        o = ref.matrix_case(s, sid, k, est)
        loss, r, c, g, rows, cols = _brute(s, sid, k, est)
        assert o["idx_rows"].shape == (b, k) and o["idx_cols"].shape == (b, k)
        for q in range(b):
            assert [v for v in o["idx_rows"][q].tolist() if v >= 0] == rows[q]
            assert [v for v in o["idx_cols"][q].tolist() if v >= 0] == cols[q]
            n = len(rows[q])
            assert o["idx_rows"][q, n:].tolist() == [-1] * (k - n)      # the tail
        assert abs(float(o["loss"]) - loss) < 1e-12
        assert torch.allclose(o["lse_rows"], torch.tensor(r, dtype=torch.float64), atol=1e-12, rtol=0)
        assert torch.allclose(o["lse_cols"], torch.tensor(c, dtype=torch.float64), atol=1e-12, rtol=0)
        assert torch.allclose(o["grad"], g, atol=1e-14, rtol=0)
        if ids == "equal":
            assert float(o["loss"]) == 0.0 and float(o["grad"].abs().max()) == 0.0
        # the gradient is the derivative of the loss with the selection held constant (autograd through the fp64 loss)
        sl = s.clone().requires_grad_(True)
        ref.loss(sl, o["idx_rows"], o["idx_cols"], est).backward()
        assert torch.allclose(sl.grad, o["grad"], atol=1e-14, rtol=0)


def test_reference_reduces_to_the_full_loss():
    """k >= every row's and column's negative count: the per-sample InfoNCE of tests/nce_reference.py."""
    import nce_reference as nce
    b = 12
    s = torch.randn(b, b, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2.0
    sid = [str(n // 2) if n < 4 else str(n) for n in range(b)]
    for est in ref.MODES:
        o, full = ref.matrix_case(s, sid, 32, est), nce.matrix_case(s, sid, est)
        assert abs(float(o["loss"] - full["loss"])) < 1e-12
        assert torch.allclose(o["grad"], full["grad"], atol=1e-14, rtol=0)


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_validation_without_gpu():
    from mutual_info_img_txt import hard_negatives as hn
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import BilinearCritic
    x, y, sid = torch.zeros(4, 8), torch.zeros(4, 8), list("abcd")
    with pytest.raises(MiCriticError):                     # CPU tensors raise as everywhere else
        hn.hard_negative_infonce(x, y, sid, BilinearCritic(8, 8), 2)
    with pytest.raises(MiCriticError):
        hn.matrix_hard_negative_infonce(torch.zeros(4, 4), sid, 2)
    for k in (0, 33, -3, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            hn.check_k(k)
    assert hn.check_k(1) == 1 and hn.check_k(32) == 32
    for doc in (hn.__doc__, hn.hard_negative_infonce.__doc__, hn.matrix_hard_negative_infonce.__doc__):
        assert "not a" in " ".join(doc.lower().split()) and "bound" in doc   # the documentation duty of the issue
    assert "NOT A MUTUAL-INFORMATION BOUND" in hn.__doc__


def test_not_an_estimator_name_and_no_graphed_or_sharded_form():
    from mutual_info_img_txt import _hip, distributed, graphed
    for name in ("hard_negative_infonce", "hardnce", "infonce_hard"):
        with pytest.raises(ValueError, match="unknown mi_estimator"):
            _hip.check_estimator(name)
    for fn in (graphed.GraphedMiStep.__init__, distributed.global_batch_mi_bound, distributed.GlobalBatchGraphStep.__init__):
        names = set(inspect.signature(fn).parameters)
        assert not names & {"hard_negatives", "k", "hard_k"}, (fn, names)


def test_manager_validation():
    from mutual_info_img_txt.main_utils import MultiModalManager
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            m = MultiModalManager(d_img=8, d_txt=8, critic=critic, d_proj=4, mi_estimator=est, hard_negatives=8)
            assert m.hard_negatives == 8
    assert MultiModalManager(d_img=8, d_txt=8, critic="bilinear").hard_negatives is None
    for est in (None, "dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="hard_negatives"):
            MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator=est, hard_negatives=8)
    with pytest.raises(ValueError):                        # the make_mlp critic has no per-sample InfoNCE step
        MultiModalManager(d_img=8, d_txt=8, critic="concat_mlp", hidden_dims=(8, 8), mi_estimator="infonce_symmetric",
                          hard_negatives=8)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k must be"):
            MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", hard_negatives=k)
    # a manager built for one form does not quietly train another
    m = MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", hard_negatives=4)
    with pytest.raises(ValueError, match="hard-negative"):
        m.mi_step(torch.zeros(4, 8), torch.zeros(4, 8), list("abcd"), "infonce_rowwise")


def test_train_py_validation():
    import train
    parse = lambda *a: train.check_training_parameters(train.construct_training_parameters(list(a)))
    args = parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", "--hard_negatives", "8")
    assert args.hard_negatives == 8
    assert parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric").hard_negatives is None
    with pytest.raises(ValueError, match="--hard_negatives"):
        parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "dv", "--hard_negatives", "8")
    with pytest.raises(ValueError):
        parse("--synthetic", "--critic", "concat_mlp", "--mi_estimator", "infonce_symmetric", "--hard_negatives", "8")
    for k in ("0", "33"):
        with pytest.raises(ValueError, match="k must be"):
            parse("--synthetic", "--critic", "separable", "--mi_estimator", "infonce_rowwise", "--hard_negatives", k)
