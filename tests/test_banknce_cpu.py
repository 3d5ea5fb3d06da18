"""CPU-side checks of the memory-bank InfoNCE: the symbols and signatures of the C ABI, every
MI_EINVAL / MI_EWORKSPACE case through ctypes (all rejected before a launch), the workspace queries (no term quadratic in
the bank size), the fp64 restatement (tests/banknce_reference.py) against a brute-force double loop, the EmbeddingQueue,
and the argument validation of the Python layer, the manager and train.py.  No GPU needed."""
import ctypes
import inspect

import pytest
import torch

import banknce_reference as ref

NEW_SYMBOLS = ("mi_banknce_bilinear_workspace_bytes", "mi_banknce_bilinear_step", "mi_banknce_separable_workspace_bytes",
               "mi_banknce_separable_step")
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
    # the step signatures are those of mi_nce_*_step plus the three bank pointers behind sid and m behind b
    nce = sig["mi_nce_bilinear_step"][1]
    assert sig["mi_banknce_bilinear_step"] == (I, nce[:4] + [P, P, P] + [I64] + [I64] + nce[5:])
    nce = sig["mi_nce_separable_step"][1]
    assert sig["mi_banknce_separable_step"] == (I, nce[:5] + [P, P, P] + [I64] + [I64] + nce[6:])
    assert sig["mi_banknce_bilinear_workspace_bytes"] == (SZ, [I64] * 4 + [I, I, I])
    assert sig["mi_banknce_separable_workspace_bytes"] == (SZ, [I64] * 5 + [I, I, I])
    assert lib.mi_abi_version() == 4


def test_estimator_table_unchanged_and_no_graphed_or_sharded_form():
    from mutual_info_img_txt import _hip, distributed, graphed
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
    assert sorted(_hip.NCE_ESTIMATORS) == ["infonce_rowwise", "infonce_symmetric"]
    for fn in (graphed.GraphedMiStep.__init__, distributed.global_batch_mi_bound, distributed.GlobalBatchGraphStep.__init__):
        names = set(inspect.signature(fn).parameters)
        assert not names & {"memory_bank", "bank", "queue"}, (fn, names)


def _bil(lib, p, *, b=64, m=128, dx=128, dy=128, mode=SYMMETRIC, precision=BF16, x=True, w=True, bank_x=True, bank_y=True,
         bank_sid=True, loss=True, gx=False, gy=False, gw=False, ws=1 << 30):
    """mi_banknce_bilinear_step with a host address standing in for every pointer asked for: the cases below are all
    rejected before anything touches the device."""
    a = lambda on: p if on else None
    return lib.mi_banknce_bilinear_step(a(x), p, a(w), p, a(bank_x), a(bank_y), a(bank_sid), b, m, dx, dy, mode, precision,
                                        None, a(loss), None, None, a(gx), a(gy), a(gw), p, ws, None)


def _sep(lib, p, *, b=64, m=128, dx=128, dy=96, kp=32, mode=SYMMETRIC, precision=BF16, wg=True, bank_x=True, bank_y=True,
         grads=(False,) * 4, ws=1 << 30):
    a = lambda on: p if on else None
    return lib.mi_banknce_separable_step(p, p, a(wg), p, p, a(bank_x), a(bank_y), p, b, m, dx, dy, kp, mode, precision, None,
                                         p, None, None, *[a(g) for g in grads], p, ws, None)


def test_every_einval_case(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    err = lambda: lib.mi_last_error().decode()
    # null required pointers
    for kw in ({"x": False}, {"loss": False}, {"bank_y": False}, {"bank_sid": False}):
        assert _bil(lib, p, **kw) == -1 and "null" in err(), kw
    # sizes
    for kw in ({"b": 0}, {"b": -3}, {"m": 0}, {"m": -1}, {"dx": 0}, {"dy": 0}):
        assert _bil(lib, p, **kw) == -1, kw
    assert _bil(lib, p, b=1 << 30, m=1 << 30) == -1 and "2^31" in err()
    assert _bil(lib, p, b=8, m=(1 << 31) - 8) == -1 and "2^31" in err()
    # the symmetric mode scores the bank's images; the row-wise mode does not read them
    assert _bil(lib, p, bank_x=False) == -1 and "bank_x" in err()
    assert _bil(lib, p, bank_x=False, mode=ROWWISE, ws=1024) == -3   # accepted up to the workspace check
    for mode in (-1, 2):
        assert _bil(lib, p, mode=mode) == -1 and "mode" in err()
    for prec in (FP8, F16, F16X3, 6, -1):
        assert _bil(lib, p, precision=prec) == -1 and "precision" in err() and "memory-bank" in err(), prec
    assert _bil(lib, p, w=False, dx=128, dy=64) == -1 and "d_img == d_txt" in err()
    assert _bil(lib, p, gx=True) == -1 and "grad" in err()                      # a partial gradient set
    assert _bil(lib, p, gx=True, gy=True) == -1 and "grad" in err()              # with w: grad_w as well
    assert _bil(lib, p, w=False, gx=True, gy=True, gw=True) == -1 and "grad" in err()   # without w: no grad_w
    assert _bil(lib, p, ws=1024) == -3 and "workspace too small" in err()        # MI_EWORKSPACE, before any launch
    small = lib.mi_banknce_bilinear_workspace_bytes(64, 128, 128, 128, SYMMETRIC, BF16, 0)
    assert _bil(lib, p, gx=True, gy=True, gw=True, ws=small) == -3               # a forward-only workspace, with gradients
    # separable step
    assert _sep(lib, p, wg=False) == -1 and "null" in err()
    assert _sep(lib, p, bank_y=False) == -1 and "null" in err()
    assert _sep(lib, p, bank_x=False) == -1 and "bank_x" in err()
    assert _sep(lib, p, bank_x=False, mode=ROWWISE, ws=1024) == -3
    for prec in (FP8, F16, F16X3):
        assert _sep(lib, p, precision=prec) == -1 and "precision" in err()
    assert _sep(lib, p, mode=2) == -1 and _sep(lib, p, kp=0) == -1 and _sep(lib, p, m=0) == -1 and _sep(lib, p, b=0) == -1
    assert _sep(lib, p, grads=(True, True, True, False)) == -1 and "gradients" in err()
    assert _sep(lib, p, ws=1024) == -3


@pytest.mark.parametrize("mode", [ROWWISE, SYMMETRIC])
@pytest.mark.parametrize("precision", [F32, BF16, BF16X3])
def test_workspace_queries(lib, precision, mode):
    b, d = 64, 512
    for q, extra in ((lib.mi_banknce_bilinear_workspace_bytes, ()), (lib.mi_banknce_separable_workspace_bytes, (256,))):
        for ms in ((4096, 8192, 16384), (4100, 8196, 16388)):  # the 16-bit chain's sizes and the generic kernels'
            full = [q(b, m, d, d, *extra, mode, precision, 1) for m in ms]
            fwd = [q(b, m, d, d, *extra, mode, precision, 0) for m in ms]
            assert all(0 < f < g for f, g in zip(fwd, full))           # forward only: below the query with gradients
            # no term quadratic in m: doubling m at most doubles the query (a term c m^2 would add 2 c m^2)
            assert full[1] <= 2 * full[0] and full[2] <= 2 * full[1], full
            assert fwd[1] <= 2 * fwd[0] and fwd[2] <= 2 * fwd[1], fwd
        assert q(0, 8, d, d, *extra, mode, precision, 1) == 0 and q(8, 0, d, d, *extra, mode, precision, 1) == 0
    # G is [b, b + m] (and [m, b], symmetric) in the chain's G type, twice (G and G^T): below ONE fp32 (b + m)^2 matrix
    m = 16384
    assert lib.mi_banknce_bilinear_workspace_bytes(b, m, d, d, mode, precision, 1) < 4 * (b + m) * (b + m)


# ------------------------------------------------------------------------------------------------ the restatement
IDS = {"unique": (list("abcde"), list("fghijkl")), "dup_batch": (list("aabcc"), list("fghijkl")),
       "bank_overlap": (list("abcde"), list("afbgchd")), "equal": (["a"] * 5, ["a"] * 7)}


@pytest.mark.parametrize("ids", sorted(IDS))
def test_reference_against_brute_force(ids):
    b, m, d = 5, 7, 6
    gen = torch.Generator().manual_seed(11)
    x, y, w = (torch.randn(n, d, generator=gen, dtype=torch.float64) for n in (b, b, d))
    bx, by = (torch.randn(m, d, generator=gen, dtype=torch.float64) for _ in range(2))
    sid, bsid = IDS[ids]
    t, u = x @ w, bx @ w
    s_top, s_left = t @ torch.cat([y, by]).t(), u @ y.t()
    for est in ref.MODES:
        o = ref.case(x, y, [w], sid, bx, by, bsid, est)
        bf = ref.brute_force(s_top, s_left, sid, bsid, est)
        assert abs(float(o["loss"]) - bf["loss"]) < 1e-12
        assert torch.allclose(o["lse_rows"], torch.tensor(bf["lse_rows"], dtype=torch.float64), atol=1e-12, rtol=0)
        if est == "infonce_symmetric":
            assert torch.allclose(o["lse_cols"], torch.tensor(bf["lse_cols"], dtype=torch.float64), atol=1e-12, rtol=0)
        else:
            assert o["lse_cols"] is None
        if ids == "equal":  # no row or column has a negative
            assert float(o["loss"]) == 0.0 and all(float(g.abs().max()) == 0.0 for g in o["grads"])
        # closed form of the gradients: G_top = dL/dS_top, G_left = dL/dS_left
        sl, ll = s_top.clone().requires_grad_(True), s_left.clone().requires_grad_(True)
        lo = ref.loss_from_scores(sl, ll if est == "infonce_symmetric" else None, sid, bsid, est)["loss"]
        gs = torch.autograd.grad(lo, [sl, ll], allow_unused=True)
        g_top, g_left = gs[0], torch.zeros_like(ll) if gs[1] is None else gs[1]
        dt, du = g_top @ torch.cat([y, by]), g_left @ y
        want = [dt @ w.t(), g_top[:, :b].t() @ t + g_left.t() @ u, x.t() @ dt + bx.t() @ du]
        for got, ww in zip(o["grads"], want):
            assert torch.allclose(got, ww, atol=1e-12, rtol=0)
        assert float(g_top[:, b:].abs().sum()) > 0 or ids == "equal"   # the bank's columns carry gradient
        # the bank is a constant: the restatement never asks for its gradient, and the rounded form is close
        r = ref.case(x, y, [w], sid, bx, by, bsid, est, rounded=True)
        assert abs(float(r["loss"] - o["loss"])) < 0.1


def test_reference_on_an_empty_bank_is_the_per_sample_infonce():
    import nce_reference as nce
    b, d = 9, 5
    gen = torch.Generator().manual_seed(2)
    x, y, w = (torch.randn(n, d, generator=gen, dtype=torch.float64) for n in (b, b, d))
    sid = [str(n // 2) if n < 4 else str(n) for n in range(b)]
    empty = torch.zeros(0, d, dtype=torch.float64)
    for est in ref.MODES:
        o = ref.case(x, y, [w], sid, empty, empty, [], est)
        full = nce.matrix_case((x @ w) @ y.t(), sid, est)
        assert abs(float(o["loss"] - full["loss"])) < 1e-12
        assert torch.allclose(o["lse_rows"], full["lse_rows"], atol=1e-12, rtol=0)
        assert torch.allclose(o["grads"][1], full["grad"].t() @ (x @ w), atol=1e-12, rtol=0)


# ------------------------------------------------------------------------------------------------ EmbeddingQueue
def test_embedding_queue():
    from mutual_info_img_txt.memory_bank import EmbeddingQueue, check_capacity
    from mutual_info_img_txt.mi_critics import study_id_codes
    q = EmbeddingQueue(5, 3, 2, "cpu")
    assert len(q) == 0 and q.img.shape == (0, 3) and q.txt.shape == (0, 2) and q.ids.shape == (0,)

    def rows(lo, hi):  # row n carries the value n on both sides and the id str(100 + n)
        n = torch.arange(lo, hi, dtype=torch.float32)
        return n[:, None].expand(-1, 3).clone(), n[:, None].expand(-1, 2).clone(), [str(100 + k) for k in range(lo, hi)]

    def content():  # {value: id code}: ids travel with their rows
        assert torch.equal(q.img[:, 0], q.txt[:, 0])
        return {int(v): int(c) for v, c in zip(q.img[:, 0], q.ids)}

    code = lambda n: int(study_id_codes([str(100 + n)], "cpu")[0])
    q.push(*rows(0, 3))
    assert len(q) == 3 and content() == {n: code(n) for n in range(3)}
    q.push(*rows(3, 5))                                   # exactly full
    assert len(q) == 5 and content() == {n: code(n) for n in range(5)}
    q.push(*rows(5, 7))                                   # wrap: the two oldest entries go
    assert len(q) == 5 and content() == {n: code(n) for n in range(2, 7)}
    q.push(*rows(10, 22))                                 # more than the capacity: the last five survive
    assert len(q) == 5 and content() == {n: code(n) for n in range(17, 22)}
    q.push(*rows(30, 30))                                 # nothing
    assert len(q) == 5
    # detached fp32 copies: the queue holds no graph and does not alias its input
    img = torch.ones(2, 3, dtype=torch.float64, requires_grad=True)
    txt = torch.ones(2, 2, requires_grad=True)
    q.push(img * 2.0, txt, ["a", "b"])
    assert not q.img.requires_grad and not q.txt.requires_grad and q.img.dtype == torch.float32 and q.ids.dtype == torch.int64
    with torch.no_grad():
        txt.zero_()
    assert float(q.txt.sum()) > 0
    q.clear()
    assert len(q) == 0 and q.img.shape == (0, 3)
    q.push(*rows(0, 2))
    assert len(q) == 2 and content() == {0: code(0), 1: code(1)}
    with pytest.raises(ValueError):
        q.push(torch.zeros(2, 4), torch.zeros(2, 2), ["a", "b"])      # widths
    with pytest.raises(ValueError):
        q.push(torch.zeros(2, 3), torch.zeros(2, 2), ["a"])            # id count
    for bad in (0, -1, 2.5, True, None, "8"):
        with pytest.raises(ValueError, match="capacity"):
            check_capacity(bad)
    assert check_capacity(1) == 1


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_validation_without_gpu():
    from mutual_info_img_txt import memory_bank as mb
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import BilinearCritic
    x, y, sid = torch.zeros(4, 8), torch.zeros(4, 8), list("abcd")
    bank = (torch.zeros(3, 8), torch.zeros(3, 8), list("xyz"))
    with pytest.raises(MiCriticError):                     # CPU tensors raise as everywhere else
        mb.memory_bank_infonce(x, y, sid, BilinearCritic(8, 8), bank)
    with pytest.raises(MiCriticError):                     # ... an empty bank included (fused_mi_bound itself)
        mb.memory_bank_infonce(x, y, sid, BilinearCritic(8, 8), mb.EmbeddingQueue(4, 8, 8))
    # the documentation duty of the issue: the ceiling and the staleness caveat, module and function
    for doc in (mb.__doc__, mb.memory_bank_infonce.__doc__):
        flat = " ".join(doc.split())
        assert "log(B + M)" in flat and "ceiling" in flat.lower() and "stale" in flat.lower()
        assert "frozen encoders" in flat
    assert "not checkpointed" in " ".join(mb.EmbeddingQueue.__doc__.split()).lower() or \
        "not part of any checkpoint" in " ".join(mb.EmbeddingQueue.__doc__.split()).lower()


def test_manager_validation():
    from mutual_info_img_txt.main_utils import MultiModalManager
    for critic in ("bilinear", "separable"):
        for est in ("infonce_rowwise", "infonce_symmetric"):
            m = MultiModalManager(d_img=8, d_txt=8, critic=critic, d_proj=4, mi_estimator=est, memory_bank=64)
            assert m.memory_bank == 64 and m.bank is None
    assert MultiModalManager(d_img=8, d_txt=8, critic="bilinear").memory_bank is None
    for est in (None, "dv", "infonce", "jsd", "nwj"):
        with pytest.raises(ValueError, match="memory_bank"):
            MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator=est, memory_bank=64)
    with pytest.raises(ValueError):                        # the make_mlp critic has no per-sample InfoNCE step
        MultiModalManager(d_img=8, d_txt=8, critic="concat_mlp", hidden_dims=(8, 8), mi_estimator="infonce_symmetric",
                          memory_bank=64)
    with pytest.raises(ValueError, match="hard_negatives"):
        MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", memory_bank=64,
                          hard_negatives=4)
    for k in (0, -5, 2.5):
        with pytest.raises(ValueError, match="capacity"):
            MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", memory_bank=k)
    m = MultiModalManager(d_img=8, d_txt=8, critic="bilinear", mi_estimator="infonce_symmetric", memory_bank=4)
    with pytest.raises(ValueError, match="memory-bank"):    # a manager built for one form does not quietly train another
        m.mi_step(torch.zeros(4, 8), torch.zeros(4, 8), list("abcd"), "infonce_rowwise")
    assert "not checkpointed" in " ".join(MultiModalManager.mi_step.__doc__.split())


def test_train_py_validation():
    import train
    parse = lambda *a: train.check_training_parameters(train.construct_training_parameters(list(a)))
    args = parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", "--memory_bank", "64")
    assert args.memory_bank == 64
    assert parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric").memory_bank is None
    with pytest.raises(ValueError, match="--memory_bank"):
        parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "dv", "--memory_bank", "64")
    with pytest.raises(ValueError):
        parse("--synthetic", "--critic", "concat_mlp", "--mi_estimator", "infonce_symmetric", "--memory_bank", "64")
    with pytest.raises(ValueError, match="hard_negatives"):
        parse("--synthetic", "--critic", "bilinear", "--mi_estimator", "infonce_symmetric", "--memory_bank", "64",
              "--hard_negatives", "4")
    with pytest.raises(ValueError, match="capacity"):
        parse("--synthetic", "--critic", "separable", "--mi_estimator", "infonce_rowwise", "--memory_bank", "0")
