"""MI estimates without a device: the fp64 reference of tests/mi_estimates_reference.py against
hand-worked values and the identities of the definitions, the C entry points' argument validation and workspace
queries through the built library, and the Python layer's eager checks."""
import ctypes
import math

import pytest
import torch

import mi_estimates_reference as ref


def _sp(x):
    return math.log1p(math.exp(-abs(x))) + max(x, 0.0)


def _lse(vals):
    m = max(vals)
    return m + math.log(sum(math.exp(v - m) for v in vals))


def _approx(got, want):
    assert got == pytest.approx(want, rel=1e-12, abs=1e-12), (got, want)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_3x3_by_hand():
    s = torch.tensor([[2.0, 0.0, -1.0], [1.0, 3.0, 0.0], [0.0, -2.0, 1.0]])
    got = ref.estimates(s, [10, 20, 30], taus=(0.5, 1.5))
    negs = [0.0, -1.0, 1.0, 0.0, 0.0, -2.0]  # row by row, off the diagonal
    pos = [2.0, 3.0, 1.0]
    pos_mean, log_n = 2.0, math.log(6.0)
    _approx(got["pos_mean"], pos_mean)
    _approx(got["neg_mean"], -2.0 / 6.0)
    _approx(got["log_n_neg"], log_n)
    lse = math.log(1.0 + math.exp(-1.0) + math.e + 1.0 + 1.0 + math.exp(-2.0))
    _approx(got["dv"], pos_mean - (lse - log_n))
    _approx(got["nwj"], pos_mean - math.exp(lse - log_n - 1.0))
    _approx(got["jsd"], -(sum(_sp(-p) for p in pos) / 3.0 + sum(_sp(n) for n in negs) / 6.0))
    rows = [_lse([2.0, 0.0, -1.0]), _lse([1.0, 3.0, 0.0]), _lse([0.0, -2.0, 1.0])]
    cols = [_lse([2.0, 1.0, 0.0]), _lse([0.0, 3.0, -2.0]), _lse([-1.0, 0.0, 1.0])]
    _approx(got["nce_i2t"], sum(p - r for p, r in zip(pos, rows)) / 3.0 + math.log(3.0))
    _approx(got["nce_t2i"], sum(p - c for p, c in zip(pos, cols)) / 3.0 + math.log(3.0))
    # clip 0.5: the negatives become 0, -0.5, 0.5, 0, 0, -0.5; clip 1.5: only the -2 moves
    _approx(got["smile"][0], pos_mean - (math.log(3.0 + 2.0 * math.exp(-0.5) + math.exp(0.5)) - log_n))
    _approx(got["smile"][1], pos_mean - (math.log(3.0 + math.exp(-1.0) + math.e + math.exp(-1.5)) - log_n))


def test_reference_5x5_one_duplicated_id_by_hand():
    s = [[1.5, -0.5, 0.25, 2.0, -1.0],
         [0.0, 2.5, 4.0, -0.75, 0.5],
         [1.0, -3.0, 0.5, 0.0, 1.25],
         [-2.0, 0.75, 0.0, 3.0, -0.25],
         [0.5, 1.0, -1.5, 0.0, 2.0]]
    ids = ["a", "b", "b", "c", "d"]  # (1, 2) and (2, 1) are dropped: 18 negatives; rows 1 and 2 have 4 candidates
    got = ref.estimates(torch.tensor(s), [0, 1, 1, 2, 3], taus=(1.0,))
    negs = [s[i][j] for i in range(5) for j in range(5) if i != j and ids[i] != ids[j]]
    assert len(negs) == 18 and 4.0 not in negs and -3.0 not in negs
    pos = [s[i][i] for i in range(5)]
    pos_mean, log_n = sum(pos) / 5.0, math.log(18.0)
    _approx(got["pos_mean"], 1.9)
    _approx(got["log_n_neg"], log_n)
    _approx(got["neg_mean"], sum(negs) / 18.0)
    _approx(got["dv"], pos_mean - (_lse(negs) - log_n))
    _approx(got["nwj"], pos_mean - math.exp(_lse(negs) - log_n - 1.0))
    _approx(got["jsd"], -(sum(_sp(-p) for p in pos) / 5.0 + sum(_sp(n) for n in negs) / 18.0))
    n_cand = [5, 4, 4, 5, 5]
    t_row = [pos[i] - _lse([s[i][j] for j in range(5) if i == j or ids[i] != ids[j]]) + math.log(n_cand[i]) for i in range(5)]
    t_col = [pos[j] - _lse([s[i][j] for i in range(5) if i == j or ids[i] != ids[j]]) + math.log(n_cand[j]) for j in range(5)]
    _approx(got["nce_i2t"], sum(t_row) / 5.0)
    _approx(got["nce_t2i"], sum(t_col) / 5.0)
    _approx(got["smile"][0], pos_mean - (_lse([min(max(n, -1.0), 1.0) for n in negs]) - log_n))


def test_reference_identities():
    gen = torch.Generator().manual_seed(3)
    s = torch.randn(37, 37, generator=gen, dtype=torch.float64) * 2.0
    sid = torch.arange(37)
    got = ref.estimates(s, sid, taus=(0.5, float(s.abs().max()), 40.0))
    # a clip at or above every negative score changes nothing: SMILE is DV
    _approx(got["smile"][1], got["dv"])
    _approx(got["smile"][2], got["dv"])
    assert got["smile"][0] != pytest.approx(got["dv"], abs=1e-3)
    # unique ids: nce_i2t = log b - cross_entropy(S, arange), nce_t2i the same on S^T
    tgt = torch.arange(37)
    _approx(got["nce_i2t"], math.log(37.0) - float(torch.nn.functional.cross_entropy(s, tgt)))
    _approx(got["nce_t2i"], math.log(37.0) - float(torch.nn.functional.cross_entropy(s.t(), tgt)))
    assert got["nwj"] <= got["dv"] + 1e-12  # log z <= z / e


@pytest.mark.parametrize("b", [1, 6])
def test_reference_without_negatives(b):
    gen = torch.Generator().manual_seed(b)
    s = torch.randn(b, b, generator=gen, dtype=torch.float64)
    got = ref.estimates(s, [7] * b, taus=(1.0, 5.0))
    for name in ("dv", "nwj", "jsd", "neg_mean"):
        assert math.isnan(got[name]), name
    assert len(got["smile"]) == 2 and all(math.isnan(v) for v in got["smile"])
    assert got["log_n_neg"] == -math.inf
    assert got["nce_i2t"] == 0.0 and got["nce_t2i"] == 0.0
    _approx(got["pos_mean"], float(torch.diagonal(s).mean()))
    if b == 1:
        assert got["pos_mean"] == float(s[0, 0])


# ------------------------------------------------------------------------------------------------ C entry points
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


D = 1 << 20  # a non-null address that is never dereferenced: validation comes first
BIG = 1 << 40


def _taus(*vals):
    return (ctypes.c_float * max(len(vals), 1))(*vals)


def _matrix(lib, scores=D, sid=D, b=64, taus=None, n_tau=2, est=D, ws=D, ws_bytes=BIG):
    return lib.mi_estimates_matrix(scores, sid, b, _taus(1.0, 5.0) if taus is None else taus, n_tau, est, ws, ws_bytes, None)


def _bilinear(lib, x=D, y=D, w=D, sid=D, b=64, dx=128, dy=128, prec=1, taus=None, n_tau=2, est=D, ws=D, ws_bytes=BIG):
    return lib.mi_estimates_bilinear(x, y, w, sid, b, dx, dy, prec, _taus(1.0, 5.0) if taus is None else taus, n_tau, est,
                                     ws, ws_bytes, None)


def _separable(lib, x=D, y=D, wg=D, wh=D, sid=D, b=64, dx=128, dy=96, k=32, prec=1, taus=None, n_tau=2, est=D, ws=D,
               ws_bytes=BIG):
    return lib.mi_estimates_separable(x, y, wg, wh, sid, b, dx, dy, k, prec, _taus(1.0, 5.0) if taus is None else taus,
                                      n_tau, est, ws, ws_bytes, None)


def test_symbols_exported_and_abi_unchanged(lib):
    from mutual_info_img_txt import _hip
    names = sorted(n for n in _hip.SIGNATURES if n.startswith("mi_estimates_"))
    assert names == ["mi_estimates_bilinear", "mi_estimates_bilinear_workspace_bytes", "mi_estimates_matrix",
                     "mi_estimates_matrix_workspace_bytes", "mi_estimates_separable",
                     "mi_estimates_separable_workspace_bytes"]
    for n in names:
        assert hasattr(lib, n)
    assert lib.mi_abi_version() == 4
    assert (_hip.MI_EST_FLOATS, _hip.MI_EST_MAX_TAUS, _hip.MI_EST_SMILE) == (12, 4, 8)


def test_workspace_queries_host_only(lib):
    assert lib.mi_estimates_matrix_workspace_bytes(0) == 0
    assert lib.mi_estimates_bilinear_workspace_bytes(0, 128, 128, 1) == 0
    assert lib.mi_estimates_separable_workspace_bytes(0, 128, 96, 32, 1) == 0
    for query in (lib.mi_estimates_matrix_workspace_bytes, lambda b: lib.mi_estimates_bilinear_workspace_bytes(b, 128, 128, 1),
                  lambda b: lib.mi_estimates_bilinear_workspace_bytes(b, 100, 100, 0),
                  lambda b: lib.mi_estimates_separable_workspace_bytes(b, 128, 96, 32, 2)):
        sizes = [query(b) for b in (8, 64, 72, 1000, 4096)]  # multiples of 8: one kernel path per query
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    # the records scale as b^2 / 64 and there is no b x b float matrix (nor G, G^T) in the plan
    b = 4096
    got = lib.mi_estimates_bilinear_workspace_bytes(b, 512, 512, 1)
    assert got < b * b * 4
    assert got < lib.mi_nce_bilinear_workspace_bytes(b, 512, 512, 1)
    records = 2 * 8 * b * (b // 64) + 48 * (b // 64) ** 2
    assert lib.mi_estimates_matrix_workspace_bytes(b) >= records
    assert lib.mi_estimates_matrix_workspace_bytes(b) <= records + 12 * b + 4096
    assert got >= lib.mi_rank_bilinear_workspace_bytes(b, 512, 512, 1) + records - 4 * b - 4096


def test_null_pointers_rejected(lib):
    assert lib.mi_estimates_matrix(None, None, 64, None, 0, None, None, 0, None) == -1
    assert b"null" in lib.mi_last_error()
    for kw in ("scores", "sid", "est", "ws"):
        assert _matrix(lib, **{kw: None}) == -1, kw
        assert b"null" in lib.mi_last_error()
    for kw in ("x", "y", "sid", "est", "ws"):
        assert _bilinear(lib, **{kw: None}) == -1, kw
        assert b"null" in lib.mi_last_error()
    for kw in ("x", "y", "wg", "wh", "sid", "est", "ws"):
        assert _separable(lib, **{kw: None}) == -1, kw
        assert b"null" in lib.mi_last_error()
    # taus_host may be NULL only with n_tau == 0 (then the call goes on to the workspace check)
    assert lib.mi_estimates_matrix(D, D, 64, None, 2, D, D, BIG, None) == -1
    assert lib.mi_estimates_matrix(D, D, 64, None, 0, D, D, 16, None) == -3


def test_bad_sizes_rejected(lib):
    for b in (0, -3, 1 << 31, 1 << 40):
        assert _matrix(lib, b=b) == -1, b
        assert _bilinear(lib, b=b) == -1, b
        assert _separable(lib, b=b) == -1, b
    for kw in ({"dx": 0}, {"dy": 0}, {"dx": -8}):
        assert _bilinear(lib, **kw) == -1, kw
        assert _separable(lib, **kw) == -1, kw
    assert _separable(lib, k=0) == -1
    # w == NULL is S = X Y^T: the widths must agree
    assert _bilinear(lib, w=None, dx=128, dy=64) == -1
    assert b"d_img == d_txt" in lib.mi_last_error()
    assert _bilinear(lib, w=None, dx=128, dy=128, ws_bytes=16) == -3  # ... and passes validation when they do


def test_bad_taus_rejected(lib):
    calls = (_matrix, _bilinear, _separable)
    for call in calls:
        for n_tau in (-1, 5, 100):
            assert call(lib, taus=_taus(1.0, 1.0, 1.0, 1.0, 1.0), n_tau=n_tau) == -1, n_tau
            assert b"n_tau" in lib.mi_last_error()
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 40.5, 1e30):
            assert call(lib, taus=_taus(1.0, bad), n_tau=2) == -1, bad
            assert b"tau" in lib.mi_last_error()
            assert call(lib, taus=_taus(bad), n_tau=1) == -1, bad
            # a bad value beyond n_tau is not read as a clip
            assert call(lib, taus=_taus(1.0, bad), n_tau=1, ws_bytes=16) == -3, bad
        # the limits themselves are fine: validation passes, the short workspace is what fails
        assert call(lib, taus=_taus(40.0, 1e-3, 5.0, 0.5), n_tau=4, ws_bytes=16) == -3
        assert call(lib, taus=None, n_tau=0, ws_bytes=16) == -3


def test_bad_precisions_rejected(lib):
    for prec in (3, 4, 5, 6, -1):  # fp8, f16, f16x3, unknown
        assert _bilinear(lib, prec=prec) == -1, prec
        assert b"precision" in lib.mi_last_error()
        assert _separable(lib, prec=prec) == -1, prec
        assert b"precision" in lib.mi_last_error()
    for prec in (0, 1, 2):
        assert _bilinear(lib, prec=prec, ws_bytes=16) == -3
        assert _separable(lib, prec=prec, ws_bytes=16) == -3


def test_short_workspace_rejected(lib):
    need = lib.mi_estimates_matrix_workspace_bytes(200)
    assert _matrix(lib, b=200, ws_bytes=need - 257) == -3
    assert b"workspace" in lib.mi_last_error()
    need = lib.mi_estimates_bilinear_workspace_bytes(200, 60, 60, 1)
    assert _bilinear(lib, b=200, dx=60, dy=60, ws_bytes=need - 257) == -3
    assert b"workspace" in lib.mi_last_error()
    need = lib.mi_estimates_separable_workspace_bytes(256, 128, 96, 32, 2)
    assert _separable(lib, b=256, prec=2, ws_bytes=need - 257) == -3
    assert b"workspace" in lib.mi_last_error()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_cpu_tensors_raise():
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.mi_estimates import matrix_mi_estimates, mi_estimates
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic, make_mlp
    x, y, ids = torch.zeros(8, 16), torch.zeros(8, 16), list("abcdefgh")
    for critic in (BilinearCritic(16, 16), SeparableCritic(16, 16, 8), make_mlp(32, [64, 256])):
        with pytest.raises(MiCriticError):
            mi_estimates(x, y, ids, critic)
    with pytest.raises(MiCriticError):
        matrix_mi_estimates(torch.zeros(8, 8), ids)
    with pytest.raises(TypeError):
        mi_estimates(x, y, ids, None)


@pytest.mark.parametrize("taus", [(0.0,), (-1.0, 1.0), (float("nan"),), (float("inf"),), (40.5,), (1.0, 2.0, 3.0, 4.0, 5.0), 3.0])
def test_bad_taus_raise_before_the_device(taus):
    from mutual_info_img_txt.mi_estimates import matrix_mi_estimates, mi_estimates
    from mutual_info_img_txt.model import BilinearCritic
    x, y, ids = torch.zeros(8, 16), torch.zeros(8, 16), list("abcdefgh")
    with pytest.raises(ValueError, match="tau|clips"):
        mi_estimates(x, y, ids, BilinearCritic(16, 16), taus=taus)  # CPU tensors: the clips are checked first
    with pytest.raises(ValueError, match="tau|clips"):
        matrix_mi_estimates(torch.zeros(8, 8), ids, taus=taus)


def test_unavailable_precisions_refused():
    from mutual_info_img_txt.mi_estimates import mi_estimates
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic, make_mlp
    x, y, ids = torch.zeros(8, 16), torch.zeros(8, 16), list("abcdefgh")
    for critic in (BilinearCritic(16, 16), SeparableCritic(16, 16, 8)):
        for precision in ("fp8", "f16", "f16x3"):
            with pytest.raises(ValueError, match="not available for the MI estimates"):
                mi_estimates(x, y, ids, critic, precision=precision)
    for precision in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match="not available for the MI estimates"):
            mi_estimates(x, y, ids, make_mlp(32, [64, 256]), precision=precision)
    with pytest.raises(ValueError, match="unknown precision"):
        mi_estimates(x, y, ids, BilinearCritic(16, 16), precision="int4")


def test_not_an_estimator_name():
    """The estimates are a monitor beside the training losses: the estimator table is untouched."""
    from mutual_info_img_txt import _hip
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
    for name in ("smile", "nce_i2t", "mi_estimates"):
        with pytest.raises(ValueError):
            _hip.check_estimator(name)
