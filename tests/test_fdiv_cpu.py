"""Jensen-Shannon and NWJ bounds without a GPU: the fp64 restatement against hand-worked values and the closed-form
gradients, the stability of "jsd" at large scores, the name plumbing, and the C entry points' argument checks."""
import math

import pytest
import torch

import fdiv_reference as ref


def _sp(x):
    return math.log1p(math.exp(x))


def test_hand_worked_logits():
    logits = torch.tensor([[1.0], [-0.5], [2.0], [0.0], [-1.0]])
    jsd = ref.logits_case(logits, 2, "jsd")
    want = (_sp(-1.0) + _sp(0.5)) / 2 + (_sp(2.0) + _sp(0.0) + _sp(-1.0)) / 3
    assert abs(float(jsd["loss"]) - want) < 1e-12
    nwj = ref.logits_case(logits, 2, "nwj")
    want = math.exp(-1.0) * (math.exp(2.0) + 1.0 + math.exp(-1.0)) / 3 - (1.0 - 0.5) / 2
    assert abs(float(nwj["loss"]) - want) < 1e-12
    assert abs(float(sum(nwj["terms"])) - float(nwj["loss"])) < 1e-12
    # gradients: the table of DESIGN.md section 9
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))  # noqa: E731
    g = jsd["grad"].reshape(-1).tolist()
    assert abs(g[0] + sig(-1.0) / 2) < 1e-12 and abs(g[2] - sig(2.0) / 3) < 1e-12
    g = nwj["grad"].reshape(-1).tolist()
    assert abs(g[1] + 0.5) < 1e-12 and abs(g[3] - math.exp(0.0 - 1.0 - math.log(3.0))) < 1e-12


@pytest.mark.parametrize("mode", ref.MODES)
def test_matrix_gradient_matches_closed_form(mode):
    gen = torch.Generator().manual_seed(5)
    s = torch.randn(9, 9, generator=gen, dtype=torch.float64) * 2
    sid = ["a", "a", "b", "c", "c", "c", "d", "e", "f"]
    o = ref.matrix_case(s, sid, mode)
    torch.testing.assert_close(o["grad"], ref.closed_form_grad(s, sid, mode), rtol=1e-12, atol=1e-14)
    pos, neg = ref.masks(sid, sid)
    assert int(pos.sum()) == 9 and int(neg.sum()) == 81 - 9 - 2 - 6


def test_jsd_stable_at_large_scores():
    s = torch.tensor([[80.0, -80.0], [80.0, -80.0]], dtype=torch.float64)
    o = ref.matrix_case(s, ["a", "b"], "jsd")
    assert math.isfinite(float(o["loss"])) and torch.isfinite(o["grad"]).all()
    # sp(80) = 80 + log1p(e^-80); positives (80, -80) -> (sp(-80) + sp(80)) / 2; negatives (-80, 80) -> the same
    assert abs(float(o["loss"]) - 80.0) < 1e-9
    o = ref.logits_case(torch.tensor([-80.0, 80.0]), 1, "jsd")
    assert abs(float(o["loss"]) - 160.0) < 1e-9 and torch.isfinite(o["grad"]).all()


def test_no_negatives_is_nan():
    for mode in ref.MODES:
        o = ref.matrix_case(torch.randn(3, 3, dtype=torch.float64), ["x"] * 3, mode)
        assert math.isnan(float(o["loss"]))


# ------------------------------------------------------------------------------------------------ names
def test_estimator_tables():
    from mutual_info_img_txt import _hip, mi_critics
    assert _hip.FDIV_ESTIMATORS == {"jsd": 0, "nwj": 1}
    assert _hip.ESTIMATORS == {"dv": 0, "infonce": 1}
    assert _hip.NCE_ESTIMATORS == {"infonce_rowwise": 0, "infonce_symmetric": 1}
    for name in ("jsd", "nwj"):
        with pytest.raises(ValueError):
            mi_critics._estimator_code(name)  # not estimator codes of the DV entry points
        for kind in ("concat_mlp", "bilinear", "separable"):
            mi_critics.check_estimator(name, kind)
    with pytest.raises(ValueError):
        mi_critics.check_estimator("infonce_symmetric", "concat_mlp")
    with pytest.raises(ValueError):
        mi_critics.check_estimator("js", "bilinear")


def test_train_py_and_manager_accept_the_names():
    import train
    from mutual_info_img_txt.main_utils import MultiModalManager
    for est in ("jsd", "nwj"):
        for critic in ("concat_mlp", "bilinear", "separable"):
            args = train.construct_training_parameters(["--synthetic", "--critic", critic, "--mi_estimator", est])
            assert train.check_training_parameters(args).mi_estimator == est
        args = train.construct_training_parameters(["--mi_estimator", est])  # the default critic: concat_mlp
        assert train.check_training_parameters(args).mi_estimator == est
        MultiModalManager(d_img=16, d_txt=16, critic="concat_mlp", hidden_dims=(8, 8), mi_estimator=est)
        MultiModalManager(d_img=16, d_txt=16, critic="bilinear", mi_estimator=est)
        MultiModalManager(d_img=16, d_txt=16, critic="separable", d_proj=8, mi_estimator=est)


def test_sharded_and_graphed_entry_points_reject_the_names():
    from mutual_info_img_txt import distributed
    from mutual_info_img_txt.graphed import GraphedMiStep
    from mutual_info_img_txt.model import BilinearCritic
    x, y, sid = torch.randn(8, 16), torch.randn(8, 16), torch.arange(8)
    w = torch.randn(16, 16)
    for est in ("jsd", "nwj"):
        with pytest.raises(ValueError, match="one GPU"):
            distributed.global_batch_mi_bound(x, y, sid, [w], estimator=est)
        with pytest.raises(ValueError, match="one GPU"):
            distributed.GlobalBatchGraphStep(x, y, sid, [w], estimator=est)
        with pytest.raises(ValueError, match="eagerly"):
            GraphedMiStep(BilinearCritic(16, 16), 8, 16, 16, estimator=est, device="cuda", capture=False)


# ------------------------------------------------------------------------------------------------ C entry points
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


def test_symbols_exported_and_abi_unchanged(lib):
    from mutual_info_img_txt import _hip
    names = [n for n in _hip.SIGNATURES if n.startswith("mi_fdiv_")]
    assert len(names) == 12
    for n in names:
        assert hasattr(lib, n)
    assert lib.mi_abi_version() == 4


def test_workspace_queries_host_only(lib):
    assert lib.mi_fdiv_bound_workspace_bytes(100) > 0
    assert lib.mi_fdiv_matrix_workspace_bytes(64) > 0
    small = lib.mi_fdiv_bilinear_workspace_bytes(64, 128, 128, 1)
    assert lib.mi_fdiv_bilinear_workspace_bytes(4096, 512, 512, 1) > small > 0
    assert lib.mi_fdiv_separable_workspace_bytes(64, 128, 96, 32, 0) > 0
    assert lib.mi_fdiv_bilinear_workspace_bytes(0, 128, 128, 1) == 0


def test_null_pointers_and_bad_modes_rejected(lib):
    d = 1 << 20  # a non-null address that is never dereferenced: validation comes first
    assert lib.mi_fdiv_bound_fwd(None, 4, 2, 0, None, None, None, None, 0, None) == -1
    assert b"null" in lib.mi_last_error()
    assert lib.mi_fdiv_bound_fwd(d, 4, 2, 7, d, None, d, d, 1 << 20, None) == -1
    assert b"mode" in lib.mi_last_error()
    assert lib.mi_fdiv_bound_fwd(d, 4, 5, 0, d, None, d, d, 1 << 20, None) == -1
    assert lib.mi_fdiv_bound_bwd(d, 4, 2, 2, d, None, d, None) == -1
    assert lib.mi_fdiv_matrix_fwd(None, None, 4, 0, None, None, None, None, 0, None) == -1
    assert lib.mi_fdiv_matrix_fwd(d, d, 4, -1, d, None, d, d, 1 << 20, None) == -1
    assert lib.mi_fdiv_matrix_bwd(d, d, 4, 9, d, None, d, None) == -1
    assert lib.mi_fdiv_bilinear_step(None, None, None, None, 64, 128, 128, 0, 1, None, None, None, None, None, None, None,
                                     None, 0, None) == -1
    for prec in (3, 4, 5):  # fp8, f16, f16x3
        assert lib.mi_fdiv_bilinear_step(d, d, d, d, 64, 128, 128, 0, prec, None, d, None, None, None, None, None, d,
                                         1 << 20, None) == -1
        assert b"precision" in lib.mi_last_error()
        assert lib.mi_fdiv_separable_step(d, d, d, d, d, 64, 128, 128, 32, 1, prec, None, d, None, None, None, None,
                                          None, None, d, 1 << 20, None) == -1
    assert lib.mi_fdiv_bilinear_step(d, d, d, d, 64, 128, 128, 5, 1, None, d, None, None, None, None, None, d, 1 << 20,
                                     None) == -1
    assert lib.mi_fdiv_concat_mlp_fwd(*[None] * 10, 64, 64, 0, 16, 16, 64, 256, 0, 1, 1, *[None] * 5, 0, None) == -1
    assert lib.mi_fdiv_concat_mlp_fwd(*[d] * 10, 64, 64, 0, 16, 16, 64, 256, 3, 1, 1, *[d] * 5, 1 << 20, None) == -1
    assert b"mode" in lib.mi_last_error()
    assert lib.mi_fdiv_concat_mlp_bwd(*[d] * 10, 64, 64, 0, 16, 16, 64, 256, 2, 1, d, None, *[d] * 10, 1 << 20,
                                      None) == -1
    assert lib.mi_fdiv_concat_mlp_bwd(*[None] * 10, 64, 64, 0, 16, 16, 64, 256, 0, 1, *[None] * 12, 0, None) == -1
