"""Per-sample InfoNCE, host side: the fp64 restatement (tests/nce_reference.py) against torch's cross-entropy and a
hand-worked case, the new C-ABI symbols (exported, host-only workspace queries, argument checks before any device
work) and the estimator plumbing of train.py / MultiModalManager.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import nce_reference as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("b", [1, 5, 33])
def test_unique_ids_equal_cross_entropy(b):
    gen = torch.Generator().manual_seed(b)
    s0 = torch.randn(b, b, generator=gen, dtype=torch.float64) * 3.0
    sid = [str(n) for n in range(b)]
    tgt = torch.arange(b)
    for est in ref.MODES:
        s = s0.clone().requires_grad_(True)
        loss = ref.nce_loss(s, sid, est)
        loss.backward()
        s2 = s0.clone().requires_grad_(True)
        want = F.cross_entropy(s2, tgt)
        if est == "infonce_symmetric":
            want = 0.5 * want + 0.5 * F.cross_entropy(s2.t(), tgt)
        want.backward()
        assert abs(float(loss) - float(want)) < 1e-12
        assert float((s.grad - s2.grad).abs().max()) < 1e-12
        assert float((ref.nce_grad_scores(s0, sid, est) - s2.grad).abs().max()) < 1e-12  # the closed form too


def test_hand_worked_4x4_with_duplicates():
    # ids a, a, b, c and S = 0: row 0 sees {0, 2, 3}, row 1 {1, 2, 3}, rows 2 and 3 see all four; the mask is symmetric,
    # so the column LSEs equal the row LSEs
    sid = ["a", "a", "b", "c"]
    s = torch.zeros(4, 4, dtype=torch.float64)
    r, c = ref.lse_rows_cols(s, sid)
    assert torch.allclose(r, torch.tensor([math.log(3), math.log(3), math.log(4), math.log(4)], dtype=torch.float64))
    assert torch.allclose(c, r)
    want = (2 * math.log(3) + 2 * math.log(4)) / 4
    for est in ref.MODES:
        assert abs(float(ref.nce_loss(s, sid, est)) - want) < 1e-14
    g = ref.nce_grad_scores(s, sid, "infonce_rowwise")
    assert abs(float(g[0, 0]) - (1 / 3 - 1) / 4) < 1e-15
    assert float(g[0, 1]) == 0.0 and float(g[1, 0]) == 0.0  # dropped pairs
    assert abs(float(g[0, 2]) - (1 / 3) / 4) < 1e-15
    assert abs(float(g[2, 0]) - (1 / 4) / 4) < 1e-15
    # a diagonal of 1: row 0 = log(e + 2) - 1
    s1 = torch.eye(4, dtype=torch.float64)
    r1, _ = ref.lse_rows_cols(s1, sid)
    assert abs(float(r1[0]) - math.log(math.e + 2)) < 1e-14
    assert abs(float(r1[2]) - math.log(math.e + 3)) < 1e-14


def test_rows_without_negatives_contribute_zero():
    s = torch.randn(4, 4, dtype=torch.float64)
    for est in ref.MODES:
        assert float(ref.nce_loss(s, ["x"] * 4, est)) == 0.0  # no negatives at all: loss 0 (the reference's DV: NaN)
        assert float(ref.nce_grad_scores(s, ["x"] * 4, est).abs().max()) < 1e-15
    # one all-same-id group of three beside a unique sample: each row of the group only has sample 3 as candidate
    sid = ["g", "g", "g", "u"]
    r, _ = ref.lse_rows_cols(s, sid)
    assert abs(float(r[0]) - float(torch.logsumexp(torch.stack([s[0, 0], s[0, 3]]), 0))) < 1e-14


# ------------------------------------------------------------------------------------------------ C ABI, host side
NEW_SYMBOLS = ("mi_nce_bilinear_workspace_bytes", "mi_nce_bilinear_step", "mi_nce_separable_workspace_bytes",
               "mi_nce_separable_step", "mi_matrix_nce_workspace_bytes", "mi_matrix_nce_fwd", "mi_matrix_nce_bwd")


def test_new_symbols_exported(lib):
    from mutual_info_img_txt import _hip
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.mi_abi_version() == 4


def test_workspace_queries_host_only_and_monotone(lib):
    from mutual_info_img_txt import _hip
    for prec in (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3):
        sizes = [lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec) for b, d in ((1, 8), (64, 128), (1024, 512),
                                                                                   (4096, 512), (4096, 768))]
        assert all(v > 0 for v in sizes) and sizes == sorted(sizes)
        sep = [lib.mi_nce_separable_workspace_bytes(b, 256, 256, k, prec) for b, k in ((3, 12), (256, 256), (1024, 512))]
        assert all(v > 0 for v in sep) and sep == sorted(sep)
    mat = [lib.mi_matrix_nce_workspace_bytes(b) for b in (1, 3, 64, 1000, 4096)]
    assert all(v > 0 for v in mat) and mat == sorted(mat)
    assert mat[-1] >= 2 * 4096 * 64 * 8  # row and column records of 64-wide tiles
    assert lib.mi_nce_bilinear_workspace_bytes(0, 8, 8, 1) == 0
    assert lib.mi_matrix_nce_workspace_bytes(-1) == 0


def test_arguments_rejected_without_gpu(lib):
    fake = 1 << 20  # never dereferenced: every call below fails its argument checks first
    assert lib.mi_matrix_nce_fwd(None, None, 4, 0, None, None, None, None, 0, None) == -1
    assert b"null" in lib.mi_last_error()
    assert lib.mi_matrix_nce_bwd(None, None, 4, 0, None, None, None, None, None) == -1
    assert lib.mi_nce_bilinear_step(None, None, None, None, 64, 128, 128, 0, 1, None, None, None, None, None, None,
                                    None, None, 0, None) == -1
    assert lib.mi_nce_separable_step(None, None, None, None, None, 64, 128, 128, 64, 0, 1, None, None, None, None,
                                     None, None, None, None, None, 0, None) == -1
    # unknown mode
    assert lib.mi_matrix_nce_fwd(fake, fake, 4, 7, fake, None, None, fake, 1 << 20, None) == -1
    assert b"mode" in lib.mi_last_error()
    assert lib.mi_matrix_nce_bwd(fake, fake, 4, 2, fake, fake, None, fake, None) == -1
    assert lib.mi_nce_bilinear_step(fake, fake, fake, fake, 64, 128, 128, 5, 1, None, fake, None, None, None, None,
                                    None, fake, 1 << 30, None) == -1
    # the symmetric backward needs the column LSEs
    assert lib.mi_matrix_nce_bwd(fake, fake, 4, 1, fake, None, None, fake, None) == -1
    # fp8 / f16 / f16x3 are not precisions of this loss
    for prec in (3, 4, 5):
        assert lib.mi_nce_bilinear_step(fake, fake, fake, fake, 64, 128, 128, 0, prec, None, fake, None, None, None,
                                        None, None, fake, 1 << 30, None) == -1
        assert b"precision" in lib.mi_last_error()
        assert lib.mi_nce_separable_step(fake, fake, fake, fake, fake, 64, 128, 128, 64, 1, prec, None, fake, None,
                                         None, None, None, None, None, fake, 1 << 30, None) == -1
    # gradients: all or none
    assert lib.mi_nce_bilinear_step(fake, fake, fake, fake, 64, 128, 128, 0, 1, None, fake, None, None, fake, None,
                                    None, fake, 1 << 30, None) == -1


# ------------------------------------------------------------------------------------------------ Python plumbing
def test_estimator_tables_stay_apart():
    from mutual_info_img_txt import _hip, mi_critics
    assert set(_hip.ESTIMATORS) == {"dv", "infonce"}
    assert _hip.NCE_ESTIMATORS == {"infonce_rowwise": 0, "infonce_symmetric": 1}
    for name in ("mine", "infonce_rowwise", "infonce_symmetric"):
        with pytest.raises(ValueError):
            mi_critics._estimator_code(name)
    for kind in ("bilinear", "separable"):
        for est in ("dv", "infonce", "infonce_rowwise", "infonce_symmetric"):
            mi_critics.check_estimator(est, kind)
    with pytest.raises(ValueError):
        mi_critics.check_estimator("infonce_symmetric", "concat_mlp")
    with pytest.raises(ValueError):
        mi_critics.check_estimator("mine", "bilinear")


def test_train_py_accepts_the_new_names():
    import train
    for est in ("infonce_rowwise", "infonce_symmetric"):
        for critic in ("bilinear", "separable"):
            args = train.construct_training_parameters(["--synthetic", "--critic", critic, "--mi_estimator", est])
            assert train.check_training_parameters(args).mi_estimator == est
        with pytest.raises(ValueError):
            train.check_training_parameters(train.construct_training_parameters(["--mi_estimator", est]))
    with pytest.raises(ValueError):
        train.check_training_parameters(train.construct_training_parameters(["--mi_estimator", "mine"]))


def test_manager_rejects_concat_critic_at_construction():
    from mutual_info_img_txt.main_utils import MultiModalManager
    MultiModalManager(d_img=16, d_txt=16, critic="bilinear", mi_estimator="infonce_symmetric")
    MultiModalManager(d_img=16, d_txt=16, critic="separable", d_proj=8, mi_estimator="infonce_rowwise")
    with pytest.raises(ValueError):
        MultiModalManager(d_img=16, d_txt=16, critic="concat_mlp", hidden_dims=(8, 8), mi_estimator="infonce_rowwise")
