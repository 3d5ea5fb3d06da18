"""Retrieval ranks, host side: the fp64 restatement (tests/retrieval_reference.py) on a hand-worked case,
``retrieval_metrics`` on a known rank vector, the mi_rank_* symbols of the C ABI (exported, argument checks before any
device work, host-only workspace queries that grow linearly in b) and the CPU-tensor errors.  No GPU needed."""
import pytest
import torch

import retrieval_reference as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ the restatement
HAND_S = [[1.0, 2.0, 0.0, 1.0],
          [0.0, 3.0, 5.0, 3.0],
          [4.0, 0.0, 2.0, 2.0],
          [0.0, 0.0, 0.0, 0.0]]
HAND_IDS = ["a", "b", "b", "c"]  # reports 1 and 2 belong to one study


def test_hand_worked_4x4_with_duplicate_and_tie():
    s = torch.tensor(HAND_S, dtype=torch.float64)
    i2t, t2i = ref.ranks(s, HAND_IDS)
    # row 0: 2 > 1 counts, the tie S[0, 3] == S[0, 0] does not.  row 1: S[1, 2] = 5 > 3 is an equal-id pair (dropped),
    # S[1, 3] ties.  row 2: 4 > 2 counts, S[2, 1] is dropped, S[2, 3] ties.  row 3: all ties.
    assert i2t.tolist() == [1, 0, 1, 0]
    # column 0: 4 > 1.  column 1: S[2, 1] dropped.  column 2: S[1, 2] = 5 dropped.  column 3: 1, 3, 2 > 0.
    assert t2i.tolist() == [1, 0, 0, 3]
    # without the mask the dropped 5 would count
    i2t_u, t2i_u = ref.ranks(s, ["a", "b", "c", "d"])
    assert i2t_u.tolist() == [1, 1, 1, 0] and t2i_u.tolist() == [1, 0, 1, 3]
    # every id equal: no negatives at all
    z = ref.ranks(s, ["x"] * 4)
    assert z[0].tolist() == [0] * 4 and z[1].tolist() == [0] * 4
    # the band: tau = 0 is the rank itself from both sides
    lo, hi = ref.rank_band(s, HAND_IDS, 0.0)
    assert lo[0].tolist() == [1, 0, 1, 0] and hi[0].tolist() == [1, 0, 1, 0]
    lo, hi = ref.rank_band(s, HAND_IDS, 0.6)
    assert lo[0].tolist() == [0, 0, 1, 0]  # 2 > 1 + 1.2 fails, 4 > 2 + 1.2 holds
    assert hi[0].tolist() == [3, 1, 2, 3]  # the ties and every negative less than 1.2 below the diagonal count
    assert all(bool((a <= b).all()) for a, b in zip(lo, hi))


def test_retrieval_metrics_known_vector():
    from mutual_info_img_txt.retrieval import retrieval_metrics
    m = retrieval_metrics(torch.tensor([0, 0, 1, 4, 9, 20], dtype=torch.int32), ks=(1, 5, 10))
    assert set(m) == {"recall@1", "recall@5", "recall@10", "median_rank", "mrr"}
    assert m["recall@1"] == pytest.approx(2 / 6, abs=1e-15)
    assert m["recall@5"] == pytest.approx(4 / 6, abs=1e-15)
    assert m["recall@10"] == pytest.approx(5 / 6, abs=1e-15)
    assert m["median_rank"] == 3.5  # 1-based: ((1 + 4) / 2) + 1
    assert m["mrr"] == pytest.approx((1 + 1 + 1 / 2 + 1 / 5 + 1 / 10 + 1 / 21) / 6, abs=1e-15)
    odd = retrieval_metrics(torch.tensor([7, 0, 2]), ks=(3,))
    assert odd == {"recall@3": pytest.approx(2 / 3), "median_rank": 3.0, "mrr": pytest.approx((1 / 8 + 1 + 1 / 3) / 3)}
    assert retrieval_metrics(torch.zeros(5, dtype=torch.int32)) == {"recall@1": 1.0, "recall@5": 1.0, "recall@10": 1.0,
                                                                    "median_rank": 1.0, "mrr": 1.0}
    with pytest.raises(ValueError):
        retrieval_metrics(torch.zeros(0, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ C ABI, host side
NEW_SYMBOLS = ("mi_rank_matrix", "mi_rank_bilinear_workspace_bytes", "mi_rank_bilinear",
               "mi_rank_separable_workspace_bytes", "mi_rank_separable")


def test_new_symbols_exported(lib):
    from mutual_info_img_txt import _hip
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.mi_abi_version() == 4
    assert sorted(n for n in _hip.SIGNATURES if n.startswith("mi_rank_")) == sorted(NEW_SYMBOLS)


FAKE = 1 << 20  # never dereferenced: every call below fails its argument checks first
BIG = 1 << 40


def _bilinear(lib, x=FAKE, y=FAKE, w=FAKE, sid=FAKE, b=64, dx=128, dy=128, prec=1, ri=FAKE, rt=FAKE, diag=None, ws=FAKE,
              nbytes=BIG):
    return lib.mi_rank_bilinear(x, y, w, sid, b, dx, dy, prec, ri, rt, diag, ws, nbytes, None)


def _separable(lib, x=FAKE, y=FAKE, wg=FAKE, wh=FAKE, sid=FAKE, b=64, dx=128, dy=128, k=64, prec=1, ri=FAKE, rt=FAKE,
               diag=None, ws=FAKE, nbytes=BIG):
    return lib.mi_rank_separable(x, y, wg, wh, sid, b, dx, dy, k, prec, ri, rt, diag, ws, nbytes, None)


def _err(lib):
    msg = lib.mi_last_error()
    assert msg
    return msg


def test_arguments_rejected_without_gpu(lib):
    EINVAL, EWORKSPACE = -1, -3
    # null pointers
    assert lib.mi_rank_matrix(None, FAKE, 4, FAKE, FAKE, None) == EINVAL and b"null" in _err(lib)
    assert lib.mi_rank_matrix(FAKE, None, 4, FAKE, FAKE, None) == EINVAL and b"null" in _err(lib)
    for arg in ("x", "y", "sid", "ws"):
        assert _bilinear(lib, **{arg: None}) == EINVAL and b"mi_rank_bilinear: null" in _err(lib)
    for arg in ("x", "y", "wg", "wh", "sid", "ws"):
        assert _separable(lib, **{arg: None}) == EINVAL and b"mi_rank_separable: null" in _err(lib)
    # b < 1
    assert lib.mi_rank_matrix(FAKE, FAKE, 0, FAKE, FAKE, None) == EINVAL and b"b must be" in _err(lib)
    assert _bilinear(lib, b=0) == EINVAL and b"sizes" in _err(lib)
    assert _separable(lib, b=-3) == EINVAL and b"sizes" in _err(lib)
    assert _separable(lib, k=0) == EINVAL and b"projection" in _err(lib)
    # both rank pointers NULL; one alone is accepted by the checks (it then fails on the workspace, the next check)
    assert lib.mi_rank_matrix(FAKE, FAKE, 4, None, None, None) == EINVAL and b"rank_i2t" in _err(lib)
    assert _bilinear(lib, ri=None, rt=None) == EINVAL and b"rank_i2t" in _err(lib)
    assert _separable(lib, ri=None, rt=None) == EINVAL and b"rank_i2t" in _err(lib)
    assert _bilinear(lib, ri=None, nbytes=16) == EWORKSPACE
    assert _separable(lib, rt=None, nbytes=16) == EWORKSPACE
    # fp8 / f16 / f16x3 are not precisions of the ranks
    for prec in (3, 4, 5):
        assert _bilinear(lib, prec=prec) == EINVAL and b"precision" in _err(lib)
        assert _separable(lib, prec=prec) == EINVAL and b"precision" in _err(lib)
    # S = X Y^T needs equal widths
    assert _bilinear(lib, w=None, dx=128, dy=64) == EINVAL and b"d_img == d_txt" in _err(lib)
    # workspace too small: one byte short of the query
    for prec in (0, 1, 2):
        need = lib.mi_rank_bilinear_workspace_bytes(64, 128, 128, prec)
        assert _bilinear(lib, prec=prec, nbytes=need - 257) == EWORKSPACE and b"workspace too small" in _err(lib)
        need = lib.mi_rank_separable_workspace_bytes(64, 128, 128, 64, prec)
        assert _separable(lib, prec=prec, nbytes=need - 257) == EWORKSPACE and b"workspace too small" in _err(lib)


def test_workspace_queries_host_only_and_linear_in_b(lib):
    from mutual_info_img_txt import _hip
    for prec in (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3):
        one, two = (lib.mi_rank_bilinear_workspace_bytes(b, 512, 512, prec) for b in (16384, 32768))
        assert 0 < one < two < 2.5 * one, (prec, one, two)  # linear growth: 2x; a b^2 term: 4x
        one, two = (lib.mi_rank_separable_workspace_bytes(b, 512, 512, 256, prec) for b in (16384, 32768))
        assert 0 < one < two < 2.5 * one, (prec, one, two)
        # no G, G^T or tile records: far below the step's workspace, and below one fp32 [b, b] matrix
        assert lib.mi_rank_bilinear_workspace_bytes(16384, 512, 512, prec) < 4 * 16384 * 16384 // 2
        assert (lib.mi_rank_bilinear_workspace_bytes(16384, 512, 512, prec) <
                lib.mi_nce_bilinear_workspace_bytes(16384, 512, 512, prec) // 4)
        # ragged shapes (the generic kernels) are planned too
        assert lib.mi_rank_bilinear_workspace_bytes(200, 60, 60, prec) > 0
        assert lib.mi_rank_separable_workspace_bytes(96, 40, 40, 48, prec) > 0
    assert lib.mi_rank_bilinear_workspace_bytes(0, 8, 8, 1) == 0
    assert lib.mi_rank_separable_workspace_bytes(8, 8, 8, 0, 1) == 0


# ------------------------------------------------------------------------------------------------ Python layer
def test_cpu_tensors_raise():
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.model import BilinearCritic
    from mutual_info_img_txt.retrieval import matrix_retrieval_ranks, retrieval_ranks
    x, y, sid = torch.randn(8, 16), torch.randn(8, 16), [str(n) for n in range(8)]
    with pytest.raises(_hip.MiCriticError):
        retrieval_ranks(x, y, sid, BilinearCritic(16, 16))
    with pytest.raises(_hip.MiCriticError):
        matrix_retrieval_ranks(torch.randn(8, 8), sid)
    with pytest.raises(_hip.MiCriticError):
        MultiModalManager(d_img=16, d_txt=16, critic="separable", d_proj=8).retrieval_eval(x, y, sid)


def test_ops_expose_the_rank_calls():
    from mutual_info_img_txt import critic_ops
    for ops in (critic_ops.HipBilinearOps, critic_ops.HipSeparableOps):
        assert callable(ops.rank_workspace_bytes) and callable(ops.rank_call)
    assert callable(critic_ops.rank_matrix)
    from mutual_info_img_txt import _hip
    # retrieval is not an estimator: the table keeps its six entries
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
