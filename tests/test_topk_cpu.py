"""Top-k retrieval over a gallery, host side: the mi_topk_* symbols of the C ABI (exported, in the signature table,
argument checks before any device work, host-only workspace queries), ``gallery_recall`` on hand-made indices, the
tie order of the fp64 restatement (tests/topk_reference.py) and the CPU-tensor errors.  No GPU needed."""
import pytest
import torch

import topk_reference as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


NEW_SYMBOLS = ("mi_topk_matrix_workspace_bytes", "mi_topk_matrix", "mi_topk_bilinear_workspace_bytes", "mi_topk_bilinear",
               "mi_topk_separable_workspace_bytes", "mi_topk_separable")


def test_new_symbols_exported(lib):
    import os
    from mutual_info_img_txt import _hip
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert sorted(n for n in _hip.SIGNATURES if n.startswith("mi_topk_")) == sorted(NEW_SYMBOLS)
    assert lib.mi_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi_critic.h")).read()
    assert "#define MI_TOPK_MAX_K 32" in header and _hip.MI_TOPK_MAX_K == 32


def test_workspace_queries_positive_and_growing(lib):
    from mutual_info_img_txt import _hip
    for axis in (0, 1):
        one, two = (lib.mi_topk_matrix_workspace_bytes(n, n, 10, axis) for n in (1000, 2000))
        assert 0 < one < two
    # the lists alone: 8 bytes per (query, slot), the query side chosen by the axis
    assert lib.mi_topk_matrix_workspace_bytes(100, 7, 32, 0) >= 100 * 32 * 8 > lib.mi_topk_matrix_workspace_bytes(100, 7, 32, 1)
    for prec in (_hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3):
        one, two = (lib.mi_topk_bilinear_workspace_bytes(n, 2 * n, 512, 512, prec, 10) for n in (8192, 16384))
        assert 0 < one < two < 2.5 * one, (prec, one, two)  # linear in the counts: no [n_img, n_txt] term
        assert two < 4 * 16384 * 32768  # below ONE fp32 [n_img, n_txt] matrix
        one, two = (lib.mi_topk_separable_workspace_bytes(n, 2 * n, 512, 512, 256, prec, 10) for n in (8192, 16384))
        assert 0 < one < two < 2.5 * one, (prec, one, two)
        # k adds 8 (n_img + n_txt) bytes per slot
        k1, k32 = (lib.mi_topk_bilinear_workspace_bytes(1024, 4096, 512, 512, prec, k) for k in (1, 32))
        assert 0 <= (k32 - k1) - 31 * 8 * (1024 + 4096) < 1024
        assert lib.mi_topk_bilinear_workspace_bytes(200, 77, 60, 60, prec, 5) > 0   # ragged: the generic kernels
        assert lib.mi_topk_separable_workspace_bytes(96, 41, 40, 40, 48, prec, 5) > 0
    assert lib.mi_topk_bilinear_workspace_bytes(0, 8, 8, 8, 1, 5) == 0
    assert lib.mi_topk_bilinear_workspace_bytes(8, 8, 8, 8, 1, 33) == 0
    assert lib.mi_topk_separable_workspace_bytes(8, 8, 8, 8, 0, 1, 5) == 0
    assert lib.mi_topk_matrix_workspace_bytes(8, 8, 0, 0) == 0 and lib.mi_topk_matrix_workspace_bytes(8, 8, 5, 2) == 0


FAKE = 1 << 20  # never dereferenced: every call below fails its argument checks first
BIG = 1 << 40
EINVAL, EWORKSPACE = -1, -3


def _matrix(lib, s=FAKE, nr=8, nc=9, sr=None, sc=None, k=5, axis=0, idx=FAKE, val=FAKE, ws=FAKE, nbytes=BIG):
    return lib.mi_topk_matrix(s, nr, nc, sr, sc, k, axis, idx, val, ws, nbytes, None)


def _bilinear(lib, x=FAKE, y=FAKE, w=FAKE, si=None, st=None, ni=64, nt=72, dx=128, dy=128, prec=1, k=5, ii=FAKE, vi=FAKE,
              it=FAKE, vt=FAKE, ws=FAKE, nbytes=BIG):
    return lib.mi_topk_bilinear(x, y, w, si, st, ni, nt, dx, dy, prec, k, ii, vi, it, vt, ws, nbytes, None)


def _separable(lib, x=FAKE, y=FAKE, wg=FAKE, wh=FAKE, si=None, st=None, ni=64, nt=72, dx=128, dy=128, dp=64, prec=1, k=5,
               ii=FAKE, vi=FAKE, it=FAKE, vt=FAKE, ws=FAKE, nbytes=BIG):
    return lib.mi_topk_separable(x, y, wg, wh, si, st, ni, nt, dx, dy, dp, prec, k, ii, vi, it, vt, ws, nbytes, None)


def _err(lib):
    msg = lib.mi_last_error()
    assert msg
    return msg


def test_arguments_rejected_without_gpu(lib):
    # null pointers
    for arg in ("s", "idx", "val", "ws"):
        assert _matrix(lib, **{arg: None}) == EINVAL and b"mi_topk_matrix: null" in _err(lib)
    for arg in ("x", "y", "ws"):
        assert _bilinear(lib, **{arg: None}) == EINVAL and b"mi_topk_bilinear: null" in _err(lib)
    for arg in ("x", "y", "wg", "wh", "ws"):
        assert _separable(lib, **{arg: None}) == EINVAL and b"mi_topk_separable: null" in _err(lib)
    # sizes below 1, sizes at or above 2^31
    assert _matrix(lib, nr=0) == EINVAL and b"sizes" in _err(lib)
    assert _matrix(lib, nc=1 << 31) == EINVAL and b"2^31" in _err(lib)
    assert _matrix(lib, nr=1 << 31) == EINVAL and b"2^31" in _err(lib)
    assert _bilinear(lib, ni=0) == EINVAL and b"sizes" in _err(lib)
    assert _bilinear(lib, nt=-2) == EINVAL and b"sizes" in _err(lib)
    for arg in ("ni", "nt", "dx", "dy"):
        assert _bilinear(lib, **{arg: 1 << 31}) == EINVAL and b"2^31" in _err(lib)
        assert _separable(lib, **{arg: 1 << 31}) == EINVAL and b"2^31" in _err(lib)
    assert _separable(lib, dp=0) == EINVAL and b"projection" in _err(lib)
    assert _separable(lib, dp=1 << 31) == EINVAL and b"projection" in _err(lib)
    # k outside [1, MI_TOPK_MAX_K]
    for k in (0, -1, 33):
        assert _matrix(lib, k=k) == EINVAL and b"k must be" in _err(lib)
        assert _bilinear(lib, k=k) == EINVAL and b"k must be" in _err(lib)
        assert _separable(lib, k=k) == EINVAL and b"k must be" in _err(lib)
    # the axis
    assert _matrix(lib, axis=2) == EINVAL and b"axis" in _err(lib)
    # ids: both or neither
    assert _matrix(lib, sr=FAKE) == EINVAL and b"sid_rows" in _err(lib)
    assert _matrix(lib, sc=FAKE) == EINVAL and b"sid_rows" in _err(lib)
    assert _bilinear(lib, si=FAKE) == EINVAL and b"sid_img" in _err(lib)
    assert _separable(lib, st=FAKE) == EINVAL and b"sid_img" in _err(lib)
    # both directions NULL; half a direction
    assert _bilinear(lib, ii=None, vi=None, it=None, vt=None) == EINVAL and b"i2t" in _err(lib)
    assert _separable(lib, ii=None, vi=None, it=None, vt=None) == EINVAL and b"i2t" in _err(lib)
    assert _bilinear(lib, vi=None) == EINVAL and b"go together" in _err(lib)
    assert _separable(lib, it=None) == EINVAL and b"go together" in _err(lib)
    # one direction alone passes the checks (it then fails on the workspace, the next check); n_img != n_txt too
    assert _bilinear(lib, ii=None, vi=None, nbytes=16) == EWORKSPACE
    assert _separable(lib, it=None, vt=None, nbytes=16) == EWORKSPACE
    assert _matrix(lib, nbytes=16) == EWORKSPACE and b"workspace too small" in _err(lib)
    # fp8 / f16 / f16x3 are not precisions of the top-k
    for prec in (3, 4, 5):
        assert _bilinear(lib, prec=prec) == EINVAL and b"precision" in _err(lib)
        assert _separable(lib, prec=prec) == EINVAL and b"precision" in _err(lib)
    # S = X Y^T needs equal widths
    assert _bilinear(lib, w=None, dx=128, dy=64) == EINVAL and b"d_img == d_txt" in _err(lib)
    # workspace one byte short of the query
    for prec in (0, 1, 2):
        need = lib.mi_topk_bilinear_workspace_bytes(64, 72, 128, 128, prec, 5)
        assert _bilinear(lib, prec=prec, nbytes=need - 257) == EWORKSPACE and b"workspace too small" in _err(lib)
        need = lib.mi_topk_separable_workspace_bytes(64, 72, 128, 128, 64, prec, 5)
        assert _separable(lib, prec=prec, nbytes=need - 257) == EWORKSPACE and b"workspace too small" in _err(lib)
    need = lib.mi_topk_matrix_workspace_bytes(8, 9, 5, 0)
    assert _matrix(lib, nbytes=need - 257) == EWORKSPACE


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_tie_order_exclusion_and_tail():
    s = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0],
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]], dtype=torch.float64)
    idx, val = ref.topk(s, 4)
    assert idx.tolist() == [[1, 2, 5, 0], [0, 1, 2, 3]]            # equal scores: the lower index first
    assert val.tolist() == [[3.0, 3.0, 3.0, 1.0], [2.0] * 4]
    idx, _ = ref.topk(s, 6)
    assert idx[0].tolist() == [1, 2, 5, 0, 3, 4]                    # -0.0 and +0.0 tie: index order
    # exclusion by id: query 0 loses candidates 1 and 5, query 1 loses candidate 0; the tail is -1 / -inf
    idx, val = ref.topk(s, 5, q_ids=[7, 9], g_ids=[9, 7, 1, 2, 3, 7])
    assert idx.tolist() == [[2, 0, 3, 4, -1], [1, 2, 3, 4, 5]]
    assert val[0].tolist() == [3.0, 1.0, 0.0, 0.0, float("-inf")]
    # k above the number of candidates, every id equal
    idx, val = ref.topk(s[:, :2], 3)
    assert idx.tolist() == [[1, 0, -1], [0, 1, -1]] and val[1].tolist() == [2.0, 2.0, float("-inf")]
    idx, val = ref.topk(s, 2, q_ids=[4, 4], g_ids=[4] * 6)
    assert idx.tolist() == [[-1, -1]] * 2 and bool(torch.isinf(val).all())
    # the two directions are the matrix and its transpose
    both = ref.both_directions(s, 2)
    assert both["i2t"][0].tolist() == [[1, 2], [0, 1]]
    assert both["t2i"][0].tolist() == [[1, 0], [0, 1], [0, 1], [1, 0], [1, 0], [0, 1]]


def test_cascade_ends_with_the_top_k_under_random_interleavings():
    """The insertion of csrc/mi_topk.h replayed on the host: a thread reads the last slot (fresh or stale) as its
    threshold, and a key above it walks the slots with one atomic max per step, carrying the smaller value on.  Steps of
    different threads interleave at random.  Whatever the order, the slots end as the k largest keys."""
    import random
    rng = random.Random(20260)
    for _ in range(2000):
        k, n = rng.randint(1, 6), rng.randint(1, 24)
        keys = rng.sample(range(1, 1000), n)   # distinct, none 0 (0 = empty)
        slots, stale = [0] * k, 0
        pending, running = list(keys), []
        while pending or running:
            if pending and (not running or rng.random() < 0.4):
                key = pending.pop()
                if key > rng.choice((stale, slots[k - 1])):
                    running.append([key, 0])
            else:
                t = rng.choice(running)
                old = slots[t[1]]
                slots[t[1]] = max(old, t[0])   # atomicMax returns old
                t[0], t[1] = min(old, t[0]), t[1] + 1
                if t[0] == 0 or t[1] == k:
                    running.remove(t)
            if rng.random() < 0.3:
                stale = slots[k - 1]           # some earlier value of the last slot
        assert sorted(slots, reverse=True) == (sorted(keys, reverse=True) + [0] * k)[:k]


# ------------------------------------------------------------------------------------------------ Python layer
def test_gallery_recall_hand_made():
    from mutual_info_img_txt.retrieval import gallery_recall
    # 4 query images of studies a, a, b, c (two images of one study) against 5 reports of studies b, a, c, d, a
    q_ids, g_ids = ["a", "a", "b", "c"], ["b", "a", "c", "d", "a"]
    idx = torch.tensor([[1, 0, 2],      # hit at place 1
                        [0, 3, 4],      # report 4 is study a too: hit at place 3
                        [3, -1, -1],    # a short list: -1 never hits, no hit
                        [0, 2, 1]],     # hit at place 2
                       dtype=torch.int32)
    m = gallery_recall(idx, q_ids, g_ids, ks=(1, 2, 3))
    assert set(m) == {"recall@1", "recall@2", "recall@3", "mrr"}
    assert m["recall@1"] == 0.25 and m["recall@2"] == 0.5 and m["recall@3"] == 0.75
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 0 + 1 / 2) / 4, abs=1e-15)
    # a -1 must not be read as "the last report" (study a would hit for query 1)
    assert gallery_recall(torch.tensor([[-1], [-1]]), ["a", "a"], g_ids, ks=(1,)) == {"recall@1": 0.0, "mrr": 0.0}
    with pytest.raises(ValueError):
        gallery_recall(idx, q_ids, g_ids, ks=(1, 5))      # K = 5 > k = 3
    with pytest.raises(ValueError):
        gallery_recall(idx, q_ids[:3], g_ids)             # one id per query
    with pytest.raises(ValueError):
        gallery_recall(torch.tensor([[5]]), ["a"], g_ids, ks=(1,))  # index outside the gallery


def test_cpu_tensors_and_bad_arguments_raise():
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.main_utils import MultiModalManager
    from mutual_info_img_txt.model import BilinearCritic
    from mutual_info_img_txt.retrieval import matrix_topk, retrieval_topk
    x, y = torch.randn(8, 16), torch.randn(12, 16)
    with pytest.raises(_hip.MiCriticError):
        retrieval_topk(x, y, BilinearCritic(16, 16), 3)
    with pytest.raises(_hip.MiCriticError):
        matrix_topk(torch.randn(8, 12), 3)
    with pytest.raises(_hip.MiCriticError):
        MultiModalManager(d_img=16, d_txt=16, critic="separable", d_proj=8).gallery_eval(
            x, list(range(8)), y, list(range(12)), ks=(1,))


def test_ops_expose_the_topk_calls():
    from mutual_info_img_txt import critic_ops
    for ops in (critic_ops.HipBilinearOps, critic_ops.HipSeparableOps):
        assert callable(ops.topk_workspace_bytes) and callable(ops.topk_call)
    assert callable(critic_ops.topk_matrix)
    from mutual_info_img_txt import _hip
    assert sorted(_hip.ESTIMATOR_TABLE) == ["dv", "infonce", "infonce_rowwise", "infonce_symmetric", "jsd", "nwj"]
