"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol declared in
include/mi_critic.h; the host wrappers validate eagerly and never fall back to the CPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "mi_critic.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib):
    from mutual_info_img_txt import _hip
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mi_critic.h but not exported"
    assert sorted(_hip.SIGNATURES) == declared, "ctypes signature table out of sync with the header"
    assert lib.mi_abi_version() == 4


def test_workspace_queries_are_host_only(lib):
    assert lib.mi_bound_workspace_bytes(10) > 0
    assert lib.mi_pair_index_workspace_bytes(4096) >= (4096 * 4095 // 1024) * 12
    small = lib.mi_bilinear_workspace_bytes(64, 64, 128, 128, 1)
    big = lib.mi_bilinear_workspace_bytes(4096, 4096, 512, 512, 1)
    assert big > small and big >= 4096 * 4096 * 2
    assert lib.mi_concat_mlp_workspace_bytes(64, 64, 768, 768, 1024, 512, 1, 1) > 0


def test_argument_validation_without_gpu(lib):
    # null pointers are rejected before anything touches the device
    assert lib.mi_bound_fwd(None, 4, 2, 0, None, None, None, 0, None) == -1
    assert b"null" in lib.mi_last_error()
    assert lib.mi_merge_partials(None, 1, 1, 0, None, None, None) == -1


def test_round3_entry_points_validate_without_gpu(lib):
    """mi_bilinear_step / prep_local / fp8_stage / bwd_records reject bad arguments before anything touches the device,
    and mi_bilinear_raw_records is a pure host query."""
    import ctypes
    assert lib.mi_bilinear_step(None, None, None, None, 64, 128, 128, 1, 1, None, None, None, None, None, None, None, None, 0,
                                None) == -1
    assert b"null" in lib.mi_last_error()
    assert lib.mi_bilinear_prep_local(None, None, 64, 64, 128, 128, 1, None, 0, None) == -1
    assert lib.mi_bilinear_fp8_stage(None, None, None, 64, 64, 128, 128, 0, None, None, 0, None) == -1
    assert lib.mi_bilinear_bwd_records(None, None, None, None, None, 64, 64, 0, 128, 128, 1, 1, None, 0, 0, None, None, None,
                                       None, None, None, None, 0, None) == -1
    off = ctypes.c_size_t(0)
    # 512-row block of a 4096 batch at d = 512, bf16: 4 row blocks of 128 x 32 column splits (the plan fills the 256 CUs)
    # x 4 waves = 512 records of 16 bytes
    n = lib.mi_bilinear_raw_records(512, 4096, 512, 512, 1, ctypes.byref(off))
    assert n == 512 and off.value % 256 == 0
    assert off.value + 16 * n <= lib.mi_bilinear_workspace_bytes(512, 4096, 512, 512, 1)
    assert lib.mi_bilinear_raw_records(4096, 4096, 512, 512, 1, None) == 512  # 32 row blocks x 4 splits x 4 waves
    # shapes / precisions outside the fused kernels have no raw records
    assert lib.mi_bilinear_raw_records(512, 4096, 768, 768, 1, None) == 0      # width 768
    assert lib.mi_bilinear_raw_records(500, 4096, 512, 512, 1, None) == 0      # ragged row block
    assert lib.mi_bilinear_raw_records(512, 4096, 512, 512, 0, None) == 0      # f32


def test_no_cpu_fallback():
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import make_mlp
    logits = torch.zeros(8, 1)
    with pytest.raises(MiCriticError):
        mi_critics.dv_bound_loss(logits, 2, "cpu")
    with pytest.raises(MiCriticError):
        mi_critics.infonce_bound_loss(logits, 2, "cpu")
    with pytest.raises(MiCriticError):
        mi_critics.fused_mi_bound(torch.zeros(4, 8), torch.zeros(4, 8), ["a", "b", "c", "d"], make_mlp(16, [8, 8]))


def test_host_logic():
    from mutual_info_img_txt import mi_critics
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic, make_mlp
    codes = mi_critics.study_id_codes(["s1", "s2", "s1", "s3"], "cpu")
    assert codes.dtype == torch.int64 and codes[0] == codes[2] and len(set(codes.tolist())) == 3
    assert mi_critics.study_id_codes(["50000002", "50000001"], "cpu").tolist() == [50000002, 50000001]  # same on every rank
    mlp = make_mlp(1536, [1024, 512])
    assert list(mlp.state_dict().keys()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
    w1, b1, w2, b2, w3, b3 = mi_critics._concat_params(mlp)
    assert w1.shape == (1024, 1536) and w2.shape == (512, 1024) and w3.shape == (1, 512)
    with pytest.raises(ValueError):
        mi_critics._concat_params(make_mlp(16, [8]))  # only two hidden layers are fused
    with pytest.raises(KeyError):
        make_mlp(16, [8, 8], activation="tanh")  # same failure mode as the reference (model.py:21-23)
    with pytest.raises(ValueError):
        mi_critics._estimator_code("mine")
    assert BilinearCritic(8, 12).weight.shape == (8, 12)
    assert SeparableCritic(8, 12, 4)(torch.zeros(3, 8), torch.zeros(3, 12)).shape == (3, 3)


def test_make_mlp_matches_reference_structure(golden):
    from mutual_info_img_txt.model import make_mlp
    g = golden("g0_make_mlp.npz")
    mlp = make_mlp(1536, [1024, 512])
    assert [type(m).__name__ for m in mlp] == list(g["kinds"])
    assert list(mlp.state_dict().keys()) == list(g["keys"])
    assert [str(tuple(v.shape)) for v in mlp.state_dict().values()] == list(g["shapes"])


def test_path_queries(lib, caplog):
    """mi_bilinear_path / mi_separable_path are host-only; the binding warns ONCE per shape that leaves the fused kernels."""
    import logging
    from mutual_info_img_txt import _hip
    assert lib.mi_bilinear_path(4096, 4096, 512, 512, _hip.MI_PREC_BF16) == _hip.MI_PATH_FUSED_TAIL
    assert lib.mi_bilinear_path(4096, 4096, 512, 512, _hip.MI_PREC_F32) == _hip.MI_PATH_GENERIC
    assert lib.mi_bilinear_path(4096, 4096, 512, 512, _hip.MI_PREC_BF16X3) == _hip.MI_PATH_GEMMS
    assert lib.mi_bilinear_path(8192, 8192, 1024, 1024, _hip.MI_PREC_FP8) == _hip.MI_PATH_FP8_GEMMS
    assert lib.mi_bilinear_path(4000, 4000, 520, 520, _hip.MI_PREC_BF16) == _hip.MI_PATH_GEMMS    # width outside the fused kernel
    assert lib.mi_bilinear_path(0, 4096, 512, 512, 1) == -1
    assert lib.mi_separable_path(256, 256, 256, 256, 256, _hip.MI_PREC_BF16) >= _hip.MI_PATH_FUSED
    with caplog.at_level(logging.WARNING, logger="mutual_info_img_txt"):
        _hip._warned_paths.clear()
        assert _hip.note_path("bilinear", (4000, 4000, 520, 520), _hip.MI_PREC_BF16) == _hip.MI_PATH_GEMMS
        assert _hip.note_path("bilinear", (4000, 4000, 520, 520), _hip.MI_PREC_BF16) == _hip.MI_PATH_GEMMS
        assert _hip.note_path("bilinear", (4096, 4096, 512, 512), _hip.MI_PREC_BF16) == _hip.MI_PATH_FUSED_TAIL
    assert sum("outside the fused" in r.getMessage() for r in caplog.records) == 1


def test_gemm16_variant_query(lib):
    """mi_gemm16_variant is host-only and reports the kernel the 16-bit GEMM launcher switches on.  The six boundary
    shapes of tests/gemm_variant_cases.py (the smallest ragged batch that reaches each kernel), a zero size, and the whole
    table with its rectangular forms -- so a threshold change fails here and does not quietly take a kernel out of
    tests/test_gemm_variants_gpu.py."""
    import gemm_variant_cases as cases
    from mutual_info_img_txt import _hip
    v = lib.mi_gemm16_variant
    assert v(136, 136, 40) == _hip.MI_GEMM16_PLAIN          # K % 64 != 0
    assert v(136, 136, 64) == _hip.MI_GEMM16_GLDS           # K < 256
    assert v(3000, 3000, 256) == _hip.MI_GEMM16_GLDS        # 24 x 24 = 576 tiles of 128 > 512
    assert v(136, 136, 256) == _hip.MI_GEMM16_GLDS4
    assert v(136, 136, 2112) == _hip.MI_GEMM16_PIPE128 and v(136, 136, 2048) == _hip.MI_GEMM16_PIPE128
    assert v(2312, 2312, 2112) == _hip.MI_GEMM16_PIPE256X128  # 10 x 19 = 190 tiles of 256 x 128
    assert v(3336, 3336, 64) == _hip.MI_GEMM16_BIG          # 14 x 14 = 196 tiles of 256 x 256
    assert v(4096, 4096, 512) == _hip.MI_GEMM16_BIG         # the product's own batch (BASELINE.json configs[3])
    # one step inside each threshold
    assert v(3328, 3328, 64) == _hip.MI_GEMM16_GLDS and v(2312, 2312, 1984) == _hip.MI_GEMM16_GLDS4
    assert v(136, 136, 192) == _hip.MI_GEMM16_GLDS and v(2816, 2816, 256) == _hip.MI_GEMM16_GLDS4  # 22 x 22 = 484 tiles
    for bad in ((0, 136, 64), (136, 0, 64), (136, 136, 0), (-8, 136, 64)):
        assert v(*bad) == -1
    assert (_hip.MI_GEMM16_PLAIN, _hip.MI_GEMM16_GLDS, _hip.MI_GEMM16_GLDS4, _hip.MI_GEMM16_PIPE128,
            _hip.MI_GEMM16_PIPE256X128, _hip.MI_GEMM16_BIG) == (0, 1, 2, 3, 4, 5)
    header = open(os.path.join(ROOT, "include", "mi_critic.h")).read()
    for name in cases.VARIANTS:
        assert re.search(rf"#define MI_GEMM16_{name} {getattr(_hip, 'MI_GEMM16_' + name)}\b", header), name
    cases.check_table()
    # the exact data of the GPU tests: exactness in bf16 is asserted inside, on the host
    for name in ("plain", "pipe128"):
        c = cases.exact_case(name)
        assert c["s_all"].shape == (136 + cases.EXTRA,) * 2 and c["x"].shape == (136, cases.D_IMG)
    assert cases.seam_ids(3336)[[3, 3335, 258, 3333]].tolist() == [2, 0, 254, 300]
    assert cases.seam_ids(136)[[3, 135, 130]].tolist() == [2, 0, 126]

