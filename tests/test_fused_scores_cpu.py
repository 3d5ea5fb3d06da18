"""The make_mlp critic as a differentiable score matrix, host side: the two C-ABI symbols (header, signature table and
library agree; arguments are checked before any device work; the workspace query is unchanged), the argument validation
of ``fused_scores.fused_critic_scores`` and the estimator table, which this route leaves as it is.  No GPU needed."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_concat_mlp_scores_fwd", "mi_concat_mlp_bwd_from_g")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


def _header_args(name):
    """Argument declarations of ``name`` in include/mi_critic.h (comments stripped)."""
    text = open(os.path.join(ROOT, "include", "mi_critic.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/mi_critic.h"
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    from ctypes import c_int, c_int64, c_size_t, c_void_p
    if "*" in decl:
        return c_void_p
    return {"int64_t": c_int64, "int": c_int, "size_t": c_size_t}[decl.split()[0]]


@pytest.mark.parametrize("name", NEW)
def test_header_signatures_and_library_agree(lib, name):
    from mutual_info_img_txt import _hip
    args = _header_args(name)
    res, argtypes = _hip.SIGNATURES[name]
    assert [_ctype_of(a) for a in args] == list(argtypes)
    assert hasattr(lib, name)
    # the argument lists the issue fixes: no study ids, no estimator, no row offset
    names = [re.split(r"[\s*]+", a)[-1] for a in args]
    assert names[:8] == ["x", "y", "w1", "b1", "w2", "b2", "w3", "b3"]
    assert names[8:15] == ["b_rows", "b", "d_img", "d_txt", "h1", "h2", "precision"]
    assert names[-3:] == ["workspace", "workspace_bytes", "stream"]
    if name == "mi_concat_mlp_scores_fwd":
        assert names[15:-3] == ["need_grad", "scores_out"]
    else:
        assert names[15:-3] == ["grad_scores", "stats_scratch", "grad_x", "grad_y", "grad_w1", "grad_b1", "grad_w2",
                                "grad_b2", "grad_w3", "grad_b3"]


def test_entry_points_validate_before_any_device_work(lib):
    one = 1  # any non-null address: the checks below fail before a pointer is used
    p8 = [one] * 8
    shape = (64, 64, 32, 32, 64, 256)
    assert lib.mi_concat_mlp_scores_fwd(*[None] * 8, *shape, 0, 1, None, None, 0, None) == -1
    assert b"mi_concat_mlp_scores_fwd: null pointer" in lib.mi_last_error()
    assert lib.mi_concat_mlp_bwd_from_g(*[None] * 8, *shape, 0, *[None] * 10, None, 0, None) == -1
    assert b"mi_concat_mlp_bwd_from_g: null pointer" in lib.mi_last_error()
    # b_rows > b
    assert lib.mi_concat_mlp_scores_fwd(*p8, 65, 64, 32, 32, 64, 256, 0, 1, one, one, 1 << 30, None) == -1
    assert b"need 1 <= b_rows <= b" in lib.mi_last_error()
    assert lib.mi_concat_mlp_bwd_from_g(*p8, 65, 64, 32, 32, 64, 256, 0, *[one] * 10, one, 1 << 30, None) == -1
    # hidden sizes outside the fused kernels, a precision of another critic
    assert lib.mi_concat_mlp_scores_fwd(*p8, 64, 64, 32, 32, 100, 256, 0, 1, one, one, 1 << 30, None) == -2
    assert b"h1 % 64 == 0" in lib.mi_last_error()
    assert lib.mi_concat_mlp_bwd_from_g(*p8, 64, 64, 32, 32, 64, 128, 0, *[one] * 10, one, 1 << 30, None) == -2
    assert lib.mi_concat_mlp_scores_fwd(*p8, *shape, 2, 1, one, one, 1 << 30, None) == -1  # MI_PREC_BF16X3
    assert b"precision 2" in lib.mi_last_error()
    # a short workspace: MI_EWORKSPACE, with the hint of mi_concat_mlp_bwd in the backward
    assert lib.mi_concat_mlp_scores_fwd(*p8, *shape, 0, 1, one, one, 256, None) == -3
    assert lib.mi_concat_mlp_bwd_from_g(*p8, *shape, 0, *[one] * 10, one, 256, None) == -3
    assert b"need_grad = 1" in lib.mi_last_error()
    # a row block is allowed (b_rows < b): it gets as far as the workspace check
    assert lib.mi_concat_mlp_bwd_from_g(*p8, 16, 64, 32, 32, 64, 256, 0, *[one] * 10, one, 256, None) == -3


def test_workspace_query_is_unchanged(lib):
    """No slot was added to the plan: the sizes the library returned before these entry points existed (b_rows, b, d_img,
    d_txt, h1, h2, precision, need_grad)."""
    want = {(130, 130, 32, 32, 64, 512, 0, 1): 4746752, (64, 130, 32, 48, 64, 256, 5, 1): 1481472,
            (4096, 4096, 768, 768, 1024, 512, 4, 1): 3471090176, (4096, 4096, 768, 768, 1024, 512, 5, 0): 69239296,
            (96, 96, 128, 128, 1024, 512, 1, 1): 22119168}
    for args, nbytes in want.items():
        assert lib.mi_concat_mlp_workspace_bytes(*args) == nbytes, args


def _mlp(d, hidden=(64, 256)):
    from mutual_info_img_txt.model import make_mlp
    return make_mlp(d, list(hidden))


def test_argument_validation_of_the_python_function():
    from mutual_info_img_txt import fused_scores
    from mutual_info_img_txt._hip import MiCriticError
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    x, y = torch.zeros(8, 16), torch.zeros(12, 24)
    good = _mlp(40)
    # not a make_mlp critic: the other critics, None, a Sequential of another structure
    for critic in (BilinearCritic(16, 24), SeparableCritic(16, 24, 8), None, _mlp(40, (64,)),
                   torch.nn.Sequential(torch.nn.Linear(40, 64), torch.nn.Tanh(), torch.nn.Linear(64, 256),
                                       torch.nn.ReLU(), torch.nn.Linear(256, 1))):
        with pytest.raises(ValueError, match="make_mlp"):
            fused_scores.fused_critic_scores(x, y, critic)
    with pytest.raises(ValueError, match="n_img <= n_txt"):
        fused_scores.fused_critic_scores(torch.zeros(13, 16), y, good)
    with pytest.raises(ValueError, match="critic expects 40 inputs"):
        fused_scores.fused_critic_scores(torch.zeros(8, 20), y, good)
    with pytest.raises(ValueError, match="unknown precision"):
        fused_scores.fused_critic_scores(x, y, good, precision="f64")
    for prec in ("bf16x3", "fp8"):
        with pytest.raises(ValueError, match="BilinearCritic only"):
            fused_scores.fused_critic_scores(x, y, good, precision=prec)
    with pytest.raises(ValueError):
        fused_scores.fused_critic_scores(torch.zeros(8), y, good)
    # valid arguments on the CPU: no fallback
    with pytest.raises(MiCriticError):
        fused_scores.fused_critic_scores(x, y, good)
    with pytest.raises(MiCriticError):
        fused_scores.concat_infonce(torch.zeros(8, 16), torch.zeros(8, 24), list("abcdefgh"), good)


def test_precision_names_resolve_as_for_dv():
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import resolve_critic
    codes = {p: resolve_critic(_mlp(40), p, 12, 16, 24)[2] for p in ("f32", "f32_exact", "bf16", "f16")}
    assert codes == {"f32": _hip.MI_PREC_F16X3, "f32_exact": _hip.MI_PREC_F32, "bf16": _hip.MI_PREC_BF16,
                     "f16": _hip.MI_PREC_F16}


def test_estimator_table_is_untouched():
    from mutual_info_img_txt import _hip
    for est in ("infonce_rowwise", "infonce_symmetric"):
        with pytest.raises(ValueError, match="bilinear and separable critics only"):
            _hip.check_estimator(est, "concat_mlp")
        assert _hip.ESTIMATOR_TABLE[est].critics == ("bilinear", "separable")
