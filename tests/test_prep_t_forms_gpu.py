"""The prep launch of the bilinear step has two forms of its T role (csrc/mi_gemm_bf16.h, bilinear_prep_t_kernel): 64-row
tiles that also write the fragment-major X^T from the X image they hold in LDS (the step with the two-launch tail: X is
read once, no conversion job for it), and the 128-row tiles with X^T from a conversion job (every other caller, and every
call under MI_PREP_T_TALL=1).  Which workgroup computes and writes what changes, the arithmetic does not: loss, statistics
and every gradient keep their bits under the switch, at the smallest shapes where the new form can go wrong -- and on a
workspace of NaN bit patterns, where an X^T block that no tile wrote would reach grad_w."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mutual_info_img_txt import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
# as tests/prep_t_forms_worker.py (CASES): B x d_img x d_txt
CASES = [(b, dx, dy) for b in (128, 384) for dx in (64, 192, 512) for dy in (128, 512)]
OUTPUTS = ("loss", "stats", "grad_x", "grad_y", "grad_param0")


def _run(path, tall):
    env = dict(os.environ)
    env.pop("MI_PREP_T_TALL", None)
    if tall:
        env["MI_PREP_T_TALL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "prep_t_forms_worker.py"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """Every case once per switch value: one fresh child process each (the library reads the switch once)."""
    d = tmp_path_factory.mktemp("prep_t_forms")
    return _run(d / "default.npz", False), _run(d / "tall.npz", True)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: the form of the T role changed bits"


@pytest.mark.gpu
@pytest.mark.parametrize("b,dx,dy", CASES)
def test_bilinear_step_keeps_every_bit_under_the_switch(forms, b, dx, dy):
    default, tall = forms
    key = f"b{b}_{dx}_{dy}"
    # both runs took the fused kernels with the two-launch tail: the only plan in which the T tiles write X^T
    assert int(default[f"{key}/path"][0]) == _hip.MI_PATH_FUSED_TAIL and int(tall[f"{key}/path"][0]) == _hip.MI_PATH_FUSED_TAIL
    for k in OUTPUTS:
        _same_bits(default[f"{key}/{k}"], tall[f"{key}/{k}"], f"{key}/{k}")
    for k in ("grad_x", "grad_y", "grad_param0"):
        g = default[f"{key}/{k}"]
        assert np.isfinite(g).all() and np.abs(g).max() > 0, f"{key}/{k}"


@pytest.mark.gpu
def test_every_xt_block_is_written(forms):
    """The same step on a workspace filled with 0xFF bytes (NaNs as bf16 and as fp32) beforehand."""
    default, tall = forms
    b, dx, dy = 384, 192, 512
    assert int(default["poisoned/path"][0]) == _hip.MI_PATH_FUSED_TAIL and int(tall["poisoned/path"][0]) == _hip.MI_PATH_FUSED_TAIL
    for k in OUTPUTS:
        _same_bits(default[f"poisoned/{k}"], tall[f"poisoned/{k}"], f"poisoned/{k}")
        _same_bits(default[f"poisoned/{k}"], default[f"b{b}_{dx}_{dy}/{k}"], f"poisoned/{k} against the clean workspace")
    assert np.isfinite(default["poisoned/grad_param0"]).all()


@pytest.mark.gpu
def test_separable_step_keeps_the_tall_form_and_its_bits(forms):
    """(B, d_img, d_txt, d_proj) = (128, 64, 96, 128): a caller whose prep launch does not change."""
    default, tall = forms
    keys = sorted(k for k in default.files if k.startswith("separable/"))
    assert keys == sorted(k for k in tall.files if k.startswith("separable/"))
    assert {"separable/loss", "separable/stats", "separable/grad_x", "separable/grad_y", "separable/grad_param0",
            "separable/grad_param1"} <= set(keys)
    for k in keys:
        _same_bits(default[k], tall[k], k)
    for k in ("separable/grad_x", "separable/grad_y", "separable/grad_param0", "separable/grad_param1"):
        assert np.isfinite(default[k]).all() and np.abs(default[k]).max() > 0, k
