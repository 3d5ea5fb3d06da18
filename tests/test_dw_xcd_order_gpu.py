"""bilinear_dw_kernel hands each XCD a block of dW tiles instead of the row-major order (csrc/mi_bilinear_tail.h).  Which
workgroup computes which tile changes, the tile's arithmetic does not: under MI_DW_XCD_NATURAL=1 (the order before) every
output of the step keeps its bits -- the bilinear step at B = 4096, d = 512 (16 x 16 tiles: 4 x 8 per XCD) and the separable
step at B = 256, d = 256 (two products of 8 x 8 tiles in one launch: 2 x 4 per XCD each)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mutual_info_img_txt import _hip

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(path, natural):
    env = dict(os.environ)
    env.pop("MI_DW_XCD_NATURAL", None)
    if natural:
        env["MI_DW_XCD_NATURAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "dw_order_worker.py"), str(path)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


@pytest.mark.gpu
def test_dw_tile_order_keeps_every_bit(tmp_path):
    blocks, natural = _run(tmp_path / "blocks.npz", False), _run(tmp_path / "natural.npz", True)
    assert sorted(blocks.files) == sorted(natural.files)
    # both steps ran the fused kernels with the two-launch tail: the dW kernel under test
    assert int(blocks["bilinear_path"][0]) == _hip.MI_PATH_FUSED_TAIL and int(blocks["separable_path"][0]) == _hip.MI_PATH_FUSED_TAIL
    assert "bilinear_grad_param0" in blocks.files and "separable_grad_param1" in blocks.files
    for k in blocks.files:
        a, b = blocks[k], natural[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{k}: the tile order changed bits"
    for k in ("bilinear_grad_param0", "separable_grad_param0", "separable_grad_param1"):
        assert np.isfinite(blocks[k]).all() and np.abs(blocks[k]).max() > 0, k
