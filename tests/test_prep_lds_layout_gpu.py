"""Two side launches of the bilinear step changed where nothing of their arithmetic lives.

The prep launch (csrc/mi_gemm_bf16.h, bilinear_prep_t_kernel): the [k][n] image of W that feeds the transposing LDS reads
of the T role has 256-byte rows under an XOR swizzle (kPrepTLdB) -- three workgroups per CU for the 64-row form.  A wrong
swizzle constant on either side (staging store, first read, the read four rows on, the second column tile) pairs a lane
with another column of W: T changes, and with it every output.  Every form of the kernel shares that image, so the
reference that knows nothing of it is the float64 oracle (orc.bilinear_step_rounded: rounds where the kernels round): loss
and every gradient of every prep case are held against it at the tolerances of tests/test_gpu_parity.py -- a lane paired
with a wrong column of W puts errors of the size of T itself into all of them.  Beside that, the step with default
settings (64-row tiles) is held bit for bit against the same step under MI_PREP_T_TALL=1 (128-row tiles, X read by
conversion job 0: another instantiation over the same image -- what that comparison covers is the forms' own addressing,
not the swizzle).

The dW launch (csrc/mi_bilinear_tail.h, bilinear_dw_kernel): both problem records are read up front and the problem picked
by selects, the tile decode is 32-bit with one division for both tile orders.  Both problem slots and both decode
branches, default against MI_DW_XCD_NATURAL=1 bit for bit, and grad_w against the oracle.  (Those shapes have a d_img that
is no multiple of 64: their T comes from the plain GEMM, not from the prep launch's T role -- they say nothing about the
W image.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mutual_info_img_txt import _hip
from oracle import mi_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
# as tests/side_launch_worker.py
PREP_CASES = [(128, 64, 128), (128, 128, 256), (256, 192, 384), (256, 192, 256), (384, 512, 512), (128, 512, 128)]
PREP_POISONED = (384, 512, 512)
# d_txt = 384 is no width of the fused B x B kernel (128 / 256 / 512): the library plans the G-materialising products for
# it (mi_bilinear_path says so without a GPU), whose prep launch has 128-row tiles with and without the switch: there the
# bit comparison is one instantiation against itself and only the oracle checks the image (three column tiles).  The case
# stays on the plan it gets; (256, 192, 256) beside it is the same three k-steps on the fused plan.
NOT_FUSED = {(256, 192, 384): _hip.MI_PATH_GEMMS}
DW_CASES = [(128, 32, 128), (128, 96, 128), (128, 160, 256)]
DW_SEPARABLE = [(128, 64, 96, 128), (128, 96, 64, 128)]
OUTPUTS = ("loss", "stats", "grad_x", "grad_y", "grad_param0")
# tests/test_gpu_parity.py, test_bilinear_full_size_vs_oracle / test_bilinear_reference_width_vs_oracle (bf16, fused and
# G-materialising plans alike): every gradient |d| <= 1e-2 * max|grad|, loss |d| < 2e-3 * max(1, max|S|)
GRAD_W_TOL = 1e-2
LOSS_TOL = 2e-3


def _run(path, **switches):
    env = dict(os.environ)
    for k in ("MI_PREP_T_TALL", "MI_DW_XCD_NATURAL"):
        env.pop(k, None)
    env.update(switches)
    r = subprocess.run([sys.executable, os.path.join(HERE, "side_launch_worker.py"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every case once per setting: one fresh child process each (the library reads its switches once)."""
    d = tmp_path_factory.mktemp("side_launches")
    return {"default": _run(d / "default.npz"), "tall": _run(d / "tall.npz", MI_PREP_T_TALL="1"),
            "natural": _run(d / "natural.npz", MI_DW_XCD_NATURAL="1")}


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ"


def _fused_tail(run, key):
    return int(run[f"{key}/path"][0]) == _hip.MI_PATH_FUSED_TAIL


@pytest.mark.gpu
@pytest.mark.parametrize("b,dx,dy", PREP_CASES)
def test_w_image_layout_keeps_every_bit_against_the_tall_form(runs, b, dx, dy):
    default, tall = runs["default"], runs["tall"]
    key = f"prep{b}_{dx}_{dy}"
    if (b, dx, dy) in NOT_FUSED:
        assert int(default[f"{key}/path"][0]) == NOT_FUSED[(b, dx, dy)] == int(tall[f"{key}/path"][0])
    else:
        assert _fused_tail(default, key) and _fused_tail(tall, key)
    for k in OUTPUTS:
        _same_bits(default[f"{key}/{k}"], tall[f"{key}/{k}"], f"{key}/{k}")
    for k in ("grad_x", "grad_y", "grad_param0"):
        g = default[f"{key}/{k}"]
        assert np.isfinite(g).all() and np.abs(g).max() > 0, f"{key}/{k}"


@pytest.fixture(scope="module")
def prep_oracle(runs):
    """orc.bilinear_step_rounded of every prep case, computed once from the inputs the default run saved."""
    out = {}
    for b, dx, dy in PREP_CASES:
        key = f"prep{b}_{dx}_{dy}"
        t = {k: torch.from_numpy(runs["default"][f"{key}/{k}"]) for k in ("x", "y", "param0", "sid")}
        out[(b, dx, dy)] = orc.bilinear_step_rounded(t["x"], t["y"], t["param0"], t["sid"], "infonce")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "tall"])
@pytest.mark.parametrize("b,dx,dy", PREP_CASES)
def test_w_image_layout_against_the_float64_oracle(runs, prep_oracle, form, b, dx, dy):
    """Loss and all three gradients depend on T = X W, the product the W image feeds, in the 64-row and the 128-row form."""
    run, o = runs[form], prep_oracle[(b, dx, dy)]
    key = f"prep{b}_{dx}_{dy}"
    sc = float(o["scores"].abs().max())
    loss = float(run[f"{key}/loss"].reshape(-1)[0])
    errs = {n: _rel(run[f"{key}/{k}"], o[n]) for k, n in (("grad_x", "dx"), ("grad_y", "dy"), ("grad_param0", "dw"))}
    print(f"{key} [{form}]: loss {loss:.6f} vs {float(o['loss']):.6f} (max|S| {sc:.2f}); grad errors / max|grad|:",
          {k: f"{v:.2e}" for k, v in errs.items()})
    assert abs(loss - float(o["loss"])) < LOSS_TOL * max(sc, 1.0), (key, loss, float(o["loss"]))
    for n, err in errs.items():
        assert err < GRAD_W_TOL, (key, n, err)


@pytest.mark.gpu
def test_w_image_layout_on_a_poisoned_workspace(runs):
    """The same step on a workspace filled with 0xFF bytes beforehand: same bits as on the clean one, in both forms."""
    default, tall = runs["default"], runs["tall"]
    key = "prep%d_%d_%d" % PREP_POISONED
    assert _fused_tail(default, "poisoned") and _fused_tail(tall, "poisoned")
    for k in OUTPUTS:
        _same_bits(default[f"poisoned/{k}"], tall[f"poisoned/{k}"], f"poisoned/{k}")
        _same_bits(default[f"poisoned/{k}"], default[f"{key}/{k}"], f"poisoned/{k} against the clean workspace")
    assert np.isfinite(default["poisoned/grad_param0"]).all()


def _rel(got, ref):
    ref = ref.numpy()
    return float(np.abs(got.astype(np.float64) - ref).max()) / float(np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("b,dx,dy", DW_CASES)
def test_dw_head_bilinear_natural_fallback(runs, b, dx, dy):
    """d_img / 32 tile rows is no multiple of 4: the decode takes the natural order with or without the switch."""
    default, natural = runs["default"], runs["natural"]
    key = f"dw{b}_{dx}_{dy}"
    assert _fused_tail(default, key) and _fused_tail(natural, key)
    for k in OUTPUTS:
        _same_bits(default[f"{key}/{k}"], natural[f"{key}/{k}"], f"{key}/{k}")
    t = {k: torch.from_numpy(default[f"{key}/{k}"]) for k in ("x", "y", "param0", "sid")}
    o = orc.bilinear_step_rounded(t["x"], t["y"], t["param0"], t["sid"], "infonce")
    err = _rel(default[f"{key}/grad_param0"], o["dw"])
    print(f"{key}: grad_w error / max|grad_w| = {err:.2e}")
    assert err < GRAD_W_TOL, (key, err)


@pytest.mark.gpu
@pytest.mark.parametrize("b,dx,dy,dp", DW_SEPARABLE)
def test_dw_head_separable_second_problem(runs, b, dx, dy, dp):
    """Two products in one dW launch: the second problem's record, its tile ids counted from the first one's end."""
    default, natural = runs["default"], runs["natural"]
    key = f"sep{b}_{dx}_{dy}_{dp}"
    assert _fused_tail(default, key) and _fused_tail(natural, key)
    for k in OUTPUTS + ("grad_param1",):
        _same_bits(default[f"{key}/{k}"], natural[f"{key}/{k}"], f"{key}/{k}")
    t = {k: torch.from_numpy(default[f"{key}/{k}"]) for k in ("x", "y", "param0", "param1", "sid")}
    o = orc.separable_step_rounded(t["x"], t["y"], t["param0"], t["param1"], t["sid"], "infonce")
    for name, got, ref in (("dwg", default[f"{key}/grad_param0"], o["dwg"]), ("dwh", default[f"{key}/grad_param1"], o["dwh"])):
        err = _rel(got, ref)
        print(f"{key}: {name} error / max|{name}| = {err:.2e}")
        assert err < GRAD_W_TOL, (key, name, err)
