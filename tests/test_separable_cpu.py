"""CPU-side checks around the separable critic's DV / InfoNCE step: the fp64 restatement of tests/separable_reference.py
against the oracle, the case table of tests/test_separable_gpu.py against the library's own path query, and the precisions
the three base entry points refuse.  Nothing here needs a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import separable_reference as ref
from oracle import mi_oracle as orc

SMALL = [(12, 5, 7, 3), (33, 16, 24, 8), (1, 4, 4, 2)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


def _close(got, want, rtol=1e-10, atol=1e-12, what=""):
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=rtol, atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("shape", SMALL + [(130, 20, 12, 10)])
@pytest.mark.parametrize("kind", ["unique", "dup"])
def test_exact_mode_is_autograd_through_the_oracle(shape, kind):
    x, y, wg, wh = (t.double() for t in ref.inputs(shape))
    sid = ref.ids(shape[0], kind)
    r = ref.step(x, y, wg, wh, sid, "exact")
    for est in orc.ESTIMATORS:
        o = orc.matrix_step(orc.separable_scores, [x, y, wg, wh], sid, est)
        _close(r["scores"], o["scores"])
        if r["n_neg"] == 0:   # logsumexp of nothing: the same non-finite loss, no gradient to compare
            assert not np.isfinite(float(o["loss"].sum())) and not np.isfinite(float(r[f"loss_{est}"]))
            continue
        _close(r[f"loss_{est}"], o["loss"].reshape(()))
        for name, want in zip(ref.GRADS, o["grads"]):
            _close(r[name], want, what=name)
    # grad_out scales every gradient and nothing else
    r2 = ref.step(x, y, wg, wh, sid, "exact", grad_out=ref.GRAD_OUT)
    assert float(r2["loss_dv"]) == float(r["loss_dv"]) or r["n_neg"] == 0
    if r["n_neg"]:
        for name in ref.GRADS:
            _close(r2[name], ref.GRAD_OUT * r[name], what=name)


@pytest.mark.parametrize("shape", SMALL[:2] + [(96, 72, 200, 128)])
@pytest.mark.parametrize("est", orc.ESTIMATORS)
def test_fused16_mode_is_the_rounded_oracle(shape, est):
    x, y, wg, wh = ref.inputs(shape)
    sid = ref.ids(shape[0], "dup")
    r = ref.step(x, y, wg, wh, sid, "fused16")
    o = orc.separable_step_rounded(x, y, wg, wh, sid, est)
    _close(r["scores"], o["scores"], rtol=0, atol=0)
    _close(r[f"loss_{est}"], o["loss"].reshape(()), rtol=0, atol=0)
    for name in ref.GRADS:
        _close(r[name], o[name], rtol=0, atol=0, what=name)


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("shape,blocks", [((33, 16, 24, 8), [(0, 10), (10, 20), (30, 3)]),
                                          ((96, 72, 200, 128), [(0, 32), (32, 32), (64, 32)])])
def test_row_blocks_add_up_to_the_full_batch(mode, shape, blocks):
    """dX rows and dWg are sums over the block's own dA rows: exact in every mode.  dY and dWh go through the block's
    partial dC, which the 16-bit modes round per block (fused16 when it is stored, generic16 when the next GEMM loads it):
    each block's part and the full batch's dC carry one bf16 rounding per element, half an ulp at the most."""
    x, y, wg, wh = ref.inputs(shape)
    sid = ref.ids(shape[0], "dup")
    full = ref.step(x, y, wg, wh, sid, mode, grad_out=ref.GRAD_OUT)
    parts = [ref.step(x, y, wg, wh, sid, mode, row_block=rb, grad_out=ref.GRAD_OUT) for rb in blocks]
    for rb, p in zip(blocks, parts):
        _close(p["dx"], full["dx"][rb[0]:rb[0] + rb[1]], what="dx")
        for name in ("scores", "lse", "pos_mean", "loss_dv", "loss_infonce"):
            _close(p[name], full[name], rtol=0, atol=0, what=name)
    _close(sum(p["dwg"] for p in parts), full["dwg"], what="dwg")
    assert sum(p["block_n_neg"] for p in parts) == full["n_neg"] == int(orc.negative_mask(sid).sum())
    _close(sum(p["block_pos_sum"] for p in parts) / shape[0], full["pos_mean"])
    _close(torch.logsumexp(torch.stack([p["block_lse"] for p in parts]), 0), full["lse"])
    dc_err = sum(ref.half_ulp_bf16(p["dc"]) for p in parts) + ref.half_ulp_bf16(full["dc"])
    if mode == "exact":
        dc_err = torch.zeros_like(dc_err)
    wh_op, y_op = (t.double() if mode == "exact" else orc.round_bf16(t.double()) for t in (wh, y))
    for name, bound in (("dy", dc_err @ wh_op.abs().t()), ("dwh", y_op.abs().t() @ dc_err)):
        err = (sum(p[name] for p in parts) - full[name]).abs()
        assert bool((err <= bound + 1e-12 * float(full[name].abs().max())).all()), (name, float((err - bound).max()))


BAND_CASES = ([(c[0], c[3], kind, ()) for c in ref.CASES if c[1] == "bf16" for kind in ("unique", "dup")] +
              [(c[0], c[3], "dup", tuple(rb[0] for rb in c[4] if rb[0])) for c in ref.ROW_BLOCK_CASES if c[1] == "bf16"] +
              [(ref.UNALIGNED_BLOCK[0], ref.UNALIGNED_BLOCK[3], "dup", (ref.UNALIGNED_BLOCK[4][0],))])


@pytest.mark.parametrize("shape,mode,kind,offsets", BAND_CASES)
def test_rounded_references_stay_inside_the_bf16_band_of_exact(shape, mode, kind, offsets):
    """The GPU tests hold the bf16 kernels to the rounded reference at 1.5e-2 max|ref| and, as a check that the rounded
    reference did not drift along with the kernels, to the exact one at 6e-2 max|ref| (the band documented in
    test_bilinear_bf16_vs_rounded_oracle).  That only works where the rounded reference itself is well inside the band:
    at most 6e-2 - 1.5e-2 away from exact, on the very inputs the GPU tests use."""
    x, y, wg, wh = ref.inputs(shape)
    sid = ref.ids(shape[0], kind, offsets)
    e = ref.step(x, y, wg, wh, sid, "exact", grad_out=ref.GRAD_OUT)
    r = ref.step(x, y, wg, wh, sid, mode, grad_out=ref.GRAD_OUT)
    if e["n_neg"] == 0:
        return
    sc = max(float(e["scores"].abs().max()), 1.0)
    assert abs(float(r["loss_dv"]) - float(e["loss_dv"])) < 3e-2 * sc
    for name in ref.GRADS:
        err = float((r[name] - e[name]).abs().max()) / float(e[name].abs().max())
        assert err < 6e-2 - 1.5e-2, (name, err)


@pytest.mark.parametrize("shape", ref.FUSED_CASES + ref.TAIL_CASES[:1])
def test_structure_inputs_tell_single_rows_apart(shape):
    """The inputs of test_structure_exact (tests/test_separable_gpu.py): S == 0, integer A and C with pairwise distinct rows,
    the closed form equal to the fp64 restatement, and one wrong row in the P C (or P^T A) sum moves the reference by more
    than the tolerance that test allows -- such an error cannot hide under the rounding of dA / dC."""
    x, y, wg, wh, sid = ref.structure_inputs(shape)
    b = shape[0]
    for t in (x, y, wg, wh):
        assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert float(wg[:, shape[3] // 2:].abs().max()) == 0.0 and float(wh[:, :shape[3] // 2].abs().max()) == 0.0
    r = ref.step(x, y, wg, wh, sid, "exact", grad_out=ref.GRAD_OUT)
    s = ref.structure_reference(x, y, wg, wh, sid, ref.GRAD_OUT)
    assert float(r["scores"].abs().max()) == 0.0 and r["n_neg"] == s["n_neg"]
    assert len(torch.unique(s["a"], dim=0)) == b and len(torch.unique(s["c"], dim=0)) == b
    assert float(s["a"].abs().max()) <= 2 and float(s["c"].abs().max()) <= 2      # integers, exact in bf16
    assert float(r["dx"].abs().max()) == 0.0 and float(r["dy"].abs().max()) == 0.0
    for name in ("dwg", "dwh", "da", "dc"):
        _close(r[name], s[name][0] if name[1] == "w" else s[name], atol=1e-15, what=name)
    assert ref.structure_row_swap_shows(x, y, wg, wh, sid, ref.GRAD_OUT)


# ------------------------------------------------------------------------------------------------ the library, host only
def test_case_table_paths(lib):
    """Every case of the GPU tests lands on the path its row of the table names (host-only query): a change of the plan
    that moves a case to another set of kernels fails here instead of silently dropping that path's coverage."""
    from mutual_info_img_txt import _hip
    assert (ref.GENERIC, ref.FUSED, ref.FUSED_TAIL) == (_hip.MI_PATH_GENERIC, _hip.MI_PATH_FUSED, _hip.MI_PATH_FUSED_TAIL)
    assert not any(os.environ.get(k) for k in ("MI_NO_TAIL", "MI_NO_FLASH", "MI_SEP_NO_FUSED_PREP", "MI_FLASH_SLAB_F32"))
    for (b, dx, dy, k), prec, path, _ in ref.CASES:
        assert lib.mi_separable_path(b, b, dx, dy, k, _hip.PRECISIONS[prec]) == path, (b, dx, dy, k, prec)
    for (b, dx, dy, k), prec, path, _, blocks in ref.ROW_BLOCK_CASES:
        for _, br in blocks:
            assert lib.mi_separable_path(br, b, dx, dy, k, _hip.PRECISIONS[prec]) == path, (br, b, dx, dy, k, prec)
    (b, dx, dy, k), prec, path, _, (_, br) = ref.UNALIGNED_BLOCK
    assert lib.mi_separable_path(br, b, dx, dy, k, _hip.PRECISIONS[prec]) == path
    # the full-batch shapes of the row-block cases
    assert lib.mi_separable_path(256, 256, 64, 64, 256, _hip.MI_PREC_BF16) == ref.FUSED_TAIL


def test_base_entry_points_refuse_bf16x3_and_fp8(lib):
    """mi_separable_fwd / _bwd / _step implement MI_PREC_F32 and MI_PREC_BF16 only; the codes of the bilinear critic's
    other modes used to fall through to single-pass bf16.  Host dummies stand in for the buffers (the null check comes
    first); nothing reaches the device: a refused precision returns before it, and the two valid codes are stopped by the
    next host-side check, an empty workspace."""
    from mutual_info_img_txt import _hip
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    b, dx, dy, k = 4, 8, 8, 4

    def fwd(prec):
        return lib.mi_separable_fwd(p, p, p, p, p, p, b, b, 0, dx, dy, k, _hip.MI_DV, prec, 1, p, p, p, p, 0, None)

    def bwd(prec):
        return lib.mi_separable_bwd(p, p, p, p, p, p, b, b, 0, dx, dy, k, prec, p, p, p, p, p, p, p, 0, 1, None)

    def step(prec):
        return lib.mi_separable_step(p, p, p, p, p, b, dx, dy, k, _hip.MI_DV, prec, p, p, p, p, p, p, p, p, p, 0, None)

    for name, fn in (("mi_separable_fwd", fwd), ("mi_separable_bwd", bwd), ("mi_separable_step", step)):
        for prec in (_hip.MI_PREC_BF16X3, _hip.MI_PREC_FP8):
            assert fn(prec) == -1, (name, prec)
            msg = lib.mi_last_error().decode()
            assert name in msg and f"precision {prec}" in msg, msg
        for prec in (_hip.MI_PREC_F32, _hip.MI_PREC_BF16):
            assert fn(prec) == -3, (name, prec)            # MI_EWORKSPACE: past the precision check
            assert "workspace too small" in lib.mi_last_error().decode()
    # the host queries keep answering for those codes (tests/golden/plan_layout.json pins what)
    assert lib.mi_separable_path(64, 64, 64, 64, 128, _hip.MI_PREC_BF16X3) == _hip.MI_PATH_GENERIC
    assert lib.mi_separable_workspace_bytes(64, 64, 64, 64, 128, _hip.MI_PREC_FP8) > 0
