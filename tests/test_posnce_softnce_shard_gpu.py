"""The row-block entry points of the study-positive and the soft-target InfoNCE at world size 1, in process and without a
process group: the ops calls composed directly (forward -> part, merge of one part, backward) give the loss, the LSEs,
n_pos / z and every gradient of the one-call steps (mi_posnce_*_step / mi_softnce_*_step) bit for bit, on the 16-bit chain
and on the generic kernels.  The sharded step over several ranks: tests/test_posnce_softnce_distributed_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (critic, precision, b, d); "bilinear_xy": S = X Y^T (no weight)
CASES = [("bilinear", "bf16", 256, 128), ("bilinear", "bf16x3", 256, 128), ("bilinear", "bf16", 192, 64),
         ("bilinear", "f32_exact", 128, 64), ("bilinear", "bf16", 200, 60), ("bilinear_xy", "bf16", 256, 128),
         ("separable", "bf16", 256, 128), ("separable", "f32", 96, 40)]
CASE_IDS = [f"{c}-{p}-{b}x{d}" for c, p, b, d in CASES]


def _problem(case):
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.critic_ops import HipBilinearOps, HipSeparableOps
    kind, precision, b, d = case
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(b * 3 + d)
    x = torch.randn(b, d, generator=gen).to(dev)
    y = torch.randn(b, d, generator=gen).to(dev)
    if kind == "separable":
        ops, k = HipSeparableOps(), 48
        params = [(torch.randn(d, k, generator=gen) * (0.7 / math.sqrt(d))).to(dev),
                  (torch.randn(d, k, generator=gen) * (0.7 / math.sqrt(d))).to(dev)]
    else:
        ops = HipBilinearOps()
        params = [] if kind == "bilinear_xy" else [(torch.randn(d, d, generator=gen) * (0.3 / math.sqrt(d))).to(dev)]
        if kind == "bilinear_xy":
            x, y = x * 0.25, y * 0.25
    return ops, x, y, params, _hip.PRECISIONS[precision], gen, dev


def _same(got, want, names):
    for name, g, w in zip(names, got, want):
        assert torch.equal(g, w), (name, float((g.float() - w.float()).abs().max()))


@pytest.mark.parametrize("mode", [0, 1], ids=["rowwise", "symmetric"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_posnce_world_one_equals_one_call_step(case, mode):
    ops, x, y, params, prec, gen, dev = _problem(case)
    b = x.shape[0]
    sid = torch.arange(b, dtype=torch.int64)
    sid[3] = sid[2]                # a pair inside one tile
    sid[b - 1] = sid[0]            # a pair in the two far corner tiles
    sid[70:75] = sid[70]           # a group of five
    sid = sid.to(dev)
    loss, r, c, n_pos, grads = ops.posnce_step(x, y, params, sid, mode, prec, True)
    part, r1, n1, saved = ops.posnce_forward(x, y, params, sid, sid, 0, mode, prec)
    assert part.numel() == 3 * b + 2 * b
    loss1, c1 = ops.posnce_merge(part.reshape(1, -1), b, mode)
    gx, gy, gp = ops.posnce_backward(saved, c1, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and int(n_pos.max()) == 5
    _same([loss1, r1, c1, n1, gx, gy, *gp], [loss, r, c, n_pos, *grads],
          ["loss", "lse_rows", "lse_cols", "n_pos", "dx", "dy", "dp0", "dp1"])


@pytest.mark.parametrize("mode", [0, 1], ids=["rowwise", "symmetric"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_softnce_world_one_equals_one_call_step(case, mode):
    ops, x, y, params, prec, gen, dev = _problem(case)
    b = x.shape[0]
    lab = torch.randint(0, 1 << 14, (b,), generator=gen, dtype=torch.int64)   # 14 findings: most pairs overlap
    lab[70:75] = lab[70]
    lab[5] = 0
    lab[6] -= 1 << 63              # bit 63 is ignored
    lab = lab.to(dev)
    tau, mix = 0.5, 0.5
    loss, r, c, z, grads = ops.softnce_step(x, y, params, lab, mode, prec, tau, mix, True)
    part, r1, z1, saved = ops.softnce_forward(x, y, params, lab, lab, 0, mode, prec, tau, mix)
    assert part.numel() == 3 * b + b
    loss1, c1 = ops.softnce_merge(part.reshape(1, -1), b, mode)
    gx, gy, gp = ops.softnce_backward(saved, c1, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and float(z.min()) >= 1.0
    _same([loss1, r1, c1, z1, gx, gy, *gp], [loss, r, c, z, *grads],
          ["loss", "lse_rows", "lse_cols", "target_norm", "dx", "dy", "dp0", "dp1"])
