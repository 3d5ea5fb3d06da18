"""The row-block entry points of the per-sample InfoNCE at world size 1, in process and without a process group: the ops
calls composed directly (forward -> part, merge of one part, backward) give the loss, the LSEs and every gradient of the
one-call step (mi_nce_bilinear_step / mi_nce_separable_step) bit for bit, on the 16-bit chain and on the generic kernels.
The sharded step over several ranks: tests/test_nce_distributed_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (critic, precision, b, d); "bilinear_xy": S = X Y^T (no weight)
CASES = [("bilinear", "bf16", 256, 128), ("bilinear", "bf16x3", 256, 128), ("bilinear", "bf16", 192, 64),
         ("bilinear", "f32_exact", 128, 64), ("bilinear", "bf16", 200, 60), ("bilinear_xy", "bf16", 256, 128),
         ("separable", "bf16", 256, 128), ("separable", "f32", 96, 40)]


@pytest.mark.parametrize("mode", [0, 1], ids=["rowwise", "symmetric"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c}-{p}-{b}x{d}" for c, p, b, d in CASES])
def test_world_one_equals_one_call_step(case, mode):
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
    sid = torch.arange(b, dtype=torch.int64)
    sid[3] = sid[2]
    sid[b - 1] = sid[0]
    sid = sid.to(dev)
    prec = _hip.PRECISIONS[precision]
    loss, r, c, grads = ops.nce_step(x, y, params, sid, mode, prec, True)
    part, r1, saved = ops.nce_forward(x, y, params, sid, sid, 0, mode, prec)
    assert part.numel() == 2 * b + 2 * b
    loss1, c1 = ops.nce_merge(part.reshape(1, -1), b, mode)
    gx, gy, gp = ops.nce_backward(saved, c1, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert torch.equal(loss1, loss)
    assert torch.equal(r1, r)
    assert torch.equal(c1, c)
    for name, got, want in [("dx", gx, grads[0]), ("dy", gy, grads[1])] + \
                           [(f"dp{n}", g, w) for n, (g, w) in enumerate(zip(gp, grads[2:]))]:
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
