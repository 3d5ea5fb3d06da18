#!/usr/bin/env python3
"""Per-kernel times of the make_mlp critic trained through its differentiable score matrix (fused_critic_scores + the
symmetric InfoNCE matrix loss) next to the DV step of the same critic, one process, interleaved rounds.
usage: fused_scores_time.py [B] [d] [modes, comma separated] [rounds]
One mode per run gives the cleanest step times: with several modes the workspaces of different sizes take turns in torch's
caching allocator and a step may pay for a device allocation (the count is printed)."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip, fused_scores, mi_critics  # noqa: E402
from mutual_info_img_txt.model import make_mlp  # noqa: E402

b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
d = int(sys.argv[2]) if len(sys.argv) > 2 else 768
modes = (sys.argv[3] if len(sys.argv) > 3 else "f16,f32").split(",")
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
dev = torch.device("cuda:0")
torch.manual_seed(0)
mlp = make_mlp(2 * d, [1024, 512]).to(dev)
gen = torch.Generator().manual_seed(3)
x = torch.randn(b, d, generator=gen).to(dev).requires_grad_(True)
y = torch.randn(b, d, generator=gen).to(dev).requires_grad_(True)
# ids as a device tensor: a host list or CPU tensor is copied to the device inside matrix_bound_loss, and that copy makes
# the host wait for the forward kernels before it can queue the loss and the backward (MI_SID_ON_HOST=1 shows the gap)
sid = torch.arange(b) if os.environ.get("MI_SID_ON_HOST") else torch.arange(b, device=dev)


def dv_step(m):
    loss = mi_critics.fused_mi_bound(x, y, sid, mlp, "dv", precision=m)
    loss.sum().backward()
    return loss


def scores_step(m):
    loss = fused_scores.concat_infonce(x, y, sid, mlp, "infonce_symmetric", precision=m)
    loss.backward()
    return loss


STEPS = {"dv": dv_step, "scores+infonce_symmetric": scores_step}
for m in modes:
    for fn in STEPS.values():
        fn(m)
torch.cuda.synchronize()
agg, wall = {}, {}
allocs0 = torch.cuda.memory_stats()["num_device_alloc"]
for r in range(2 * rounds):  # whole steps between two events, no per-kernel events inside
    for m in modes:
        for tag, fn in STEPS.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(m)
            t1.record()
            torch.cuda.synchronize()
            wall.setdefault((m, tag), []).append(t0.elapsed_time(t1))
for r in range(rounds):
    for m in modes:
        for tag, fn in STEPS.items():
            with _hip.kernel_profile() as prof:
                loss = fn(m)
            for name, v in prof.by_name().items():
                agg.setdefault((m, tag), {}).setdefault(name, []).append(v["ms_total"])
for (m, tag), kernels in agg.items():
    tot = 0.0
    w = sorted(wall[(m, tag)])
    print(f"== {m} {tag}: step between events, min {w[0]:.3f} ms  median {w[len(w) // 2]:.3f}")
    for name, v in sorted(kernels.items(), key=lambda kv: -min(kv[1])):
        tot += min(v)
        if min(v) > 0.02:
            print(f"   {name:44s} min {min(v):8.3f} ms  median {sorted(v)[len(v) // 2]:8.3f}")
    print(f"   sum of library kernel minima: {tot:.3f} ms")
print("device allocations during the timed rounds:", torch.cuda.memory_stats()["num_device_alloc"] - allocs0)
