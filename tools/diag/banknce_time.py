#!/usr/bin/env python3
"""HIP-event times of the memory-bank InfoNCE step (mi_banknce_bilinear_step, symmetric, with gradients), bf16 and "f32"
(bf16x3), at (B, M, d) = (64, 4096, 512), (256, 16384, 512), (1024, 16384, 512), beside the torch route on the same
device, alternating with it inside one run:
  * torch: logsumexp over cat((x W) y^T, (x W) bank_y^T) and its mirror over cat(S[:B, :B], (bank_x W) y^T), then
    .backward() -- it materialises the [B, B + M] and [M, B] score and gradient matrices in fp32 (ids unique, so no mask).
The yardstick: the step is not slower than the torch route, at a fraction of its memory.  Median of
`reps` timed batches of `calls` calls each with min - max, the per-launch split of one call (_hip.kernel_profile), the
step's workspace beside the torch route's peak allocation.
usage: banknce_time.py [reps] [calls] [B M d]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip  # noqa: E402

PRECS = {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3}
SHAPES = [(64, 4096, 512), (256, 16384, 512), (1024, 16384, 512)]


def _batch_ms(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) / calls


def _torch_route(x, y, w, bx, by):
    b = x.shape[0]
    for t in (x, y, w):
        t.grad = None
    t_ = x @ w
    top = torch.cat((t_ @ y.t(), t_ @ by.t()), dim=1)
    left = (bx @ w) @ y.t()
    d = torch.diagonal(top[:, :b])
    r = torch.logsumexp(top, dim=1)
    c = torch.logsumexp(torch.cat((top[:, :b], left), dim=0), dim=0)
    loss = 0.5 * (r - d).mean() + 0.5 * (c - d).mean()
    loss.backward()
    return loss


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    shapes = [tuple(int(v) for v in sys.argv[3:6])] if len(sys.argv) > 5 else SHAPES
    lib, dev = _hip.load(), torch.device("cuda:0")
    st = _hip.stream_ptr(dev)
    mode = _hip.MI_NCE_SYMMETRIC
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    for b, m, d in shapes:
        gen = torch.Generator().manual_seed(b + m + d)
        x, y, bx, by = (torch.randn(n, d, generator=gen).to(dev) for n in (b, b, m, m))
        w = (torch.randn(d, d, generator=gen) * (0.3 / d ** 0.5)).to(dev)
        sid, bsid = torch.arange(b, dtype=torch.int64, device=dev), torch.arange(b, b + m, dtype=torch.int64, device=dev)
        xt, yt, wt = (t.clone().requires_grad_(True) for t in (x, y, w))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        tl = _torch_route(xt, yt, wt, bx, by)
        torch.cuda.synchronize()
        torch_peak = torch.cuda.max_memory_allocated(dev) - base
        for pname, prec in PRECS.items():
            ws = _hip.workspace(lib.mi_banknce_bilinear_workspace_bytes(b, m, d, d, mode, prec, 1), dev)
            loss, r, c, gx, gy, gw = f32(1), f32(b), f32(b), f32(b, d), f32(b, d), f32(d, d)
            args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), bx.data_ptr(), by.data_ptr(), bsid.data_ptr(),
                    b, m, d, d, mode, prec, None, loss.data_ptr(), r.data_ptr(), c.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                    gw.data_ptr(), ws.data_ptr(), ws.numel(), st)
            legs = {"banknce": lambda: lib.mi_banknce_bilinear_step(*args),
                    "torch": lambda: _torch_route(xt, yt, wt, bx, by)}
            _hip.check(legs["banknce"](), "banknce")
            for fn in legs.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ts = {name: [] for name in legs}
            for _ in range(reps):  # alternating: every leg sees the same clocks and the same neighbours
                for name, fn in legs.items():
                    ts[name].append(_batch_ms(fn, calls))
            med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
            with _hip.kernel_profile() as prof:
                legs["banknce"]()
                torch.cuda.synchronize()
            split = {name: round(v["ms_total"], 4) for name, v in prof.by_name().items()}
            row = {"b": b, "m": m, "d": d, "precision": pname, "mode": "symmetric",
                   **{f"{name}_ms": round(med[name], 4) for name in legs},
                   **{f"{name}_ms_min_max": [round(min(ts[name]), 4), round(max(ts[name]), 4)] for name in legs},
                   "banknce_over_torch": round(med["banknce"] / med["torch"], 3), "launches": len(prof.records),
                   "loss": [round(float(loss), 5), round(float(tl), 5)],
                   "workspace_mib": round(ws.numel() / 2 ** 20, 1), "torch_peak_mib": round(torch_peak / 2 ** 20, 1),
                   "banknce_kernels_ms": split}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
