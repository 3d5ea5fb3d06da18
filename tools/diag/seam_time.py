#!/usr/bin/env python3
"""Diagnostic: what the four launches of the headline step (mi_bilinear_step, B = 4096, d = 512, bf16) pay at their
kernel boundaries.  Needs the stamped library (`make STAMPS=1` -> lib_stamps/; add SEAM=... flags by hand for a variant):

    python tools/diag/seam_time.py [--lib PATH] [--steps 30]

Per launch it prints
  (a) the event-bracketed time from the profiling hook (mi_profile_begin / mi_profile_end): what every per-kernel table of
      this project shows, write-back of the dirty L2 lines included;
  (b) the in-kernel wall span: first workgroup in to last workgroup out with its stores acknowledged, from s_memrealtime
      (100 MHz) stamps (csrc/mi_common.h, WallScope);
  (a) - (b): launch overhead + write-back behind the last wave = what the boundary costs;
  the shader clock the kernel really ran at: delta s_memtime / delta s_memrealtime, median over the workgroups that ran
  for more than 2 us;
and the gaps between the launches on the device's wall clock (last workgroup out -> first workgroup of the next in).
Medians over --steps steps.  The stamps cost a few hundred cycles per workgroup: compare (a) here with the unstamped build.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from mutual_info_img_txt import _hip  # noqa: E402

WALL_MAX_WG = 8192  # csrc/mi_common.h, kWallMaxWg
KERNELS = ["prep + T", "fused kernel", "tail", "dW"]
TICK_US = 0.01  # s_memrealtime: 100 MHz


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "mutual-information-multimodal_amd", "lib_stamps", "libmi_critic_hip.so"))
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--dim", type=int, default=512)
    a = p.parse_args()
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    for name, (res, args) in _hip.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.mi_debug_set_wall.argtypes = [ctypes.c_void_p]
    dev = torch.device("cuda:0")
    b, d = a.batch, a.dim
    x, y, sid = bench.make_inputs(b, d, d, 3, 0, 1, dev)
    x, y = x.bfloat16().float().contiguous(), y.bfloat16().float().contiguous()
    w = bench.make_critic("bilinear", d, d, 3, dev).weight.detach().float().contiguous()
    gx, gy, gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
    loss, go, stats = torch.empty(1, device=dev), torch.ones(1, device=dev), _hip.new_stats(dev)
    rec = torch.empty(_hip.RECORD_FLOATS, device=dev)
    ws = _hip.workspace(lib.mi_bilinear_workspace_bytes(b, b, d, d, _hip.MI_PREC_BF16), dev)
    wall = torch.zeros(4 * WALL_MAX_WG * 4, dtype=torch.int64, device=dev)

    def step():
        rc = lib.mi_bilinear_step(x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, _hip.MI_INFONCE,
                                  _hip.MI_PREC_BF16, go.data_ptr(), loss.data_ptr(), stats.data_ptr(), rec.data_ptr(),
                                  gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mi_last_error()

    for _ in range(200):
        step()
    torch.cuda.synchronize()
    assert lib.mi_debug_set_wall(wall.data_ptr()) == 0
    ev, span, clock, gaps = [[] for _ in KERNELS], [[] for _ in KERNELS], [[] for _ in KERNELS], [[] for _ in range(3)]
    cap = 64
    for _ in range(a.steps):
        wall.zero_()
        for _ in range(3):  # the launches in front keep the device busy: the profiled step is not a cold one
            step()
        assert lib.mi_profile_begin() == 0
        step()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(cap * 48)
        ms = (ctypes.c_float * cap)()
        n = ctypes.c_int(0)
        assert lib.mi_profile_end(names, len(names), ms, cap, ctypes.byref(n)) == 0
        assert n.value == 4, f"expected the four launches of the fused path, got {n.value}"
        s = wall.cpu().numpy().reshape(4, WALL_MAX_WG, 2, 2)  # [kernel][workgroup][start / end][realtime, shader clock]
        first, last = [], []
        for k in range(4):
            g = s[k][(s[k, :, 0, 0] != 0) & (s[k, :, 1, 0] != 0)]
            first.append(int(g[:, 0, 0].min()))
            last.append(int(g[:, 1, 0].max()))
            ev[k].append(float(ms[k]) * 1e3)
            span[k].append((last[k] - first[k]) * TICK_US)
            dr = (g[:, 1, 0] - g[:, 0, 0]).astype(np.float64)
            dc = (g[:, 1, 1] - g[:, 0, 1]).astype(np.float64)
            long_ = dr > 200
            if long_.any():
                clock[k].append(float(np.median(dc[long_] / dr[long_])) * 100.0)  # shader ticks per 10 ns -> MHz
        for k in range(3):
            gaps[k].append((first[k + 1] - last[k]) * TICK_US)
    assert lib.mi_debug_set_wall(None) == 0
    med = statistics.median
    out = {"shape": [b, d], "steps": a.steps, "launches": {}}
    print(f"{'launch':14s} {'(a) events us':>14s} {'(b) wall span us':>17s} {'(a)-(b) us':>11s} {'clock MHz':>10s}")
    tot = 0.0
    for k, name in enumerate(KERNELS):
        ca = med(ev[k]); cb = med(span[k]); ck = med(clock[k]) if clock[k] else float("nan")
        tot += ca - cb
        out["launches"][name] = {"events_us": round(ca, 2), "wall_span_us": round(cb, 2), "boundary_us": round(ca - cb, 2),
                                 "clock_mhz": round(ck, 1)}
        print(f"{name:14s} {ca:14.2f} {cb:17.2f} {ca - cb:11.2f} {ck:10.1f}")
    out["boundary_sum_us"] = round(tot, 2)
    out["gaps_us"] = [round(med(g), 2) for g in gaps]
    print(f"sum of (a) - (b): {tot:.2f} us;  device-clock gaps last-out -> first-in: {out['gaps_us']} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
