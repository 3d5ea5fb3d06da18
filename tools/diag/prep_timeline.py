#!/usr/bin/env python3
"""Diagnostic: when the workgroups of the prep launch (conversions + T = X W) of the headline step start and end, by role,
on ONE clock -- the 100 MHz s_memrealtime stamps that the stamped build (make STAMPS=1 -> lib_stamps/) takes in every
workgroup (csrc/mi_common.h, WallScope).  The s_memtime stamps of stamps_prep_t.py compare within one CU only; this is the
launch's timeline: which role ends it.

    python tools/diag/prep_timeline.py [--lib PATH] [--tall 128-row form: the roles' block ranges differ] [--steps 30]

The roles are told apart by block index, as launch_prep_t lays them out: T tiles first, then (MI_PREP_T_TALL=1: last) the
equal-id flag blocks, then the conversion blocks.  Times in us from the first workgroup's entry; medians over --steps steps.
"""
import argparse
import ctypes
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "mutual-information-multimodal_amd", "lib_stamps", "libmi_critic_hip.so"))
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--dim", type=int, default=512)
    p.add_argument("--tile-rows", type=int, default=0, help="rows of a T tile in this run (default: 128 under MI_PREP_T_TALL, else 64)")
    p.add_argument("--x-job", type=int, default=-1, help="1: the launch has the X^T conversion job (default: under MI_PREP_T_TALL=1)")
    p.add_argument("--flags-last", type=int, default=-1, help="1: flag blocks behind the conversion blocks (default: under MI_PREP_T_TALL=1)")
    a = p.parse_args()
    tall = os.environ.get("MI_PREP_T_TALL", "0")
    tm = a.tile_rows or (128 if tall in ("1", "2") else 64)
    x_job = a.x_job if a.x_job >= 0 else int(tall == "1")
    flags_last = a.flags_last if a.flags_last >= 0 else int(tall == "1")
    b, d = a.batch, a.dim
    n_t = 8 * (d // 128) * ((b // tm + 7) // 8)
    n_c = (b // 64) * (d // 64) * (1 + x_job) + (d // 64) * (d // 64)
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    for name, (res, args) in _hip.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.mi_debug_set_wall.argtypes = [ctypes.c_void_p]
    dev = torch.device("cuda:0")
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
    rows = {}
    n = 0
    for _ in range(a.steps):
        wall.zero_()
        for _ in range(4):  # the launches in front keep the device busy: the stamped step is not a cold one
            step()
        torch.cuda.synchronize()
        g = wall.cpu().numpy().reshape(4, WALL_MAX_WG, 2, 2)[0]  # the prep launch: [workgroup][start / end][realtime, shader clock]
        n = int(((g[:, 0, 0] != 0) & (g[:, 1, 0] != 0)).sum())
        assert n >= n_t + n_c, f"{n} workgroups stamped, expected at least {n_t} tiles + {n_c} conversion blocks"
        st, en = g[:n, 0, 0].astype(np.int64), g[:n, 1, 0].astype(np.int64)
        t0 = st.min()
        st, en = (st - t0) * 0.01, (en - t0) * 0.01
        roles = {"T tiles": slice(0, n_t)}
        if flags_last:
            roles["conversion blocks"], roles["flag blocks"] = slice(n_t, n_t + n_c), slice(n_t + n_c, n)
        else:
            roles["flag blocks"], roles["conversion blocks"] = slice(n_t, n - n_c), slice(n - n_c, n)
        rows.setdefault("launch span", []).append(float(en.max()))
        for role, sl in roles.items():
            if sl.stop <= sl.start:
                continue
            for what, v in (("first start", st[sl].min()), ("median start", np.median(st[sl])), ("last start", st[sl].max()),
                            ("median duration", np.median(en[sl] - st[sl])), ("median end", np.median(en[sl])),
                            ("last end", en[sl].max())):
                rows.setdefault(f"{role}: {what}", []).append(float(v))
    assert lib.mi_debug_set_wall(None) == 0
    print(f"{a.lib}: {n} workgroups, {n_t} tile blocks of {tm} rows, {n_c} conversion blocks, MI_PREP_T_TALL={tall}")
    for k, v in rows.items():
        print(f"  {k:36s} median {statistics.median(v):7.2f} us   min {min(v):7.2f}  max {max(v):7.2f}")


if __name__ == "__main__":
    main()
