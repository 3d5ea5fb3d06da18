#!/usr/bin/env python3
"""HIP-event times of the hard-negative InfoNCE step (mi_hardnce_bilinear_step, symmetric, with gradients) at B = 4096,
d = 512, k = 10, bf16 and "f32" (bf16x3), beside the two calls it replaces, alternating with it inside one run:
  * mi_topk_bilinear -- both directions, with the ids (the mining call);
  * mi_nce_bilinear_step -- the symmetric per-sample InfoNCE with gradients (the training call).
The yardstick: the step must not exceed the sum of the two -- it issues one prep + T instead of
two and no statistics sweep.  Median of `reps` timed batches of `calls` calls each with min - max, then the per-kernel
split of one call of each (_hip.kernel_profile) and the workspace sizes.
usage: hardnce_time.py [reps] [calls] [B] [d] [k]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip  # noqa: E402

PRECS = {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3}


def _tensors(b, d, dev):
    gen = torch.Generator().manual_seed(b + d)
    x = torch.randn(b, d, generator=gen).to(dev)
    y = torch.randn(b, d, generator=gen).to(dev)
    w = (torch.randn(d, d, generator=gen) * (0.3 / d ** 0.5)).to(dev)
    sid = torch.arange(b, dtype=torch.int64)
    for n in range(b // 8):
        sid[n] = n - n % 2
    return x, y, w, sid.to(dev)


def _batch_ms(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) / calls


def _split(fn):
    with _hip.kernel_profile() as prof:
        fn()
        torch.cuda.synchronize()
    return {name: round(v["ms_total"], 4) for name, v in prof.by_name().items()}, len(prof.records)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    b = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    d = int(sys.argv[4]) if len(sys.argv) > 4 else 512
    k = int(sys.argv[5]) if len(sys.argv) > 5 else 10
    lib, dev = _hip.load(), torch.device("cuda:0")
    x, y, w, sid = _tensors(b, d, dev)
    st = _hip.stream_ptr(dev)
    mode = _hip.MI_NCE_SYMMETRIC
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    for pname, prec in PRECS.items():
        ws_h = _hip.workspace(lib.mi_hardnce_bilinear_workspace_bytes(b, d, d, prec, k, 1), dev)
        ws_k = _hip.workspace(lib.mi_topk_bilinear_workspace_bytes(b, b, d, d, prec, k), dev)
        ws_n = _hip.workspace(lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec), dev)
        ii, it = (torch.empty(b, k, dtype=torch.int32, device=dev) for _ in range(2))
        vi, vt = f32(b, k), f32(b, k)
        loss, r, c, gx, gy, gw = f32(1), f32(b), f32(b), f32(b, d), f32(b, d), f32(d, d)
        xp, yp, wp, sp = x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr()
        hard_args = (xp, yp, wp, sp, b, d, d, mode, prec, k, None, loss.data_ptr(), r.data_ptr(), c.data_ptr(),
                     ii.data_ptr(), it.data_ptr(), gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws_h.data_ptr(),
                     ws_h.numel(), st)
        topk_args = (xp, yp, wp, sp, sp, b, b, d, d, prec, k, ii.data_ptr(), vi.data_ptr(), it.data_ptr(), vt.data_ptr(),
                     ws_k.data_ptr(), ws_k.numel(), st)
        nce_args = (xp, yp, wp, sp, b, d, d, mode, prec, None, loss.data_ptr(), r.data_ptr(), c.data_ptr(), gx.data_ptr(),
                    gy.data_ptr(), gw.data_ptr(), ws_n.data_ptr(), ws_n.numel(), st)
        legs = {"hardnce": lambda: lib.mi_hardnce_bilinear_step(*hard_args),
                "topk": lambda: lib.mi_topk_bilinear(*topk_args), "nce": lambda: lib.mi_nce_bilinear_step(*nce_args)}
        for name, fn in legs.items():
            _hip.check(fn(), name)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in legs}
        for _ in range(reps):  # alternating: every leg sees the same clocks and the same neighbours
            for name, fn in legs.items():
                ts[name].append(_batch_ms(fn, calls))
        med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
        splits = {name: _split(fn) for name, fn in legs.items()}
        row = {"b": b, "d": d, "k": k, "precision": pname, "mode": "symmetric",
               **{f"{name}_ms": round(med[name], 4) for name in legs},
               **{f"{name}_ms_min_max": [round(min(ts[name]), 4), round(max(ts[name]), 4)] for name in legs},
               "topk_plus_nce_ms": round(med["topk"] + med["nce"], 4),
               "hardnce_over_sum": round(med["hardnce"] / (med["topk"] + med["nce"]), 3),
               "launches": {name: s[1] for name, s in splits.items()},
               "workspace_mib": {"hardnce": round(ws_h.numel() / 2 ** 20, 1), "topk": round(ws_k.numel() / 2 ** 20, 1),
                                 "nce": round(ws_n.numel() / 2 ** 20, 1)},
               **{f"{name}_kernels_ms": s[0] for name, s in splits.items()}}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
