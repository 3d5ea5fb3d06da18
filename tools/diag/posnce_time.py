#!/usr/bin/env python3
"""HIP-event times of the study-positive InfoNCE step (mi_posnce_bilinear_step, symmetric, with gradients), bf16 and
"f32" (bf16x3), at (B, d) = (4096, 512) and (256, 512), with unique ids and with every id shared by two samples, beside
the per-sample InfoNCE step (mi_nce_bilinear_step) on the same inputs, alternating with it inside one run.
The yardstick is that step: both run the same GEMMs, so the difference is the two epilogues and
the merge.  Median of `reps` timed batches of `calls` calls each with min - max, and the per-launch split of one call of
either step (_hip.kernel_profile).
usage: posnce_time.py [reps] [calls] [B d]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip  # noqa: E402

PRECS = {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3}
SHAPES = [(4096, 512), (256, 512)]


def _batch_ms(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) / calls


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    shapes = [tuple(int(v) for v in sys.argv[3:5])] if len(sys.argv) > 4 else SHAPES
    lib, dev = _hip.load(), torch.device("cuda:0")
    st = _hip.stream_ptr(dev)
    mode = _hip.MI_NCE_SYMMETRIC
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    for b, d in shapes:
        gen = torch.Generator().manual_seed(b + d)
        x, y = (torch.randn(b, d, generator=gen).to(dev) for _ in range(2))
        w = (torch.randn(d, d, generator=gen) * (0.3 / d ** 0.5)).to(dev)
        ids = {"unique": torch.arange(b, dtype=torch.int64, device=dev),
               "pairs": torch.arange(b, dtype=torch.int64, device=dev) // 2}
        for pname, prec in PRECS.items():
            for iname, sid in ids.items():
                ws_p = _hip.workspace(lib.mi_posnce_bilinear_workspace_bytes(b, d, d, prec, 1), dev)
                ws_n = _hip.workspace(lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec), dev)
                out = {n: (f32(1), f32(b), f32(b), f32(b, d), f32(b, d), f32(d, d)) for n in ("posnce", "nce")}
                n_pos = torch.empty(b, dtype=torch.int32, device=dev)
                head = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, mode, prec, None)
                lo, r, c, gx, gy, gw = (t.data_ptr() for t in out["posnce"])
                args_p = head + (lo, r, c, n_pos.data_ptr(), gx, gy, gw, ws_p.data_ptr(), ws_p.numel(), st)
                lo, r, c, gx, gy, gw = (t.data_ptr() for t in out["nce"])
                args_n = head + (lo, r, c, gx, gy, gw, ws_n.data_ptr(), ws_n.numel(), st)
                legs = {"posnce": lambda: lib.mi_posnce_bilinear_step(*args_p),
                        "nce": lambda: lib.mi_nce_bilinear_step(*args_n)}
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
                split = {}
                for name, fn in legs.items():
                    with _hip.kernel_profile() as prof:
                        fn()
                        torch.cuda.synchronize()
                    split[name] = {k: round(v["ms_total"], 4) for k, v in prof.by_name().items()}
                row = {"b": b, "d": d, "precision": pname, "ids": iname, "mode": "symmetric",
                       **{f"{name}_ms": round(med[name], 4) for name in legs},
                       **{f"{name}_ms_min_max": [round(min(ts[name]), 4), round(max(ts[name]), 4)] for name in legs},
                       "posnce_over_nce": round(med["posnce"] / med["nce"], 3),
                       "loss": [round(float(out["posnce"][0]), 5), round(float(out["nce"][0]), 5)],
                       "workspace_mib": [round(ws_p.numel() / 2 ** 20, 1), round(ws_n.numel() / 2 ** 20, 1)],
                       "posnce_kernels_ms": split["posnce"], "nce_kernels_ms": split["nce"]}
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
