#!/usr/bin/env python3
"""HIP-event times of the soft-target InfoNCE step (mi_softnce_bilinear_step, symmetric, with gradients), bf16, at
(B, d) = (4096, 512), beside the study-positive InfoNCE step (mi_posnce_bilinear_step) of the same build on the same
inputs, alternating with it inside one process.
The yardstick is that step, an existing chain and not the code under test: both run the same
GEMMs, so the difference is the label-norm launch, the two epilogues and the merge.  Every leg is warmed up at its own
shape first; then `reps` timed batches of `calls` whole steps each between two HIP events, the legs taking turns so that
each sees the same clocks and the same neighbours; median with min - max.  The per-launch split of either step comes from
a separate pass under _hip.kernel_profile (event pairs around every launch slow the host, so it is kept out of the timed
batches).  Labels: 14 random findings per sample (the CheXpert table), tau 0.5, mix 0.3.
usage: softnce_time.py [reps] [calls] [B d] [precision: bf16 | f32]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip  # noqa: E402

PRECS = {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3}
TAU, MIX = 0.5, 0.3


def _batch_ms(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) / calls


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    b, d = (int(v) for v in sys.argv[3:5]) if len(sys.argv) > 4 else (4096, 512)
    pname = sys.argv[5] if len(sys.argv) > 5 else "bf16"
    prec = PRECS[pname]
    lib, dev = _hip.load(), torch.device("cuda:0")
    st = _hip.stream_ptr(dev)
    mode = _hip.MI_NCE_SYMMETRIC
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(b + d)
    x, y = (torch.randn(b, d, generator=gen).to(dev) for _ in range(2))
    w = (torch.randn(d, d, generator=gen) * (0.3 / d ** 0.5)).to(dev)
    lab = torch.randint(0, 1 << 14, (b,), generator=gen, dtype=torch.int64).to(dev)
    sid = torch.arange(b, dtype=torch.int64, device=dev)
    ws_s = _hip.workspace(lib.mi_softnce_bilinear_workspace_bytes(b, d, d, prec, 1), dev)
    ws_p = _hip.workspace(lib.mi_posnce_bilinear_workspace_bytes(b, d, d, prec, 1), dev)
    out = {n: (f32(1), f32(b), f32(b), f32(b, d), f32(b, d), f32(d, d)) for n in ("softnce", "posnce")}
    z, n_pos = f32(b), torch.empty(b, dtype=torch.int32, device=dev)
    lo, r, c, gx, gy, gw = (t.data_ptr() for t in out["softnce"])
    args_s = (x.data_ptr(), y.data_ptr(), w.data_ptr(), lab.data_ptr(), b, d, d, mode, prec, TAU, MIX, None, lo, r, c,
              z.data_ptr(), gx, gy, gw, ws_s.data_ptr(), ws_s.numel(), st)
    lo, r, c, gx, gy, gw = (t.data_ptr() for t in out["posnce"])
    args_p = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, mode, prec, None, lo, r, c,
              n_pos.data_ptr(), gx, gy, gw, ws_p.data_ptr(), ws_p.numel(), st)
    legs = {"softnce": lambda: lib.mi_softnce_bilinear_step(*args_s),
            "posnce": lambda: lib.mi_posnce_bilinear_step(*args_p)}
    for name, fn in legs.items():   # warm-up: first launches load code objects
        _hip.check(fn(), name)
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            ts[name].append(_batch_ms(fn, calls))
    med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
    split = {}
    for name, fn in legs.items():
        per = {}
        for _ in range(5):
            with _hip.kernel_profile() as prof:
                fn()
                torch.cuda.synchronize()
            for k, v in prof.by_name().items():
                per.setdefault(k, []).append(v["ms_total"])
        split[name] = {k: round(sorted(v)[len(v) // 2], 4) for k, v in per.items()}
    row = {"b": b, "d": d, "precision": pname, "mode": "symmetric", "tau": TAU, "mix": MIX, "reps": reps, "calls": calls,
           **{f"{name}_ms": round(med[name], 4) for name in legs},
           **{f"{name}_ms_min_max": [round(min(ts[name]), 4), round(max(ts[name]), 4)] for name in legs},
           "softnce_over_posnce": round(med["softnce"] / med["posnce"], 3),
           "loss": [round(float(out["softnce"][0]), 5), round(float(out["posnce"][0]), 5)],
           "workspace_mib": [round(ws_s.numel() / 2 ** 20, 1), round(ws_p.numel() / 2 ** 20, 1)],
           "softnce_kernels_ms": split["softnce"], "posnce_kernels_ms": split["posnce"]}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
