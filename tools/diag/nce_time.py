#!/usr/bin/env python3
"""HIP-event times of the per-sample InfoNCE step (mi_nce_bilinear_step: forward, loss and every gradient) beside the DV
step on the same G-materialising GEMM chain (mi_bilinear_step), at B = 4096, d = 512 and 768, precisions bf16 and "f32"
(bf16x3).  At d = 512 the DV step would take the fused B x B kernel, so its figures come from a child process with
MI_NO_FLASH=1 (the GEMM chain); d = 768 is on that chain already.  Median of `reps` timed batches of `calls` calls.
usage: nce_time.py [reps] [calls]          (nce_time.py --dv B D PREC reps calls: the child's leg)"""
import json
import os
import subprocess
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


def _time(fn, reps, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        e.record()
        e.synchronize()
        ts.append(a.elapsed_time(e) / calls)
    return sorted(ts)[len(ts) // 2]


def nce_ms(b, d, prec, mode, reps, calls):
    lib, dev = _hip.load(), torch.device("cuda:0")
    x, y, w, sid = _tensors(b, d, dev)
    ws = _hip.workspace(lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec), dev)
    loss = torch.empty(1, device=dev)
    r, c = torch.empty(b, device=dev), torch.empty(b, device=dev)
    gx, gy, gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
    st = _hip.stream_ptr(dev)
    args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, mode, prec, None, loss.data_ptr(),
            r.data_ptr(), c.data_ptr(), gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _hip.check(lib.mi_nce_bilinear_step(*args), "mi_nce_bilinear_step")
    return _time(lambda: lib.mi_nce_bilinear_step(*args), reps, calls)


def dv_ms(b, d, prec, reps, calls):
    lib, dev = _hip.load(), torch.device("cuda:0")
    x, y, w, sid = _tensors(b, d, dev)
    path = lib.mi_bilinear_path(b, b, d, d, prec)
    ws = _hip.workspace(lib.mi_bilinear_workspace_bytes(b, b, d, d, prec), dev)
    loss, stats = torch.empty(1, device=dev), _hip.new_stats(dev)
    rec = torch.empty(_hip.RECORD_FLOATS, device=dev)
    gx, gy, gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
    st = _hip.stream_ptr(dev)
    args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, _hip.MI_DV, prec, None, loss.data_ptr(),
            stats.data_ptr(), rec.data_ptr(), gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _hip.check(lib.mi_bilinear_step(*args), "mi_bilinear_step")
    return _time(lambda: lib.mi_bilinear_step(*args), reps, calls), path


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--dv":
        b, d, prec, reps, calls = (int(v) for v in sys.argv[2:7])
        ms, path = dv_ms(b, d, prec, reps, calls)
        print(json.dumps({"ms": ms, "path": path}))
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    b = 4096
    rows = []
    for d in (512, 768):
        for pname, prec in PRECS.items():
            env = dict(os.environ, MI_NO_FLASH="1")  # the G-materialising chain for the DV step
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dv", str(b), str(d), str(prec), str(reps),
                                str(calls)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:])
                sys.exit(r.returncode)
            dv = json.loads(r.stdout.strip().splitlines()[-1])
            row = {"b": b, "d": d, "precision": pname, "dv_ms": round(dv["ms"], 4), "dv_path": _hip.PATH_NAMES[dv["path"]]}
            for mname, mode in _hip.NCE_ESTIMATORS.items():
                row[f"{mname}_ms"] = round(nce_ms(b, d, prec, mode, reps, calls), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
