#!/usr/bin/env python3
"""HIP-event times of the retrieval ranks (mi_rank_bilinear) beside the forward-only per-sample InfoNCE step
(mi_nce_bilinear_step with every gradient pointer NULL) at B = 4096, d = 512, bf16 and "f32" (bf16x3).  The two share the
prep, T = X W and the score sweep and differ in the epilogue (counts against row / column LSE records), in what runs
before it (the diagonal) and after it (nothing against the merge and loss kernels).  The two calls alternate inside one
run: median of `reps` timed batches of `calls` calls each, then the per-kernel split of one call of each
(_hip.kernel_profile).
usage: rank_time.py [reps] [calls] [B] [d]"""
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
    return {name: round(v["ms_total"], 4) for name, v in prof.by_name().items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    b = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    d = int(sys.argv[4]) if len(sys.argv) > 4 else 512
    lib, dev = _hip.load(), torch.device("cuda:0")
    x, y, w, sid = _tensors(b, d, dev)
    st = _hip.stream_ptr(dev)
    for pname, prec in PRECS.items():
        ws_r = _hip.workspace(lib.mi_rank_bilinear_workspace_bytes(b, d, d, prec), dev)
        ws_n = _hip.workspace(lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec), dev)
        ri, rt = (torch.empty(b, dtype=torch.int32, device=dev) for _ in range(2))
        loss, r, c = torch.empty(1, device=dev), torch.empty(b, device=dev), torch.empty(b, device=dev)
        rank_args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, prec, ri.data_ptr(), rt.data_ptr(),
                     None, ws_r.data_ptr(), ws_r.numel(), st)
        nce_args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, _hip.MI_NCE_SYMMETRIC, prec, None,
                    loss.data_ptr(), r.data_ptr(), c.data_ptr(), None, None, None, ws_n.data_ptr(), ws_n.numel(), st)
        _hip.check(lib.mi_rank_bilinear(*rank_args), "mi_rank_bilinear")
        _hip.check(lib.mi_nce_bilinear_step(*nce_args), "mi_nce_bilinear_step")
        legs = {"rank": lambda: lib.mi_rank_bilinear(*rank_args), "nce_fwd": lambda: lib.mi_nce_bilinear_step(*nce_args)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in legs}
        for _ in range(reps):  # alternating: both legs see the same clocks and the same neighbours
            for k, fn in legs.items():
                ts[k].append(_batch_ms(fn, calls))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        row = {"b": b, "d": d, "precision": pname, "rank_ms": round(med["rank"], 4), "nce_fwd_ms": round(med["nce_fwd"], 4),
               "rank_over_nce_fwd": round(med["rank"] / med["nce_fwd"], 3),
               "rank_ms_min_max": [round(min(ts["rank"]), 4), round(max(ts["rank"]), 4)],
               "nce_fwd_ms_min_max": [round(min(ts["nce_fwd"]), 4), round(max(ts["nce_fwd"]), 4)],
               "workspace_mib": {"rank": round(ws_r.numel() / 2 ** 20, 1), "nce": round(ws_n.numel() / 2 ** 20, 1)},
               "rank_kernels_ms": _split(legs["rank"]), "nce_fwd_kernels_ms": _split(legs["nce_fwd"])}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
