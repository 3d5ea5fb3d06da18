#!/usr/bin/env python3
"""HIP-event times of the top-k retrieval (mi_topk_bilinear, both directions) at B = 4096, d = 512, k = 10, bf16 and "f32"
(bf16x3), beside two neighbours that alternate with it inside one run:
  * mi_rank_bilinear -- the same prep, T = X W and score sweep (one sweep for both directions, against one per direction
    here), a counting epilogue instead of the key atomics;
  * the torch route a user has without this entry point: torch.topk((x @ w) @ y.T, k) in both directions, which holds
    the [B, B] fp32 matrix.
Median of `reps` timed batches of `calls` calls each, then the per-kernel split of one call (_hip.kernel_profile) and
the workspace sizes.
usage: topk_time.py [reps] [calls] [B] [d] [k]"""
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
    k = int(sys.argv[5]) if len(sys.argv) > 5 else 10
    lib, dev = _hip.load(), torch.device("cuda:0")
    x, y, w, sid = _tensors(b, d, dev)
    st = _hip.stream_ptr(dev)
    for pname, prec in PRECS.items():
        ws_k = _hip.workspace(lib.mi_topk_bilinear_workspace_bytes(b, b, d, d, prec, k), dev)
        ws_r = _hip.workspace(lib.mi_rank_bilinear_workspace_bytes(b, d, d, prec), dev)
        ii, it = (torch.empty(b, k, dtype=torch.int32, device=dev) for _ in range(2))
        vi, vt = (torch.empty(b, k, dtype=torch.float32, device=dev) for _ in range(2))
        ri, rt = (torch.empty(b, dtype=torch.int32, device=dev) for _ in range(2))
        topk_args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), None, None, b, b, d, d, prec, k, ii.data_ptr(), vi.data_ptr(),
                     it.data_ptr(), vt.data_ptr(), ws_k.data_ptr(), ws_k.numel(), st)
        rank_args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, prec, ri.data_ptr(), rt.data_ptr(),
                     None, ws_r.data_ptr(), ws_r.numel(), st)
        _hip.check(lib.mi_topk_bilinear(*topk_args), "mi_topk_bilinear")
        _hip.check(lib.mi_rank_bilinear(*rank_args), "mi_rank_bilinear")
        xt, wt, yt = (x.bfloat16(), w.bfloat16(), y.bfloat16()) if pname == "bf16" else (x, w, y)

        def torch_route():
            s = ((xt @ wt) @ yt.t()).float()
            return torch.topk(s, k, dim=1), torch.topk(s, k, dim=0)

        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        torch_route()
        torch.cuda.synchronize()
        torch_mib = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        legs = {"topk": lambda: lib.mi_topk_bilinear(*topk_args), "rank": lambda: lib.mi_rank_bilinear(*rank_args),
                "torch": torch_route}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in legs}
        for _ in range(reps):  # alternating: every leg sees the same clocks and the same neighbours
            for name, fn in legs.items():
                ts[name].append(_batch_ms(fn, calls))
        med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
        row = {"b": b, "d": d, "k": k, "precision": pname,
               **{f"{name}_ms": round(med[name], 4) for name in legs},
               **{f"{name}_ms_min_max": [round(min(ts[name]), 4), round(max(ts[name]), 4)] for name in legs},
               "topk_over_rank": round(med["topk"] / med["rank"], 3), "topk_over_torch": round(med["topk"] / med["torch"], 3),
               "workspace_mib": {"topk": round(ws_k.numel() / 2 ** 20, 1), "rank": round(ws_r.numel() / 2 ** 20, 1),
                                 "torch_peak": round(torch_mib, 1)},
               "topk_kernels_ms": _split(legs["topk"]), "rank_kernels_ms": _split(legs["rank"])}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
