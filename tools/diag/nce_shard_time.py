#!/usr/bin/env python3
"""HIP-event times of ONE rank's local launches of the sharded per-sample InfoNCE step, on one GPU:
mi_nce_bilinear_shard_fwd on a row block of B / G rows, mi_nce_merge_parts over G parts, mi_nce_bilinear_shard_bwd,
at B = 4096, G in {1, 2, 4, 8}, d in {512, 768}, precisions bf16 and "f32" (bf16x3), symmetric mode.  The G parts of the
merge are copies of this rank's part (the merge's cost does not depend on their values).  No collective is timed: the
all-gathers, the reduce-scatter and the all-reduce need several GPUs.  G = 1 also times the one-call step
(mi_nce_bilinear_step) for comparison.  Median of `reps` timed batches of `calls` calls.
usage: nce_shard_time.py [reps] [calls]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
import torch  # noqa: E402

from mutual_info_img_txt import _hip  # noqa: E402

PRECS = {"bf16": _hip.MI_PREC_BF16, "f32": _hip.MI_PREC_BF16X3}


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


def rank_ms(b, g, d, prec, mode, reps, calls):
    lib, dev = _hip.load(), torch.device("cuda:0")
    br = b // g
    off = (g - 1) * br  # the last rank: its diagonal is in the last row block
    gen = torch.Generator().manual_seed(b + d)
    x = torch.randn(br, d, generator=gen).to(dev)
    y = torch.randn(b, d, generator=gen).to(dev)
    w = (torch.randn(d, d, generator=gen) * (0.3 / d ** 0.5)).to(dev)
    sid = torch.arange(b, dtype=torch.int64)
    for n in range(b // 8):
        sid[n] = n - n % 2
    sid = sid.to(dev)
    sid_rows = sid[off:off + br].contiguous()
    ws = _hip.workspace(lib.mi_nce_bilinear_shard_workspace_bytes(br, b, d, d, prec), dev)
    mws = _hip.workspace(lib.mi_nce_merge_workspace_bytes(b), dev)
    pf = lib.mi_nce_part_floats(br, b)
    parts = torch.empty(g, pf, device=dev)
    r = torch.empty(br, device=dev)
    loss, c = torch.empty(1, device=dev), torch.empty(b, device=dev)
    go = torch.ones(1, device=dev)
    gx, gy, gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
    st = _hip.stream_ptr(dev)
    fwd = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid_rows.data_ptr(), sid.data_ptr(), br, b, off, d, d, mode, prec,
           parts[g - 1].data_ptr(), r.data_ptr(), ws.data_ptr(), ws.numel(), st)
    mrg = (parts.data_ptr(), g, br, b, mode, loss.data_ptr(), c.data_ptr(), mws.data_ptr(), mws.numel(), st)
    bwd = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid_rows.data_ptr(), sid.data_ptr(), br, b, off, d, d, mode, prec,
           c.data_ptr(), go.data_ptr(), gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _hip.check(lib.mi_nce_bilinear_shard_fwd(*fwd), "mi_nce_bilinear_shard_fwd")
    parts.copy_(parts[g - 1].expand(g, pf))
    _hip.check(lib.mi_nce_merge_parts(*mrg), "mi_nce_merge_parts")
    _hip.check(lib.mi_nce_bilinear_shard_bwd(*bwd), "mi_nce_bilinear_shard_bwd")
    torch.cuda.synchronize()
    out = {"fwd_ms": _time(lambda: lib.mi_nce_bilinear_shard_fwd(*fwd), reps, calls),
           "merge_ms": _time(lambda: lib.mi_nce_merge_parts(*mrg), reps, calls),
           "bwd_ms": _time(lambda: lib.mi_nce_bilinear_shard_bwd(*bwd), reps, calls)}

    def rank_step():
        lib.mi_nce_bilinear_shard_fwd(*fwd)
        lib.mi_nce_merge_parts(*mrg)
        lib.mi_nce_bilinear_shard_bwd(*bwd)
    out["rank_step_ms"] = _time(rank_step, reps, calls)
    if g == 1:
        wsw = _hip.workspace(lib.mi_nce_bilinear_workspace_bytes(b, d, d, prec), dev)
        lr, lc = torch.empty(b, device=dev), torch.empty(b, device=dev)
        one = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, mode, prec, None, loss.data_ptr(),
               lr.data_ptr(), lc.data_ptr(), gx.data_ptr(), gy.data_ptr(), gw.data_ptr(), wsw.data_ptr(), wsw.numel(), st)
        _hip.check(lib.mi_nce_bilinear_step(*one), "mi_nce_bilinear_step")
        out["one_call_step_ms"] = _time(lambda: lib.mi_nce_bilinear_step(*one), reps, calls)
    return {k: round(v, 4) for k, v in out.items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    b = 4096
    for d in (512, 768):
        for pname, prec in PRECS.items():
            for g in (1, 2, 4, 8):
                row = {"b": b, "G": g, "b_rows": b // g, "d": d, "precision": pname, "mode": "infonce_symmetric"}
                row.update(rank_ms(b, g, d, prec, _hip.MI_NCE_SYMMETRIC, reps, calls))
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
