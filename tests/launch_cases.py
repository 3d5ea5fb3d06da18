"""The calls whose launch sequences tests/golden/launch_sequences.json pins: one function per case, shared by the
generator (tests/golden/make_launch_sequences.py, run against a build of the PARENT commit) and the test
(tests/test_launch_sequences_gpu.py).  The shapes are the smallest that reach each host path of the DV / InfoNCE drivers
of csrc/mi_bilinear.hip.  Every case runs on seeded inputs with repeated study ids, through the C ABI of the library
`_hip.load()` returns, and gives (launch labels in order, {output name: tensor})."""
import ctypes

import torch

from mutual_info_img_txt import _hip

F32, BF16, BF16X3, FP8 = _hip.MI_PREC_F32, _hip.MI_PREC_BF16, _hip.MI_PREC_BF16X3, _hip.MI_PREC_FP8
PREC_NAMES = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3", FP8: "fp8"}
EST = _hip.MI_INFONCE


def _inputs(dev, b, widths, weights, seed=0):
    """Embeddings [b][width] for every width, weights [r][c] for every (r, c), study ids with repeats, dL/dloss."""
    g = torch.Generator().manual_seed(1000 + seed)
    emb = [torch.randn(b, d, generator=g).to(dev) for d in widths]
    ws = [(torch.randn(r, c, generator=g) / r ** 0.5).to(dev) for r, c in weights]
    sid = torch.randint(0, max(2, (3 * b) // 4), (b,), generator=g, dtype=torch.int64).to(dev)
    go = torch.full((1,), 0.75, device=dev)
    return emb, ws, sid, go


class _Out:
    """Zero-initialised outputs of one case (zero: bytes the library leaves alone compare equal between two builds)."""

    def __init__(self, dev):
        self.dev, self.t = dev, {}

    def f32(self, name, *shape):
        self.t[name] = torch.zeros(*shape, dtype=torch.float32, device=self.dev)
        return self.t[name].data_ptr()

    def bf16(self, name, *shape):
        self.t[name] = torch.zeros(*shape, dtype=torch.bfloat16, device=self.dev)
        return self.t[name].data_ptr()

    def stats(self, name="stats"):
        self.t[name] = torch.zeros(_hip.STATS_BYTES, dtype=torch.uint8, device=self.dev)
        return self.t[name].data_ptr()


def _ws(nbytes, dev):
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _call(name, *args):
    _hip.check(getattr(_hip.load(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def bilinear_step(dev, b, dx, dy, prec):
    lib = _hip.load()
    (x, y), (w,), sid, go = _inputs(dev, b, (dx, dy), ((dx, dy),))
    o = _Out(dev)
    ws = _ws(lib.mi_bilinear_workspace_bytes(b, b, dx, dy, prec), dev)
    _call("mi_bilinear_step", x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, dx, dy, EST, prec, go.data_ptr(),
          o.f32("loss", 1), o.stats(), o.f32("partials", _hip.RECORD_FLOATS), o.f32("grad_x", b, dx), o.f32("grad_y", b, dy),
          o.f32("grad_w", dx, dy), ws.data_ptr(), ws.numel())
    return o.t


def bilinear_step_bf16(dev, b, dx, dy, grads_bf16):
    lib = _hip.load()
    (x, y), (w,), sid, go = _inputs(dev, b, (dx, dy), ((dx, dy),))
    xb, yb = x.bfloat16().contiguous(), y.bfloat16().contiguous()
    o = _Out(dev)
    grad = o.bf16 if grads_bf16 else o.f32
    ws = _ws(lib.mi_bilinear_workspace_bytes(b, b, dx, dy, BF16), dev)
    _call("mi_bilinear_step_bf16", xb.data_ptr(), yb.data_ptr(), w.data_ptr(), sid.data_ptr(), b, dx, dy, EST, go.data_ptr(),
          o.f32("loss", 1), o.stats(), o.f32("partials", _hip.RECORD_FLOATS), grad("grad_x", b, dx), grad("grad_y", b, dy),
          grads_bf16, o.f32("grad_w", dx, dy), ws.data_ptr(), ws.numel())
    return o.t


def bilinear_fwd_bwd(dev, br, b, row_offset, dx, dy, prec, scores, from_forward):
    """mi_bilinear_fwd then mi_bilinear_bwd of the row block [row_offset, row_offset + br) (the statistics of the block
    alone stand in for the merged ones: the launches do not depend on their values)."""
    lib = _hip.load()
    (x, y), (w,), sid, go = _inputs(dev, b, (dx, dy), ((dx, dy),))
    x, sid_rows = x[row_offset:row_offset + br].contiguous(), sid[row_offset:row_offset + br].contiguous()
    o = _Out(dev)
    ws = _ws(lib.mi_bilinear_workspace_bytes(br, b, dx, dy, prec), dev)
    stats = o.stats()
    _call("mi_bilinear_fwd", x.data_ptr(), y.data_ptr(), w.data_ptr(), sid_rows.data_ptr(), sid.data_ptr(), br, b, row_offset,
          dx, dy, EST, prec, 1, o.f32("loss", 1), stats, o.f32("partials", _hip.RECORD_FLOATS),
          o.f32("scores", br, b) if scores else None, ws.data_ptr(), ws.numel())
    _call("mi_bilinear_bwd", x.data_ptr(), y.data_ptr(), w.data_ptr(), sid_rows.data_ptr(), sid.data_ptr(), br, b, row_offset,
          dx, dy, prec, stats, go.data_ptr(), o.f32("grad_x", br, dx), o.f32("grad_y", b, dy), o.f32("grad_w", dx, dy),
          ws.data_ptr(), ws.numel(), from_forward)
    return o.t


def bilinear_sharded(dev, br, b, dx, dy):
    """The sharded step of the LAST rank of b / br: prep_local -> fwd(need_grad | 4 | 8) -> bwd_records(grad_w = NULL)
    -> bwd_dw.  The records of the ranks before it come from plain forwards issued first (their launches are part of the
    recorded sequence: the recording is per case)."""
    lib = _hip.load()
    (x, y), (w,), sid, go = _inputs(dev, b, (dx, dy), ((dx, dy),))
    off = ctypes.c_size_t(0)
    n = lib.mi_bilinear_raw_records(br, b, dx, dy, BF16, ctypes.byref(off))
    assert n > 0
    o = _Out(dev)
    nbytes = lib.mi_bilinear_workspace_bytes(br, b, dx, dy, BF16)
    records, dummy = [], _Out(dev)
    for r in range(b // br):
        ro = r * br
        xr, sr = x[ro:ro + br].contiguous(), sid[ro:ro + br].contiguous()
        ws = _ws(nbytes, dev)
        bits = 1 | 8
        if ro + br == b:
            _call("mi_bilinear_prep_local", xr.data_ptr(), w.data_ptr(), br, b, dx, dy, BF16, ws.data_ptr(), ws.numel())
            bits |= 4
        _call("mi_bilinear_fwd", xr.data_ptr(), y.data_ptr(), w.data_ptr(), sr.data_ptr(), sid.data_ptr(), br, b, ro, dx, dy,
              EST, BF16, bits, None, dummy.stats(), None, None, ws.data_ptr(), ws.numel())
        records.append(ws[off.value:off.value + 16 * n].view(torch.float32).clone())
    rec = torch.cat(records).contiguous()
    o.t["records"] = rec
    _call("mi_bilinear_bwd_records", xr.data_ptr(), y.data_ptr(), w.data_ptr(), sr.data_ptr(), sid.data_ptr(), br, b, ro, dx,
          dy, BF16, EST, rec.data_ptr(), rec.numel() // 4, b, go.data_ptr(), o.f32("loss", 1), o.stats(),
          o.f32("grad_x", br, dx), o.f32("grad_y", b, dy), None, ws.data_ptr(), ws.numel())
    _call("mi_bilinear_bwd_dw", br, b, dx, dy, BF16, o.f32("grad_w", dx, dy), ws.data_ptr(), ws.numel())
    return o.t


def separable_step(dev, b, dx, dy, k, prec):
    lib = _hip.load()
    (x, y), (wg, wh), sid, go = _inputs(dev, b, (dx, dy), ((dx, k), (dy, k)))
    o = _Out(dev)
    ws = _ws(lib.mi_separable_workspace_bytes(b, b, dx, dy, k, prec), dev)
    _call("mi_separable_step", x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(), sid.data_ptr(), b, dx, dy, k, EST, prec,
          go.data_ptr(), o.f32("loss", 1), o.stats(), o.f32("partials", _hip.RECORD_FLOATS), o.f32("grad_x", b, dx),
          o.f32("grad_y", b, dy), o.f32("grad_wg", dx, k), o.f32("grad_wh", dy, k), ws.data_ptr(), ws.numel())
    return o.t


def separable_fwd_bwd(dev, b, dx, dy, k, prec, from_forward):
    lib = _hip.load()
    (x, y), (wg, wh), sid, go = _inputs(dev, b, (dx, dy), ((dx, k), (dy, k)))
    o = _Out(dev)
    ws = _ws(lib.mi_separable_workspace_bytes(b, b, dx, dy, k, prec), dev)
    stats = o.stats()
    _call("mi_separable_fwd", x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(), sid.data_ptr(), sid.data_ptr(), b, b, 0,
          dx, dy, k, EST, prec, 1, o.f32("loss", 1), stats, o.f32("partials", _hip.RECORD_FLOATS), ws.data_ptr(), ws.numel())
    _call("mi_separable_bwd", x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(), sid.data_ptr(), sid.data_ptr(), b, b, 0,
          dx, dy, k, prec, stats, go.data_ptr(), o.f32("grad_x", b, dx), o.f32("grad_y", b, dy), o.f32("grad_wg", dx, k),
          o.f32("grad_wh", dy, k), ws.data_ptr(), ws.numel(), from_forward)
    return o.t


def chain_separable_step(dev, family, b, dx, dy, k, prec):
    """mi_nce_separable_step (symmetric) / mi_fdiv_separable_step (JSD) with every gradient."""
    lib = _hip.load()
    (x, y), (wg, wh), sid, go = _inputs(dev, b, (dx, dy), ((dx, k), (dy, k)))
    o = _Out(dev)
    ws = _ws(getattr(lib, f"mi_{family}_separable_workspace_bytes")(b, dx, dy, k, prec), dev)
    head = (x.data_ptr(), y.data_ptr(), wg.data_ptr(), wh.data_ptr(), sid.data_ptr(), b, dx, dy, k)
    grads = lambda: (o.f32("grad_x", b, dx), o.f32("grad_y", b, dy), o.f32("grad_wg", dx, k), o.f32("grad_wh", dy, k))
    if family == "nce":
        _call("mi_nce_separable_step", *head, _hip.MI_NCE_SYMMETRIC, prec, go.data_ptr(), o.f32("loss", 1),
              o.f32("lse_rows", b), o.f32("lse_cols", b), *grads(), ws.data_ptr(), ws.numel())
    else:
        _call("mi_fdiv_separable_step", *head, _hip.MI_FDIV_JSD, prec, go.data_ptr(), o.f32("loss", 1), o.f32("terms", 2),
              o.stats(), *grads(), ws.data_ptr(), ws.numel())
    return o.t


def _cases():
    c = {}
    for b, dx, dy, prec in ((128, 32, 128, BF16), (96, 128, 128, BF16), (40, 24, 40, BF16), (64, 64, 64, BF16X3),
                            (37, 19, 23, F32), (37, 19, 23, BF16), (64, 64, 64, FP8)):
        c[f"bilinear_step-{b}-{dx}-{dy}-{PREC_NAMES[prec]}"] = lambda dev, a=(b, dx, dy, prec): bilinear_step(dev, *a)
    # (the bf16 boundary needs d_img % 64 == 0 on top of the fused tail's shapes: 128/32/128 is MI_ESHAPE there)
    for gb in (0, 1):
        c[f"bilinear_step_bf16-128-64-128-grads_bf16={gb}"] = lambda dev, gb=gb: bilinear_step_bf16(dev, 128, 64, 128, gb)
    for scores in (0, 1):
        for wff in (0, 1):
            c[f"bilinear_fwd_bwd-128-32-128-bf16-scores={scores}-from_forward={wff}"] = (
                lambda dev, s=scores, f=wff: bilinear_fwd_bwd(dev, 128, 128, 0, 32, 128, BF16, s, f))
    c["bilinear_sharded-rows128..255of256-32-128-bf16"] = lambda dev: bilinear_sharded(dev, 128, 256, 32, 128)
    # a row block at a width outside the fused kernel: the dT split-K branch of the G-materialising backward
    c["bilinear_fwd_bwd-rows128..255of512-64-64-bf16"] = lambda dev: bilinear_fwd_bwd(dev, 128, 512, 128, 64, 64, BF16, 0, 1)
    for b, dx, dy, k, prec in ((128, 64, 96, 128, BF16), (96, 64, 96, 128, BF16), (64, 64, 64, 48, BF16), (64, 64, 64, 48, F32)):
        c[f"separable_step-{b}-{dx}-{dy}-{k}-{PREC_NAMES[prec]}"] = lambda dev, a=(b, dx, dy, k, prec): separable_step(dev, *a)
    for wff in (0, 1):
        c[f"separable_fwd_bwd-128-64-96-128-bf16-from_forward={wff}"] = (
            lambda dev, f=wff: separable_fwd_bwd(dev, 128, 64, 96, 128, BF16, f))
    for family in ("nce", "fdiv"):
        for prec in (BF16, F32):
            c[f"{family}_separable_step-64-64-64-48-{PREC_NAMES[prec]}"] = (
                lambda dev, fam=family, p=prec: chain_separable_step(dev, fam, 64, 64, 64, 48, p))
    return c


CASES = _cases()


def run_case(name, dev):
    """(launch labels of the case in order, its outputs)"""
    with _hip.kernel_profile() as prof:
        out = CASES[name](dev)
        torch.cuda.synchronize()
    return [label for label, _ in prof.records], out
