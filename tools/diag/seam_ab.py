#!/usr/bin/env python3
"""A/B timing of several builds of libmi_critic_hip.so in ONE process on ONE device: the headline step (mi_bilinear_step,
B = 4096, d = 512, bf16, fp32 boundary, the seeded inputs of bench.py) through each library in alternating rounds.

    python tools/diag/seam_ab.py parent=/path/to/parent/libmi_critic_hip.so branch=mutual-information-multimodal_amd/lib/libmi_critic_hip.so
        [--rounds 9] [--steps 200] [--profile-rounds 3] [--profile-steps 20] [--batch 4096] [--dim 512]

NAME=PATH@VAR=1,VAR2=x sets environment switches for that library alone (e.g. branch_nat=...so@MI_DW_XCD_NATURAL=1): the
library reads such switches once, on its first launch, so they are set around that build's first steps only; the same file
may be given twice under two names (it is copied, so that the loader maps it twice).

Boxes differ by ~4 % and a profiled run by ~8 %, so only this kind of timing may rank two builds.  Per build it prints
the median / min / max over the rounds of the whole step (HIP events around --steps back-to-back calls) and the median
per launch from the library's own profiling hook (mi_profile_begin / mi_profile_end, rounds of their own: the events
between the launches cost time).  The first library is the reference of the bitwise comparison of every output, and of
the verdict line: "<name> slowest round < <reference> fastest round".  Per launch it also prints the median of every
profiled round and, against the first library, the gain over that library's own round-to-round spread (max - min of its
round medians): a launch counts as faster when the gain exceeds three spreads.  One JSON line at the end.
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
import torch  # noqa: E402

import bench  # noqa: E402
from mutual_info_img_txt import _hip  # noqa: E402


def open_lib(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _hip.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Build:
    def __init__(self, name, path, x, y, w, sid, dev):
        path, _, env = path.partition("@")
        self.env = dict(kv.split("=", 1) for kv in env.split(",")) if env else {}
        if self.env:  # a private copy: dlopen of a path already loaded would hand back the same library and its state
            import shutil
            import tempfile
            private = os.path.join(tempfile.mkdtemp(prefix="seam_ab_"), os.path.basename(path))
            shutil.copy(path, private)
            path = private
        self.name, self.lib = name, open_lib(path)
        b, d = x.shape
        self.gx, self.gy, self.gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
        self.loss = torch.empty(1, device=dev)
        self.stats = _hip.new_stats(dev)
        self.record = torch.empty(_hip.RECORD_FLOATS, device=dev)
        self.go = torch.ones(1, device=dev)
        self.ws = _hip.workspace(self.lib.mi_bilinear_workspace_bytes(b, b, d, d, _hip.MI_PREC_BF16), dev)
        self.args = (x.data_ptr(), y.data_ptr(), w.data_ptr(), sid.data_ptr(), b, d, d, _hip.MI_INFONCE, _hip.MI_PREC_BF16,
                     self.go.data_ptr(), self.loss.data_ptr(), self.stats.data_ptr(), self.record.data_ptr(),
                     self.gx.data_ptr(), self.gy.data_ptr(), self.gw.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        self.step_ms, self.launch_ms, self.launch_rounds = [], {}, {}

    def step(self):
        rc = self.lib.mi_bilinear_step(*self.args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{self.name}: mi_bilinear_step -> {rc}: {self.lib.mi_last_error()}")

    def timed(self, steps):
        for _ in range(10):
            self.step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            self.step()
        e1.record()
        e1.synchronize()
        self.step_ms.append(e0.elapsed_time(e1) / steps)

    def profiled(self, steps):
        cap = 64 * steps
        assert self.lib.mi_profile_begin() == 0
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(cap * 48)
        ms = (ctypes.c_float * cap)()
        n = ctypes.c_int(0)
        assert self.lib.mi_profile_end(names, len(names), ms, cap, ctypes.byref(n)) == 0
        parts = names.raw.split(b"\0")
        this = {}
        for k in range(n.value):
            self.launch_ms.setdefault(parts[k].decode(), []).append(float(ms[k]))
            this.setdefault(parts[k].decode(), []).append(float(ms[k]))
        for k, v in this.items():
            self.launch_rounds.setdefault(k, []).append(statistics.median(v) * 1e3)

    def outputs(self):
        torch.cuda.synchronize()
        return {"loss": self.loss, "grad_x": self.gx, "grad_y": self.gy, "grad_w": self.gw}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("libs", nargs="+", metavar="NAME=PATH")
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--profile-steps", type=int, default=20)
    p.add_argument("--profile-rounds", type=int, default=3)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--dim", type=int, default=512)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    # which box this is: rows of different boxes differ by 2-4 % and must not be compared with each other
    import hashlib
    import socket
    prop = torch.cuda.get_device_properties(0)
    box = hashlib.sha1((socket.gethostname() + str(getattr(prop, "uuid", ""))).encode()).hexdigest()[:8]
    print(f"device: {prop.name}, box id {box} (hash of host name and device uuid)")
    x, y, sid = bench.make_inputs(a.batch, a.dim, a.dim, 3, 0, 1, dev)
    x, y = x.bfloat16().float().contiguous(), y.bfloat16().float().contiguous()  # as bench.py: bf16-representable values
    w = bench.make_critic("bilinear", a.dim, a.dim, 3, dev).weight.detach().float().contiguous()
    builds = [Build(*s.split("=", 1), x, y, w, sid, dev) for s in a.libs]

    for bd in builds:  # warm-up, then every output against the first library's, bit for bit
        os.environ.update(bd.env)
        for _ in range(20):
            bd.step()
        for k in bd.env:
            del os.environ[k]
    ref = {k: v.clone() for k, v in builds[0].outputs().items()}
    same = {}
    for bd in builds[1:]:
        same[bd.name] = {k: bool(torch.equal(v.view(torch.int32), ref[k].view(torch.int32))) for k, v in bd.outputs().items()}
        print(f"bits {bd.name} == {builds[0].name}:", same[bd.name])

    warm = torch.cuda.Event(enable_timing=True)
    for _ in range(3000):  # ~0.3 s of the step itself: clocks settled before the first round
        builds[0].step()
    warm.record()
    warm.synchronize()
    for r in range(a.rounds):
        for bd in (builds if r % 2 == 0 else builds[::-1]):
            bd.timed(a.steps)
    for r in range(a.profile_rounds):
        for bd in (builds if r % 2 == 0 else builds[::-1]):
            bd.profiled(a.profile_steps)

    out = {"box": box, "shape": [a.batch, a.dim], "rounds": a.rounds, "steps": a.steps, "bits_equal": same, "builds": {}}
    base = builds[0]
    for bd in builds:
        t = bd.step_ms
        per = {k: round(statistics.median(v) * 1e3, 2) for k, v in bd.launch_ms.items()}
        out["builds"][bd.name] = {"step_us_median": round(statistics.median(t) * 1e3, 2), "step_us_min": round(min(t) * 1e3, 2),
                                  "step_us_max": round(max(t) * 1e3, 2), "step_us_rounds": [round(v * 1e3, 2) for v in t],
                                  "launch_us_median": per,
                                  "launch_us_rounds": {k: [round(x, 2) for x in v] for k, v in bd.launch_rounds.items()}}
        print(f"{bd.name:14s} step median {statistics.median(t) * 1e3:8.2f} us  min {min(t) * 1e3:8.2f}  max {max(t) * 1e3:8.2f}"
              f"   launches {per}")
    for k, v in base.launch_rounds.items():
        spread = max(v) - min(v)
        print(f"{k}: {base.name} round medians {min(v):.2f} .. {max(v):.2f} us (spread {spread:.2f})")
        for bd in builds[1:]:
            w = bd.launch_rounds.get(k)
            if w:
                gain = statistics.median(v) - statistics.median(w)
                print(f"    {bd.name}: {min(w):.2f} .. {max(w):.2f} us, gain {gain:+.2f} us = {gain / spread if spread > 0 else float('inf'):+.1f} spreads")
    for bd in builds[1:]:
        ok = max(bd.step_ms) < min(base.step_ms)
        out["builds"][bd.name]["slowest_below_reference_fastest"] = ok
        print(f"{bd.name}: slowest round {max(bd.step_ms) * 1e3:.2f} us {'<' if ok else '>='} {base.name} fastest round "
              f"{min(base.step_ms) * 1e3:.2f} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
