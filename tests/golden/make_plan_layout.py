#!/usr/bin/env python3
"""Writes tests/golden/plan_layout.json: what the host-side planners of csrc/mi_bilinear.hip answer for a table of shapes
-- workspace sizes, the raw-record region, the kernel path -- for the bilinear and the separable critic and for the
per-sample InfoNCE / f-divergence chains that embed the bilinear plan.  Host arithmetic only: no GPU is needed.

    MI_CRITIC_LIB=/path/to/libmi_critic_hip.so python tests/golden/make_plan_layout.py

Run it against a build of the commit whose layout is the contract (the parent of a host-code refactor), never against the
branch under test.  tests/test_plan_layout.py asserts that the library under test answers the same."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "plan_layout.json")

PRECISIONS = {"f32": 0, "bf16": 1, "bf16x3": 2, "fp8": 3}  # MI_PREC_* of include/mi_critic.h

# (b_rows, b, d_img, d_txt[, d_proj]); every row is queried in all four precisions
ROWS = [
    (4096, 4096, 512, 512),       # the headline
    (512, 4096, 512, 512),        # a row block of it
    (4096, 4096, 768, 768),       # the reference's width: outside the fused kernel
    (512, 4096, 768, 768),
    (128, 128, 32, 128),          # fused kernels with the two-launch tail, at its edge
    (128, 256, 32, 128),
    (96, 96, 128, 128),           # fused kernels, no tail
    (32, 32, 128, 128),
    (256, 256, 256, 256),
    (128, 512, 64, 64),           # row block on the GEMM chain: dT split-K
    (40, 40, 24, 40),             # GEMMs only
    (37, 37, 19, 23),             # odd: generic kernels
    (64, 64, 64, 64),             # fp8 takes it
    (64, 64, 24, 24),             # fp8 rejects it
    (128, 128, 64, 96, 128),      # separable: tail
    (96, 96, 64, 96, 128),        # separable: fused, no tail
    (64, 64, 64, 64, 48),         # separable: generic
    (4096, 4096, 512, 512, 256),
    (512, 4096, 512, 512, 256),
    (37, 37, 19, 23, 11),
]

_SZ, _I64, _I = ctypes.c_size_t, ctypes.c_int64, ctypes.c_int


def _fn(lib, name, res, args):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = res, args
    return fn


def query(lib, row, precision):
    """Every planner answer for one row and precision, as a flat dict of ints."""
    br, b, dx, dy = row[:4]
    off = _SZ(0)
    n_rec = _fn(lib, "mi_bilinear_raw_records", _SZ, [_I64] * 4 + [_I, ctypes.c_void_p])(br, b, dx, dy, precision, ctypes.byref(off))
    q = {
        "bilinear_workspace_bytes": _fn(lib, "mi_bilinear_workspace_bytes", _SZ, [_I64] * 4 + [_I])(br, b, dx, dy, precision),
        "raw_records": n_rec,
        "raw_records_offset": off.value if n_rec else 0,
        "bilinear_path": _fn(lib, "mi_bilinear_path", _I, [_I64] * 4 + [_I])(br, b, dx, dy, precision),
        "nce_bilinear_workspace_bytes": _fn(lib, "mi_nce_bilinear_workspace_bytes", _SZ, [_I64] * 3 + [_I])(b, dx, dy, precision),
        "nce_bilinear_shard_workspace_bytes":
            _fn(lib, "mi_nce_bilinear_shard_workspace_bytes", _SZ, [_I64] * 4 + [_I])(br, b, dx, dy, precision),
        "fdiv_bilinear_workspace_bytes": _fn(lib, "mi_fdiv_bilinear_workspace_bytes", _SZ, [_I64] * 3 + [_I])(b, dx, dy, precision),
    }
    if len(row) == 5:
        k = row[4]
        q.update({
            "separable_workspace_bytes": _fn(lib, "mi_separable_workspace_bytes", _SZ, [_I64] * 5 + [_I])(br, b, dx, dy, k, precision),
            "separable_path": _fn(lib, "mi_separable_path", _I, [_I64] * 5 + [_I])(br, b, dx, dy, k, precision),
            "nce_separable_workspace_bytes":
                _fn(lib, "mi_nce_separable_workspace_bytes", _SZ, [_I64] * 4 + [_I])(b, dx, dy, k, precision),
            "nce_separable_shard_workspace_bytes":
                _fn(lib, "mi_nce_separable_shard_workspace_bytes", _SZ, [_I64] * 5 + [_I])(br, b, dx, dy, k, precision),
            "fdiv_separable_workspace_bytes":
                _fn(lib, "mi_fdiv_separable_workspace_bytes", _SZ, [_I64] * 4 + [_I])(b, dx, dy, k, precision),
        })
    return q


def key(row, precision_name):
    return "/".join(str(v) for v in row) + "/" + precision_name


def table(lib):
    return {key(row, name): query(lib, row, code) for row in ROWS for name, code in PRECISIONS.items()}


def ab_switches_set():
    """Environment switches of the library (MI_NO_TAIL, MI_FLASH_TILES, ...) that would change the plans."""
    return sorted(k for k in os.environ if k.startswith("MI_") and k not in ("MI_CRITIC_LIB", "MI_SKIP_SLOW"))


def main():
    if ab_switches_set():
        sys.exit(f"refusing to record plans with A/B switches set: {ab_switches_set()}")
    path = os.environ.get("MI_CRITIC_LIB")
    if not path:
        sys.exit("set MI_CRITIC_LIB to the library of the commit whose layout is the contract")
    with open(OUT, "w") as f:
        json.dump(table(ctypes.CDLL(os.path.abspath(path))), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
