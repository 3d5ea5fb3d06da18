#!/usr/bin/env python3
"""Writes tests/golden/launch_sequences.json: for every case of tests/launch_cases.py the launch labels the library's
profiling hook (mi_profile_begin / mi_profile_end, `_hip.kernel_profile`) sees, in order.  Needs a GPU.

    MI_CRITIC_LIB=/path/to/libmi_critic_hip.so python tests/golden/make_launch_sequences.py [--dump-outputs DIR]

Run it against a build of the commit whose launch sequences are the contract (the parent of a host-code refactor), never
against the branch under test.  --dump-outputs DIR also writes every output of every case to DIR/<case>.npz (raw bytes),
for a bit-for-bit comparison of two builds; DIR then gets its own launch_sequences.json and the fixture is left alone."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "mutual-information-multimodal_amd"), ROOT):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump-outputs", metavar="DIR")
    a = ap.parse_args()
    switches = sorted(k for k in os.environ if k.startswith("MI_") and k not in ("MI_CRITIC_LIB", "MI_SKIP_SLOW"))
    if switches:
        sys.exit(f"refusing to record launch sequences with A/B switches set: {switches}")
    if not os.environ.get("MI_CRITIC_LIB"):
        sys.exit("set MI_CRITIC_LIB to the library of the commit whose launch sequences are the contract")
    import numpy as np
    import torch

    import launch_cases

    dev = torch.device("cuda:0")
    seqs = {}
    for name in launch_cases.CASES:
        labels, out = launch_cases.run_case(name, dev)
        seqs[name] = labels
        print(f"{name}: {len(labels)} launches", flush=True)
        if a.dump_outputs:
            os.makedirs(a.dump_outputs, exist_ok=True)
            np.savez(os.path.join(a.dump_outputs, name + ".npz"),
                     **{k: v.contiguous().view(torch.uint8).cpu().numpy() for k, v in out.items()})
    dst = os.path.join(a.dump_outputs, "launch_sequences.json") if a.dump_outputs else os.path.join(HERE, "launch_sequences.json")
    with open(dst, "w") as f:
        json.dump(seqs, f, indent=1)
        f.write("\n")
    print(f"wrote {dst}")


if __name__ == "__main__":
    main()
