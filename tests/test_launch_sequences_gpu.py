"""Every entry point and host path of the DV / InfoNCE drivers (csrc/mi_bilinear.hip) issues the launches that
tests/golden/launch_sequences.json recorded -- the same kernels under the same labels in the same order -- and leaves
finite outputs.  The fixture comes from the commit BEFORE the bilinear and the separable driver were folded into one
fused-stage description (tests/golden/make_launch_sequences.py); the labels are what mi_profile_begin / mi_profile_end,
`bench.py --full` and profiles/ show.  The cases and their shapes are in tests/launch_cases.py."""
import json
import os

import pytest
import torch

import launch_cases

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences.json")) as _f:
    FIXTURE = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(FIXTURE) == sorted(launch_cases.CASES)
    assert all(len(v) >= 2 for v in FIXTURE.values())


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(launch_cases.CASES))
def test_launch_sequence(built, name):
    labels, out = launch_cases.run_case(name, torch.device("cuda:0"))
    assert labels == FIXTURE[name]
    for key, t in out.items():
        if t.dtype != torch.uint8:  # (the statistics block holds integer counts beside its floats)
            assert bool(torch.isfinite(t.float()).all()), f"{name}: {key} is not finite"
