"""The host-side planners of csrc/mi_bilinear.hip answer what tests/golden/plan_layout.json recorded: workspace sizes, the
raw-record region the sharded step all-gathers by offset, and the kernel path, for the bilinear and separable critics and
the InfoNCE / f-divergence chains that embed the bilinear plan.  The fixture comes from the commit BEFORE the drivers were
folded into one fused-stage description (tests/golden/make_plan_layout.py): a reordered or resized workspace `take` would
break `workspace_from_forward`, `need_grad | 4` and multi-GPU runs silently.  Host arithmetic only: no GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_plan_layout", os.path.join(GOLDEN, "make_plan_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
with open(os.path.join(GOLDEN, "plan_layout.json")) as _f:
    FIXTURE = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


def test_fixture_covers_the_table():
    assert sorted(FIXTURE) == sorted(GEN.key(row, name) for row in GEN.ROWS for name in GEN.PRECISIONS)
    paths = {FIXTURE[k]["bilinear_path"] for k in FIXTURE}
    assert paths == {-2, 0, 1, 2, 3, 4}  # the fp8 shape error and every MI_PATH_*
    assert {FIXTURE[k]["separable_path"] for k in FIXTURE if "separable_path" in FIXTURE[k]} == {0, 2, 3}


@pytest.mark.parametrize("row", GEN.ROWS, ids=lambda r: "/".join(str(v) for v in r))
def test_plans_match_the_recorded_layout(lib, row):
    assert not GEN.ab_switches_set(), "the library's A/B switches change the plans: unset them"
    for name, code in GEN.PRECISIONS.items():
        assert GEN.query(lib, row, code) == FIXTURE[GEN.key(row, name)], GEN.key(row, name)
