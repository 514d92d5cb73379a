"""The update's launch plan, pinned: for every case of tools/gen_launch_plan.py (fused updates of
both depths and dtypes, the ride-along placements, the draw-ahead, prioritized replay with and
without feedback, each opt-in feature, the data-parallel sequences over a loopback communicator)
the launches the host planner enqueues are those of tests/golden/launch_plan.json, launch for
launch: site name, kernel, grid, and the site's algorithmic FLOPs and bytes.

The fixture was recorded on the commit before the planner in csrc/sacmi.hip was split into its
pieces, twice, and the two records were identical: every case, the side-stream
(prioritized replay) ones included, is reported in the order the planner marked its sites, so
the comparison is of ordered lists, not of multisets.  FLOPs and bytes are compared for exact
equality: the same host expressions produce them in the same order.

What the timeline cannot see stays with the bit-exact tests: the launches that carry no stamp
(the sharded sequence's chunk Adam and standalone Polyak pass, the collectives' stand-ins) and
kernel arguments other than the grid.  The Polyak ride shows as L12's grid."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_launch_plan",
                                               os.path.join(ROOT, "tools", "gen_launch_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "launch_plan.json")) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(golden):
    assert sorted(golden) == sorted(gen.CASES)


@pytest.mark.parametrize("case", list(gen.CASES))
def test_launch_plan(case, golden):
    got, want = gen.run_plan(case), golden[case]
    print(f"  [launch plan] {case}: {len(got)} launches (fixture {len(want)})")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, dict(zip(gen.FIELDS, g)), dict(zip(gen.FIELDS, w)))
    assert len(got) == len(want), (case, [r[0] for r in got[len(want):]], [r[0] for r in want[len(got):]])
