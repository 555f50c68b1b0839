"""The step plan in effect across the feature states (engine.cpp: one StepPlan per form, plan()).

tools/step_plan_walk.py walks six tiny engines (a 12x12 group engine created with the switches
unset, with FFM_STEP_SHARDS=2 and with FFM_GROUP_ONE=0; a lane, a wave and a block engine) through
per-env parameters and rooms on and off, in the order that exercises every hand-over between the
create plan, the two per-env plans and the room plan.  Every state's launch_info(),
group_occupancy() of both forms, counter slots, set and room counts and the sha256 of the state
after reset() + step(3) must equal tests/golden/step_plan_walk.json, which was recorded with the
same tool from the library of the commit before the plans were introduced (the file names it).
"""
import json
import os
import sys

import pytest

from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import step_plan_walk as W   # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "step_plan_walk.json")) as f:
        doc = json.load(f)
    assert doc["recorded_from"], "the golden file names the commit it was recorded from"
    return doc["walks"]


@pytest.mark.parametrize("name", sorted(W.ENGINES))
def test_walk_matches_the_recorded_plans(golden, name):
    got = json.loads(json.dumps(W.walk(name)))
    want = golden[name]
    assert [s for s, _ in got] == [s for s, _ in want] == ["created"] + [w[0] for w in W.WALKS[name]]
    # off again: the create plan, untouched by what the walk computed in between
    assert got[-1][1]["launch_info"] == got[0][1]["launch_info"]
    assert W.differences({name: got}, {name: want}) == []
    for (state, g), (_, w) in zip(got, want):
        assert g == w, f"{name} / {state}"


def test_walks_cover_every_plan(golden):
    """The recorded walks are not vacuous: the group engine steps with all three kernels' plans, the
    shard count distinguishes the create plan, and the states' results differ from one another."""
    kernels = [r["launch_info"]["kernel"] for _, r in golden["group"]]
    assert kernels == ["group", "lane", "group", "lane", "group", "group", "group", "group", "group", "lane", "group"]
    shards = [r["launch_info"]["step_shards"] for _, r in golden["group_shards2"]]
    assert shards[0] == shards[-1] == shards[5] == 2 and shards[2] == 1
    assert [r["launch_info"]["kernel"] for _, r in golden["wave"]] == ["wave", "block", "wave", "block", "wave"]
    assert [r["launch_info"]["kernel"] for _, r in golden["lane"]] == ["lane"] * 5
    assert not golden["group_loop"][0][1]["launch_info"]["group_one"] and golden["group_loop"][6][1]["launch_info"]["group_one"]
    assert len({r["sha256"] for _, r in golden["group"]}) >= 4
