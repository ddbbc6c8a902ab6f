"""No-GPU check of the weight-gradient scheduling policy (conv._WgradScheduler): the driver of tools/record_wgrad_schedule.py is
replayed on the scheduler with the launches stubbed out, and every scenario must equal tests/golden/wgrad_schedule.json -- recorded
once, with the same driver, from the commit before the scheduler was one object.  Per scenario: every launch (after which event, which
geometry, how many problems, which entry point, which weights in which order), every workspace request, the order in which weights
were reported written, the members of ops.GRAD_DEFERRED after every event, the warnings, and what is left at the end.  A difference
is a weight gradient that left in another launch or at another time (a speed matter) -- or one that was never issued."""
import json
import os

import pytest

from mrfp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_schedule.json")
SCENARIOS = ["stage_pattern", "group_maximum", "byte_cap", "changing_expectation", "alternating_kinds", "dead_pass"]


@pytest.fixture(scope="module")
def schedules():
    build.build()                            # (the group maximum is asked of the library)
    from mrfp_amd import conv, ops
    from tools import record_wgrad_schedule as rec
    def state():
        return ({k: id(v) for k, v in vars(conv._WGRADS).items()}, conv.call, conv.wgrad_workspace, conv.stream, ops.GRAD_NOTIFY[0])
    before = state()
    got = json.loads(json.dumps(rec.record()))
    assert state() == before                 # the recorder leaves the module as it found it
    return json.load(open(GOLDEN)), got


def test_the_fixture_holds_every_scenario(schedules):
    gold, got = schedules
    assert sorted(gold) == sorted(got) == sorted(SCENARIOS + ["group_max"])
    assert got["group_max"] == gold["group_max"] == 32
    stage = gold["stage_pattern"]
    assert stage["end"]["group_launches"] == [1, 6, 5, 5, 1] * 3                 # the boundary flush, then the learnt counts
    assert len(gold["alternating_kinds"]["end"]["kinds"]) == 64                    # 68 kinds were seen
    assert [w[1] for w in gold["dead_pass"]["warnings"]] == ["RuntimeWarning"] * 2
    assert all("queued weight gradients" in w[2] for w in gold["dead_pass"]["warnings"])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_schedule_equals_the_recorded_one(schedules, scenario):
    gold, got = schedules
    want, mine = gold[scenario], got[scenario]
    for what in ("events", "launches", "workspaces", "notified", "warnings", "end"):
        assert mine[what] == want[what], (scenario, what)
    assert len(mine["deferred"]) == len(want["deferred"])
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(mine["deferred"], want["deferred"])) if a != b]
    assert not bad, (scenario, bad[:5])
    # every weight that was submitted in a pass that finished was launched exactly once, and the workspace was sized for its launch
    launched = [w for launch in mine["launches"] for w in launch[4]]
    assert len(launched) == len(set(launched)) and sorted(launched) == sorted(mine["notified"])
    assert mine["workspaces"] == [launch[:3] for launch in mine["launches"]]
    assert mine["end"]["queued"] == 0 and not mine["end"]["callback_queued"] and mine["deferred"][-1] == []
