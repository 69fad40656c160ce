"""The frame run's routing (csrc/run_plan.h) on the device (run with -m gpu on an MI355X): for the 16 stage lists x
{whole run, band run after a whole run, re-render after a whole run, re-render before any run} and a handful of single
cases (a spline, noise, the strip flag, lazy chroma, an LF-only group, a Modular band) on a 40 x 600 frame, the timer
scopes with their launch counts and the SHA-256 of read_planes() equal what tools/record_run_launches.py recorded from
the commit before the routing moved into run_plan.h (tests/golden/run_plan_launches.json): the same work enqueued, the
same bytes."""
import json
import os

import pytest

from run_plan_cases import CASES, run_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "run_plan_launches.json")))


def test_the_recording_holds_exactly_the_cases(recorded):
    assert sorted(recorded) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_run_enqueues_and_leaves_what_was_recorded(ctx, recorded, case):
    got = run_case(ctx, case)
    want = recorded[case["name"]]
    assert got["launches"] == want["launches"], case["name"]
    assert got["sha256"] == want["sha256"], case["name"]
