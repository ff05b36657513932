"""The handle's state machine and launch context, end to end: the fixed script of tests/_state_trace.py -- every transition of
runtime/state.h, on every form of the schedule a knob can force -- run on the library and on the oracle.  After every call the
fields equal the oracle's; the counters, istep and the launches per kernel of the profiled steps equal
tests/golden/state_trace.json, recorded (tests/golden/make_state_trace.py) from the commit before the state moved into
runtime/state.h.  Nothing in the fixture is a measurement: it is reproduced exactly."""
import json
import os

import pytest

import _state_trace as st
from util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "state_trace.json")) as f:
        return json.load(f)


def assert_same_trace(got, want, case):
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, row %d (%s): %r, recorded %r" % (case, n, w.get("op"), g, w)
    assert len(got) == len(want), (case, len(got), len(want))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(st.CASES))
def test_script_matches_the_oracle_and_the_recorded_trace(hip_api, oracle_api, golden, case):
    assert_same_trace(st.run_case(hip_api, oracle_api, case), golden[case], case)


@pytest.mark.gpu
def test_two_emulated_strips_match_the_single_domain_and_the_recorded_trace(hip_api, golden):
    assert_same_trace(st.run_strips(hip_api), golden["strips"], "strips")
