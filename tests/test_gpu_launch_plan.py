"""GPU: the executor runs every op of the model programs in the launch, and the variant, it ran them in when tests/golden/launch_plan.json was
recorded (scripts/record_launch_plan.py, at the commit before the executor's host code was rewritten around named op fields), and computes the
same bits.  The cases -- tests/launch_plan_cases.py -- are the model programs at each fold threshold of the executor and just below it."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_plan_cases as C      # noqa: E402

_plan = None


def _recorded(cid):
    global _plan
    if _plan is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_plan.json')) as f:
            _plan = json.load(f)
    return _plan[cid]


def test_fixture_has_exactly_the_cases():
    _recorded(C.case_id(C.cases()[0]))
    assert sorted(_plan) == sorted(C.case_id(c) for c in C.cases())
    for cid, rec in _plan.items():
        if cid.startswith('mars'):
            assert 'output' in rec, cid       # no MARS case goes without its output digest


@pytest.mark.gpu
@pytest.mark.parametrize('case', C.cases(), ids=C.case_id)
def test_same_launches_same_variants_same_bits(case):
    want = _recorded(C.case_id(case))
    got = C.run(case)
    assert got['launches'] == want['launches']
    assert got['variants'] == want['variants']
    for key in ('output', 'decoded'):
        if key in want:
            assert got[key] == want[key], key
