"""CPU: the host association decision (dd_match_cascade, where = 0: the code Tracker.update runs under association='host') equals the
reference's matching_cascade + min_cost_matching under tracker.py:95-133's glue on every case of tests/golden/cascade_cases.npz
(scripts/make_golden_cascade.py), element for element and in the reference's order."""
import os
import pytest

import cascade_cases as cc

G = os.path.join(os.path.dirname(__file__), 'golden', 'cascade_cases.npz')


@pytest.fixture(scope='module')
def cases():
    return cc.load_cases(G)


def test_fixture_covers_what_it_claims(cases):
    shapes = {(c['T'], c['n']) for c in cases}
    assert {(63, 63), (64, 64), (65, 65), (64, 70), (70, 64), (256, 256)} <= shapes
    assert {c['kind'] for c in cases} == {0, 1, 2, 3}
    assert sum(1 for c in cases if c['T'] <= 15 and c['n'] <= 15) >= 60


def test_host_decision_equals_reference(cases):
    for c in cases:
        m, ur, ud = cc.match_cascade(c, 0)
        assert m == c['matches'], f"case {c['i']} ({c['T']} x {c['n']}, kind {c['kind']}): matches"
        assert ur == c['un_rows'], f"case {c['i']}: unmatched tracks"
        assert ud == c['un_dets'], f"case {c['i']}: unmatched detections"


def test_argument_checks_are_codes():
    from deepdish_amd._lib import lib
    l = lib()
    assert l.dd_match_cascade(None, 2, None, None, 0, 0, None, None, 0.2, 0.7, 3, None, None, None, None, None, None) < 0
    assert b'dd_match_cascade' in l.dd_last_error()
    assert l.dd_lsap_batch(None, None, None, None, None, 1, None, None) < 0
    assert b'dd_lsap_batch' in l.dd_last_error()
    assert l.dd_tracker_set_association(None, 1) < 0 and l.dd_pipeline_association(None, 1) < 0
