"""CPU: the restated per-stream skip schedule (tests/skip_streams_ref.py) against the reference's rule (tests/skip_frames_ref.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skip_frames_ref as ref  # noqa: E402
import skip_streams_ref as sref  # noqa: E402


def test_without_a_phase_the_schedule_is_the_references():
    for n in range(5):
        assert sref.schedule(n, None, 20) == ref.schedule(n, 20)
        assert sref.schedule(n, n, 20) == ref.schedule(n, 20)          # phase = N is no phase


def test_phases_stagger_four_streams_one_detector_run_per_step():
    N, F = 3, 20
    sched = [sref.schedule(N, ph, F) for ph in range(N + 1)]
    assert all(s[0] for s in sched)
    for f in range(1, F):
        assert sum(s[f] for s in sched) == 1, f
    for ph, s in enumerate(sched):                                         # after the first cycle every stream has the reference's period
        on = [f for f in range(F) if s[f]]
        assert on[1] == ph + 1 and all(b - a == N + 1 for a, b in zip(on[1:], on[2:]))


def test_stream_class_follows_the_schedule_without_touching_the_oracle_chain():
    """Stream.step's skipped flag over 12 frames equals schedule() -- with an encoder that is never asked for rows (no boxes)."""
    for n, ph in ((3, 0), (3, 2), (2, None), (0, 0)):
        st = sref.Stream(lambda frame, boxes: None, [[320, 0], [320, 480]], n=n, phase=ph, ratio=None)
        got = [not st.step(None, ([], [], []))[0] for _ in range(12)]
        assert got == sref.schedule(n, ph, 12), (n, ph)
