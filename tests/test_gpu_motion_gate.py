"""GPU: the motion gate of the batched pipeline (MultiStreamPipeline(motion_gate=...), dd_pipeline_motion_gate) and of HotPath.  The
contract under test: with a threshold of 0 a gated pipeline is, after every step, bit for bit the ungated one -- track tables, galleries,
counts, frames seen, motion mask -- while the streams where nothing moved run neither detector nor encoder; which stream-steps those
are is what oracle/mog2_np.py's masks say, computed here on the CPU.  Every comparison is equality.  Frames are 64 x 48."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, S, F = 64, 48, 4, 14
ENC_BATCH = 64                           # one encoder_max_batch everywhere: the engine's max_batch fixes the K split of its convolutions
KW = dict(input_size=(W, H), run_detector=False, background_subtraction_ratio=0.25, encoder_max_batch=ENC_BATCH)
SQ_W, SQ_H = 12, 16
STILL_BOX = (8, 6, 20, 30)               # what a detector might keep reporting on a still picture: positive area, rejected by an empty mask


def _still(z):
    return np.random.default_rng(900 + z).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _square(z, f):
    xs = [2, 14, 26, 38, 50, 38, 26, 14]
    return xs[(f + z) % len(xs)], 4 + 3 * z + (f % 3) * 4


def _moving(z, f):
    fr = np.full((H, W, 3), 50 + 10 * z, np.uint8)
    x, y = _square(z, f)
    v = 110 + 20 * (f % 8)               # a colour of its own in every frame: where the square returns to, it is foreground again
    fr[y:y + SQ_H, x:x + SQ_W] = (v, v, 250) if f < 8 else (v, 250, v)
    return fr


def _frames(f):
    """Streams 0 and 2 show one unchanging picture; 1 and 3 a bright square that moves by its own width and changes colour every frame."""
    return np.stack([_still(0), _moving(1, f), _still(2), _moving(3, f)])


def _injected(f):
    """The boxes follow the squares; the still streams keep reporting one box.  All of positive area after the hygiene."""
    per = []
    for z in range(S):
        box = STILL_BOX if z in (0, 2) else _square(z, f) + (SQ_W, SQ_H)
        per.append(([box], ['person'], [0.9 - 0.01 * z]))
    return per


@functools.lru_cache(maxsize=None)
def _oracle_counts(n_frames=F):
    """int [n_frames][S]: np.count_nonzero of the oracle's mask of every stream after every frame."""
    from oracle.mog2_np import MOG2
    ora = [MOG2() for _ in range(S)]
    return tuple(tuple(int(np.count_nonzero(ora[z].apply(_frames(f)[z]))) for z in range(S)) for f in range(n_frames))


def _state(mp):
    """Everything the contract names, as comparable values."""
    out = []
    for z in range(mp.S):
        ints, means = mp.tracker(z).table()
        gal = [mp.tracker(z).gallery(int(t)) for t in ints[:, 0]]
        out.append((ints, means, gal))
    return out, mp.counts(), mp.frames_seen(), mp.motion_mask()[0]


def _assert_same_state(a, b, what):
    (ta, ca, sa, ma), (tb, cb, sb, mb) = a, b
    assert len(ta) == len(tb)
    for z, ((ia, mea, ga), (ib, meb, gb)) in enumerate(zip(ta, tb)):
        np.testing.assert_array_equal(ia, ib, err_msg='%s: track ints, stream %d' % (what, z))
        np.testing.assert_array_equal(mea, meb, err_msg='%s: track means, stream %d' % (what, z))
        assert len(ga) == len(gb)
        for (ra, na), (rb, nb) in zip(ga, gb):
            np.testing.assert_array_equal(ra, rb, err_msg='%s: gallery, stream %d' % (what, z))
            assert na == nb
    np.testing.assert_array_equal(ca, cb, err_msg='%s: counts' % what)
    np.testing.assert_array_equal(sa, sb, err_msg='%s: frames seen' % what)
    np.testing.assert_array_equal(ma, mb, err_msg='%s: motion mask' % what)


def _pipe(motion_gate=None, n=S, **kw):
    from deepdish_amd.multipipe import MultiStreamPipeline
    args = dict(KW)
    args.update(kw)
    return MultiStreamPipeline(n, motion_gate=motion_gate, **args)


@functools.lru_cache(maxsize=None)
def _ungated_states():
    """The ungated pipeline over the F frames, its state after every step: computed once, shared, never changed."""
    mp = _pipe()
    states = []
    for f in range(F):
        mp.step(torch.from_numpy(_frames(f)).cuda(), mp.pack_injected(_injected(f)))
        states.append(_state(mp))
    return states, mp.motion_mask(read=False)[1], mp.skip_stats()


def test_threshold_zero_is_the_ungated_pipeline_and_gates_what_the_oracle_says():
    """motion_gate=0 against motion_gate=None after every one of 14 steps; gate_stats() after every step is the oracle's counts and
    `count <= 0`; a gated step leaves an empty adaptor output although rows were injected for the stream."""
    want_states, want_rejected, want_skip = _ungated_states()
    counts = _oracle_counts()
    mp = _pipe(0)
    gated_total, tracked = 0, 0
    for f in range(F):
        mp.step(torch.from_numpy(_frames(f)).cuda(), mp.pack_injected(_injected(f)))
        _assert_same_state(_state(mp), want_states[f], 'step %d' % f)
        st = mp.gate_stats()
        want_gated = [c <= 0 for c in counts[f]]
        gated_total += sum(want_gated)
        assert st['count'].tolist() == list(counts[f]) and st['gated'].tolist() == want_gated, f
        assert st['steps'] == f + 1 and st['gated_stream_steps'] == gated_total
        for z in range(S):
            n_rows = len(mp.detections(z)[2])
            assert n_rows == (0 if want_gated[z] else 1), (f, z)
            assert not (z in (1, 3) and counts[f][z] > 0 and want_gated[z])
        tracked += sum(len(t[0]) for t in want_states[f][0])
    assert gated_total > 0 and tracked > 0
    assert all(counts[f][z] > 0 for f in range(F) for z in (1, 3)), 'the squares must move in every frame'
    assert all(counts[f][z] == 0 for f in range(1, F) for z in (0, 2)) and counts[0] == (H * W,) * S
    sk = mp.skip_stats()
    assert sk['detector_stream_steps'] == want_skip['detector_stream_steps'] - gated_total == S * F - gated_total
    assert sk['skip_stream_steps'] == 0 and not sk['skipped'].any()
    # the motion test does not count what was never made: one injected box per gated stream-step
    assert mp.motion_mask(read=False)[1] == want_rejected - gated_total


def test_frames_next_on_every_step_changes_nothing():
    want_states, _, _ = _ungated_states()
    mp = _pipe(0)
    dev = [torch.from_numpy(_frames(f)).cuda() for f in range(F)]
    for f in range(F):
        mp.step(dev[f], mp.pack_injected(_injected(f)), dev[f + 1] if f + 1 < F else None)
        _assert_same_state(_state(mp), want_states[f], 'step %d' % f)
    assert mp.gate_stats()['gated_stream_steps'] == sum(c <= 0 for row in _oracle_counts() for c in row) > 0


# ------------------------------------------------------------------ thresholds above 0
PATCH = [10, 200, 90, 250, 40, 160, 120, 220, 70, 180, 20, 140, 240, 100]      # far apart: the patch is foreground in every frame


def _patch_frame(f):
    fr = _still(1).copy()
    fr[20:22, 30:33] = PATCH[f]
    return fr


def _frames_t(f):
    """Stream 1 now shows a still picture in which a 2 x 3 patch changes every frame."""
    fr = _frames(f)
    fr[1] = _patch_frame(f)
    return fr


@functools.lru_cache(maxsize=None)
def _oracle_counts_t():
    from oracle.mog2_np import MOG2
    ora = [MOG2() for _ in range(S)]
    return tuple(tuple(int(np.count_nonzero(ora[z].apply(_frames_t(f)[z]))) for z in range(S)) for f in range(F))


def test_a_threshold_above_zero_gates_at_k_and_not_at_k_minus_one():
    """k = what the oracle's mask holds of the changing patch (not assumed).  One-stream pipelines with T = k and T = k - 1 on that
    stream; then the four streams with [0, k, 0, 10 ** 6]: the decisions the oracle's counts predict, every step."""
    counts = _oracle_counts_t()
    k = counts[F - 1][1]
    assert 0 < k < H * W and all(counts[f][1] == k for f in range(2, F)), counts
    at, below = _pipe(k, n=1), _pipe(k - 1, n=1)
    for f in range(F):
        for mp in (at, below):
            mp.step(torch.from_numpy(_frames_t(f)[1:2]).cuda(), mp.pack_injected([([(28, 16, 10, 10)], ['person'], [0.9])]))
        assert at.gate_stats()['count'].tolist() == below.gate_stats()['count'].tolist() == [counts[f][1]]
        assert at.gate_stats()['gated'].tolist() == [counts[f][1] <= k] and below.gate_stats()['gated'].tolist() == [counts[f][1] <= k - 1]
    assert at.gate_stats()['gated_stream_steps'] >= F - 2 and below.gate_stats()['gated_stream_steps'] == 0
    assert len(at.detections(0)[2]) == 0 and len(below.detections(0)[2]) == 1
    thr = [0, k, 0, 10 ** 6]
    mp = _pipe(thr)
    total = 0
    for f in range(F):
        mp.step(torch.from_numpy(_frames_t(f)).cuda(), mp.pack_injected(_injected(f)))
        st = mp.gate_stats()
        want = [counts[f][z] <= thr[z] for z in range(S)]
        total += sum(want)
        assert st['count'].tolist() == list(counts[f]) and st['gated'].tolist() == want and st['gated_stream_steps'] == total, f
    assert len(mp.tracker(3).table()[0]) == 0 and mp.frames_seen().tolist() == [F] * S      # stream 3 never reached its tracker with a box


# ------------------------------------------------------------------ the documented deviation
def test_a_zero_area_box_is_a_detection_ungated_and_none_gated():
    """A box the hygiene clips to w * h == 0 passes the reference's test on any mask (0 >= ratio * 0): ungated it reaches the tracker, on a
    gated step it does not exist.  Pins the stated difference."""
    box = ([(W + 6, 5, 10, 10)], ['person'], [0.9])          # x clips to W, so w clips to 0
    seen = {}
    for name, gate in (('ungated', None), ('gated', 0)):
        mp = _pipe(gate, n=1)
        per_step = []
        for f in range(2):               # (the first frame is all foreground; the box comes with the second, whose mask is empty)
            mp.step(torch.from_numpy(_still(0)[None]).cuda(), mp.pack_injected([box if f > 0 else ([], [], [])]))
            per_step.append(len(mp.overlay([0])[0]['det_tlbr']))
        seen[name] = (per_step, len(mp.tracker(0).table()[0]), len(mp.detections(0)[2]))
    assert seen['ungated'] == ([0, 1], 1, 1), seen
    assert seen['gated'] == ([0, 0], 0, 0), seen


# ------------------------------------------------------------------ presence masks, reset, masking
def test_an_absent_stream_is_neither_counted_nor_touched():
    from oracle.mog2_np import MOG2
    ora = [MOG2() for _ in range(S)]
    a, b = _pipe(0), _pipe()
    last, flag, total, k = [-1] * S, [False] * S, 0, [0] * S
    for step in range(12):
        present = [1, 1, 1, 1] if step == 0 else [int(step % (z + 1) == 0) for z in range(S)]
        frames = np.full((S, H, W, 3), 0xA5, np.uint8)
        for z in range(S):
            if present[z]:
                frames[z] = _frames(k[z])[z]
                last[z] = int(np.count_nonzero(ora[z].apply(frames[z])))
                flag[z] = last[z] <= 0
                total += flag[z]
                k[z] += 1
        per = [(_injected(max(k[z] - 1, 0))[z] if present[z] else ([(1, 1, 30, 30)], ['person'], [0.99])) for z in range(S)]
        for mp in (a, b):
            mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        _assert_same_state(_state(a), _state(b), 'step %d' % step)
        st = a.gate_stats()
        assert st['count'].tolist() == last and st['gated'].tolist() == flag and st['gated_stream_steps'] == total, step
    assert a.frames_seen().tolist() == k and total > 0
    a.step(torch.from_numpy(frames).cuda(), None, present=[0] * S)          # a step without a stream: the gate does not run
    assert a.gate_stats()['steps'] == 12 and a.gate_stats()['count'].tolist() == last


def test_reset_on_a_still_stream_matches_a_fresh_one_stream_pipeline():
    mp, one = _pipe(0), None
    for f in range(10):
        if f == 5:
            mp.reset([0])
            assert mp.gate_stats()['count'].tolist()[0] == -1 and not mp.gate_stats()['gated'][0]
            one = _pipe(0, n=1)
        per = _injected(f)
        mp.step(torch.from_numpy(_frames(f)).cuda(), mp.pack_injected(per))
        if one is not None:
            one.step(torch.from_numpy(_frames(f)[0:1]).cuda(), one.pack_injected(per[0:1]))
            (ta, ca, sa, ma), (tb, cb, sb, mb) = _state(mp), _state(one)
            _assert_same_state((ta[0:1], ca[0:1], sa[0:1], ma[0:1]), (tb, cb, sb, mb), 'step %d' % f)
            assert mp.gate_stats()['count'][0] == one.gate_stats()['count'][0] and mp.gate_stats()['gated'][0] == one.gate_stats()['gated'][0]
    assert mp.gate_stats()['count'][0] == 0 and mp.gate_stats()['gated'][0] and mp.frames_seen().tolist() == [5, 10, 10, 10]
    assert one.gate_stats()['gated_stream_steps'] == 4          # the first frame after the reset is all foreground again


def test_background_masking_with_the_gate_equals_the_ungated_masking_pipeline():
    a, b = _pipe(0, background_masking=True), _pipe(None, background_masking=True)
    for f in range(8):
        for mp in (a, b):
            mp.step(torch.from_numpy(_frames(f)).cuda(), mp.pack_injected(_injected(f)))
        _assert_same_state(_state(a), _state(b), 'step %d' % f)
    assert a.gate_stats()['gated_stream_steps'] == sum(c <= 0 for row in _oracle_counts()[:8] for c in row) > 0


# ------------------------------------------------------------------ with a detector running
def test_with_the_uint8_ssd_running_tables_and_counts_are_equal_and_the_detector_runs_less():
    """The synthetic uint8 SSD on the same four streams, look-ahead requested on every step.  No stream-step is left out of the
    comparison: the ungated run must hold no zero-area candidate on a step the other pipeline gates (the one stated difference)."""
    from deepdish_amd.pipeline import DEFAULT_LABELS
    labels = [l.strip() for l in open(DEFAULT_LABELS)][1:]
    kw = dict(run_detector=True, model='synthetic-ssd_mobilenet_v1-uint8', wanted_labels=labels)
    a, b = _pipe(0, **kw), _pipe(None, **kw)
    counts = _oracle_counts()
    dev = [torch.from_numpy(_frames(f)).cuda() for f in range(F)]
    gated_total, made = 0, 0
    for f in range(F):
        for mp in (a, b):
            mp.step(dev[f], None, dev[f + 1] if f + 1 < F else None)
        for z in range(S):
            boxes = b.detections(z)[0]
            made += len(boxes)
            if counts[f][z] <= 0:
                gated_total += 1
                assert len(a.detections(z)[2]) == 0
                for x, y, w, h in boxes:         # the hygiene's clipping (deepdish.py:951-952)
                    x, y = int(np.clip(x, 0, W)), int(np.clip(y, 0, H))
                    assert int(np.clip(w, 0, W - x)) * int(np.clip(h, 0, H - y)) > 0, 'a zero-area candidate on gated step %d stream %d' % (f, z)
            else:
                np.testing.assert_array_equal(a.detections(z)[0], boxes)
        _assert_same_state(_state(a), _state(b), 'step %d' % f)
        assert a.gate_stats()['count'].tolist() == list(counts[f])
    assert gated_total > 0 and made > 0
    assert a.skip_stats()['detector_stream_steps'] == b.skip_stats()['detector_stream_steps'] - gated_total
    assert a.gate_stats()['gated_stream_steps'] == gated_total


# ------------------------------------------------------------------ one stream, the Python path
@pytest.mark.parametrize('moving', [False, True])
def test_hotpath_gate_equals_hotpath(moving):
    from deepdish_amd.pipeline import HotPath
    from oracle.mog2_np import MOG2
    kw = dict(input_size=(W, H), run_detector=False, disable_background_subtraction=False)
    a, b = HotPath(motion_gate=0, **kw), HotPath(**kw)
    ora = MOG2()
    gated = 0
    key = lambda hp: [(t.track_id, t.state, t.time_since_update, t.hits, tuple(t.mean)) for t in hp.tracker.tracks]
    for f in range(10):
        frame = _moving(1, f) if moving else _still(0)
        box = _square(1, f) + (SQ_W, SQ_H) if moving else STILL_BOX
        want_gated = int(np.count_nonzero(ora.apply(frame))) <= 0
        gated += want_gated
        for hp in (a, b):
            hp.step(torch.from_numpy(frame).cuda(), injected=([box], ['person'], [0.9]))
        assert key(a) == key(b), f
        np.testing.assert_array_equal(a.counts(), b.counts())
        assert ('objd' in a.timings) == ('feat' in a.timings) == (not want_gated), f
        assert 'objd' in b.timings and 'feat' in b.timings and 'e2e' in a.timings
    assert a.gated_frames == gated == (0 if moving else 9)
