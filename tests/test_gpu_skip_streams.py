"""GPU: --object-detector-skip-frames with one counter per stream (MultiStreamPipeline(object_detector_skip_frames=[...],
object_detector_skip_phase=[...]), dd_pipeline_detector_skip_streams) and under presence masks.  The definition under test: every stream
is in the state of the reference run for that camera alone (tests/skip_streams_ref.py over the oracle chain, or a 1-stream pipeline)
stepped on its present frames only -- whatever the other streams' counters, encoder runs and absences do to the shared buffers."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import skip_frames_ref as ref  # noqa: E402
import skip_streams_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu

JUNK = 0xA5                              # what the frame slots of absent streams hold
ENC_BATCH = 128                          # one encoder_max_batch everywhere: the engine's max_batch fixes the K split of its convolutions
WRONG = ([(5, 5, 50, 80), (300, 200, 60, 120)], ['person', 'person'], [0.99, 0.98])      # injected rows that must not be read


def _inj(sc, f):
    boxes, scores, _, _ = sc.detections(f)
    return [tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]


def _compare(got_ints, got_means, tracker, what):
    """tests/test_gpu_skip_frames.py::_compare: the int columns equal, the Kalman means within 1e-6."""
    want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in tracker.tracks], dtype=np.int64).reshape(-1, 5)
    np.testing.assert_array_equal(np.asarray(got_ints)[:, :5].reshape(-1, 5), want, err_msg=what)
    if len(want):
        np.testing.assert_allclose(got_means, np.array([t.mean for t in tracker.tracks]), rtol=1e-6, atol=1e-6, err_msg=what)
    return len(want)


def _tables(mp):
    return [mp.tracker(z).table() for z in range(mp.S)]


def _assert_same_tables(a, b, msg=''):
    for z, ((ia, ma), (ib, mb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ia, ib, err_msg='%s stream %d' % (msg, z))
        np.testing.assert_array_equal(ma, mb, err_msg='%s stream %d' % (msg, z))


def _same_detections(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), what


# ------------------------------------------------------------------ 1. (and 6.) per-stream counters under masks against the oracle per camera
MAIN_N, MAIN_PERIOD, MAIN_F = [0, 1, 2, 3, 1], [1, 2, 3, 1, None], 30


def _main_run(ratio, association, oracle):
    """S = 5, N = 0, 1, 2, 3, 1, presence periods 1, 2, 3, 1, never, 30 steps; junk in absent frame slots, WRONG rows injected for absent
    streams and for streams on a skip step.  -> per step the tables, at the end counts and skip_stats."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 5, MAIN_F
    scenes = [Scene(seed=81 + z, n_obj=10 + 2 * z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=True, background_subtraction_ratio=ratio, object_detector_skip_frames=MAIN_N,
                             association=association)
    sts = None
    if oracle:
        enc = ref.mars_encoder(mp.enc_weights)
        sts = [sref.Stream(enc, sc.countline(), n=MAIN_N[z], ratio=ratio) for z, sc in enumerate(scenes)]
    k = [0] * S
    sched = [sref.schedule(MAIN_N[z], None, F) for z in range(S)]           # per stream over its OWN frames
    per_step, n_det, n_skip, tracked, more = [], 0, 0, 0, 0
    for step in range(F):
        present = [int(p is not None and step % p == 0) for p in MAIN_PERIOD]
        frames = np.full((S, mp.H, mp.W, 3), JUNK, np.uint8)
        per = [WRONG] * S
        for z in range(S):
            if present[z]:
                frames[z] = scenes[z].frame(k[z])
                if sched[z][k[z]]:
                    per[z] = _inj(scenes[z], k[z])
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        per_step.append(_tables(mp))
        stats = mp.skip_stats()
        masks = mp.motion_mask()[0] if (oracle and ratio is not None) else [None] * S
        for z in range(S):
            if not present[z]:
                continue
            n_det += sched[z][k[z]]
            n_skip += not sched[z][k[z]]
            assert bool(stats['skipped'][z]) == (not sched[z][k[z]]), (step, z)
            if oracle:
                rows_then = len(sts[z].prev_features) if sts[z].prev_features is not None else 0
                skipped, kept, _ = sts[z].step(frames[z], per[z], masks[z])
                assert skipped == (not sched[z][k[z]])
                more += skipped and len(kept) > rows_then
                np.testing.assert_array_equal(mp.detections(z)[0], np.asarray(sts[z].prev_objd[0], np.float64).reshape(-1, 4))
                ints, means = per_step[-1][z]
                tracked += _compare(ints, means, sts[z].tracker, 'step %d stream %d' % (step, z))
            k[z] += 1
        assert stats['detector_stream_steps'] == n_det and stats['skip_stream_steps'] == n_skip
        if oracle:
            assert stats['rows_retained'] == sum(len(st.prev_features) for st in sts if st.prev_features is not None), step
    counts, stats = mp.counts(), mp.skip_stats()
    assert mp.frames_seen().tolist() == k == [30, 15, 10, 30, 0]
    if oracle:
        for z in range(S):
            np.testing.assert_array_equal(counts[z], sts[z].counter.vector())
        assert tracked > 0 and len(mp.tracker(4).table()[0]) == 0 and mp.detections(4)[2].size == 0
        if ratio is not None:            # (14 such steps with these scenes)
            assert more > 0, 'no skip step kept more boxes than its stream had rows: the truncation went untested'
    assert stats['carry_launches'] > 0 and stats['store_bytes'] > 0 and mp.stage_ms()['steps'] == F
    return per_step, counts, stats


@pytest.mark.parametrize('ratio', [None, 0.25])
def test_per_stream_counters_under_masks_equal_the_oracle_per_camera(ratio):
    """Raises ValueError before this form existed (a mask with skip frames).  After every step every present stream's table, adaptor
    output and skipped flag are its oracle stream's, which was stepped on that stream's frames alone; with ratio = 0.25 the motion test of
    a skip step runs on the retained boxes against THIS frame's mask."""
    _, counts, _ = _main_run(ratio, 'host', oracle=True)
    assert counts.sum() > 0


def test_device_association_equals_host_on_the_same_run():
    a, b = _main_run(None, 'host', oracle=False), _main_run(None, 'device', oracle=False)
    for step, (ta, tb) in enumerate(zip(a[0], b[0])):
        _assert_same_tables(ta, tb, 'step %d' % step)
    np.testing.assert_array_equal(a[1], b[1])
    assert sum(len(t[0]) for t in a[0][-1]) > 0
    sa, sb = dict(a[2]), dict(b[2])
    assert sa.pop('skipped').tolist() == sb.pop('skipped').tolist() and sa == sb


# ------------------------------------------------------------------ 2. phase
def test_phases_stagger_the_detector_runs():
    """S = 4, N = 3, phases 0 .. 3, no mask, 12 steps: all four detect on step 0, exactly one on every later step -- so objd and feat
    grow on every step -- and every stream is its oracle stream with that phase."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F, N = 4, 12, 3
    scenes = [Scene(seed=91 + z, n_obj=9 + z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=True, object_detector_skip_frames=[N] * S, object_detector_skip_phase=list(range(S)))
    enc = ref.mars_encoder(mp.enc_weights)
    sts = [sref.Stream(enc, sc.countline(), n=N, phase=z, ratio=None) for z, sc in enumerate(scenes)]
    sched = [sref.schedule(N, z, F) for z in range(S)]
    prev, n_det = None, 0
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        per = [_inj(sc, f) if sched[z][f] else WRONG for z, sc in enumerate(scenes)]
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per))
        stats, stage = mp.skip_stats(), mp.stage_ms()
        totals = {k: stage[k] * stage['steps'] for k in ('objd', 'feat')}
        assert stats['detector_stream_steps'] - n_det == (S if f == 0 else 1), f
        assert stats['skipped'].tolist() == [not sched[z][f] for z in range(S)]
        n_det = stats['detector_stream_steps']
        if prev is not None:
            assert totals['objd'] > prev['objd'] and totals['feat'] > prev['feat'], f
        prev = totals
        for z in range(S):
            skipped, _, _ = sts[z].step(frames[z], per[z])
            assert skipped == (not sched[z][f])
            ints, means = mp.tracker(z).table()
            _compare(ints, means, sts[z].tracker, 'frame %d stream %d' % (f, z))
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], sts[z].counter.vector())
    assert mp.skip_stats()['skip_stream_steps'] == S * F - n_det and sum(len(t[0]) for t in _tables(mp)) > 0


# ------------------------------------------------------------------ 3. retention
def _grid(n):
    """n boxes of 36 x 70 that do not touch: NMS keeps every one."""
    return [(10 + 50 * (j % 12), 20 + 100 * (j // 12), 36, 70) for j in range(n)]


def test_rows_survive_absence_other_encoder_runs_and_reallocation():
    """Stream A (N = 1) has a detector step that keeps 3 of its 5 boxes (the motion test rejects the two whose pixels did not change),
    is then absent for 8 steps and returns on a skip step on which all 5 pass: its tracker input is the 3 retained rows, by zip.  In
    between B and C (N = 0) run the encoder on every step with more rows than A had and one more on every step, so the encoder's output
    buffer and the store are reallocated while A's rows wait.  (A MOG2 model calls its whole first frame foreground, so the detector
    step under test is A's third frame: two identical frames come first, one detector and one skip step.)"""
    from deepdish_amd.multipipe import MultiStreamPipeline
    S, A, ratio = 3, 0, 0.25
    mp = MultiStreamPipeline(S, run_detector=False, background_subtraction_ratio=ratio, object_detector_skip_frames=[1, 0, 0])
    st = sref.Stream(ref.mars_encoder(mp.enc_weights), [[320, 0], [320, 480]], n=1, ratio=ratio)
    rng = np.random.default_rng(5)
    bg = rng.integers(0, 256, (mp.H, mp.W, 3), dtype=np.uint8)
    boxes = _grid(5)

    def a_frame(moved):
        f = bg.copy()
        for j in moved:
            x, y, w, h = boxes[j]
            f[y:y + h, x:x + w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        return f
    a_dets = (boxes, ['person'] * 5, [0.9, 0.85, 0.8, 0.75, 0.7])
    a_steps = {0: a_frame([]), 1: a_frame([]), 2: a_frame([0, 1, 2]), 11: a_frame([0, 1, 2, 3, 4])}
    kept_at, bytes_seen, rows = {}, [], 0
    for step in range(12):
        present = [int(step in a_steps), 1, 1]
        frames = rng.integers(0, 256, (S, mp.H, mp.W, 3), dtype=np.uint8)          # B and C: every pixel moves on every step
        if present[A]:
            frames[A] = a_steps[step]
        nb = 6 + step
        per = [a_dets if present[A] else WRONG, (_grid(nb), ['person'] * nb, [0.9] * nb), (_grid(nb + 1), ['person'] * (nb + 1), [0.8] * (nb + 1))]
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        stats = mp.skip_stats()
        bytes_seen.append(stats['store_bytes'])
        if present[A]:
            skipped, kept, dets = st.step(frames[A], a_dets, mp.motion_mask()[0][A])
            assert skipped == bool(stats['skipped'][A]) == (step in (1, 11))
            kept_at[step] = (len(kept), len(dets))
            if not skipped:
                rows = len(kept)
            ints, means = mp.tracker(A).table()
            _compare(ints, means, st.tracker, 'step %d' % step)
            assert len(mp.overlay([A])[0]['det_tlbr']) == len(dets)
        assert stats['rows_retained'] == rows + 2 * nb + 1, step
    assert kept_at[2] == (3, 3) and kept_at[11] == (5, 3), kept_at            # the condition the frames were built for
    assert bytes_seen[-1] > bytes_seen[2] > 0, bytes_seen                      # the store grew while A's rows waited in it
    assert len(mp.tracker(A).table()[0]) > 0 and len(mp.tracker(1).table()[0]) > 0
    np.testing.assert_array_equal(mp.counts()[A], st.counter.vector())


# ------------------------------------------------------------------ 4. detector on, no injection
def _labels(yolo):
    from deepdish_amd.pipeline import DEFAULT_LABELS, DEFAULT_YOLO_LABELS
    return sorted({l.strip() for l in open(DEFAULT_YOLO_LABELS if yolo else DEFAULT_LABELS)} - {'???'})


DETECTORS = {
    'ssd-uint8': dict(model='synthetic-ssd_mobilenet_v1-uint8'),
    'yolov5': dict(model='synthetic-yolov5s-fp16.tflite'),
    'yolov5-letterbox': dict(model='synthetic-yolov5s-fp16.tflite', detector_letterbox=True),
    'tflite': dict(model='synthetic-efficientdet_lite0.tflite'),
}
DET_N, DET_PHASE, DET_PERIOD = [2, 1, 1], [1, 1, 0], [1, 2, 1]


def _det_frames(scenes, F, H, W):
    """Stream z present when step % DET_PERIOD[z] == 0, its k-th present step showing frame k of its scene -> per step (mask, frames)."""
    k, out = [0] * len(scenes), []
    for step in range(F):
        present = [int(step % p == 0) for p in DET_PERIOD]
        fr = np.full((len(scenes), H, W, 3), JUNK, np.uint8)
        for z, sc in enumerate(scenes):
            if present[z]:
                fr[z] = sc.frame(k[z])
                k[z] += 1
        out.append((present, torch.from_numpy(fr).cuda()))
    return out


@pytest.mark.parametrize('name', list(DETECTORS))
def test_detector_on_equals_single_stream_pipelines(name):
    """The tracker is fed by the detector's own output, which runs on the compacted frames of the streams on a detector step: against
    three 1-stream pipelines with that stream's N and phase, stepped on its present frames -- tables, detections and counts equal."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 10
    kw = dict(wanted_labels=_labels('yolov5' in name), encoder_max_batch=ENC_BATCH, **DETECTORS[name])
    scenes = [Scene(seed=3, n_obj=8, n_frames=F), Scene(seed=5, n_obj=5, n_frames=F), Scene(seed=9, n_obj=8, n_frames=F)]
    mp = MultiStreamPipeline(S, object_detector_skip_frames=DET_N, object_detector_skip_phase=DET_PHASE, **kw)
    one = [MultiStreamPipeline(1, object_detector_skip_frames=[DET_N[z]], object_detector_skip_phase=[DET_PHASE[z]], **kw) for z in range(S)]
    seen = 0
    for step, (present, frames) in enumerate(_det_frames(scenes, F, mp.H, mp.W)):
        mp.step(frames, present=present)
        sk = mp.skip_stats()['skipped']
        for z in range(S):
            if present[z]:
                one[z].step(frames[z:z + 1].contiguous())
            assert bool(sk[z]) == bool(one[z].skip_stats()['skipped'][0])
            _assert_same_tables([mp.tracker(z).table()], [one[z].tracker(0).table()], '%s step %d (stream %d)' % (name, step, z))
            _same_detections(mp.detections(z), one[z].detections(0), (name, step, z))
            seen = max(seen, len(mp.tracker(z).table()[0]))
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    stats = mp.skip_stats()
    assert stats['detector_stream_steps'] == sum(o.skip_stats()['detector_stream_steps'] for o in one)
    assert stats['skip_stream_steps'] == sum(o.skip_stats()['skip_stream_steps'] for o in one) > 0
    assert seen > 0 and mp.frames_seen().tolist() == [10, 5, 10]


# ------------------------------------------------------------------ 5. look-ahead
def _lookahead_run(ahead, wrong_at=None):
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 10
    scenes = [Scene(seed=120 + z, n_obj=10, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, wanted_labels=_labels(False), encoder_max_batch=ENC_BATCH, object_detector_skip_frames=DET_N,
                             object_detector_skip_phase=DET_PHASE)
    sched = _det_frames(scenes, F, mp.H, mp.W)
    steps = []
    for step, (present, frames) in enumerate(sched):
        if ahead and step + 1 < F:
            nxt = list(sched[step + 1][0])
            if step + 1 == wrong_at:
                nxt = [1 - v for v in nxt] if sum(nxt) < S else [1, 0, 0]
                assert nxt != sched[step + 1][0]
            mp.step(frames, None, sched[step + 1][1], present=present, present_next=nxt)
        else:
            mp.step(frames, present=present)
        steps.append(_tables(mp))
    return steps, mp.counts(), [mp.detections(z) for z in range(S)], mp.frames_seen().tolist(), mp.skip_stats()


@pytest.mark.parametrize('form', ['early', 'late', 'late-wrong'])
def test_lookahead_gives_the_same_results(form, monkeypatch):
    """frames_next / present_next queue the detector run of the NEXT step's detector streams, under both DD_DET_LATE forms; once the
    announced mask is not the one that arrives (the queued run is discarded).  Every step's tables equal the run without look-ahead."""
    base = _lookahead_run(False)
    monkeypatch.setenv('DD_DET_LATE', '0' if form == 'early' else '1')
    got = _lookahead_run(True, wrong_at=4 if form == 'late-wrong' else None)
    for step, (ta, tb) in enumerate(zip(base[0], got[0])):
        _assert_same_tables(ta, tb, 'step %d' % step)
    np.testing.assert_array_equal(base[1], got[1])
    for z, (da, db) in enumerate(zip(base[2], got[2])):
        _same_detections(da, db, z)
    assert base[3] == got[3] == [10, 5, 10] and sum(len(t[0]) for t in base[0][-1]) > 0
    for key in ('detector_stream_steps', 'skip_stream_steps', 'rows_retained'):
        assert base[4][key] == got[4][key]


# ------------------------------------------------------------------ 7. the lock-step form is untouched
def test_int_form_has_no_store_and_the_equal_sequence_form_gives_the_same_results():
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F, N = 3, 9, 2
    scenes = [Scene(seed=70 + z, n_obj=9 + 2 * z, n_frames=F) for z in range(S)]
    a = MultiStreamPipeline(S, run_detector=True, object_detector_skip_frames=N, encoder_max_batch=ENC_BATCH)
    b = MultiStreamPipeline(S, run_detector=True, object_detector_skip_frames=[N] * S, encoder_max_batch=ENC_BATCH)
    plain = MultiStreamPipeline(S, run_detector=False, encoder_max_batch=ENC_BATCH)
    for f in range(F):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        per = [_inj(sc, f) for sc in scenes]
        for mp in (a, b, plain):
            mp.step(frames, mp.pack_injected(per))
        _assert_same_tables(_tables(a), _tables(b), 'frame %d' % f)
        assert a.skip_stats()['skipped'].tolist() == b.skip_stats()['skipped'].tolist() == [f % (N + 1) != 0] * S
    np.testing.assert_array_equal(a.counts(), b.counts())
    sa, sb, sp = a.skip_stats(), b.skip_stats(), plain.skip_stats()
    assert sa['carry_launches'] == 0 and sa['store_bytes'] == 0 and sa['rows_retained'] == 0
    assert sp['carry_launches'] == 0 and sp['store_bytes'] == 0 and sp['skip_stream_steps'] == 0 and sp['detector_stream_steps'] == S * F
    assert sb['carry_launches'] > 0 and sb['store_bytes'] > 0
    assert sa['detector_stream_steps'] == sb['detector_stream_steps'] == 3 * S and sa['skip_stream_steps'] == sb['skip_stream_steps'] == 6 * S
    assert sum(len(t[0]) for t in _tables(a)) > 0


# ------------------------------------------------------------------ 8. refusals
def test_refusals():
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    S = 3
    for kw in (dict(object_detector_skip_frames=[1, 2]),                                        # a wrong length
               dict(object_detector_skip_frames=[1, 2, 1, 1]),
               dict(object_detector_skip_frames=[1, -1, 1]),                                    # a negative N
               dict(object_detector_skip_frames=[1, 2, 1], object_detector_skip_phase=[0, 3, 1]),      # a phase outside 0 .. N[z]
               dict(object_detector_skip_frames=[1, 2, 1], object_detector_skip_phase=[0, -1, 1]),
               dict(object_detector_skip_frames=[1, 2, 1], object_detector_skip_phase=[0, 1]),
               dict(object_detector_skip_frames=[1, 2, 1], object_detector_skip_phase=2),       # one phase for all: above N[0]
               dict(object_detector_skip_phase=[0, 1, 0]),                                      # a phase with no N
               dict(object_detector_skip_frames=2, object_detector_skip_phase=[0, 1, 0]),       # the int form has no phase
               dict(object_detector_skip_frames=2, object_detector_skip_phase=1)):
        with pytest.raises(ValueError, match='object_detector_skip'):
            MultiStreamPipeline(S, run_detector=False, **kw)
    # the C entries check for themselves
    mp = MultiStreamPipeline(S, run_detector=False)
    n, bad = np.array([1, 2, 1], np.int32), np.array([1, -2, 1], np.int32)
    assert lib().dd_pipeline_detector_skip_streams(mp._h, ptr(bad), None) == -1 and b'n[1] = -2' in lib().dd_last_error()
    assert lib().dd_pipeline_detector_skip_streams(mp._h, ptr(n), ptr(np.array([0, 3, 1], np.int32))) == -1 and b'phase[1] = 3' in lib().dd_last_error()
    assert lib().dd_pipeline_detector_skip_streams(mp._h, None, None) == -1
    assert mp.skip_stats()['store_bytes'] == 0
    # both entries on one pipeline, either order
    assert lib().dd_pipeline_detector_skip_streams(mp._h, ptr(n), None) == 0
    assert lib().dd_pipeline_detector_skip_frames(mp._h, 2) == -3 and b'dd_pipeline_detector_skip_streams' in lib().dd_last_error()      # DD_E_STATE
    lock = MultiStreamPipeline(S, run_detector=False, object_detector_skip_frames=2)
    assert lib().dd_pipeline_detector_skip_streams(lock._h, ptr(n), None) == -3 and b'dd_pipeline_detector_skip_frames' in lib().dd_last_error()
    # the new entry after the first step
    fr = torch.zeros((S, mp.H, mp.W, 3), dtype=torch.uint8, device='cuda')
    late = MultiStreamPipeline(S, run_detector=False)
    late.step(fr)
    assert lib().dd_pipeline_detector_skip_streams(late._h, ptr(n), None) == -3 and b'before the first step' in lib().dd_last_error()
    # the int form with a mask is still refused, by name, and the message names the way out; the sequence form takes the mask
    with pytest.raises(ValueError, match=r'object_detector_skip_frames=\[2\] \* 3'):
        lock.step(fr, present=[1, 1, 0])
    ones = np.ones(S, np.uint8)
    assert lib().dd_pipeline_step3(lock._h, ptr(fr), ptr(ones), None, None, None, None, None, None) == -3
    assert lock.stage_ms()['steps'] == 0
    mp.step(fr, present=[1, 1, 0])
    assert mp.frames_seen().tolist() == [1, 1, 0] and mp.skip_stats()['detector_stream_steps'] == 2
    # a scalar phase is one phase for every stream
    ok = MultiStreamPipeline(S, run_detector=False, object_detector_skip_frames=[1, 2, 1], object_detector_skip_phase=1)
    ok.step(fr)
    ok.step(fr)
    assert ok.skip_stats()['skipped'].tolist() == [True, True, True]


# ------------------------------------------------------------------ 9. a JPEG ring drives the mask
def test_ingest_ring_masks_a_pipeline_with_per_stream_counters():
    """tests/test_gpu_present_ingest.py's ring (stream 1: two files missing, one cut short) in front of a pipeline with N = 1, 2, 1:
    tracks and counts equal three 1-stream pipelines that never saw the dropped frames."""
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'scripts'))
    import make_jpeg_corpus
    from jpeg_dec_cases import pillow_file, reference
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    S, W, H, F, N = 3, 56, 40, 8, [1, 2, 1]
    _, damaged = make_jpeg_corpus.damaged_for_the_card()
    files = [[pillow_file(H, W, 'scene', 90, '4:2:0', 'row1' if z else 'none', seed=10 * f + z) for z in range(S)] for f in range(F)]
    missing, cut = (1, 4), 2
    kw = dict(input_size=(W, H), run_detector=False, encoder_max_batch=64)
    mp = MultiStreamPipeline(S, object_detector_skip_frames=N, **kw)
    one = [MultiStreamPipeline(1, object_detector_skip_frames=[N[z]], **kw) for z in range(S)]
    ring = FrameIngest(S, (W, H), slots=2, context=mp.ctx, pixel_format='jpeg', jpeg_slot_bytes=S * W * H * 3)
    for f in range(F):
        slot = f % 2
        per = [([(float(4 + 3 * f + z), float(2 + 12 * k), 10.0, 12.0) for k in range(3)], ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(S)]
        for z in range(S):
            if not (z == 1 and f in missing):
                ring.put(slot, z, damaged['cut'] if (z == 1 and f == cut) else files[f][z])
        ring.submit(slot)
        frames, present = ring.frames(slot), ring.present(slot)
        assert present.tolist() == [1, int(f not in missing and f != cut), 1]
        mp.step(frames, mp.pack_injected(per), present=present)
        ring.release(slot)
        for z in range(S):
            if present[z]:
                one[z].step(torch.from_numpy(reference(files[f][z])[None].copy()).cuda(), one[z].pack_injected([per[z]]))
    assert mp.frames_seen().tolist() == [F, F - 3, F]
    assert mp.skip_stats()['skip_stream_steps'] == sum(o.skip_stats()['skip_stream_steps'] for o in one) > 0
    for z in range(S):
        (ia, ma), (ib, mb) = mp.tracker(z).table(), one[z].tracker(0).table()
        assert len(ia) > 0
        np.testing.assert_array_equal(ia, ib, err_msg='stream %d' % z)
        np.testing.assert_array_equal(ma, mb, err_msg='stream %d' % z)
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
