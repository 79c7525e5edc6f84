"""GPU: snapshot / restore with everything on -- the uint8 SSD detector, per-stream skip counters [0, 1, 2] with phases, MOG2 with one ratio
per stream.  The snapshot is taken on a step where streams 1 and 2 are in the middle of their cycles, so the retained detector output and
the retained encoder rows (csrc/featrows.hip) are part of the state; restored into a NEW pipeline every later step equals the
uninterrupted run, and the background model and the motion-mask plane equal it right after the restore and three steps later.  With
background=False the restored streams' models are those of streams reset at that step.  Equality throughout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENC_BATCH = 128
S, F, CUT = 3, 12, 7                      # steps 0 .. 6 before the snapshot: step 6 is a skip step of streams 1 and 2
N, PHASE, RATIO = [0, 1, 2], [0, 0, 1], [0.0, 0.25, 0.9]


def _labels():
    from deepdish_amd.pipeline import DEFAULT_LABELS
    return sorted({l.strip() for l in open(DEFAULT_LABELS)} - {'???'})


def _build():
    from deepdish_amd.multipipe import MultiStreamPipeline
    return MultiStreamPipeline(S, model='synthetic-ssd_mobilenet_v1-uint8', wanted_labels=_labels(), encoder_max_batch=ENC_BATCH,
                               object_detector_skip_frames=N, object_detector_skip_phase=PHASE, background_subtraction_ratio=RATIO)


def _same_model(a, b, z, msg):
    for name, x, y in zip(('weight', 'variance', 'mean', 'nmodes'), a.mog2_state(z), b.mog2_state(z)):
        np.testing.assert_array_equal(x, y, err_msg='MOG2 %s, %s' % (name, msg))
    np.testing.assert_array_equal(a.motion_mask()[0][z], b.motion_mask()[0][z], err_msg='mask plane, ' + msg)


def _same_step(a, b, msg):
    for z in range(S):
        ta, tb = a.tracker(z).table(), b.tracker(z).table()
        np.testing.assert_array_equal(ta[0], tb[0], err_msg='table, %s stream %d' % (msg, z))
        np.testing.assert_array_equal(ta[1], tb[1], err_msg='means, %s stream %d' % (msg, z))
        for x, y in zip(a.detections(z), b.detections(z)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), 'detections, %s stream %d' % (msg, z)
    np.testing.assert_array_equal(a.counts(), b.counts(), err_msg=msg)
    np.testing.assert_array_equal(a.skip_stats()['skipped'], b.skip_stats()['skipped'], err_msg=msg)
    np.testing.assert_array_equal(a.frames_seen(), b.frames_seen(), err_msg=msg)


def test_detector_skip_counters_and_background_continue_after_a_restore():
    from deepdish_amd.synth import Scene
    scenes = [Scene(seed=3 + z, n_obj=8, n_frames=F) for z in range(S)]
    frames = [torch.from_numpy(np.stack([scenes[z].frame(f) for z in range(S)])).cuda() for f in range(F)]
    a = _build()
    for f in range(CUT):
        a.step(frames[f], None, frames[f + 1])
    sk = a.skip_stats()
    print('skipped at the cut', sk['skipped'].tolist(), 'rows retained', sk['rows_retained'], 'detections', [len(a.detections(z)[2]) for z in range(S)],
          'tracks', [len(a.tracker(z).table()[0]) for z in range(S)])
    # streams 1 and 2 are mid-cycle: their last step was a skip step, their next is one too or ends the cycle; retained rows exist
    assert sk['skipped'].tolist() == [False, True, True]
    assert sk['rows_retained'] > 0
    snap, lean = a.snapshot(), a.snapshot(background=False)
    assert all(i['has_background'] for i in snap.info) and not any(i['has_background'] for i in lean.info)
    assert all(i['bytes'] - j['bytes'] == 8 + 640 * 480 * 102 for i, j in zip(snap.info, lean.info))      # the planes and the frame count
    b = _build()
    b.restore(snap)
    _same_step(b, a, 'right after restore')
    assert b.skip_stats()['rows_retained'] == sk['rows_retained']
    for z in range(S):
        _same_model(b, a, z, 'right after restore, stream %d' % z)
    # background=False: the model of a stream reset at that step
    c, d = _build(), _build()
    for f in range(2):                                                   # some history the restore must clear
        c.step(frames[f])
        d.step(frames[f])
    c.restore(lean)
    d.reset([0, 1, 2])
    for z in range(S):
        _same_model(c, d, z, 'background=False against reset, stream %d' % z)
    np.testing.assert_array_equal(c.frames_seen(), a.frames_seen())
    for f in range(CUT, F):
        nxt = frames[f + 1] if f + 1 < F else None
        a.step(frames[f], None, nxt)
        b.step(frames[f], None, nxt)
        _same_step(b, a, 'step %d' % f)
        if f == CUT + 2:
            for z in range(S):
                _same_model(b, a, z, 'three steps after restore, stream %d' % z)
    sa, sb = a.skip_stats(), b.skip_stats()
    assert sb['rows_retained'] == sa['rows_retained']
    assert sb['skip_stream_steps'] > 0 and sb['detector_stream_steps'] + sb['skip_stream_steps'] == S * (F - CUT)
