"""GPU: per-stream presence masks (MultiStreamPipeline.step(..., present=), dd_pipeline_step3).  The definition under test: every stream of
a masked pipeline is in exactly the state of a pipeline that was stepped only on the steps where that stream was present, with that
stream's frames of those steps.  Streams share nothing, so the yardstick is the reference run per camera: oracle/deepsort_np,
oracle/countline_np and oracle/mog2_np applied per stream on its present frames only, or a second pipeline stepped that way."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

JUNK = 0xA5                              # what the frame slots of absent streams hold
ENC_BATCH = 128                          # one encoder_max_batch everywhere: the engine's max_batch fixes the K split of its convolutions


def _want_table(trk):
    return np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in trk.tracks], dtype=np.int64).reshape(-1, 5)


def _tables(mp):
    return [mp.tracker(z).table() for z in range(mp.S)]


def _assert_same_tables(a, b, msg=''):
    for z, ((ia, ma), (ib, mb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ia, ib, err_msg='%s stream %d' % (msg, z))
        np.testing.assert_array_equal(ma, mb, err_msg='%s stream %d' % (msg, z))


def _dets(sc, f):
    boxes, scores, _, _ = sc.detections(f)
    return [tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]


WRONG = ([(5, 5, 50, 80), (300, 200, 60, 120)], ['person', 'person'], [0.99, 0.98])      # the injected rows of an absent stream


# ------------------------------------------------------------------ 1. masked steps equal independent streams
def test_masked_steps_equal_independent_oracle_streams():
    """S = 4 over 45 steps with injected detections: stream 0 present every step, stream 1 on even steps, stream 2 on every third,
    stream 3 never; a stream's k-th present step gets frame k of its scene.  After every step every stream's table is its oracle
    tracker's, which was advanced only when the stream was present.  (Oracle alone, on the CPU: seed 22 counts 2 crossings by frame 45,
    seed 23 one by frame 23, seed 24 holds 17 tracks after 15 frames.)"""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    S, F = 4, 45
    scenes = [Scene(seed=22, n_obj=13, n_frames=F), Scene(seed=23, n_obj=16, n_frames=F), Scene(seed=24, n_obj=19, n_frames=F), None]
    period = [1, 2, 3, None]
    mp = MultiStreamPipeline(S, run_detector=True)
    otrk = [ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for _ in range(S)]
    ocnt = [cl.CountLine(scenes[0].countline()) for _ in range(S)]
    k = [0] * S                                                      # every stream's own frame number
    for step in range(F):
        present = [int(p is not None and step % p == 0) for p in period]
        frames = np.full((S, mp.H, mp.W, 3), JUNK, np.uint8)
        per = []
        for z in range(S):
            if not present[z]:
                per.append(WRONG)
                continue
            sc, f = scenes[z], k[z]
            frames[z] = sc.frame(f)
            boxes, scores, _, _ = sc.detections(f)
            per.append(_dets(sc, f))
            keep = ds.non_max_suppression(boxes, 0.6, scores)
            patches = np.stack([image_np.extract_image_patch(frames[z], boxes[i], (64, 32)) for i in keep])
            feats = nets_torch.mars_forward(mp.enc_weights, patches)
            otrk[z].predict()
            otrk[z].update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
            ocnt[z].step(otrk[z])
            k[z] += 1
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        for z in range(S):
            ints, means = mp.tracker(z).table()
            want = _want_table(otrk[z])
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'step {step} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in otrk[z].tracks]), rtol=1e-6, atol=1e-6)
    got = mp.counts()
    for z in range(S):
        np.testing.assert_array_equal(got[z], ocnt[z].vector())
    assert mp.frames_seen().tolist() == [45, 23, 15, 0] == k
    assert len(mp.tracker(3).table()[0]) == 0 and mp.detections(3)[2].size == 0
    assert got[0].sum() > 0 and got[1].sum() > 0 and len(mp.tracker(2).table()[0]) > 0      # the condition the scenes were chosen for
    st = mp.present_stats()
    assert st['masked_steps'] == F and st['streams_stepped'] == 45 + 23 + 15 and st['gather_launches'] > 0
    assert mp.stage_ms()['steps'] == F
    ov = mp.overlay()
    assert len(ov[3]['track_ids']) == 0 and len(ov[3]['det_tlbr']) == 0


# ------------------------------------------------------------------ 2. mask patterns against pipelines stepped on the present frames only
PATTERNS = {
    'none': lambda step: [0, 0, 0, 0],
    'first': lambda step: [1, 0, 0, 0],
    'last': lambda step: [0, 0, 0, 1],
    'alternating': lambda step: [1, 0, 1, 0] if step % 2 == 0 else [0, 1, 0, 1],
    'ones': lambda step: [1, 1, 1, 1],
}


@functools.lru_cache(maxsize=None)
def _pattern_scenes():
    from deepdish_amd.synth import Scene
    return [Scene(seed=40 + z, n_obj=8 + z, n_frames=8) for z in range(4)]


@pytest.mark.parametrize('name', list(PATTERNS))
def test_mask_patterns_equal_a_second_pipeline_exactly(name):
    """The masked 4-stream pipeline (detector on, its output replaced by injected rows) against four 1-stream pipelines that are stepped
    only when their stream is present -- tables, means, counts and frames_seen equal exactly.  All ones must also equal present=None
    exactly and gather nothing."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    S, F = 4, 8
    scenes = _pattern_scenes()
    mp = MultiStreamPipeline(S, run_detector=True, encoder_max_batch=ENC_BATCH)
    one = [MultiStreamPipeline(1, run_detector=False, encoder_max_batch=ENC_BATCH) for _ in range(S)]
    plain = MultiStreamPipeline(S, run_detector=True, encoder_max_batch=ENC_BATCH) if name == 'ones' else None
    k = [0] * S
    for step in range(F):
        present = PATTERNS[name](step)
        frames = np.full((S, mp.H, mp.W, 3), JUNK, np.uint8)
        per = [WRONG] * S
        for z in range(S):
            if present[z]:
                frames[z] = scenes[z].frame(k[z])
                per[z] = _dets(scenes[z], k[z])
                one[z].step(torch.from_numpy(frames[z:z + 1]).cuda(), one[z].pack_injected([per[z]]))
                k[z] += 1
        fd = torch.from_numpy(frames).cuda()
        mp.step(fd, mp.pack_injected(per), present=np.array(present, dtype=bool) if step % 2 else present)
        if plain is not None:
            plain.step(fd, plain.pack_injected(per))
        for z in range(S):
            _assert_same_tables([mp.tracker(z).table()], [one[z].tracker(0).table()], 'step %d (stream %d)' % (step, z))
    assert mp.frames_seen().tolist() == k
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    st = mp.present_stats()
    assert st['masked_steps'] == F and st['streams_stepped'] == sum(k) and mp.stage_ms()['steps'] == F
    if name == 'none':
        assert sum(len(t[0]) for t in _tables(mp)) == 0 and st['gather_launches'] == 0
    else:
        assert sum(len(t[0]) for t in _tables(mp)) > 0
    if plain is not None:
        _assert_same_tables(_tables(mp), _tables(plain), 'all ones against present=None')
        np.testing.assert_array_equal(mp.counts(), plain.counts())
        assert st['gather_launches'] == 0 and plain.present_stats() == dict(masked_steps=0, gather_launches=0, streams_stepped=S * F)
    elif name != 'none':
        assert st['gather_launches'] == F


# ------------------------------------------------------------------ 3. detector on, no injection
def _labels(yolo):
    from deepdish_amd.pipeline import DEFAULT_LABELS, DEFAULT_YOLO_LABELS
    return sorted({l.strip() for l in open(DEFAULT_YOLO_LABELS if yolo else DEFAULT_LABELS)} - {'???'})


DETECTORS = {
    'ssd-uint8': dict(model='synthetic-ssd_mobilenet_v1-uint8'),
    'yolov5': dict(model='synthetic-yolov5s-fp16.tflite'),
    'yolov5-letterbox': dict(model='synthetic-yolov5s-fp16.tflite', detector_letterbox=True),
    'tflite': dict(model='synthetic-efficientdet_lite0.tflite'),
}


def _schedule(S, F):
    """Stream z is present when step % (z + 1) == 0; -> per step (mask, per stream its own frame number or None)."""
    k, out = [0] * S, []
    for step in range(F):
        present = [int(step % (z + 1) == 0) for z in range(S)]
        out.append((present, [k[z] if present[z] else None for z in range(S)]))
        for z in range(S):
            k[z] += present[z]
    return out


def _schedule_frames(scenes, sched, H, W):
    out = []
    for present, ks in sched:
        fr = np.full((len(scenes), H, W, 3), JUNK, np.uint8)
        for z, kz in enumerate(ks):
            if kz is not None:
                fr[z] = scenes[z].frame(kz)
        out.append(torch.from_numpy(fr).cuda())
    return out


@pytest.mark.parametrize('name', list(DETECTORS))
def test_detector_on_masked_equals_single_stream_pipelines(name):
    """No injection: the tracker is fed by the detector's own output, which under a mask runs on the compacted present frames (the
    generic adaptor: on a box table over the present streams).  MultiStreamPipeline(3) with periods 1, 2, 3 over 8 steps against three
    MultiStreamPipeline(1) stepped on the present frames only: tables, detections(z) and counts exactly equal."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 8
    kw = dict(wanted_labels=_labels('yolov5' in name), encoder_max_batch=ENC_BATCH, **DETECTORS[name])
    scenes = [Scene(seed=3, n_obj=8, n_frames=F), Scene(seed=5, n_obj=5, n_frames=F), Scene(seed=9, n_obj=8, n_frames=F)]
    mp = MultiStreamPipeline(S, **kw)
    one = [MultiStreamPipeline(1, **kw) for _ in range(S)]
    sched = _schedule(S, F)
    frames = _schedule_frames(scenes, sched, mp.H, mp.W)
    seen = 0
    for step, (present, ks) in enumerate(sched):
        mp.step(frames[step], present=present)
        for z in range(S):
            if present[z]:
                one[z].step(frames[step][z:z + 1].contiguous())
            if ks[z] is not None or step:
                _assert_same_tables([mp.tracker(z).table()], [one[z].tracker(0).table()], '%s step %d (stream %d)' % (name, step, z))
                for a, b in zip(mp.detections(z), one[z].detections(0)):
                    assert np.array_equal(np.asarray(a), np.asarray(b)), (name, step, z)
            seen = max(seen, len(mp.tracker(z).table()[0]))
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    partial = sum(1 for present, _ in sched if sum(present) < S)          # steps 0 and 6 have every stream: they gather nothing
    assert 0 < partial < F and seen > 0
    assert mp.present_stats()['gather_launches'] == (0 if name == 'tflite' else partial)      # the generic adaptor resizes through a box table
    assert mp.frames_seen().tolist() == [8, 4, 3]


# ------------------------------------------------------------------ 4. look-ahead
@pytest.mark.parametrize('wrong_at', [None, 3])
def test_lookahead_under_masks_gives_the_same_results(wrong_at):
    """The same masked schedule with frames_next / present_next and without: equal.  With wrong_at, the mask announced for that step is
    deliberately not the one that arrives: the queued run is discarded, the detector runs in the step, and the results are still equal."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 8
    scenes = [Scene(seed=120 + z, n_obj=10, n_frames=F) for z in range(S)]
    sched = _schedule(S, F)
    res = []
    for ahead in (False, True):
        mp = MultiStreamPipeline(S, wanted_labels=_labels(False), encoder_max_batch=ENC_BATCH)
        frames = _schedule_frames(scenes, sched, mp.H, mp.W)
        for step, (present, _) in enumerate(sched):
            if ahead and step + 1 < F:
                nxt = list(sched[step + 1][0])
                if step + 1 == wrong_at:
                    nxt = [1 - v for v in nxt] if sum(nxt) < S else [1, 0, 0]
                    assert nxt != sched[step + 1][0]
                mp.step(frames[step], None, frames[step + 1], present=present, present_next=nxt)
            else:
                mp.step(frames[step], present=present)
        res.append((_tables(mp), mp.counts(), [mp.detections(z) for z in range(S)], mp.frames_seen().tolist()))
    _assert_same_tables(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    for da, db in zip(res[0][2], res[1][2]):
        for a, b in zip(da, db):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    assert res[0][3] == res[1][3] == [8, 4, 3] and sum(len(t[0]) for t in res[0][0]) > 0


# ------------------------------------------------------------------ 5. background subtraction
def _mog2_frames(rng, z, h, w, t):
    yy, xx = np.mgrid[0:h, 0:w]
    bg = np.stack([(yy * 3 + xx * 2 + 40 * z) % 230, (yy + xx * 5) % 180 + 20, (yy * 7 + z * 9) % 250], -1)
    f = np.clip(bg + rng.integers(-6, 7, bg.shape), 0, 255).astype(np.uint8)
    if w > 9 and h > 4:
        x = (3 + 2 * t + 5 * z) % (w - 3)
        f[h // 4:h // 4 + 3, x:x + 3] = rng.integers(0, 256, f[h // 4:h // 4 + 3, x:x + 3].shape)
    elif t % 3 == 1:
        f[...] = rng.integers(0, 256, f.shape)
    return f


MOG2_MASKS = [[1, 1, 1], [1, 0, 1], [0, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 0], [1, 1, 1], None, [0, 0, 1], None, [1, 0, 1], [0, 1, 1]]


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (53, 71)])
@pytest.mark.parametrize('masked_out', [False, True])
def test_mog2_apply_device_present_equals_the_oracle_per_stream(shape, masked_out):
    """apply_device(..., present=): model (state(z) against live_state), mask plane and masked frame of the listed streams are the
    per-stream oracle's applied on the present frames only, bit for bit; those of an absent stream are what they were; the all-listed
    steps at equal counts (the first) and the unmasked steps after masked ones (None) are right too."""
    from deepdish_amd.background import createBackgroundSubtractorMOG2
    from oracle.mog2_np import MOG2, live_state
    S, (h, w) = 3, shape
    sub = createBackgroundSubtractorMOG2(n_streams=S)
    ora = [MOG2() for _ in range(S)]
    rng = np.random.default_rng(5)
    want_mask = np.full((S, h, w), 77, np.uint8)
    want_out = np.full((S, h, w, 3), 78, np.uint8)
    out_dev = torch.from_numpy(want_out.copy()).cuda() if masked_out else None
    seen = set()
    for t, m in enumerate(MOG2_MASKS):
        fr = np.stack([_mog2_frames(rng, z, h, w, t) for z in range(S)])
        for z in range(S):
            if m is None or m[z]:
                want_mask[z] = ora[z].apply(fr[z])
                want_out[z] = np.where(want_mask[z][..., None] != 0, fr[z], 0)
            else:
                fr[z] = JUNK
        got = sub.apply_device(torch.from_numpy(fr).cuda(), masked_out=out_dev, present=m)
        sub.ctx.sync()                                               # (the launch ran on the context's stream, .cpu() copies on torch's)
        np.testing.assert_array_equal(got.cpu().numpy(), want_mask, err_msg='mask planes, step %d' % t)
        if masked_out:
            np.testing.assert_array_equal(out_dev.cpu().numpy(), want_out, err_msg='masked frames, step %d' % t)
        for z in range(S):
            for name, a, b in zip(('weight', 'variance', 'mean', 'nmodes'), sub.state(z), live_state(ora[z])):
                np.testing.assert_array_equal(a, b, err_msg='%s, stream %d step %d' % (name, z, t))
        seen |= set(np.unique(want_mask).tolist())
    assert {0, 255} <= seen
    for bad in ([1, 1], [1, 2, 0], [[1, 0, 1]]):
        with pytest.raises(ValueError):
            sub.apply_device(torch.from_numpy(fr).cuda(), present=bad)


@pytest.mark.parametrize('masking', [False, True])
def test_pipeline_background_subtraction_under_masks(masking):
    """S = 3 with background_subtraction_ratio = 0.25: the motion-mask planes equal the per-stream oracle applied on the present frames
    only (an absent stream's plane is that of its last present step), an unmasked step after masked ones is still right, and tables and
    counts equal three 1-stream pipelines with the same setting stepped on the present frames only."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle.mog2_np import MOG2
    S, F, W, H = 3, 12, 320, 240
    scenes = [Scene(seed=200 + z, n_obj=7, n_frames=F, width=W, height=H, wrange=(14, 30), hrange=(30, 60), vmax=2.5) for z in range(S)]
    phantom = [(6, 8, 30, 44), (250, 150, 40, 60)]
    kw = dict(input_size=(W, H), run_detector=False, background_subtraction_ratio=0.25, background_masking=masking, encoder_max_batch=ENC_BATCH)
    mp = MultiStreamPipeline(S, **kw)
    one = [MultiStreamPipeline(1, **kw) for _ in range(S)]
    ora = [MOG2() for _ in range(S)]
    want = np.zeros((S, H, W), np.uint8)
    k = [0] * S
    for step in range(F):
        present = None if step in (7, 10) else [int(step % (z + 1) == 0) for z in range(S)]
        frames = np.full((S, H, W, 3), JUNK, np.uint8)
        per = [WRONG] * S
        for z in range(S):
            if present is None or present[z]:
                frames[z] = scenes[z].frame(k[z])
                b, l, s = _dets(scenes[z], k[z])
                per[z] = (b + phantom, l + ['person'] * 2, s + [0.55, 0.54])
                want[z] = ora[z].apply(frames[z])
                one[z].step(torch.from_numpy(frames[z:z + 1]).cuda(), one[z].pack_injected([per[z]]))
                k[z] += 1
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        got, _ = mp.motion_mask()
        for z in range(S):
            if k[z]:
                np.testing.assert_array_equal(got[z], want[z], err_msg='mask plane, stream %d step %d' % (z, step))
            _assert_same_tables([mp.tracker(z).table()], [one[z].tracker(0).table()], 'step %d (stream %d)' % (step, z))
    assert mp.motion_mask(read=False)[1] == sum(o.motion_mask(read=False)[1] for o in one) > 0
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    assert mp.frames_seen().tolist() == k and sum(len(t[0]) for t in _tables(mp)) > 0


# ------------------------------------------------------------------ 6. device association
def test_device_association_masked_equals_host_masked():
    from deepdish_amd.multipipe import MultiStreamPipeline
    S, F = 4, 8
    scenes = _pattern_scenes()
    res = {}
    for where in ('host', 'device'):
        mp = MultiStreamPipeline(S, run_detector=False, association=where, encoder_max_batch=ENC_BATCH)
        k = [0] * S
        for step in range(F):
            present = [int(step % (z + 1) == 0) for z in range(S)]
            frames = np.full((S, mp.H, mp.W, 3), JUNK, np.uint8)
            per = [WRONG] * S
            for z in range(S):
                if present[z]:
                    frames[z], per[z] = scenes[z].frame(k[z]), _dets(scenes[z], k[z])
                    k[z] += 1
            mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per), present=present)
        res[where] = (_tables(mp), mp.counts(), mp.association_stats())
    _assert_same_tables(res['host'][0], res['device'][0])
    np.testing.assert_array_equal(res['host'][1], res['device'][1])
    assert sum(len(t[0]) for t in res['host'][0]) > 0
    dev, host = res['device'][2], res['host'][2]
    assert dev['device_updates'] == F and dev['host_updates'] == 0 and dev['fallback_streams'] == 0, dev
    assert host['device_updates'] == 0 and host['host_updates'] == F, host


# ------------------------------------------------------------------ 7. refusals
def test_refusals_and_the_null_mask():
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    S = 3
    mp = MultiStreamPipeline(S, run_detector=False)
    fr = torch.zeros((S, mp.H, mp.W, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    for bad in ([1, 0], [1, 0, 1, 1], [[1, 0, 1]], [1, 2, 0], [0.5, 1, 0], np.array([1, 0, 255], np.uint8), [-1, 0, 1]):
        with pytest.raises(ValueError):
            mp.step(fr, present=bad)
        with pytest.raises(ValueError):
            mp.step(fr, None, fr.clone(), present_next=bad)
    with pytest.raises(ValueError, match='frames_next'):
        mp.step(fr, present_next=[1, 1, 1])
    assert mp.stage_ms()['steps'] == 0 and mp.frames_seen().tolist() == [0] * S          # nothing was stepped by the refused calls
    # the C entry point checks for itself
    two = np.array([1, 2, 0], np.uint8)
    assert lib().dd_pipeline_step3(mp._h, ptr(fr), ptr(two), None, None, None, None, None, None) == -1
    assert b'present[1] = 2' in lib().dd_last_error()
    assert lib().dd_pipeline_step3(mp._h, ptr(fr), None, None, ptr(two), None, None, None, None) == -1
    assert b'present_next without frames_next' in lib().dd_last_error()
    # object_detector_skip_frames and a mask: refused by name
    sk = MultiStreamPipeline(S, run_detector=False, object_detector_skip_frames=2)
    with pytest.raises(ValueError, match='object_detector_skip_frames'):
        sk.step(fr, present=[1, 1, 1])
    ones = np.ones(S, np.uint8)
    rc = lib().dd_pipeline_step3(sk._h, ptr(fr), ptr(ones), None, None, None, None, None, None)
    assert rc == -3 and b'object_detector_skip_frames' in lib().dd_last_error()             # DD_E_STATE
    sk.step(fr)                                                       # without a mask it steps as before
    assert sk.stage_ms()['steps'] == 1
    # a NULL mask through dd_pipeline_step3 behaves as dd_pipeline_step2
    from deepdish_amd.synth import Scene
    sc = Scene(seed=3, n_obj=6, n_frames=4)
    a, b = (MultiStreamPipeline(1, run_detector=False) for _ in range(2))
    for f in range(4):
        frame = torch.from_numpy(sc.frame(f)[None]).cuda()
        bx, sco, cl, off = a.pack_injected([_dets(sc, f)])
        assert lib().dd_pipeline_step2(a._h, ptr(frame), None, ptr(bx), ptr(sco), ptr(cl), ptr(off)) == 0
        assert lib().dd_pipeline_step3(b._h, ptr(frame), None, None, None, ptr(bx), ptr(sco), ptr(cl), ptr(off)) == 0
    _assert_same_tables(_tables(a), _tables(b))
    assert len(a.tracker(0).table()[0]) > 0 and a.present_stats() == b.present_stats()
    assert b.present_stats() == dict(masked_steps=0, gather_launches=0, streams_stepped=4)
