"""GPU: per-stream count lines, labels and tracker settings, and reset(streams), of MultiStreamPipeline.  The definition under test is the
README's: a stream of the pipeline is in exactly the state of the reference run for that camera, and the reference is one process per
camera with its own flags.  Streams share nothing, so the yardstick is the one tests/test_gpu_present.py uses: S separate one-stream
pipelines built with SCALAR parameters (the unchanged code path), bit-equal; for the injected runs also the per-stream oracle
(oracle/deepsort_np, oracle/countline_np.CountLine(line, wanted_labels)): ints equal, means to 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENC_BATCH = 128                          # one encoder_max_batch everywhere: the engine's max_batch fixes the K split of its convolutions
S = 4


def _tables(mp):
    return [mp.tracker(z).table() for z in range(mp.S)]


def _assert_same_table(a, b, msg=''):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)


def _dets(sc, f, label='person'):
    boxes, scores, _, _ = sc.detections(f)
    return [tuple(int(v) for v in b) for b in boxes], [label] * len(boxes), [float(s) for s in scores]


def _want_table(trk):
    return np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in trk.tracks], dtype=np.int64).reshape(-1, 5)


def _labels(yolo=False):
    from deepdish_amd.pipeline import DEFAULT_LABELS, DEFAULT_YOLO_LABELS
    return sorted({l.strip() for l in open(DEFAULT_YOLO_LABELS if yolo else DEFAULT_LABELS)} - {'???'})


# ------------------------------------------------------------------ 1. lines
def test_every_stream_counts_across_its_own_line():
    """Four streams see the same 45 frames and injected detections (a scene whose oracle counts crossings of the default line) and differ
    in their count line only: the default vertical, a horizontal at H / 2, a diagonal, a segment outside the frame.  After every step
    tables, counts and overlay line / crossings equal stream z's one-stream pipeline, tables and counts also the oracle tracker and
    the CountLine oracle of that line."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    F = 45
    sc = Scene(seed=22, n_obj=13, n_frames=F)
    W, H = 640, 480
    lines = np.array([[W / 2, 0, W / 2, H], [0, H / 2, W, H / 2], [0, 0, W, H], [-100, -100, -50, -10]], dtype=np.float64)
    mp = MultiStreamPipeline(S, run_detector=False, line=lines.reshape(S, 2, 2), encoder_max_batch=ENC_BATCH)
    one = [MultiStreamPipeline(1, run_detector=False, line=lines[z], encoder_max_batch=ENC_BATCH) for z in range(S)]
    otrk = ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60)       # the four oracle runs have the same tracker: advanced once
    ocnt = [cl.CountLine(lines[z]) for z in range(S)]
    crossings = [0] * S
    for f in range(F):
        frame = sc.frame(f)
        boxes, scores, _, _ = sc.detections(f)
        keep = ds.non_max_suppression(boxes, 0.6, scores)
        patches = np.stack([image_np.extract_image_patch(frame, boxes[i], (64, 32)) for i in keep])
        feats = nets_torch.mars_forward(mp.enc_weights, patches)
        otrk.predict()
        otrk.update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
        fd = torch.from_numpy(np.stack([frame] * S)).cuda()
        per = _dets(sc, f)
        mp.step(fd, mp.pack_injected([per] * S))
        got, ov = mp.counts(), mp.overlay()
        want = _want_table(otrk)
        for z in range(S):
            one[z].step(fd[z:z + 1].contiguous(), one[z].pack_injected([per]))
            ocnt[z].step(otrk)
            tab = mp.tracker(z).table()
            _assert_same_table(tab, one[z].tracker(0).table(), 'step %d stream %d' % (f, z))
            np.testing.assert_array_equal(tab[0][:, :5], want, err_msg='step %d stream %d' % (f, z))
            if len(want):
                np.testing.assert_allclose(tab[1], np.array([t.mean for t in otrk.tracks]), rtol=1e-6, atol=1e-6)
            np.testing.assert_array_equal(got[z], one[z].counts()[0], err_msg='step %d stream %d' % (f, z))
            np.testing.assert_array_equal(got[z], ocnt[z].vector(), err_msg='step %d stream %d' % (f, z))
            o1 = one[z].overlay()[0]
            np.testing.assert_array_equal(ov[z]['line'], lines[z])
            np.testing.assert_array_equal(ov[z]['line'], o1['line'])
            np.testing.assert_array_equal(ov[z]['crossings'], o1['crossings'], err_msg='step %d stream %d' % (f, z))
            np.testing.assert_array_equal(ov[z]['counts'], o1['counts'])
            crossings[z] += len(ov[z]['crossings'])
    got = mp.counts()
    print('counts per stream:', got[:, 0].tolist(), 'crossing segments drawn:', crossings)
    # the test's own teeth
    assert got[0].sum() > 0 and crossings[0] > 0, 'the default line must count'
    assert got[3].sum() == 0 and crossings[3] == 0, 'a line outside the frame counts nothing'
    assert len({tuple(got[z].ravel().tolist()) for z in range(S)}) >= 2
    assert not np.array_equal(got[0], got[1]) or not np.array_equal(got[0], got[2])
    assert mp.stream_param_stats() == dict(nms_stream_launches=0, association_stream_launches=0, resets=0, streams_reset=0)
    np.testing.assert_array_equal(mp.overlay([2])[0]['line'], lines[2])


# ------------------------------------------------------------------ 2. tracker settings
AGE, N_INIT = [60, 5, 60, 30], [3, 3, 1, 3]
COS, IOU = [0.2, 0.3, 0.2, 0.3], [0.7, 0.7, 0.5, 0.5]


def _settings_scene(F):
    from deepdish_amd.synth import Scene
    return Scene(seed=3, n_obj=20, n_frames=F, p_miss=0.1)             # the scene behind tests/golden/scene_n20_age5.npz


@pytest.mark.parametrize('where', ['host', 'device'])
def test_every_stream_tracks_with_its_own_settings(where):
    """max_age, n_init, max_cosine_distance and max_iou_distance per stream over the scene whose golden shows max_age = 5 changing the
    ids: every stream equals the one-stream pipeline built with its scalars, ids included, decided on the host and on the device."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    F = 45
    sc = _settings_scene(F)
    kw = dict(run_detector=False, association=where, encoder_max_batch=ENC_BATCH)
    mp = MultiStreamPipeline(S, max_age=AGE, n_init=N_INIT, max_cosine_distance=COS, max_iou_distance=IOU, **kw)
    one = [MultiStreamPipeline(1, max_age=AGE[z], n_init=N_INIT[z], max_cosine_distance=COS[z], max_iou_distance=IOU[z], **kw) for z in range(S)]
    differ = set()
    for f in range(F):
        fd = torch.from_numpy(np.stack([sc.frame(f)] * S)).cuda()
        per = _dets(sc, f)
        mp.step(fd, mp.pack_injected([per] * S))
        tabs = _tables(mp)
        for z in range(S):
            one[z].step(fd[z:z + 1].contiguous(), one[z].pack_injected([per]))
            _assert_same_table(tabs[z], one[z].tracker(0).table(), '%s step %d stream %d' % (where, f, z))
            if not np.array_equal(tabs[z][0], tabs[0][0]):
                differ.add(z)
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
        assert mp.tracker(z).next_id == one[z].tracker(0).next_id
    print('streams whose table left stream 0\'s:', sorted(differ), 'next ids:', [mp.tracker(z).next_id for z in range(S)])
    assert {1, 2} <= differ, 'max_age = 5 and n_init = 1 must change the tables'
    a, sp = mp.association_stats(), mp.stream_param_stats()
    if where == 'device':
        assert a['device_updates'] == F and a['fallback_streams'] == 0, a
        assert sp['association_stream_launches'] > 0, sp
        assert all(o.stream_param_stats()['association_stream_launches'] == 0 for o in one)
    else:
        assert a['host_updates'] == F and sp['association_stream_launches'] == 0


def test_equal_sequences_are_the_scalar_pipeline():
    """Sequences whose entries are all equal select no variant: the same launches as the pipeline built from scalars, the same results."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    F = 12
    sc = _settings_scene(F)
    kw = dict(run_detector=False, association='device', encoder_max_batch=ENC_BATCH)
    seq = MultiStreamPipeline(S, max_age=[60] * S, n_init=[3] * S, max_cosine_distance=[0.2] * S, max_iou_distance=[0.7] * S,
                              nms_max_overlap=[0.6] * S, line=np.tile([320., 0., 320., 480.], (S, 1)), wanted_labels=[['person']] * S, **kw)
    sca = MultiStreamPipeline(S, **kw)
    for f in range(F):
        fd = torch.from_numpy(np.stack([sc.frame(f)] * S)).cuda()
        per = _dets(sc, f)
        seq.step(fd, seq.pack_injected([per] * S))
        sca.step(fd, sca.pack_injected([per] * S))
        for z in range(S):
            _assert_same_table(seq.tracker(z).table(), sca.tracker(z).table(), 'step %d stream %d' % (f, z))
    np.testing.assert_array_equal(seq.counts(), sca.counts())
    zero = dict(nms_stream_launches=0, association_stream_launches=0, resets=0, streams_reset=0)
    assert seq.stream_param_stats() == zero == sca.stream_param_stats()
    assert seq.association_stats() == sca.association_stats() and seq.association_stats()['device_updates'] == F
    assert seq.wanted == ['person'] and seq.wanted_of(3) == ['person'] and sum(len(t[0]) for t in _tables(seq)) > 0


# ------------------------------------------------------------------ 3. NMS
def _overlapping(sc, f):
    """The scene's boxes, each followed by a copy shifted by a quarter of its width with a lower score: pairs that overlap by ~3/4."""
    b, l, s = _dets(sc, f)
    boxes, scores = [], []
    for (x, y, w, h), v in zip(b, s):
        boxes += [(x, y, w, h), (max(0, x - w // 4), y, w, h)]
        scores += [v, v - 0.2]
    return boxes, ['person'] * len(boxes), scores


def _grid65():
    """65 candidates, the smallest count that leaves the batched one-wave kernel: a 13 x 5 grid of 30 x 50 boxes in which every second
    box of a row is pushed 35 pixels onto its left neighbour (two thirds of its area: suppressed at 0.6)."""
    boxes = []
    for j in range(5):
        for i in range(13):
            boxes.append((10 + 45 * i - (35 if i % 2 else 0), 10 + 90 * j, 30, 50))
    scores = [0.99 - 0.005 * k for k in range(65)]
    return boxes, ['person'] * 65, scores


def test_every_stream_suppresses_at_its_own_overlap():
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    NMS = [1.0, 0.3, 0.6, 0.6]
    F = 6
    scenes = [Scene(seed=40 + z, n_obj=8 + z, n_frames=F + 1) for z in range(S)]
    kw = dict(run_detector=False, encoder_max_batch=ENC_BATCH)
    mp = MultiStreamPipeline(S, nms_max_overlap=NMS, **kw)
    one = [MultiStreamPipeline(1, nms_max_overlap=NMS[z], **kw) for z in range(S)]
    kept = np.zeros(S, np.int64)

    def step(f, per):
        fd = torch.from_numpy(np.stack([scenes[z].frame(f) for z in range(S)])).cuda()
        mp.step(fd, mp.pack_injected(per))
        ov = mp.overlay()
        for z in range(S):
            one[z].step(fd[z:z + 1].contiguous(), one[z].pack_injected([per[z]]))
            np.testing.assert_array_equal(ov[z]['det_tlbr'], one[z].overlay()[0]['det_tlbr'], err_msg='kept rows, step %d stream %d' % (f, z))
            _assert_same_table(mp.tracker(z).table(), one[z].tracker(0).table(), 'step %d stream %d' % (f, z))
        return [len(o['det_tlbr']) for o in ov]
    # the same candidates for streams 0 and 1, so that only their thresholds tell them apart
    for f in range(F):
        per = [_overlapping(scenes[0], f), _overlapping(scenes[0], f), _overlapping(scenes[2], f), _overlapping(scenes[3], f)]
        kept += step(f, per)
    print('rows kept per stream over %d steps:' % F, kept.tolist())
    assert kept[0] > kept[1] > 0, 'overlap 1.0 keeps every candidate, 0.3 drops the shifted copies'
    assert mp.stream_param_stats()['nms_stream_launches'] == F
    assert all(o.stream_param_stats()['nms_stream_launches'] == 0 for o in one)
    # one more step: stream 2 has 65 candidates, so the step leaves the batched kernel for one call per stream, each with its own value
    per = [_overlapping(scenes[0], F), _overlapping(scenes[0], F), _grid65(), _overlapping(scenes[3], F)]
    last = step(F, per)
    print('rows kept in the 65-candidate step:', last)
    assert last[0] > last[1] > 0 and 0 < last[2] < 65
    assert mp.stream_param_stats()['nms_stream_launches'] == F


# ------------------------------------------------------------------ 4. labels
def test_every_stream_wants_its_own_labels():
    """Detector on (the synthetic uint8 SSD), wanted_labels = [[a], [b], [a, b], []] with a, b the two labels the detector reports most
    often on these frames: tables, detections and counts, through the union layout, equal one-stream pipelines with wanted_labels =
    list_z; un-wanted rows of counts() stay zero; the stream that wants nothing tracks nothing; render draws the stream's own counters."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import default_context
    from deepdish_amd.synth import Scene
    F = 8
    sc = Scene(seed=3, n_obj=8, n_frames=F)
    kw = dict(model='synthetic-ssd_mobilenet_v1-uint8', encoder_max_batch=ENC_BATCH)
    frames = [torch.from_numpy(np.stack([sc.frame(f)] * S)).cuda() for f in range(F)]
    probe = MultiStreamPipeline(1, wanted_labels=_labels(), **kw)
    seen = {}
    for f in range(F):
        probe.step(frames[f][:1].contiguous())
        for l in probe.detections(0)[1]:
            seen[l] = seen.get(l, 0) + 1
    ranked = sorted(seen, key=lambda l: (-seen[l], l))
    assert len(ranked) >= 2, 'the synthetic detector reports fewer than two labels on these frames: %r' % (seen,)
    a, b = ranked[:2]
    lists = [[a], [b], [a, b], []]
    mp = MultiStreamPipeline(S, wanted_labels=lists, **kw)
    one = [MultiStreamPipeline(1, wanted_labels=lists[z], **kw) for z in range(S)]
    assert mp.wanted == [a, b] and [mp.wanted_of(z) for z in range(S)] == lists and mp.counts().shape == (S, 2, 4)
    ctx = default_context()
    n_det = [0] * S
    for f in range(F):
        mp.step(frames[f])
        got = mp.counts()
        for z in range(S):
            one[z].step(frames[f][z:z + 1].contiguous())
            _assert_same_table(mp.tracker(z).table(), one[z].tracker(0).table(), 'step %d stream %d' % (f, z))
            da, db = mp.detections(z), one[z].detections(0)
            for x, y in zip(da, db):
                assert np.array_equal(np.asarray(x), np.asarray(y)), (f, z)
            assert set(da[1]) <= set(lists[z])
            n_det[z] += len(da[1])
            want = one[z].counts()[0]
            for i, l in enumerate(mp.wanted):
                if l in lists[z]:
                    np.testing.assert_array_equal(got[z][i], want[lists[z].index(l)])
                else:
                    assert not got[z][i].any(), 'an un-wanted row of counts() moved'
        if f in (F // 2, F - 1):
            img = ctx.to_host(mp.render(frames[f], streams=[0, 2]))
            for k, z in enumerate((0, 2)):
                np.testing.assert_array_equal(img[k], ctx.to_host(one[z].render(frames[f][z:z + 1].contiguous()))[0], err_msg='render, step %d stream %d' % (f, z))
    print('labels', a, b, 'detections per stream:', n_det, 'tracks:', [len(t[0]) for t in _tables(mp)])
    assert n_det[0] > 0 and n_det[1] > 0 and n_det[2] == n_det[0] + n_det[1] and n_det[3] == 0
    assert len(mp.tracker(3).table()[0]) == 0 and mp.tracker(3).next_id == 1 and len(mp.tracker(2).table()[0]) > 0


# ------------------------------------------------------------------ 5. motion ratio
def test_every_stream_tests_motion_against_its_own_ratio():
    """background_subtraction_ratio per stream on the frames of tests/test_gpu_present.py's MOG2 pipeline test (scene boxes plus two
    phantom boxes over still background): tables and motion masks equal the one-stream pipelines, which reject what their ratio says."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    RATIO = [0.0, 0.25, 0.9, 0.25]
    F, W, H = 12, 320, 240
    scenes = [Scene(seed=200 + z, n_obj=7, n_frames=F, width=W, height=H, wrange=(14, 30), hrange=(30, 60), vmax=2.5) for z in range(S)]
    phantom = [(6, 8, 30, 44), (250, 150, 40, 60)]
    kw = dict(input_size=(W, H), run_detector=False, encoder_max_batch=ENC_BATCH)
    mp = MultiStreamPipeline(S, background_subtraction_ratio=RATIO, **kw)
    one = [MultiStreamPipeline(1, background_subtraction_ratio=RATIO[z], **kw) for z in range(S)]
    for f in range(F):
        fd = torch.from_numpy(np.stack([scenes[z].frame(f) for z in range(S)])).cuda()
        per = []
        for z in range(S):
            b, l, s = _dets(scenes[z], f)
            per.append((b + phantom, l + ['person'] * 2, s + [0.55, 0.54]))
        mp.step(fd, mp.pack_injected(per))
        got, _ = mp.motion_mask()
        for z in range(S):
            one[z].step(fd[z:z + 1].contiguous(), one[z].pack_injected([per[z]]))
            np.testing.assert_array_equal(got[z], one[z].motion_mask()[0][0], err_msg='mask plane, step %d stream %d' % (f, z))
            _assert_same_table(mp.tracker(z).table(), one[z].tracker(0).table(), 'step %d stream %d' % (f, z))
    rejected = [o.motion_mask(read=False)[1] for o in one]
    print('boxes rejected per one-stream pipeline:', rejected, 'by the four-stream pipeline:', mp.motion_mask(read=False)[1])
    assert mp.motion_mask(read=False)[1] == sum(rejected)
    assert rejected[0] == 0 and rejected[2] > rejected[1] > 0 and rejected[0] != rejected[2]
    for z in range(S):
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    with pytest.raises(ValueError, match='background_subtraction_ratio'):
        mp.background_subtraction([0.25, None, 0.25, 0.25])


# ------------------------------------------------------------------ 6. reset
def _assert_stream_equals(mp, z, o, step):
    msg = 'step %d stream %d' % (step, z)
    _assert_same_table(mp.tracker(z).table(), o.tracker(0).table(), msg)
    assert mp.tracker(z).next_id == o.tracker(0).next_id, msg
    np.testing.assert_array_equal(mp.counts()[z], o.counts()[0], err_msg=msg)
    assert mp.frames_seen()[z] == o.frames_seen()[0], msg
    assert mp.skip_stats()['skipped'][z] == o.skip_stats()['skipped'][0], msg
    for x, y in zip(mp.detections(z), o.detections(0)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), msg
    for name, x, y in zip(('weight', 'variance', 'mean', 'nmodes'), mp.mog2_state(z), o.mog2_state(0)):
        np.testing.assert_array_equal(x, y, err_msg='MOG2 %s, %s' % (name, msg))
    if o.frames_seen()[0]:
        np.testing.assert_array_equal(mp.motion_mask()[0][z], o.motion_mask()[0][0], err_msg='mask plane, ' + msg)
    a, b = mp.overlay([z])[0], o.overlay()[0]
    for key in ('track_ids', 'track_tlbr', 'points', 'crossings', 'det_tlbr', 'counts'):
        np.testing.assert_array_equal(a[key], b[key], err_msg='overlay %s, %s' % (key, msg))


def test_reset_gives_a_stream_a_fresh_start_and_leaves_the_others_alone():
    """Three streams, per-stream skip counters [0, 1, 2], MOG2 on, detector on with the look-ahead queued every step (its output is
    replaced by the scenes' rows, which a skip step ignores as it ignores the detector: moving boxes pass the motion test).  reset([1]) after
    step 7: from then on stream 1's yardstick is a NEW one-stream pipeline fed the same later frames, streams 0 and 2 stay on theirs;
    everything equal after every later step.  Then reset([0, 2]) with presence masks in force, and the same check."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S3, F, N = 3, 14, [0, 1, 2]
    scenes = [Scene(seed=81 + z, n_obj=10 + 2 * z, n_frames=F) for z in range(S3)]
    kw = dict(run_detector=True, encoder_max_batch=ENC_BATCH, background_subtraction_ratio=0.25)
    frames = [torch.from_numpy(np.stack([scenes[z].frame(f) for z in range(S3)])).cuda() for f in range(F)]
    mp = MultiStreamPipeline(S3, object_detector_skip_frames=N, **kw)

    def fresh(z):
        return MultiStreamPipeline(1, object_detector_skip_frames=[N[z]], **kw)
    one = [fresh(z) for z in range(S3)]
    masks = {11: [1, 0, 1], 12: [0, 1, 1], 13: [1, 1, 1]}

    def step(f):
        present = masks.get(f)
        nxt = frames[f + 1] if f + 1 < F else None
        per = [_dets(scenes[z], f) for z in range(S3)]
        mp.step(frames[f], mp.pack_injected(per), nxt, present=present, present_next=masks.get(f + 1) if nxt is not None else None)
        for z in range(S3):
            if present is None or present[z]:
                one[z].step(frames[f][z:z + 1].contiguous(), one[z].pack_injected([per[z]]))
            _assert_stream_equals(mp, z, one[z], f)
    for f in range(8):
        step(f)
    assert sum(len(t[0]) for t in _tables(mp)) > 0 and mp.tracker(1).next_id > 1
    mp.reset([])                                                        # nothing
    assert mp.stream_param_stats()['resets'] == 0
    mp.reset([1])                                                       # (the look-ahead run of step 8 is queued: discarded)
    one[1] = fresh(1)
    assert mp.stream_param_stats() == dict(nms_stream_launches=0, association_stream_launches=0, resets=1, streams_reset=1)
    assert len(mp.tracker(1).table()[0]) == 0 and mp.tracker(1).next_id == 1 and not mp.counts()[1].any()
    assert mp.detections(1)[2].size == 0 and mp.frames_seen().tolist() == [8, 0, 8]
    ov = mp.overlay([1])[0]
    assert len(ov['track_ids']) == 0 and len(ov['det_tlbr']) == 0 and len(ov['points']) == 0
    assert not mp.mog2_state(1)[3].any() and mp.mog2_state(0)[3].any()
    for z in (0, 2):
        _assert_stream_equals(mp, z, one[z], 7)
    for f in range(8, 11):
        step(f)
    assert mp.frames_seen().tolist() == [11, 3, 11] and mp.tracker(1).next_id == one[1].tracker(0).next_id
    mp.reset(np.array([2, 0]))
    one[0], one[2] = fresh(0), fresh(2)
    assert mp.frames_seen().tolist() == [0, 3, 0]
    for f in range(11, F):
        step(f)
    assert mp.frames_seen().tolist() == [2, 5, 3]
    assert mp.stream_param_stats()['resets'] == 2 and mp.stream_param_stats()['streams_reset'] == 3
    assert mp.skip_stats()['rows_retained'] == sum(o.skip_stats()['rows_retained'] for o in one)
    assert sum(len(t[0]) for t in _tables(mp)) > 0


def test_reset_refusals():
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    mp = MultiStreamPipeline(3, run_detector=False)
    for bad in ([3], [-1], [0, 0], [1, 2, 1]):
        with pytest.raises(ValueError, match='streams'):
            mp.reset(bad)
    two = np.array([1, 1], np.int32)
    assert lib().dd_pipeline_reset_streams(mp._h, ptr(two), 2) == -1 and b'listed twice' in lib().dd_last_error()
    out = np.array([3], np.int32)
    assert lib().dd_pipeline_reset_streams(mp._h, ptr(out), 1) == -1 and b'stream 3 of 3' in lib().dd_last_error()
    assert mp.stream_param_stats()['resets'] == 0
    lock = MultiStreamPipeline(3, run_detector=False, object_detector_skip_frames=2)
    with pytest.raises(ValueError, match=r'object_detector_skip_frames=\[2\] \* 3'):
        lock.reset([1])
    one = np.array([1], np.int32)
    assert lib().dd_pipeline_reset_streams(lock._h, ptr(one), 1) == -3                   # DD_E_STATE
    assert b'dd_pipeline_detector_skip_streams' in lib().dd_last_error()
    MultiStreamPipeline(3, run_detector=False, object_detector_skip_frames=0).reset([1])  # N = 0: no counter to share
    mp.reset([0, 2])
    assert mp.stream_param_stats()['streams_reset'] == 2


# ------------------------------------------------------------------ 7. a setter after the first step
def test_setters_after_the_first_step_are_refused():
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    S3 = 3
    mp = MultiStreamPipeline(S3, run_detector=False, background_subtraction_ratio=0.25)
    d, i, m = np.full(S3 * 4, 0.5), np.full(S3, 3, np.int32), np.ones(S3, np.uint8)
    # before the first step they are accepted, and bad values are DD_E_ARG
    assert lib().dd_pipeline_stream_motion_ratio(mp._h, ptr(d)) == 0
    assert lib().dd_pipeline_stream_tracker_params(mp._h, None, None, ptr(i), None) == 0
    neg, nan = np.array([0.5, -1.0, 0.5]), np.full(S3 * 4, np.nan)
    assert lib().dd_pipeline_stream_motion_ratio(mp._h, ptr(neg)) == -1
    assert lib().dd_pipeline_stream_lines(mp._h, ptr(nan)) == -1
    off = MultiStreamPipeline(S3, run_detector=False)
    assert lib().dd_pipeline_stream_motion_ratio(off._h, ptr(d)) == -3 and b'background subtraction is off' in lib().dd_last_error()
    mp.step(torch.zeros((S3, mp.H, mp.W, 3), dtype=torch.uint8, device='cuda'))
    calls = dict(dd_pipeline_stream_lines=(ptr(d),), dd_pipeline_stream_wanted=(ptr(m),), dd_pipeline_stream_nms_overlap=(ptr(d),),
                 dd_pipeline_stream_motion_ratio=(ptr(d),), dd_pipeline_stream_tracker_params=(ptr(d), ptr(d), ptr(i), ptr(i)))
    for name, args in calls.items():
        assert getattr(lib(), name)(mp._h, *args) == -3, name           # DD_E_STATE
        assert name.encode() in lib().dd_last_error() and b'before the first step' in lib().dd_last_error()
    lines, idx = np.zeros((S3, 4)), np.arange(S3, dtype=np.int32)
    assert lib().dd_pipeline_lines(mp._h, ptr(idx), S3, ptr(lines)) == 0
    np.testing.assert_array_equal(lines, [[mp.W / 2, 0, mp.W / 2, mp.H]] * S3)


# ------------------------------------------------------------------ 8. the subtractor's own reset
@pytest.mark.parametrize('shape', [(5, 7), (53, 71)])
def test_mog2_reset_streams_equals_a_new_oracle_subtractor(shape):
    """BackgroundSubtractorMOG2.reset([1]) after four frames: stream 1 continues as a NEW oracle subtractor (model, frame count and so its
    learning rate), streams 0 and 2 as theirs, bit for bit; an index out of range is refused."""
    from deepdish_amd.background import createBackgroundSubtractorMOG2
    from oracle.mog2_np import MOG2, live_state
    S3, (h, w) = 3, shape
    sub = createBackgroundSubtractorMOG2(n_streams=S3)
    ora = [MOG2() for _ in range(S3)]
    rng = np.random.default_rng(11)
    sub.reset([1])                                                      # before the first frame there is no model yet: nothing to do
    for t in range(9):
        if t == 4:
            sub.reset([1])
            ora[1] = MOG2()
        if t == 7:
            sub.reset([])
        base = np.stack([np.full((h, w, 3), 40 * z + 30, np.int64) for z in range(S3)])
        fr = np.clip(base + rng.integers(-8, 9, base.shape), 0, 255).astype(np.uint8)
        if t % 3 == 2:
            fr[:, h // 2:, w // 2:] = rng.integers(0, 256, fr[:, h // 2:, w // 2:].shape)
        want = np.stack([ora[z].apply(fr[z]) for z in range(S3)])
        got = sub.apply_device(torch.from_numpy(fr).cuda())
        sub.ctx.sync()
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='mask planes, frame %d' % t)
        for z in range(S3):
            for name, a, b in zip(('weight', 'variance', 'mean', 'nmodes'), sub.state(z), live_state(ora[z])):
                np.testing.assert_array_equal(a, b, err_msg='%s, stream %d frame %d' % (name, z, t))
    for bad in ([3], [-1], [[0]]):
        with pytest.raises(ValueError, match='streams'):
            sub.reset(bad)
