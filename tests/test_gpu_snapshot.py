"""GPU: MultiStreamPipeline.snapshot / restore with injected detections (run_detector=False).  The contract under test: a stream restored
from a snapshot is, from its next step on, bit for bit the stream the snapshot was taken from -- in a new pipeline, in a pipeline with
another number of streams, under presence masks -- and a snapshot is a pure read.  The yardstick is always the uninterrupted run: both
sides run the same kernels on the same inputs, so every comparison is equality, means included.  One encoder_max_batch everywhere (the
engine's max_batch fixes the K split of its convolutions)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENC_BATCH = 128
F, CUT = 45, 37                          # steps 0 .. 36 before the snapshot, 37 .. 44 after it


def _scene():
    from deepdish_amd.synth import Scene
    return Scene(seed=3, n_obj=20, n_frames=F, p_miss=0.1)              # the scene behind tests/golden/scene_n20_age5.npz


def _dets(sc, f, label='person'):
    boxes, scores, _, _ = sc.detections(f)
    return [tuple(int(v) for v in b) for b in boxes], [label] * len(boxes), [float(s) for s in scores]


def _frames(sc, f, S):
    return torch.from_numpy(np.stack([sc.frame(f)] * S)).cuda()


def _step(mp, sc, f, present=None, nxt=None):
    mp.step(_frames(sc, f, mp.S), mp.pack_injected([_dets(sc, f)] * mp.S), nxt, present=present)


def _same_stream(a, za, b, zb, msg, galleries=False):
    """Every getter the contract lists: stream za of pipeline a == stream zb of pipeline b."""
    ta, tb = a.tracker(za).table(), b.tracker(zb).table()
    np.testing.assert_array_equal(ta[0], tb[0], err_msg='table, ' + msg)
    np.testing.assert_array_equal(ta[1], tb[1], err_msg='means, ' + msg)
    assert a.tracker(za).next_id == b.tracker(zb).next_id, msg
    np.testing.assert_array_equal(a.counts()[za], b.counts()[zb], err_msg='counts, ' + msg)
    assert a.frames_seen()[za] == b.frames_seen()[zb], msg
    assert a.skip_stats()['skipped'][za] == b.skip_stats()['skipped'][zb], msg
    for x, y in zip(a.detections(za), b.detections(zb)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), 'detections, ' + msg
    oa, ob = a.overlay([za])[0], b.overlay([zb])[0]
    for key in ('line', 'track_ids', 'track_tlbr', 'path_counts', 'points', 'crossings', 'det_tlbr', 'counts'):
        np.testing.assert_array_equal(oa[key], ob[key], err_msg='overlay %s, %s' % (key, msg))
    assert oa['track_labels'] == ob['track_labels'], msg
    if a.ground is not None:
        ga, gb = a.ground_paths([za])[0], b.ground_paths([zb])[0]
        for key in ('track_ids', 'path_counts', 'points'):
            np.testing.assert_array_equal(ga[key], gb[key], err_msg='ground %s, %s' % (key, msg))
    if galleries:
        for tid in ta[0][:, 0]:
            ra, na = a.tracker(za).gallery(tid)
            rb, nb = b.tracker(zb).gallery(tid)
            assert na == nb, msg
            np.testing.assert_array_equal(ra, rb, err_msg='gallery of track %d, %s' % (tid, msg))


# ------------------------------------------------------------------ 1. continuation
@pytest.mark.parametrize('where', ['host', 'device'])
def test_a_restored_pipeline_continues_as_the_uninterrupted_run(where):
    """S = 3 over the scene whose golden shows max_age = 5 changing the ids (stream 1 has it), snapshot after step 36, restore into a NEW
    pipeline: immediately every getter and every gallery equal, after every later step tables, ids, counts, overlay and frames_seen.
    Nothing of this scene crosses the default line x = 320 in steps 37 .. 44, so stream 2 counts across x = 246: object 14 of the scene
    is detected in every frame from 30 on and its bottom centre moves from x = 235.9 (frame 36) through 246.2 (frame 40) to 256.5
    (frame 44), 2.6 px a frame against a detection jitter of 2 px -- its path is left of that line at the cut and right of it at the end."""
    from deepdish_amd.ground import GroundPlane
    from deepdish_amd.multipipe import MultiStreamPipeline
    sc = _scene()
    centre = sc.xy[:, 14, 0] + sc.w[14] / 2
    assert sc.t0[14] <= 30 and sc.t1[14] >= F and centre[36] < 246 - 8 and centre[44] > 246 + 8, 'the scene is not the one the line was chosen for'
    cam = GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=4.0, tilt_deg=60.0)
    lines = np.array([[320, 0, 320, 480], [320, 0, 320, 480], [246, 0, 246, 480]], dtype=np.float64)
    kw = dict(run_detector=False, association=where, encoder_max_batch=ENC_BATCH, max_age=[60, 5, 60], ground=cam, line=lines)
    a = MultiStreamPipeline(3, **kw)
    for f in range(CUT):
        _step(a, sc, f)
    snap = a.snapshot()
    assert len(snap) == 3 and [i['frames_seen'] for i in snap.info] == [CUT] * 3
    live = [len(a.tracker(z).table()[0]) for z in range(3)]
    rows = [max(a.tracker(z).gallery(t)[0].shape[0] for t in a.tracker(z).table()[0][:, 0]) for z in range(3)]
    states = set(a.tracker(1).table()[0][:, 1].tolist()) | set(a.tracker(0).table()[0][:, 1].tolist())
    missed = int((a.tracker(0).table()[0][:, 2] > 0).sum())
    print('tracks', [i['n_tracks'] for i in snap.info], 'live', live, 'longest gallery', rows, 'states', states, 'missed', missed,
          'bytes', [i['bytes'] for i in snap.info])
    # the test's own teeth: a gallery over two chunks and a deleted track at the cut (and, below, a crossing after it)
    assert max(rows) > 32
    assert any(i['n_tracks'] > n for i, n in zip(snap.info, live)), 'no deleted track at the cut'
    assert all(i['gallery_rows'] > 0 and not i['has_background'] and i['next_id'] == a.tracker(z).next_id for z, i in enumerate(snap.info))
    b = MultiStreamPipeline(3, **kw)
    b.restore(snap)
    for z in range(3):
        _same_stream(b, z, a, z, '%s, right after restore, stream %d' % (where, z), galleries=True)
    crossings, counts0 = 0, a.counts().copy()
    for f in range(CUT, F):
        _step(a, sc, f)
        _step(b, sc, f)
        for z in range(3):
            _same_stream(b, z, a, z, '%s, step %d stream %d' % (where, f, z))
            crossings += len(a.overlay([z])[0]['crossings'])
    print('crossings after the cut', crossings, 'counts moved by', (a.counts() - counts0).sum(axis=(1, 2)).tolist())
    assert crossings > 0, 'no crossing after the cut: the counters were not exercised'
    for z in range(3):
        _same_stream(b, z, a, z, '%s, at the end, stream %d' % (where, z), galleries=True)
    st = b.association_stats()
    assert st['fallback_streams'] == 0, st
    assert (st['device_updates'] if where == 'device' else st['host_updates']) == F - CUT, st


# ------------------------------------------------------------------ 2. read-only
def test_a_snapshot_is_a_pure_read_and_keeps_the_look_ahead():
    """Detector on, the look-ahead queued in every step, streams 0 and 2 present: every queued detector run gathers its frames with one
    frames_gather_k launch, so the launches count the runs.  A snapshot between two steps: the next steps equal a twin that was never
    snapshotted and the queued run was consumed (8 runs in 7 steps, as the twin); a third pipeline that calls reset() there -- which does
    discard the queued run -- needs a ninth."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    sc = _scene()
    kw = dict(run_detector=True, encoder_max_batch=ENC_BATCH)
    a, b, c = (MultiStreamPipeline(3, **kw) for _ in range(3))
    frames = [_frames(sc, f, 3) for f in range(8)]
    present = [1, 0, 1]
    for f in range(7):
        for mp in (a, b, c):
            mp.step(frames[f], mp.pack_injected([_dets(sc, f)] * 3), frames[f + 1], present=present, present_next=present)
        if f == 3:
            before = a.stage_ms()['steps']
            snap = a.snapshot()
            assert a.stage_ms()['steps'] == before and len(snap) == 3
            assert snap.to_bytes() == a.snapshot().to_bytes(), 'two snapshots of one state differ'
            c.reset([1])
        for z in range(3):
            _same_stream(a, z, b, z, 'step %d stream %d' % (f, z))
    runs = [mp.present_stats()['gather_launches'] for mp in (a, b, c)]
    print('detector runs', runs)
    assert runs == [8, 8, 9], 'the look-ahead of step 4 was discarded by the snapshot, or reset() no longer discards it'
    assert len(a.tracker(0).table()[0]) > 0


# ------------------------------------------------------------------ 3. migration
def test_a_stream_migrates_into_a_pipeline_of_another_size():
    """Stream 1 of a 3-stream pipeline goes -- through to_bytes / from_bytes / select -- to stream 0 of a 2-stream pipeline that already has
    history: stream 0 continues as the source stream would have, stream 1 of the destination equals a twin that saw no restore."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.snapshot import StreamSnapshot
    from deepdish_amd.synth import Scene
    sc = _scene()
    other = Scene(seed=22, n_obj=13, n_frames=F)
    kw = dict(run_detector=False, encoder_max_batch=ENC_BATCH)
    src = MultiStreamPipeline(3, max_age=[60, 5, 60], **kw)
    dst, twin = MultiStreamPipeline(2, max_age=[5, 60], **kw), MultiStreamPipeline(2, max_age=[5, 60], **kw)
    for f in range(20):
        _step(src, sc, f)
        for mp in (dst, twin):
            _step(mp, other, f)
    snap = StreamSnapshot.from_bytes(src.snapshot().to_bytes())
    one = snap.select([1])
    assert len(snap) == 3 and len(one) == 1 and one.info[0] == snap.info[1]
    assert snap.select([2, 0]).info == [snap.info[2], snap.info[0]]
    assert StreamSnapshot.from_bytes(one.to_bytes()).to_bytes() == src.snapshot([1]).to_bytes(), 'select is a slice of the entries'
    assert dst.tracker(0).next_id > 1 and len(dst.tracker(0).table()[0]) > 0, 'the destination must have history'
    dst.restore(one, [0])
    _same_stream(dst, 0, src, 1, 'right after the migration', galleries=True)
    _same_stream(dst, 1, twin, 1, 'the other stream, right after the migration', galleries=True)
    for f in range(20, 30):
        _step(src, sc, f)
        per_dst = [_dets(sc, f), _dets(other, f)]
        fd = torch.from_numpy(np.stack([sc.frame(f), other.frame(f)])).cuda()
        dst.step(fd, dst.pack_injected(per_dst))
        _step(twin, other, f)
        _same_stream(dst, 0, src, 1, 'migrated stream, step %d' % f)
        _same_stream(dst, 1, twin, 1, 'untouched stream, step %d' % f)
    _same_stream(dst, 0, src, 1, 'at the end', galleries=True)
    assert len(dst.tracker(0).table()[0]) > 0 and dst.tracker(0).next_id == src.tracker(1).next_id


# ------------------------------------------------------------------ 4. under masks
def test_a_stream_absent_before_the_snapshot_continues():
    """Stream 1 is absent for its last five steps before the snapshot (its tracks carry the time since their update of step 9, its
    frame number stays behind): restored into a new pipeline it continues as in the uninterrupted run."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    sc = _scene()
    kw = dict(run_detector=False, encoder_max_batch=ENC_BATCH)
    a = MultiStreamPipeline(2, **kw)
    for f in range(15):
        _step(a, sc, f, present=None if f < 10 else [1, 0])
    assert a.frames_seen().tolist() == [15, 10]
    snap = a.snapshot()
    assert [i['frames_seen'] for i in snap.info] == [15, 10]
    b = MultiStreamPipeline(2, **kw)
    b.restore(snap)
    for z in range(2):
        _same_stream(b, z, a, z, 'right after restore, stream %d' % z, galleries=True)
    for f in range(15, 24):
        present = [1, 1] if f % 3 else [0, 1]
        _step(a, sc, f, present=present)
        _step(b, sc, f, present=present)
        for z in range(2):
            _same_stream(b, z, a, z, 'step %d stream %d' % (f, z))
    assert len(b.tracker(1).table()[0]) > 0 and b.frames_seen().tolist() == a.frames_seen().tolist()


# ------------------------------------------------------------------ 5. refusals
def test_restore_refusals_leave_the_pipeline_as_it_was():
    from deepdish_amd._lib import lib, DeepDishHipError
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.snapshot import StreamSnapshot
    sc = _scene()
    kw = dict(run_detector=False, encoder_max_batch=ENC_BATCH)
    src = MultiStreamPipeline(2, **kw)
    for f in range(8):
        _step(src, sc, f)
    snap = src.snapshot()
    assert all(i['n_tracks'] > 4 for i in snap.info)
    dst = MultiStreamPipeline(3, **kw)
    for bad in ([3, 0], [-1, 0], [1, 1]):                                   # out of range, listed twice
        with pytest.raises(ValueError, match='streams'):
            dst.restore(snap, bad)
    with pytest.raises(ValueError, match='2 entries'):                       # len(streams) != len(snapshot)
        dst.restore(snap, [0])
    with pytest.raises(ValueError, match='2 entries'):
        dst.restore(snap, [0, 1, 2])
    # parameter mismatches, each named
    for name, other in (('max_age', dict(max_age=[60, 7])), ('max_cosine_distance', dict(max_cosine_distance=np.nextafter(0.2, 1.0))),
                        ('nms_max_overlap', dict(nms_max_overlap=0.5)), ('metric', dict(metric='euclidean')), ('line', dict(line=[0, 240, 640, 240])),
                        ('W', dict(input_size=(320, 480))), ('wanted labels', dict(wanted_labels=('person', 'car'))),
                        ('background_subtraction_ratio', dict(background_subtraction_ratio=0.25)),
                        ('object_detector_skip_frames', dict(object_detector_skip_frames=[1, 1]))):
        p2 = MultiStreamPipeline(2, **dict(kw, **other))
        with pytest.raises(ValueError, match=name + ' differs'):
            p2.restore(snap)
        assert p2.tracker(0).next_id == 1 and p2.frames_seen().tolist() == [0, 0]
    # a snapshot with background into a pipeline with subtraction off
    bg = MultiStreamPipeline(1, input_size=(64, 48), background_subtraction_ratio=0.25, **kw)
    blank = torch.zeros((1, 48, 64, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    bg.step(blank)
    sb = bg.snapshot()
    assert sb.info[0]['has_background'] and not bg.snapshot(background=False).info[0]['has_background']
    with pytest.raises(ValueError):
        MultiStreamPipeline(1, input_size=(64, 48), **kw).restore(sb)
    # the lock-step int form with N > 0: DD_E_STATE, naming the sequence form
    lock = MultiStreamPipeline(2, object_detector_skip_frames=2, **kw)
    with pytest.raises(DeepDishHipError, match=r'\(-3\).*dd_pipeline_detector_skip_streams'):
        lock.restore(snap)
    # more tracks than the destination's track_capacity, and a corrupt blob: the destination steps on equal to a twin that never saw the attempt
    small, twin = MultiStreamPipeline(2, track_capacity=4, **kw), MultiStreamPipeline(2, track_capacity=4, **kw)
    few = lambda f: [([(100 + 6 * f, 100, 40, 90), (420 - 6 * f, 220, 44, 96)], ['person'] * 2, [0.9, 0.8])] * 2      # two tracks per stream
    for f in range(5):
        for mp in (small, twin):
            mp.step(_frames(sc, f, 2), mp.pack_injected(few(f)))
    with pytest.raises(DeepDishHipError, match=r'\(-4\).*track_capacity'):
        small.restore(snap)
    raw = bytearray(snap.to_bytes())
    with pytest.raises(ValueError, match='refused'):
        StreamSnapshot.from_bytes(bytes(raw[:-1]))
    raw[16 + 2 * 16 + 8] ^= 0xFF                                             # the feature length of the first entry: 128 -> 127
    with pytest.raises(ValueError, match='refused'):
        StreamSnapshot.from_bytes(bytes(raw))
    blob = np.frombuffer(bytes(raw), dtype=np.uint8)
    assert lib().dd_pipeline_restore(small._h, blob.ctypes.data, blob.size, None, 2) == -1 and b'refused' in lib().dd_last_error()
    for z in range(2):
        _same_stream(small, z, twin, z, 'after the refused restores, stream %d' % z, galleries=True)
    for f in range(5, 9):
        for mp in (small, twin):
            mp.step(_frames(sc, f, 2), mp.pack_injected(few(f)))
        for z in range(2):
            _same_stream(small, z, twin, z, 'step %d after the refused restores, stream %d' % (f, z))
    assert small.association_stats()['fallback_streams'] == 0
    assert small.stream_param_stats()['resets'] == 0


# ------------------------------------------------------------------ 6. retained rows of streams in the middle of a skip cycle
def test_streams_in_a_skip_cycle_take_their_retained_rows_along():
    """Per-stream skip counters [1, 2], no detector: on a skip step a stream ignores the injected rows and pairs its retained detector
    output with its retained encoder rows (csrc/featrows.hip).  Snapshot after step 4 (stream 1 has one more skip step to go), restore
    into streams 1 and 2 of a three-stream pipeline whose store already holds stream 0's rows: both continue as in the source, stream 0
    as in a twin, and the rows retained add up."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    sc = _scene()
    other = Scene(seed=22, n_obj=13, n_frames=F)
    kw = dict(run_detector=False, encoder_max_batch=ENC_BATCH)
    src = MultiStreamPipeline(2, object_detector_skip_frames=[1, 2], **kw)
    dst, twin = (MultiStreamPipeline(3, object_detector_skip_frames=[2, 1, 2], **kw) for _ in range(2))

    def step3(mp, f):
        fd = torch.from_numpy(np.stack([other.frame(f), sc.frame(f), sc.frame(f)])).cuda()
        mp.step(fd, mp.pack_injected([_dets(other, f), _dets(sc, f), _dets(sc, f)]))
    for f in range(5):
        _step(src, sc, f)
        step3(dst, f + 7)                                                # another history: other frames, another point of its cycles
        step3(twin, f + 7)
    assert src.skip_stats()['skipped'].tolist() == [False, True] and src.skip_stats()['rows_retained'] > 0
    kept0 = dst.skip_stats()['rows_retained']
    dst.restore(src.snapshot(), [1, 2])
    assert dst.skip_stats()['rows_retained'] > 0
    for z in range(2):
        _same_stream(dst, z + 1, src, z, 'right after restore, stream %d' % z, galleries=True)
    _same_stream(dst, 0, twin, 0, 'the other stream, right after restore', galleries=True)
    skips = 0
    for f in range(5, 12):
        _step(src, sc, f)
        fd = torch.from_numpy(np.stack([other.frame(f + 7), sc.frame(f), sc.frame(f)])).cuda()
        dst.step(fd, dst.pack_injected([_dets(other, f + 7), _dets(sc, f), _dets(sc, f)]))
        step3(twin, f + 7)
        for z in range(2):
            _same_stream(dst, z + 1, src, z, 'step %d stream %d' % (f, z))
        _same_stream(dst, 0, twin, 0, 'the other stream, step %d' % f)
        skips += int(src.skip_stats()['skipped'].sum())
    assert skips > 0 and len(dst.tracker(2).table()[0]) > 0
    print('rows retained before', kept0, 'after', dst.skip_stats()['rows_retained'], 'skip steps compared', skips)
