"""GPU: the association decision on the device (csrc/assoc.hip) -- the wave-parallel assignment solver against the host solver pair for
pair, the cascade kernel against the reference fixture, and Tracker / HotPath / MultiStreamPipeline under association='device' against
the goldens and against the host path, with the counters showing that the device really decided."""
import os
import numpy as np
import pytest
import torch

import cascade_cases as cc
import euclidean_ref as er

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), 'golden')


# ----------------------------------------------------------------------------- dd_lsap_batch
def _lsap_problems():
    from test_lsap import _cases
    probs = list(_cases(np.random.default_rng(7), 2500))                  # tests/test_lsap.py's matrices: same generator, same seed
    rng = np.random.default_rng(21)
    for nr, nc in ((1, 1), (1, 256), (256, 1), (63, 64), (64, 64), (65, 65), (64, 70), (70, 64)):
        probs.append(rng.random((nr, nc)))                                # tie-free
        c = rng.random((nr, nc)); c[c > 0.3] = 0.2 + 1e-5                 # clamped as min_cost_matching clamps
        probs.append(c)
        probs.append(rng.integers(0, 3, (nr, nc)).astype(float))          # exact ties
    c = np.random.default_rng(8).random((256, 256)); c[c > 0.2] = 0.2 + 1e-5    # test_lsap_large_and_degenerate's
    probs.append(c)
    return probs


def test_lsap_batch_equals_host_solver_pair_for_pair():
    from deepdish_amd.deep_sort.linear_assignment import linear_sum_assignment, linear_sum_assignment_batch
    probs = _lsap_problems()
    got = linear_sum_assignment_batch(probs, device=True)                 # ONE launch, one wave per problem
    assert len(got) == len(probs) == 2500 + 24 + 1
    for i, (c, (r, q)) in enumerate(zip(probs, got)):
        wr, wq = linear_sum_assignment(c)
        assert r.tolist() == wr.tolist() and q.tolist() == wq.tolist(), f'problem {i} ({c.shape[0]} x {c.shape[1]})'
    r, q = linear_sum_assignment(probs[7], device=True)                   # the single-matrix form goes the same way
    wr, wq = linear_sum_assignment(probs[7])
    assert r.tolist() == wr.tolist() and q.tolist() == wq.tolist()


def test_lsap_batch_errors_name_the_problem():
    from deepdish_amd._lib import DeepDishHipError
    from deepdish_amd.deep_sort.linear_assignment import linear_sum_assignment_batch
    rng = np.random.default_rng(3)
    with pytest.raises(DeepDishHipError, match=r'problem 1 is 300 x 40'):
        linear_sum_assignment_batch([rng.random((4, 4)), rng.random((300, 40))])
    bad = rng.random((9, 7)); bad[4, 2] = np.nan
    with pytest.raises(DeepDishHipError, match=r'problem 2 .*NaN'):
        linear_sum_assignment_batch([rng.random((4, 4)), rng.random((70, 3)), bad, rng.random((2, 2))])
    bad = rng.random((5, 6)); bad[0, 5] = -np.inf
    with pytest.raises(DeepDishHipError, match=r'problem 0 .*NaN'):
        linear_sum_assignment_batch([bad])


# ----------------------------------------------------------------------------- assoc_match_k against the reference fixture
def test_device_decision_equals_reference():
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    for c in cc.load_cases(os.path.join(G, 'cascade_cases.npz')):
        m, ur, ud = cc.match_cascade(c, 1, ctx)
        assert m == c['matches'], f"case {c['i']} ({c['T']} x {c['n']}, kind {c['kind']}): matches"
        assert ur == c['un_rows'], f"case {c['i']}: unmatched tracks"
        assert ud == c['un_dets'], f"case {c['i']}: unmatched detections"


# ----------------------------------------------------------------------------- Tracker(association='device') on the golden scenes
def _table(trk):
    return np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in trk.tracks], dtype=np.int64).reshape(-1, 5)


def _all_on_device(stats, updates):
    assert stats == dict(device_updates=updates, host_updates=0, fallback_streams=0), stats


@pytest.mark.parametrize('name', ['n5', 'n20', 'n20_age5', 'n256'])
def test_scene_golden_on_device(name):
    """tests/test_gpu_tracker.py::test_scene_golden with the decision on the device: same goldens, same tolerances."""
    from test_gpu_tracker import _scene_for
    from deepdish_amd.deep_sort import nn_matching, preprocessing
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    from deepdish_amd.tools.countline import CountLine
    g = np.load(os.path.join(G, f'scene_{name}.npz'))
    scene = _scene_for(g, name)
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric('cosine', 0.2, None), max_iou_distance=0.7, max_age=int(g['max_age']),
                  association='device')
    counter = CountLine(scene.countline())
    fp, kp = g['frame_ptr'], g['keep_ptr']
    for f in range(int(g['n_frames'])):
        boxes, scores, who, feats = scene.detections(f)
        keep = preprocessing.non_max_suppression(boxes, 0.6, scores)
        assert keep == g['nms_keep'][kp[f]:kp[f + 1]].tolist(), f'nms frame {f}'
        trk.predict()
        trk.update([Detection(boxes[i], 'person', scores[i], feats[i]) for i in keep])
        counter.step(trk)
        np.testing.assert_array_equal(_table(trk), g['track_int'][fp[f]:fp[f + 1]], err_msg=f'frame {f}')
        if len(trk.tracks):
            np.testing.assert_allclose(np.array([t.mean for t in trk.tracks]), g['track_mean'][fp[f]:fp[f + 1]], rtol=1e-8, atol=1e-8,
                                       err_msg=f'frame {f}')
    assert trk._next_id == int(g['next_id'])
    np.testing.assert_array_equal(counter.vector()[0], g['counts'])
    _all_on_device(trk.association_stats(), int(g['n_frames']))


def test_scene_euclidean_golden_on_device():
    from deepdish_amd.deep_sort import nn_matching, preprocessing
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    from deepdish_amd.synth import Scene
    name = 'euclid_n20_age5'
    g = np.load(os.path.join(G, f'scene_{name}.npz'))
    kw, n_frames, max_age, (lo, hi), _ = er.SCENES[name]
    scene = Scene(**kw)
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric('euclidean', float(g['threshold']), None), max_iou_distance=0.7,
                  max_age=int(g['max_age']), association='device')
    fp, kp = g['frame_ptr'], g['keep_ptr']
    for f in range(n_frames):
        boxes, scores, who, feats = er.scene_detections(scene, f, lo, hi)
        keep = preprocessing.non_max_suppression(boxes, 0.6, scores)
        assert keep == g['nms_keep'][kp[f]:kp[f + 1]].tolist(), f'nms frame {f}'
        trk.predict()
        far = np.array([t.time_since_update > 1 for t in trk.tracks])
        trk.update([Detection(boxes[i], 'person', scores[i], feats[i]) for i in keep])
        np.testing.assert_array_equal(_table(trk), g['track_int'][fp[f]:fp[f + 1]], err_msg=f'frame {f}')
        if len(trk.tracks):
            np.testing.assert_allclose(np.array([t.mean for t in trk.tracks]), g['track_mean'][fp[f]:fp[f + 1]], rtol=1e-8, atol=1e-8,
                                       err_msg=f'frame {f}')
        if f == 50:                                     # the parity aid still answers: the matrices are fetched from the device
            app, iou = trk.last_cost()
            assert app.shape == iou.shape and app.shape[1] == len(keep) and np.isfinite(iou).all()
            # iou_matching.py:74-76: rows of tracks that missed the last frame are barred, every other entry is 1 - IoU
            assert far.any() and np.all(iou[far] == 1e5) and np.all((iou[~far] >= 0) & (iou[~far] <= 1))
    assert trk._next_id == int(g['next_id'])
    _all_on_device(trk.association_stats(), n_frames)


def test_tie_storm_host_and_device_trackers_agree():
    """About 20 objects, max_age 5, a fifth of the detections missing so time_since_update spreads over the cascade's levels; on every
    second frame each detection is teleported and given a fresh random feature, so every appearance cost is gated or above the threshold
    and every IoU cost is 1: all clamped, the decision is ties only.  Here the host path is the yardstick."""
    from deepdish_amd.deep_sort import nn_matching
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    from deepdish_amd.synth import Scene
    F = 40
    scene = Scene(seed=11, n_obj=20, n_frames=F, p_miss=0.2, n_dup=0.0)
    trks = [Tracker(nn_matching.NearestNeighborDistanceMetric('cosine', 0.2, None), max_iou_distance=0.7, max_age=5, association=a)
            for a in ('host', 'device')]
    rng = np.random.default_rng(5)
    levels = set()
    for f in range(F):
        boxes, scores, who, feats = scene.detections(f)
        if f % 2:
            boxes = boxes.copy()
            boxes[:, 0] = rng.integers(2, 640 - 60, len(boxes)); boxes[:, 1] = rng.integers(2, 480 - 130, len(boxes))
            feats = rng.standard_normal(feats.shape).astype(np.float32)
            feats /= np.linalg.norm(feats, axis=1, keepdims=True)
        dets = [Detection(boxes[i], 'person', scores[i], feats[i]) for i in range(len(boxes))]
        for t in trks:
            t.predict()
        levels |= {t.time_since_update for t in trks[0].tracks if t.is_confirmed()}
        for t in trks:
            t.update(dets)
        np.testing.assert_array_equal(_table(trks[1]), _table(trks[0]), err_msg=f'frame {f}')
        assert trks[1].last_matches() == trks[0].last_matches(), f'frame {f}'
        assert trks[1]._next_id == trks[0]._next_id, f'frame {f}'
        if len(trks[0].tracks):
            np.testing.assert_array_equal(np.array([t.mean for t in trks[1].tracks]), np.array([t.mean for t in trks[0].tracks]))
    assert len(levels) >= 3, levels                     # the cascade had several levels to walk
    assert trks[0]._next_id > 150                       # the teleported frames founded tracks by the dozen
    _all_on_device(trks[1].association_stats(), F)
    assert trks[0].association_stats() == dict(device_updates=0, host_updates=F, fallback_streams=0)


# ----------------------------------------------------------------------------- pipelines
def test_multistream_ragged_and_empty_inputs_on_device():
    """tests/test_gpu_pipeline.py::test_multistream_ragged_and_empty_inputs's inputs (a stream with nothing, one box, boxes that vanish,
    a NaN frame) through two pipelines, association='host' and 'device': the same per-stream tables every frame."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 14
    sc = Scene(seed=77, n_obj=6, n_frames=F, p_miss=0.0, churn=False)
    mps = [MultiStreamPipeline(S, run_detector=False, association=a) for a in ('host', 'device')]
    for f in range(F):
        frame = sc.frame(f)
        boxes, scores, _, _ = sc.detections(f)
        full = ([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores])
        per = [full if f not in (5, 6) else ([], [], []),
               ([], [], []),
               (full[0][:1], full[1][:1], full[2][:1]) if f < 9 else ([], [], [])]
        if f == 3:
            per[0] = ([(float('nan'), 1.0, 2.0, 3.0)] + full[0], ['person'] + full[1], [0.9] + full[2])
        frames = torch.from_numpy(np.stack([frame] * S)).cuda()
        for mp in mps:
            mp.step(frames, mp.pack_injected(per))
        for z in range(S):
            (hi, hm), (di, dm) = mps[0].tracker(z).table(), mps[1].tracker(z).table()
            np.testing.assert_array_equal(di, hi, err_msg=f'frame {f} stream {z}')
            np.testing.assert_array_equal(dm, hm, err_msg=f'frame {f} stream {z}')
        np.testing.assert_array_equal(mps[1].counts(), mps[0].counts())
    assert len(mps[0].tracker(0).table()[0]) > 0 and len(mps[0].tracker(1).table()[0]) == 0
    _all_on_device(mps[1].association_stats(), F)
    assert mps[0].association_stats() == dict(device_updates=0, host_updates=F, fallback_streams=0)


def test_group_with_a_stream_above_the_cap_runs_on_the_host_path():
    """Two streams, one with 257 detections (one above DD_ASSOC_DEVICE_MAX): every update of the group is decided on the host, the
    counters say so, and the tables equal the host pipeline's."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    frame = Scene(seed=4, n_obj=3).frame(0)
    grid = [(2 + 26 * (k % 24), 2 + 34 * (k // 24), 20, 28) for k in range(257)]            # 257 boxes that do not touch
    many = (grid, ['person'] * 257, [0.9 - 1e-3 * k for k in range(257)])
    few = (grid[:3], ['person'] * 3, [0.9, 0.8, 0.7])
    mps = [MultiStreamPipeline(2, run_detector=False, track_capacity=600, association=a) for a in ('host', 'device')]
    frames = torch.from_numpy(np.stack([frame] * 2)).cuda()
    for f in range(3):
        for mp in mps:
            mp.step(frames, mp.pack_injected([many, few]))
    for z in range(2):
        (hi, hm), (di, dm) = mps[0].tracker(z).table(), mps[1].tracker(z).table()
        np.testing.assert_array_equal(di, hi)
        np.testing.assert_array_equal(dm, hm)
    assert len(mps[1].tracker(0).table()[0]) == 257 and len(mps[1].tracker(1).table()[0]) == 3
    assert mps[1].association_stats() == dict(device_updates=0, host_updates=3, fallback_streams=0)
    for mp in mps:                                       # below the cap again (but 257 tracks are still alive in stream 0: still the host)
        mp.step(frames, mp.pack_injected([few, few]))
    assert mps[1].association_stats() == dict(device_updates=0, host_updates=4, fallback_streams=0)


def _drive_group(assoc, poison):
    """Three streams of ONE tracker group (a pipeline's), each stream updated through its own handle; poison(f, z, tlwh, feats) may
    damage stream z's inputs at frame f.  -> per-stream tables after every frame, the group's counters."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    from deepdish_amd.synth import Scene
    S, F = 3, 10
    mp = MultiStreamPipeline(S, run_detector=False, association=assoc)
    scenes = [Scene(seed=60 + z, n_obj=7, n_frames=F, p_miss=0.1, churn=False, n_dup=0.0) for z in range(S)]
    tables = []
    for f in range(F):
        for z in range(S):
            boxes, _, _, feats = scenes[z].detections(f)
            tlwh, feats = np.ascontiguousarray(boxes, dtype=np.float64), np.ascontiguousarray(feats, dtype=np.float32)
            poison(f, z, tlwh, feats)
            h = mp.tracker(z)._h
            check(lib().dd_tracker_predict(h), 'dd_tracker_predict')
            check(lib().dd_tracker_update(h, ptr(tlwh), ptr(feats), 0, len(tlwh)), 'dd_tracker_update')
            tables.append(mp.tracker(z).table())
    return tables, mp.association_stats(), S * F


def _same_tables(a, b):
    for k, ((ai, am), (bi, bm)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ai, bi, err_msg=f'update {k}')
        np.testing.assert_array_equal(am, bm, err_msg=f'update {k}')          # (NaN == NaN here)


def test_nan_feature_in_one_stream_of_three():
    """A NaN feature reaches the decision as a cost of +inf (the association kernel's maximum over the gallery skips NaN products; 1 - (-inf)),
    which both paths clamp like any cost above the threshold: the tables equal the host run's and every update stays on the device."""
    def poison(f, z, tlwh, feats):
        if f == 5 and z == 1:
            feats[2, 17] = np.nan
    host, hs, n = _drive_group('host', poison)
    dev, ds, _ = _drive_group('device', poison)
    _same_tables(dev, host)
    assert ds['device_updates'] == n and ds['host_updates'] == 0 and hs['device_updates'] == 0


def _step_group_with_a_nan_track(assoc):
    """Three streams stepped TOGETHER (one group update per dd_pipeline_step: one tracker_assoc_k launch, one assoc_match_k launch, all
    three streams in it).  After step 3 stream 1's tracker is handed, through its own handle, one detection whose width is NaN: nothing
    is decided on it (the tracks have time_since_update 0, so no cascade level and no IoU row exists), it founds a tentative track with a
    NaN mean.  At step 4 that track's row of stream 1's IoU matrix is NaN, and a new box keeps a detection unmatched after the cascade, so
    the IoU stage reads the row.  -> per-stream tables after every step, the group's counters."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    from deepdish_amd.synth import Scene
    S, F = 3, 8
    scs = [Scene(seed=70 + z, n_obj=6, n_frames=F, p_miss=0.0, churn=False, n_dup=0.0) for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=False, association=assoc)
    tables = []
    for f in range(F):
        per = []
        for z, sc in enumerate(scs):
            boxes, scores, _, _ = sc.detections(f)
            b, l, c = [tuple(int(v) for v in q) for q in boxes], ['person'] * len(boxes), [float(v) for v in scores]
            if z == 1 and f >= 4:                      # a box that touches no other box of the stream: a detection no track claims
                free = next((x, y, 24, 60) for y in range(4, 400, 8) for x in range(4, 600, 8)
                            if all(x + 24 <= q[0] or q[0] + q[2] <= x or y + 60 <= q[1] or q[1] + q[3] <= y for q in b))
                b, l, c = b + [free], l + ['person'], c + [0.55]
            per.append((b, l, c))
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scs])).cuda()
        mp.step(frames, mp.pack_injected(per))
        if f == 3:
            tlwh = np.array([[300.0, 200.0, np.nan, 80.0]])
            feat = np.random.default_rng(1).standard_normal((1, 128)).astype(np.float32)
            check(lib().dd_tracker_update(mp.tracker(1)._h, ptr(tlwh), ptr(feat), 0, 1), 'dd_tracker_update')
        tables.append([mp.tracker(z).table() for z in range(S)])
    return tables, mp.association_stats(), F


def test_one_stream_of_a_three_stream_update_falls_back():
    """One group update holding three streams, one of which meets a NaN cost: that stream's decision stops with its status word set, its
    two matrices (they sit behind stream 0's in the cost buffer) are fetched and the host code decides it, the other two streams of the
    SAME update are decided by the device, and every table equals the host run's (whatever the host code makes of such a matrix)."""
    host, hs, F = _step_group_with_a_nan_track('host')
    dev, ds, _ = _step_group_with_a_nan_track('device')
    for f, (a, b) in enumerate(zip(dev, host)):
        for z in range(3):
            np.testing.assert_array_equal(a[z][0], b[z][0], err_msg=f'step {f} stream {z}')
            np.testing.assert_array_equal(a[z][1], b[z][1], err_msg=f'step {f} stream {z}')     # (NaN == NaN here)
    assert np.isnan(host[3][1][1]).any() and not np.isnan(host[4][1][1]).any()      # the NaN track lived from step 3 to step 4
    assert all(len(host[4][z][0]) >= 6 for z in range(3))                           # all three streams had tracks in the update at step 4
    # F steps + the single-stream update that planted the track; exactly one stream of one update handed back
    assert ds == dict(device_updates=F + 1, host_updates=0, fallback_streams=1), ds
    assert hs == dict(device_updates=0, host_updates=F + 1, fallback_streams=0), hs


def test_unknown_association_is_a_value_error():
    from deepdish_amd.deep_sort import nn_matching
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    with pytest.raises(ValueError, match='association'):
        Tracker(nn_matching.NearestNeighborDistanceMetric('cosine', 0.2, None), association='nonsense')
    with pytest.raises(ValueError, match='association'):
        HotPath(run_detector=False, association='nonsense')
    with pytest.raises(ValueError, match='association'):
        MultiStreamPipeline(3, run_detector=False, association='nonsense')


def test_default_association_is_host_and_hotpath_takes_the_option():
    from deepdish_amd._lib import lib
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    sc = Scene(seed=8, n_obj=5)
    hps = [HotPath(run_detector=False), HotPath(run_detector=False, association='device')]
    for f in range(5):
        boxes, scores, _, _ = sc.detections(f)
        inj = ([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores])
        fr = torch.from_numpy(sc.frame(f)).cuda()
        for hp in hps:
            hp.step(fr, injected=inj)
    np.testing.assert_array_equal(_table(hps[1].tracker), _table(hps[0].tracker))
    assert hps[0].tracker.association_stats() == dict(device_updates=0, host_updates=5, fallback_streams=0)
    _all_on_device(hps[1].tracker.association_stats(), 5)
    assert lib().dd_tracker_set_association(hps[0].tracker._h, 2) < 0 and b'association' in lib().dd_last_error()
