"""GPU: the "euclidean" nearest-neighbour metric (upstream deep_sort/nn_matching.py:5-28,57-75) -- the stand-alone cost kernel, the
HBM-resident tracker on un-normalised features (scene fixtures produced by the reference, scripts/make_golden_euclidean.py), the
budget ring, dd_tracker_track_update, and both pipelines -- and the cosine path through dd_tracker_create_metric.

Costs compare with |got - want| <= 2e-6 * (max_g |g|^2 + |q|^2) per entry, the maximum over the target's stored rows
(tests/euclidean_ref.py: tolerance): the cosine tolerance of tests/test_gpu_deepsort.py (2e-6 on 1 - a.b for unit vectors) carried
over to |a|^2 + |b|^2 - 2 a.b.  Track decisions are compared exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import euclidean_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TARGETS = list(range(1, 13))


@pytest.fixture(scope='module')
def fix():
    """euclidean.npz + the tolerance of every (target, query) entry, computed once."""
    g = np.load(os.path.join(G, 'euclidean.npz'))
    d = {k: g[k] for k in g.files}
    d['off'] = np.concatenate([[0], np.cumsum(d['gallery_sizes'])]).astype(np.int32)
    d['tol'] = np.array([er.tolerance(d['gallery'][d['off'][t]:d['off'][t + 1]], d['query']) for t in range(12)])
    for v in d.values():
        v.setflags(write=False)
    return d


def _check_cost(got, want, tol, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    err = np.abs(got - want) / tol
    print('%s: worst error %.3f tolerances over %d entries' % (what, err.max(), err.size))
    assert got.min() >= 0.0, what                              # results are never negative
    assert np.all(err <= 1.0), (what, float(err.max()))


@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65])
def test_standalone_cost_matches_the_reference(fix, n):
    """dd_euclidean_nn_cost and NearestNeighborDistanceMetric('euclidean').distance against the reference's metric.distance: galleries
    of 1 .. 65 rows (around the 16-row MFMA tile), n queries (around the wave's 16 and the block's 64), row norms 0.05 .. 2."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context, ptr
    from deepdish_amd.deep_sort.nn_matching import NearestNeighborDistanceMetric
    assert n in fix['query_counts']
    ctx = default_context()
    q = fix['query'][:n].copy()                                  # (the shared fixture arrays are read-only)
    gal, df = ctx.to_device(fix['gallery'].copy()), ctx.to_device(q)
    out = torch.full((12, n), -7.0, dtype=torch.float64, device=gal.device)
    check(lib().dd_euclidean_nn_cost(ctx.handle, ptr(gal), ptr(np.ascontiguousarray(fix['off'])), 12, ptr(df), n, ptr(out), None),
          'dd_euclidean_nn_cost')
    got = ctx.to_host(out)
    want, tol = fix[f'nn_cost_{n}'], fix['tol'][:, :n]
    _check_cost(got, want, tol, f'dd_euclidean_nn_cost n={n}')
    m = NearestNeighborDistanceMetric('euclidean', 0.4, None)
    m.partial_fit(fix['gallery'], np.repeat(np.arange(1, 13), fix['gallery_sizes']), TARGETS)
    got_m = m.distance(q, TARGETS)
    np.testing.assert_array_equal(got_m, got)                 # the same kernel through the Python surface
    # a query that equals a gallery row bit for bit: its cost lies in [0, tolerance]
    qi, t, _ = fix['equal_query'].tolist()
    assert 0.0 <= got[t - 1, qi] <= tol[t - 1, qi], got[t - 1, qi]
    # the single-target helpers' values: one target of 65 rows is the column min of _pdist
    if n == 17:
        np.testing.assert_array_equal(fix['pdist'].min(axis=0), fix['nn'])
        assert np.all(np.abs(got[8] - fix['nn']) <= tol[8])


def test_standalone_cost_argument_checks(fix):
    from deepdish_amd._lib import lib
    from deepdish_amd.runtime import default_context, ptr
    ctx = default_context()
    gal = ctx.to_device(fix['gallery'][:4].copy())
    out = ctx.empty((2, 4), torch.float64)
    l = lib()
    assert l.dd_euclidean_nn_cost(ctx.handle, ptr(gal), ptr(np.array([0, 2, 2], np.int32)), 2, ptr(gal), 4, ptr(out), None) < 0
    assert b'dd_euclidean_nn_cost' in l.dd_last_error()       # an empty target is refused, as in dd_cosine_nn_cost
    assert l.dd_euclidean_nn_cost(ctx.handle, None, None, 0, None, 0, None, None) == 0
    h = ctypes.c_void_p()
    assert l.dd_tracker_create_metric(ctx.handle, 2, 0.2, 0.7, 30, 3, 0, 8, 32, ctypes.byref(h)) == -1     # DD_E_ARG
    assert b'metric' in l.dd_last_error() and not h.value


def _table(trk):
    return np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in trk.tracks], dtype=np.int64).reshape(-1, 5)


@pytest.mark.parametrize('name', sorted(er.SCENES))
def test_scene_golden(name):
    """Both euclidean scenes through the Python Tracker, frame by frame: the reference's track table exactly (it differs from the
    cosine run of the same inputs in 36 / 72 frames, so normalising the features or reusing the cosine path fails here), means at
    tests/test_gpu_tracker.py::test_scene_golden's tolerances, and at four frames the appearance costs the device associated with."""
    from deepdish_amd.deep_sort import nn_matching, preprocessing
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    from deepdish_amd.synth import Scene
    g = np.load(os.path.join(G, f'scene_{name}.npz'))
    kw, n_frames, max_age, (lo, hi), cost_frames = er.SCENES[name]
    scene = Scene(**kw)
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric('euclidean', float(g['threshold']), None), max_iou_distance=0.7,
                  max_age=int(g['max_age']))
    ref = er.Metric(float(g['threshold']))                      # host copy of every track's rows: only for the tolerances
    fp, kp = g['frame_ptr'], g['keep_ptr']
    compared, worst = 0, 0.0
    for f in range(n_frames):
        boxes, scores, who, feats = er.scene_detections(scene, f, lo, hi)
        keep = preprocessing.non_max_suppression(boxes, 0.6, scores)
        assert keep == g['nms_keep'][kp[f]:kp[f + 1]].tolist(), f'nms frame {f}'
        dets = [Detection(boxes[i], 'person', scores[i], feats[i]) for i in keep]
        trk.predict()
        before = [(t.track_id, t.is_confirmed()) for t in trk.tracks]
        trk.update(dets)
        np.testing.assert_array_equal(_table(trk), g['track_int'][fp[f]:fp[f + 1]], err_msg=f'frame {f}')
        if len(trk.tracks):
            np.testing.assert_allclose(np.array([t.mean for t in trk.tracks]), g['track_mean'][fp[f]:fp[f + 1]], rtol=1e-8, atol=1e-8,
                                       err_msg=f'frame {f}')
        if f in cost_frames:
            app, _ = trk.last_cost()
            rows = [r for r, (_, conf) in enumerate(before) if conf]          # confirmed rows only
            ids = g[f'cost_ids_{f}'].tolist()
            assert [before[r][0] for r in rows] == ids
            assert [len(ref.samples[i]) for i in ids] == g[f'cost_samples_{f}'].tolist()
            got, want = app[rows], g[f'cost_{f}']
            tol = ref.tolerance(np.array([d.feature for d in dets]), ids)
            live = got < 1e4                                                 # gated entries are 1e5 (linear_assignment.py:181-189)
            err = np.abs(got[live] - want[live]) / tol[live]
            assert got[live].min() >= 0.0 and np.all(err <= 1.0), (f, float(err.max()))
            worst = max(worst, float(err.max())); compared += int(live.sum())
        for t in trk.tracks:                                                 # every feature a track was founded or updated with
            if t.time_since_update == 0:
                ref.samples.setdefault(t.track_id, []).append(t.detections[-1].feature)
    print('scene %s: %d live appearance costs compared, worst %.3f tolerances' % (name, compared, worst))
    assert compared >= 20
    assert trk._next_id == int(g['next_id'])


@pytest.mark.parametrize('budget', [40])
def test_budget_ring_across_chunks_matches_oracle(budget):
    """nn_budget = 40 under the euclidean metric: a ring over two gallery chunks holding RAW rows, on a scene with births, deaths and
    misses -- track table every frame and the associated appearance costs equal the oracle tracker's with the test-side metric
    (the pattern of tests/test_gpu_tracker.py::test_budget_ring_across_chunks_matches_oracle)."""
    from deepdish_amd.deep_sort import nn_matching, preprocessing
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds
    scene = Scene(seed=17, n_obj=10, n_frames=150, p_miss=0.08)
    lo, hi = 0.6, 1.6
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric('euclidean', er.THRESHOLD, budget), max_iou_distance=0.7, max_age=8,
                  track_capacity=24, gallery_capacity=32)
    otrk = ds.Tracker(er.Metric(er.THRESHOLD, budget), max_iou_distance=0.7, max_age=8)
    compared, worst = 0, 0.0
    for f in range(150):
        boxes, scores, who, feats = er.scene_detections(scene, f, lo, hi)
        keep = preprocessing.non_max_suppression(boxes, 0.6, scores)
        trk.predict(); otrk.predict()
        ids = [t.track_id for t in otrk.tracks if t.state == 2]
        odets = [ds.Det(boxes[i], 'person', scores[i], feats[i]) for i in keep]
        q = np.array([d.feature for d in odets])
        want = otrk.metric.distance(q, ids) if ids and odets else None
        tol = otrk.metric.tolerance(q, ids) if want is not None else None
        before = [(t.track_id, t.is_confirmed()) for t in trk.tracks]
        trk.update([Detection(boxes[i], 'person', scores[i], feats[i]) for i in keep])
        otrk.update(odets)
        got_i = [(t.track_id, t.state, t.time_since_update, t.hits, t.age) for t in trk.tracks]
        assert got_i == [(t.track_id, t.state, t.time_since_update, t.hits, t.age) for t in otrk.tracks], f
        if want is not None:
            app, _ = trk.last_cost()
            rows = [r for r, (_, conf) in enumerate(before) if conf]
            assert [before[r][0] for r in rows] == ids
            got = app[rows]
            live = got < 1e4
            if live.any():
                assert got[live].min() >= 0.0
                worst = max(worst, float((np.abs(got[live] - want[live]) / tol[live]).max()))
                compared += int(live.sum())
    assert compared > 300 and worst <= 1.0, (compared, worst)
    assert trk._next_id > 12                                   # tracks died and were born: slots and chunks were recycled
    assert max(len(v) for v in otrk.metric.samples.values()) == budget


def test_track_update_stores_the_raw_row():
    """dd_tracker_track_update under the euclidean metric appends the feature as given: a detection that repeats it bit for bit
    then costs [0, tolerance] against the track; had the row been normalised on its way in the cost would be (1 - 0.5)^2 = 0.25."""
    from deepdish_amd.deep_sort import nn_matching
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    rng = np.random.default_rng(3)
    a = rng.standard_normal(128).astype(np.float32); a *= np.float32(1.5) / np.linalg.norm(a)
    b = rng.standard_normal(128).astype(np.float32); b *= np.float32(0.5) / np.linalg.norm(b)
    box = [100, 100, 40, 90]
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric('euclidean', 0.4, None), max_age=5, track_capacity=8, gallery_capacity=32)
    for _ in range(3):
        trk.predict(); trk.update([Detection(box, 'person', 0.9, a)])
    assert len(trk.tracks) == 1 and trk.tracks[0].is_confirmed()
    trk.tracks[0].update(trk.kf, Detection(box, 'person', 1.0, b))              # track.py:127-152 for this one track
    assert trk.tracks[0].hits == 4
    trk.predict(); trk.update([Detection(box, 'person', 0.9, b), Detection(box, 'person', 0.8, a)])
    app, _ = trk.last_cost()
    assert app.shape == (1, 2)
    stored = [a, a, a, b]
    want = er.nn_euclidean_distance(np.array(stored), np.array([b, a]))
    tol = er.tolerance(stored, [b, a])
    assert np.all(app[0] >= 0.0) and np.all(app[0] <= tol), (app, tol)          # both detections repeat a stored row
    assert np.all(np.abs(app[0] - want) <= tol)
    assert trk.tracks[0].hits == 5 and trk.tracks[0].time_since_update == 0


# The pipelines' encoder ends in an L2 normalisation, so there the squared distance is twice the cosine distance and the two metrics at
# one threshold part only where a track's cosine cost falls into (0.1, 0.2].  The synthetic encoder puts a moving object's consecutive
# crops well below 0.1, so the frames carry a lighting change: from frame `dim_from` on every frame is dimmed to 30 %, which moves a crop's
# feature by 0.12 .. 0.2 (cosine) from its lit self.  Tracks that miss a detection across the change are then re-found under the cosine
# metric and re-born under the euclidean one: on the CPU oracle all four streams differ from that frame on (next ids 24 / 33 / 36 / 38
# against 22 / 22 / 29 / 33 after 24 frames).
PIPE_SCENES = dict(base=60, n_obj=12, p_miss=0.25, frames=24, dim_from=12, dim=0.3)


def test_pipelines_under_the_euclidean_metric():
    """MultiStreamPipeline(4, metric='euclidean') with injected detections == four HotPath(metric='euclidean') on the same frames:
    track tables and counts, per stream (as tests/test_gpu_pipeline.py::test_multistream_pipeline_matches_oracle_per_stream compares
    them).  The same threshold under the cosine metric tracks differently on at least one stream, and dd_pipeline_metric after a
    step is DD_E_STATE."""
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    S, F = 4, PIPE_SCENES['frames']
    scenes = [Scene(seed=PIPE_SCENES['base'] + z, n_obj=PIPE_SCENES['n_obj'] + 2 * z, n_frames=F, p_miss=PIPE_SCENES['p_miss'])
              for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=False, metric='euclidean', max_cosine_distance=0.2)
    mc = MultiStreamPipeline(S, run_detector=False, metric='cosine', max_cosine_distance=0.2)
    hps = [HotPath(run_detector=False, metric='euclidean', max_cosine_distance=0.2) for _ in range(S)]
    assert mp.metric == 'euclidean' and hps[0].tracker.metric.metric == 'euclidean'
    differs = set()
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        if f >= PIPE_SCENES['dim_from']:
            frames = (frames * PIPE_SCENES['dim']).astype(np.uint8)
        frames = torch.from_numpy(frames).cuda()
        per = []
        for sc in scenes:
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]))
        mp.step(frames, mp.pack_injected(per))
        mc.step(frames, mc.pack_injected(per))
        for z, hp in enumerate(hps):
            hp.step(frames[z], injected=per[z])
            ints, means = mp.tracker(z).table()
            want = _table(hp.tracker)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-9, atol=1e-9)
            ci, _ = mc.tracker(z).table()
            if ci[:, :5].shape != want.shape or not np.array_equal(ci[:, :5], want):
                differs.add(z)
    got = mp.counts()
    for z, hp in enumerate(hps):
        np.testing.assert_array_equal(got[z], hp.counts())
    print('streams on which the cosine pipeline tracks differently: %s' % sorted(differs))
    assert differs, 'the cosine pipeline at the same threshold must track differently on at least one stream'
    assert lib().dd_pipeline_metric(mp._h, 0) == -3 and b'before the first step' in lib().dd_last_error()      # DD_E_STATE
    with pytest.raises(ValueError):
        MultiStreamPipeline(S, run_detector=False, metric='manhattan')


def _raw_run(handle, g, n_frames):
    """Drive a dd_tracker handle over scene n5's recorded inputs; -> per frame (ints6, means, confirmed rows of the appearance cost, IoU cost)."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    l = lib()
    kp = g['keep_ptr']
    out = []
    for f in range(n_frames):
        keep = g['nms_keep'][kp[f]:kp[f + 1]]
        tlwh = np.ascontiguousarray(g[f'boxes_{f}'][keep], dtype=np.float64).reshape(-1, 4)
        feats = np.ascontiguousarray(g[f'feats_{f}'][keep], dtype=np.float32).reshape(-1, 128)
        check(l.dd_tracker_predict(handle), 'dd_tracker_predict')
        n = ctypes.c_int()
        check(l.dd_tracker_count(handle, 0, ctypes.byref(n)), 'dd_tracker_count')
        pre = np.zeros((n.value, 6), dtype=np.int64)
        if n.value:
            check(l.dd_tracker_read(handle, 0, ptr(pre), None, None), 'dd_tracker_read')
        check(l.dd_tracker_update(handle, ptr(tlwh), ptr(feats), 0, len(tlwh)), 'dd_tracker_update')
        check(l.dd_tracker_count(handle, 0, ctypes.byref(n)), 'dd_tracker_count')
        ints, means = np.zeros((n.value, 6), dtype=np.int64), np.zeros((n.value, 8))
        if n.value:
            check(l.dd_tracker_read(handle, 0, ptr(ints), ptr(means), None), 'dd_tracker_read')
        r, c = ctypes.c_int(), ctypes.c_int()
        check(l.dd_tracker_last_cost(handle, None, None, 0, ctypes.byref(r), ctypes.byref(c)), 'dd_tracker_last_cost')
        app, iou = np.zeros((r.value, c.value)), np.zeros((r.value, c.value))
        if app.size:
            check(l.dd_tracker_last_cost(handle, ptr(app), ptr(iou), app.size, ctypes.byref(r), ctypes.byref(c)), 'dd_tracker_last_cost')
        out.append((ints, means, app[pre[:r.value, 1] == 2], iou))
    return out


def test_cosine_through_create_metric_is_bit_identical():
    """dd_tracker_create_metric(ctx, 0, ...) is dd_tracker_create: scene n5 through both handles gives the same bits -- track table,
    means, the confirmed rows of the appearance cost and the IoU cost of every frame -- and the reference's track table."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context
    g = np.load(os.path.join(G, 'scene_n5.npz'))
    ctx = default_context()
    l = lib()
    ha, hb = ctypes.c_void_p(), ctypes.c_void_p()
    check(l.dd_tracker_create(ctx.handle, 0.2, 0.7, int(g['max_age']), 3, 0, 64, 256, ctypes.byref(ha)), 'dd_tracker_create')
    check(l.dd_tracker_create_metric(ctx.handle, 0, 0.2, 0.7, int(g['max_age']), 3, 0, 64, 256, ctypes.byref(hb)), 'dd_tracker_create_metric')
    try:
        F = int(g['n_frames'])
        ra, rb = _raw_run(ha, g, F), _raw_run(hb, g, F)
        fp = g['frame_ptr']
        costs = 0
        for f, (x, y) in enumerate(zip(ra, rb)):
            for u, v in zip(x, y):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), f
            np.testing.assert_array_equal(x[0][:, :5], g['track_int'][fp[f]:fp[f + 1]], err_msg=f'frame {f}')
            costs += x[2].size
        assert costs > 100
    finally:
        l.dd_tracker_destroy(ha); l.dd_tracker_destroy(hb)
