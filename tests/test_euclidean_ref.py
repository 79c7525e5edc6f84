"""CPU: the test-side restatement of the reference's euclidean metric (tests/euclidean_ref.py) against the fixtures the
reference itself produced (scripts/make_golden_euclidean.py): _pdist / _nn_euclidean_distance / metric.distance values, and both
euclidean scenes through oracle.deepsort_np.Tracker; and the metric names NearestNeighborDistanceMetric accepts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import euclidean_ref as er  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def fix():
    g = np.load(os.path.join(G, 'euclidean.npz'))
    return {k: g[k] for k in g.files}


def test_fixture_holds_the_stated_cases(fix):
    sizes = fix['gallery_sizes'].tolist()
    assert len(sizes) == 12 and set(sizes) >= {1, 15, 16, 17, 31, 32, 33, 64, 65}
    assert fix['query_counts'].tolist() == [1, 15, 16, 17, 63, 64, 65]
    assert fix['gallery'].shape == (sum(sizes), 128) and fix['gallery'].dtype == np.float32
    norms = np.linalg.norm(fix['gallery'], axis=1)
    assert 0.05 <= norms.min() < 0.2 and 1.8 < norms.max() <= 2.0 + 1e-6
    qi, _, row = fix['equal_query'].tolist()
    assert fix['query'][qi].tobytes() == fix['gallery'][row].tobytes()              # one query bit-equal to a gallery row
    near = np.linalg.norm(fix['query'][1:9] - fix['gallery'][fix['dup_rows']], axis=1)
    assert np.all(near > 0) and np.all(near < 0.01 * np.sqrt(128) * 1.5)              # row + 0.01 N


def test_restatement_equals_the_reference_values(fix):
    off = np.concatenate([[0], np.cumsum(fix['gallery_sizes'])])
    a, b = fix['gallery'][off[8]:off[9]], fix['query'][:17]
    got = er.pdist(a, b)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, fix['pdist'])
    np.testing.assert_array_equal(er.nn_euclidean_distance(a, b), fix['nn'])
    m = er.Metric(0.4)
    targets = np.repeat(np.arange(1, 13), fix['gallery_sizes'])
    m.partial_fit(fix['gallery'], targets, list(range(1, 13)))
    for n in fix['query_counts']:
        q = fix['query'][:n]
        want = fix[f'nn_cost_{n}']
        got = m.distance(q, list(range(1, 13)))
        np.testing.assert_array_equal(got, want)
        assert got.min() >= 0.0
        exact = np.array([er.nn_euclidean_distance_f64(m.samples[t], q) for t in range(1, 13)])
        assert np.all(np.abs(want - exact) <= m.tolerance(q, list(range(1, 13))))      # the reference sits inside the stated tolerance


def test_metric_budget_keeps_the_last_samples():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((9, 128)).astype(np.float32)
    m = er.Metric(0.4, budget=4)
    m.partial_fit(rows, [7] * 9, [7])
    assert len(m.samples[7]) == 4 and all(np.array_equal(a, b) for a, b in zip(m.samples[7], rows[-4:]))
    np.testing.assert_array_equal(m.distance(rows[:2], [7])[0], er.nn_euclidean_distance(rows[-4:], rows[:2]))
    m.partial_fit(rows[:1], [8], [8])
    assert list(m.samples) == [8]


def test_scale_helper_is_seeded_per_frame():
    f = np.ones((5, 128), np.float32)
    a, b = er.scale_features(f, 3, 0.5, 2.0), er.scale_features(f, 3, 0.5, 2.0)
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, er.scale_features(f, 4, 0.5, 2.0))
    want = np.random.default_rng(1003).uniform(0.5, 2.0, (5, 1)).astype(np.float32)
    np.testing.assert_array_equal(a, f * want)
    assert a.min() >= 0.5 and a.max() <= 2.0


@pytest.mark.parametrize('name', sorted(er.SCENES))
def test_oracle_tracker_with_the_euclidean_metric_reproduces_the_scene(name):
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds
    g = np.load(os.path.join(G, f'scene_{name}.npz'))
    kw, n_frames, max_age, (lo, hi), cost_frames = er.SCENES[name]
    assert (int(g['n_frames']), int(g['max_age']), float(g['scale_lo']), float(g['scale_hi'])) == (n_frames, max_age, lo, hi)
    scene = Scene(**kw)
    trk = ds.Tracker(er.Metric(float(g['threshold'])), max_iou_distance=0.7, max_age=max_age)
    fp, kp = g['frame_ptr'], g['keep_ptr']
    seen = 0
    for f in range(n_frames):
        boxes, scores, who, feats = er.scene_detections(scene, f, lo, hi)
        keep = ds.non_max_suppression(boxes, 0.6, scores)
        assert keep == g['nms_keep'][kp[f]:kp[f + 1]].tolist(), f'nms frame {f}'
        dets = [ds.Det(boxes[i], 'person', scores[i], feats[i]) for i in keep]
        trk.predict()
        if f in cost_frames:
            ids = [t.track_id for t in trk.tracks if t.is_confirmed()]
            assert ids == g[f'cost_ids_{f}'].tolist()
            assert [len(trk.metric.samples[i]) for i in ids] == g[f'cost_samples_{f}'].tolist()
            np.testing.assert_array_equal(trk.metric.distance(np.array([d.feature for d in dets]), ids), g[f'cost_{f}'])
            seen += 1
        trk.update(dets)
        got = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in trk.tracks], dtype=np.int64).reshape(-1, 5)
        np.testing.assert_array_equal(got, g['track_int'][fp[f]:fp[f + 1]], err_msg=f'frame {f}')
        if len(got):
            np.testing.assert_allclose(np.array([t.mean for t in trk.tracks]), g['track_mean'][fp[f]:fp[f + 1]], rtol=1e-8, atol=1e-8)
    assert trk._next_id == int(g['next_id']) and seen == 4


def test_metric_names():
    """nn_matching.py:126-132: "euclidean" and "cosine" construct, anything else is the reference's ValueError.  Needs no GPU."""
    from deepdish_amd.deep_sort.nn_matching import NearestNeighborDistanceMetric
    e = NearestNeighborDistanceMetric('euclidean', 0.4, 7)
    c = NearestNeighborDistanceMetric('cosine', 0.2, None)
    assert (e.metric, e.kind, e.matching_threshold, e.budget) == ('euclidean', 1, 0.4, 7)
    assert (c.metric, c.kind, c.budget) == ('cosine', 0, None)
    rows = np.arange(3 * 128, dtype=np.float32).reshape(3, 128)
    e.partial_fit(rows, [1, 1, 2], [1])                                                   # partial_fit is the metric-independent one
    assert list(e.samples) == [1] and len(e.samples[1]) == 2
    with pytest.raises(ValueError, match="Invalid metric; must be either 'euclidean' or 'cosine'"):
        NearestNeighborDistanceMetric('manhattan', 0.4, None)


def test_pipelines_refuse_unknown_metric_names():
    """HotPath / MultiStreamPipeline take metric='cosine' | 'euclidean'; the name is checked before any device work."""
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.multipipe import MultiStreamPipeline
    for cls, args in ((HotPath, ()), (MultiStreamPipeline, (2,))):
        with pytest.raises(ValueError, match="must be either 'euclidean' or 'cosine'"):
            cls(*args, metric='manhattan')
