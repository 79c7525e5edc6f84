#!/usr/bin/env python3
"""Generate the euclidean-metric fixtures under tests/golden/ by running the REFERENCE's own modules
(deep_sort/nn_matching.py:5-28,57-75,99-177 and deep_sort/tracker.py): euclidean.npz and scene_euclid_*.npz.

Runs only where the reference tree is (DEEPDISH_REFERENCE, as scripts/make_golden.py, whose shims and per-frame driver
this follows); what it writes is plain data.  The scenes are deepdish_amd.synth scenes whose detection features are
scaled per detection (tests/euclidean_ref.py: scale_features), so the euclidean metric sees un-normalised rows.

Before anything is written the script asserts, per scene, that
  * the track tables differ from a cosine-0.2 run of the same inputs (an implementation that normalises fails them),
  * they are identical when the metric is evaluated exactly in f64,
  * they stay identical under +-1 tolerance of noise on every appearance cost, over 8 seeds,
  * every appearance cost the tracker reads lies at least 100 tolerances from the matching threshold.
"""
import os
import sys
import io
import types
import hashlib
import zipfile
import numpy as np

REF = os.environ.get('DEEPDISH_REFERENCE', '/root/reference')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

np.float = float
np.int = int
sys.modules.setdefault('cv2', types.ModuleType('cv2'))
sys.path.insert(0, REF)

from deep_sort import nn_matching, preprocessing  # noqa: E402
from deep_sort.tracker import Tracker  # noqa: E402
from deep_sort.detection import Detection  # noqa: E402

from deepdish_amd.synth import Scene  # noqa: E402
import euclidean_ref as er  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
os.makedirs(OUT, exist_ok=True)

GALLERY_SIZES = (1, 15, 16, 17, 31, 32, 33, 64, 65, 2, 3, 47)       # 12 targets: around the 16-row tile and the 32-row chunk
QUERY_COUNTS = (1, 15, 16, 17, 63, 64, 65)                          # around the wave's 16 and the block's 64 detections


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint64)[0]


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed member time stamp: re-running the script reproduces the file byte for byte."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ----------------------------------------------------------------------------- per-function
def golden_euclidean(seed=23):
    rng = np.random.default_rng(seed)
    ident = rng.standard_normal((12, 128)).astype(np.float32)
    rows, targets = [], []
    for t, g in enumerate(GALLERY_SIZES):
        f = ident[t] + 0.05 * rng.standard_normal((g, 128)).astype(np.float32)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        f *= rng.uniform(0.05, 2.0, (g, 1)).astype(np.float32)              # row norms 0.05 .. 2
        rows.append(f.astype(np.float32)); targets += [t + 1] * g
    gal = np.concatenate(rows)
    nq = max(QUERY_COUNTS)
    q = ident[rng.integers(0, 12, nq)] + 0.05 * rng.standard_normal((nq, 128)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = (q * rng.uniform(0.05, 2.0, (nq, 1))).astype(np.float32)
    # the query counts are prefixes of q: row 0 is bit-equal to a gallery row (of target 8, 64 rows), rows 1..8 are
    # near-duplicates of gallery rows (row + 0.01 N) of eight different targets
    off = np.concatenate([[0], np.cumsum(GALLERY_SIZES)])
    equal_row = int(off[7] + 40)
    q[0] = gal[equal_row]
    dup_rows = [int(off[t] + rng.integers(0, GALLERY_SIZES[t])) for t in (1, 2, 3, 4, 5, 6, 8, 11)]
    q[1:9] = gal[dup_rows] + np.float32(0.01) * rng.standard_normal((8, 128)).astype(np.float32)
    norms = np.linalg.norm(gal, axis=1)
    assert 0.05 <= norms.min() and norms.max() <= 2.0 + 1e-6, (norms.min(), norms.max())
    metric = nn_matching.NearestNeighborDistanceMetric('euclidean', 0.4, None)
    metric.partial_fit(gal, np.array(targets), list(range(1, 13)))
    out = dict(gallery=gal, gallery_sizes=np.array(GALLERY_SIZES, dtype=np.int64), query=q,
               query_counts=np.array(QUERY_COUNTS, dtype=np.int64), equal_query=np.array([0, 8, equal_row], dtype=np.int64),
               dup_rows=np.array(dup_rows, dtype=np.int64))
    a, b = gal[off[8]:off[9]], q[:17]                                        # 65 rows against 17 queries
    out['pdist'] = nn_matching._pdist(a, b)
    out['nn'] = nn_matching._nn_euclidean_distance(a, b)
    assert out['pdist'].dtype == np.float32 and out['nn'].dtype == np.float32
    for n in QUERY_COUNTS:
        c = metric.distance(q[:n], list(range(1, 13)))
        assert c.shape == (12, n) and c.min() >= 0.0
        exact = np.array([er.nn_euclidean_distance_f64(gal[off[t]:off[t + 1]], q[:n]) for t in range(12)])
        tol = np.array([er.tolerance(gal[off[t]:off[t + 1]], q[:n]) for t in range(12)])
        assert np.all(np.abs(c - exact) <= tol), 'the reference itself must sit inside the stated tolerance'
        out[f'nn_cost_{n}'] = c
    assert out['nn_cost_65'][7, 0] <= er.tolerance(gal[off[7]:off[8]], q[:1])[0]
    save_npz(os.path.join(OUT, 'euclidean.npz'), **out)


# ----------------------------------------------------------------------------- sequence level
class RecordingMetric(nn_matching.NearestNeighborDistanceMetric):
    """The reference metric; distance() optionally evaluated in f64 or perturbed, and the margins of what it returns recorded."""

    def __init__(self, name, thr, exact=False, noise_seed=None):
        super().__init__(name, thr, None)
        self.exact = exact
        self.rng = np.random.default_rng(noise_seed) if noise_seed is not None else None
        self.min_margin = np.inf                       # min |cost - threshold| / tolerance over every entry read

    def distance(self, features, targets):
        cost = super().distance(features, targets)
        if self._metric is not nn_matching._nn_euclidean_distance:
            return cost
        tol = np.array([er.tolerance(self.samples[t], features) for t in targets]).reshape(cost.shape)
        if self.exact:
            cost = np.array([er.nn_euclidean_distance_f64(self.samples[t], features) for t in targets]).reshape(cost.shape)
        if self.rng is not None:
            cost = np.maximum(0.0, cost + self.rng.uniform(-1.0, 1.0, cost.shape) * tol)
        if cost.size:
            self.min_margin = min(self.min_margin, float((np.abs(cost - self.matching_threshold) / tol).min()))
        return cost


def run_scene(scene, n_frames, max_age, lo, hi, metric, cost_frames=()):
    tracker = Tracker(metric, max_iou_distance=0.7, max_age=max_age)          # deepdish.py:517
    rows, frame_ptr, keeps, keep_ptr, sums = [], [0], [], [0], []
    extra = {}
    for f in range(n_frames):
        boxes, scores, who, feats = er.scene_detections(scene, f, lo, hi)
        sums.append(digest(boxes, scores, feats))
        keep = preprocessing.non_max_suppression(boxes, 0.6, scores)          # deepdish.py:995
        keeps += list(keep); keep_ptr.append(len(keeps))
        dets = [Detection(boxes[i], 'person', scores[i], feats[i]) for i in keep]   # deepdish.py:1014
        tracker.predict()                                                     # deepdish.py:1028
        if f in cost_frames:       # what tracker._match's gated_metric reads from the metric (tracker.py:98-101)
            ids = [t.track_id for t in tracker.tracks if t.is_confirmed()]
            extra[f'cost_{f}'] = nn_matching.NearestNeighborDistanceMetric.distance(metric, np.array([d.feature for d in dets]), ids)
            extra[f'cost_ids_{f}'] = np.array(ids, dtype=np.int64)
            extra[f'cost_samples_{f}'] = np.array([len(metric.samples[i]) for i in ids], dtype=np.int64)
        tracker.update(dets)                                                  # deepdish.py:1029
        for t in tracker.tracks:
            rows.append([t.track_id, t.state, t.time_since_update, t.hits, t.age] + list(t.mean))
        frame_ptr.append(len(rows))
    rows = np.array(rows, dtype=np.float64).reshape(-1, 13)
    return dict(track_int=rows[:, :5].astype(np.int64), track_mean=rows[:, 5:], frame_ptr=np.array(frame_ptr),
                nms_keep=np.array(keeps, dtype=np.int64), keep_ptr=np.array(keep_ptr),
                input_digest=np.array(sums, dtype=np.uint64), next_id=tracker._next_id, **extra)


def frames_differing(a, b, n_frames):
    out = []
    for f in range(n_frames):
        x = a['track_int'][a['frame_ptr'][f]:a['frame_ptr'][f + 1]]
        y = b['track_int'][b['frame_ptr'][f]:b['frame_ptr'][f + 1]]
        if x.shape != y.shape or not np.array_equal(x, y):
            out.append(f)
    return out


def golden_scene_euclidean(name):
    kw, n_frames, max_age, (lo, hi), cost_frames = er.SCENES[name]
    scene = Scene(**kw)
    run = lambda metric, cf=(): run_scene(scene, n_frames, max_age, lo, hi, metric, cf)
    m = RecordingMetric('euclidean', er.THRESHOLD)
    gold = run(m, cost_frames)
    for f in cost_frames:
        assert gold[f'cost_{f}'].size > 0, f'frame {f} records no appearance cost: pick another'
    cos = run(RecordingMetric('cosine', 0.2))
    diff = frames_differing(gold, cos, n_frames)
    assert diff, 'the euclidean run must differ from the cosine-0.2 run of the same inputs'
    exact = run(RecordingMetric('euclidean', er.THRESHOLD, exact=True))
    assert not frames_differing(gold, exact, n_frames) and gold['next_id'] == exact['next_id'], 'f64 evaluation changes the tracks'
    np.testing.assert_array_equal(gold['track_mean'], exact['track_mean'])
    for seed in range(8):
        noisy = run(RecordingMetric('euclidean', er.THRESHOLD, noise_seed=seed))
        assert not frames_differing(gold, noisy, n_frames) and gold['next_id'] == noisy['next_id'], f'noise seed {seed} changes the tracks'
        np.testing.assert_array_equal(gold['track_mean'], noisy['track_mean'])
    assert m.min_margin >= 100.0, m.min_margin
    save_npz(os.path.join(OUT, f'scene_{name}.npz'), seed=scene.seed, n_obj=scene.n_obj, W=scene.W, H=scene.H,
                        n_frames=n_frames, max_age=max_age, scale_lo=lo, scale_hi=hi, threshold=er.THRESHOLD, **gold)
    print(f'scene_{name}: frames={n_frames} rows={len(gold["track_int"])} next_id={gold["next_id"]}; differs from cosine 0.2 in '
          f'{len(diff)} frames (first {diff[0]}); closest appearance cost {m.min_margin:.0f} tolerances from the threshold')


if __name__ == '__main__':
    golden_euclidean()
    for name in er.SCENES:
        golden_scene_euclidean(name)
    for fn in ('euclidean.npz',) + tuple(f'scene_{n}.npz' for n in er.SCENES):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))
