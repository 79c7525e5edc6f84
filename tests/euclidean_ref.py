"""TEST INFRASTRUCTURE ONLY -- the reference's "euclidean" nearest-neighbour metric restated for the tests
(upstream deep_sort/nn_matching.py:5-28 _pdist, :57-75 _nn_euclidean_distance, :99-177 the metric class), the
per-detection feature scaling the euclidean scenes use, and the tolerance the costs are compared at.

Parity of this file against the real reference is pinned by tests/golden/euclidean.npz and
tests/golden/scene_euclid_*.npz (scripts/make_golden_euclidean.py imports the reference's own modules to write
them); tests/test_euclidean_ref.py checks it on the CPU.
"""
import numpy as np

# |got - want| <= TOL * (max_g |g|^2 + |q|^2) per entry, the maximum over the target's stored rows: the cosine tolerance of
# tests/test_gpu_deepsort.py (2e-6 on 1 - a.b for unit vectors) carried over to |a|^2 + |b|^2 - 2 a.b
TOL = 2e-6

# name -> (Scene keywords, n_frames, max_age, (lo, hi) of the feature scales, frames whose cost matrices are recorded)
SCENES = {
    'euclid_n20_age5': (dict(seed=3, n_obj=20, n_frames=100, p_miss=0.1), 100, 5, (0.6, 1.6), (20, 45, 70, 99)),
    'euclid_n12': (dict(seed=5, n_obj=12, n_frames=80, p_miss=0.25), 80, 30, (0.5, 2.0), (15, 35, 55, 79)),
}
THRESHOLD = 0.4          # matching_threshold of both scenes (on the squared distance)


def pdist(a, b):
    """nn_matching.py:5-28: pair-wise SQUARED distance, in the dtype of the inputs (f32 for f32 rows)."""
    a, b = np.asarray(a), np.asarray(b)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    a2, b2 = np.square(a).sum(axis=1), np.square(b).sum(axis=1)
    r2 = -2. * np.dot(a, b.T) + a2[:, None] + b2[None, :]
    return np.clip(r2, 0., float(np.inf))


def nn_euclidean_distance(x, y):
    """nn_matching.py:57-75: for every query row of y the smallest squared distance to a sample of x."""
    return np.maximum(0.0, pdist(x, y).min(axis=0))


def nn_euclidean_distance_f64(x, y):
    """The same quantity evaluated exactly (differences in f64): what the tolerance is measured around."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return ((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2).min(axis=0)


def tolerance(samples, queries):
    """TOL * (max_g |g|^2 + |q|^2) for every query row against one target's stored rows."""
    g2 = np.square(np.asarray(samples, dtype=np.float64)).sum(axis=1).max()
    q2 = np.square(np.asarray(queries, dtype=np.float64)).sum(axis=1)
    return TOL * (g2 + q2)


class Metric:
    """nn_matching.py:99-177 with metric == "euclidean": the interface oracle.deepsort_np.Tracker expects."""

    def __init__(self, matching_threshold, budget=None, nn=nn_euclidean_distance):
        self.matching_threshold = matching_threshold
        self.budget = budget
        self.samples = {}
        self._nn = nn

    def partial_fit(self, features, targets, active_targets):
        for f, t in zip(features, targets):
            self.samples.setdefault(t, []).append(f)
            if self.budget is not None:
                self.samples[t] = self.samples[t][-self.budget:]
        self.samples = {k: self.samples[k] for k in active_targets}

    def distance(self, features, targets):
        cost = np.zeros((len(targets), len(features)))
        for r, t in enumerate(targets):
            cost[r, :] = self._nn(self.samples[t], features)
        return cost

    def tolerance(self, features, targets):
        """[len(targets), len(features)] tolerances of distance()'s entries."""
        return np.array([tolerance(self.samples[t], features) for t in targets]).reshape(len(targets), len(features))


def scale_features(feats, f, lo, hi):
    """The euclidean scenes' inputs: frame f's detection features (unit rows from deepdish_amd.synth.Scene), each multiplied
    by its own scale BEFORE NMS -- so the metric sees un-normalised rows and differs from the cosine one."""
    feats = np.asarray(feats, dtype=np.float32)
    scale = np.random.default_rng(1000 + f).uniform(lo, hi, (len(feats), 1)).astype(np.float32)
    return feats * scale


def scene_detections(scene, f, lo, hi):
    """Scene.detections(f) with the scaled features."""
    boxes, scores, who, feats = scene.detections(f)
    return boxes, scores, who, scale_features(feats, f, lo, hi)
