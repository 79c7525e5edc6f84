"""NearestNeighborDistanceMetric (deep_sort/nn_matching.py:99-177 upstream), "cosine" and "euclidean".

Stand-alone use (partial_fit / distance) runs csrc/cost.hip's exact-f32 MFMA kernels on a gallery
uploaded per call: 1 - max cosine of the normalised rows, or the minimum squared euclidean distance of
the rows as they are (nn_matching.py:5-28,57-75).  When handed to `Tracker`, only the metric's kind,
matching_threshold and budget are read: the tracker keeps its own gallery resident in HBM.
"""
import numpy as np
import torch

from .._lib import lib, check
from ..runtime import default_context, ptr


METRIC_KINDS = {'cosine': 0, 'euclidean': 1}


def metric_kind(name):
    """'cosine' / 'euclidean' -> the C ABI's metric number; anything else is the reference's ValueError."""
    if name not in METRIC_KINDS:
        raise ValueError("Invalid metric; must be either 'euclidean' or 'cosine'")
    return METRIC_KINDS[name]


class NearestNeighborDistanceMetric(object):
    def __init__(self, metric, matching_threshold, budget=None):
        self.kind = metric_kind(metric)                         # nn_matching.py:126-132; what dd_tracker_create_metric takes
        self.metric = metric
        self.matching_threshold = matching_threshold
        self.budget = budget
        self.samples = {}

    def partial_fit(self, features, targets, active_targets):
        for feature, target in zip(features, targets):
            self.samples.setdefault(target, []).append(np.asarray(feature, dtype=np.float32))
            if self.budget is not None:
                self.samples[target] = self.samples[target][-self.budget:]
        self.samples = {k: self.samples[k] for k in active_targets}

    def distance(self, features, targets, context=None):
        ctx = context or default_context()
        feats = np.asarray(features, dtype=np.float32).reshape(-1, 128)
        nt, nd = len(targets), len(feats)
        if nt == 0 or nd == 0:
            return np.zeros((nt, nd))
        offsets = np.zeros(nt + 1, dtype=np.int32)
        rows = []
        for i, t in enumerate(targets):
            rows += list(self.samples[t])
            offsets[i + 1] = len(rows)
        gal = ctx.to_device(np.asarray(rows, dtype=np.float32).reshape(-1, 128))
        df = ctx.to_device(feats)
        out = ctx.empty((nt, nd), torch.float64)
        name = 'dd_euclidean_nn_cost' if self.metric == 'euclidean' else 'dd_cosine_nn_cost'
        check(getattr(lib(), name)(ctx.handle, ptr(gal), ptr(offsets), nt, ptr(df), nd, ptr(out), None), name)
        return ctx.to_host(out)
