#!/usr/bin/env python3
"""Generate tests/golden/cascade_cases.npz by running the REFERENCE's own deep_sort/linear_assignment.py (min_cost_matching :11-75,
matching_cascade :78-141) under the glue of deep_sort/tracker.py:95-133 (_match), restated below.

Runs only where the reference tree is (DEEPDISH_REFERENCE, as scripts/make_golden.py, whose numpy shims this uses); what it writes is
plain data.  The inputs come from tests/cascade_cases.py: a case is (seed, T, n, kind, max_age), the test regenerates the matrices
from it and checks them against the digest stored here.  Stub tracks carry time_since_update and is_confirmed(); the distance
metrics index the case's matrices.  Stored per case: the three lists the tracker acts on -- matches, unmatched tracks, unmatched
detections -- in the order the reference builds them.  (tracker.py:132 passes the unmatched tracks through set() once more; that only
reorders a list whose order nothing reads, and it is stored here as unmatched_tracks_a + unmatched_tracks_b.)
"""
import io
import os
import sys
import types
import zipfile
import numpy as np

REF = os.environ.get('DEEPDISH_REFERENCE', '/root/reference')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

np.float = float
np.int = int
sys.modules.setdefault('cv2', types.ModuleType('cv2'))
sys.path.insert(0, REF)

from deep_sort import linear_assignment  # noqa: E402

import cascade_cases as cc  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'cascade_cases.npz')


class StubTrack:
    def __init__(self, state, tsu):
        self.state, self.time_since_update = int(state), int(tsu)

    def is_confirmed(self):
        return self.state == cc.CONFIRMED


def indexer(matrix):
    def distance_metric(tracks, dets, track_indices, detection_indices):
        return matrix[np.ix_(list(track_indices), list(detection_indices))].copy()      # min_cost_matching clamps it in place (:57)
    return distance_metric


def match(app, iou, state, tsu, max_cos, max_iou, max_age):
    """tracker.py:95-133 with the two metrics replaced by look-ups; also returns len(confirmed), len(matches_a) for the set branch."""
    tracks = [StubTrack(s, t) for s, t in zip(state, tsu)]
    detections = list(range(app.shape[1]))
    confirmed_tracks = [i for i, t in enumerate(tracks) if t.is_confirmed()]
    unconfirmed_tracks = [i for i, t in enumerate(tracks) if not t.is_confirmed()]
    matches_a, unmatched_tracks_a, unmatched_detections = linear_assignment.matching_cascade(
        indexer(app), max_cos, max_age, tracks, detections, confirmed_tracks)
    n_a = len(matches_a)
    iou_track_candidates = unconfirmed_tracks + [k for k in unmatched_tracks_a if tracks[k].time_since_update == 1]
    unmatched_tracks_a = [k for k in unmatched_tracks_a if tracks[k].time_since_update != 1]
    matches_b, unmatched_tracks_b, unmatched_detections = linear_assignment.min_cost_matching(
        indexer(iou), max_iou, tracks, detections, iou_track_candidates, unmatched_detections)
    matches = matches_a + matches_b
    return ([(int(r), int(c)) for r, c in matches], [int(k) for k in list(unmatched_tracks_a) + list(unmatched_tracks_b)],
            [int(d) for d in unmatched_detections], len(confirmed_tracks), n_a)


def case_list():
    cases, seed = [], 1000
    rng = np.random.default_rng(99)
    for kind in range(4):                                   # T, n in 1 .. 15
        for _ in range(18):
            T, n = (int(v) for v in rng.integers(1, 16, 2))
            cases.append((seed, T, n, kind, 10)); seed += 1
    for T, n in ((63, 63), (64, 64), (65, 65), (64, 70), (70, 64)):      # around the wave width
        for kind in (0, 1, 2):
            cases.append((seed, T, n, kind, 10)); seed += 1
    cases.append((seed, 40, 33, 3, 10)); seed += 1
    cases.append((seed, 30, 30, 0, 3)); seed += 1          # a cascade shorter than the tracks' ages: levels beyond it never run
    cases.append((seed, 256, 256, 2, 10))                   # the device cap
    return cases


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


def main():
    cases = case_list()
    digests, states, tsus, row_ptr = [], [], [], [0]
    ms, mp, urs, up, uds, dp = [], [0], [], [0], [], [0]
    copy_branch = other_branch = multi_level = 0
    for seed, T, n, kind, max_age in cases:
        app, iou, state, tsu = cc.make_case(seed, T, n, kind, max_age)
        max_cos, max_iou = cc.thresholds(kind)
        m, ur, ud, n_conf, n_a = match(app, iou, state, tsu, max_cos, max_iou, max_age)
        assert sorted([r for r, _ in m] + ur) == list(range(T)) and sorted([d for _, d in m] + ud) == list(range(n))
        if n_conf // 4 > n_a:                               # set_copy_and_difference: len(a) / 4 > len(b)
            copy_branch += 1
        elif n_conf:
            other_branch += 1
        multi_level += len(set(tsu[state == cc.CONFIRMED].tolist())) >= 3
        digests.append(cc.digest(app, iou, state, tsu))
        states += state.tolist(); tsus += tsu.tolist(); row_ptr.append(len(states))
        ms += [v for pair in m for v in pair]; mp.append(len(ms))
        urs += ur; up.append(len(urs))
        uds += ud; dp.append(len(uds))
    assert copy_branch >= 10 and other_branch >= 10, (copy_branch, other_branch)
    assert multi_level >= 20, multi_level
    save_npz(OUT, cases=np.array(cases, dtype=np.int64), input_digest=np.array(digests, dtype=np.uint64),
             state=np.array(states, dtype=np.int32), tsu=np.array(tsus, dtype=np.int32), row_ptr=np.array(row_ptr, dtype=np.int64),
             matches=np.array(ms, dtype=np.int32), match_ptr=np.array(mp, dtype=np.int64),
             un_rows=np.array(urs, dtype=np.int32), un_rows_ptr=np.array(up, dtype=np.int64),
             un_dets=np.array(uds, dtype=np.int32), un_dets_ptr=np.array(dp, dtype=np.int64))
    print(f'{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes; set difference by copy-and-discard in {copy_branch} cases, '
          f'by re-insertion in {other_branch}; {multi_level} cases with confirmed tracks on three or more cascade levels')


if __name__ == '__main__':
    main()
