"""CPU: the test-side restatement of --object-detector-skip-frames (tests/skip_frames_ref.py) on hand-worked cases -- the detector
schedule (deepdish.py:892,929-938) and the zip() pairing of a skipped frame's boxes with the last encoder call's rows (:1003-1014) --
and what wire.initialisation_payload reports for the flag."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skip_frames_ref as ref  # noqa: E402


@pytest.mark.parametrize('n,want', [
    (None, [1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (-1, [1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (0, [1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (1, [1, 0, 1, 0, 1, 0, 1, 0, 1]),
    (3, [1, 0, 0, 0, 1, 0, 0, 0, 1]),
])
def test_schedule(n, want):
    assert ref.schedule(n, len(want)) == [bool(v) for v in want]


def test_pair_truncates_to_the_shorter_list():
    boxes, labels, scores = [(1, 1, 2, 2), (5, 5, 2, 2), (9, 9, 2, 2)], ['a', 'b', 'c'], [0.9, 0.8, 0.7]
    rows = np.arange(2 * 128, dtype=np.float32).reshape(2, 128)
    got = ref.pair(boxes, labels, scores, rows)
    assert [g[:3] for g in got] == [((1, 1, 2, 2), 'a', 0.9), ((5, 5, 2, 2), 'b', 0.8)]
    np.testing.assert_array_equal(np.stack([g[3] for g in got]), rows)
    assert len(ref.pair(boxes[:1], labels[:1], scores[:1], rows)) == 1
    assert ref.pair(boxes, labels, scores, np.array([])) == []


A, B = (10, 10, 20, 40), (100, 10, 20, 40)          # disjoint: NMS keeps both, A first (higher score)


def _onehot_encoder(frame, boxes):
    """A feature row that names its box: a one-hot at the box's x."""
    out = np.zeros((len(boxes), 128), np.float32)
    for i, b in enumerate(boxes):
        out[i, int(b[0]) % 128] = 1.0
    return out


def _mask(*moving):
    m = np.zeros((480, 640), np.uint8)
    for x, y, w, h in moving:
        m[y:y + h, x:x + w] = 255
    return m


def _run(mask0, mask1):
    """Frame 0 runs the detector on {A, B}; frame 1 is skipped (n = 1) and is handed a different detection that it must ignore."""
    s = ref.Stream(_onehot_encoder, [[320, 0], [320, 480]], n=1, ratio=0.25)
    frame = np.zeros((480, 640, 3), np.uint8)
    sk0, kept0, dets0 = s.step(frame, ([A, B], ['person'] * 2, [0.9, 0.8]), mask0)
    sk1, kept1, dets1 = s.step(frame, ([(300, 300, 30, 30)], ['person'], [0.99]), mask1)
    assert (sk0, sk1) == (False, True)
    return kept0, dets0, kept1, dets1


def test_skipped_frame_with_more_boxes_than_feature_rows():
    kept0, dets0, kept1, dets1 = _run(_mask(A), _mask(A, B))            # B has no motion on the detector frame
    assert kept0 == [A] and kept1 == [A, B]
    assert len(dets1) == 1 and tuple(dets1[0].tlwh) == A and dets1[0].feature[A[0]] == 1.0


def test_skipped_frame_with_fewer_boxes_pairs_by_position():
    kept0, dets0, kept1, dets1 = _run(_mask(A, B), _mask(B))            # A has no motion on the skipped frame
    assert kept0 == [A, B] and kept1 == [B]
    # the reference's quirk: B takes row 0, which the encoder computed for A
    assert len(dets1) == 1 and tuple(dets1[0].tlwh) == B and dets1[0].feature[A[0]] == 1.0 and dets1[0].feature[B[0] % 128] == 0.0


def test_skipped_frame_after_an_encoder_call_without_boxes():
    kept0, dets0, kept1, dets1 = _run(_mask(), _mask(A, B))
    assert kept0 == [] and dets0 == [] and kept1 == [A, B] and dets1 == []


def test_initialisation_payload_reports_the_hot_paths_skip_frames():
    from deepdish_amd import wire
    hp = SimpleNamespace(object_detector=SimpleNamespace(width=300, height=300, num_threads=4),
                         encoder=SimpleNamespace(image_encoder=object(), width=32, height=64),
                         tracker=SimpleNamespace(max_age=60, max_iou_distance=0.7, metric=SimpleNamespace(matching_threshold=0.2)),
                         nms_max_overlap=0.6, background_subtraction=False, background_subtraction_ratio=0.25,
                         object_detector_skip_frames=2)
    args = ('2026', 'acp', hp, 'model', 'enc', 'input')
    assert wire.initialisation_payload(*args)['object_detector_skip_frames'] == 2
    assert wire.initialisation_payload(*args, args={'object_detector_skip_frames': 5})['object_detector_skip_frames'] == 5
    hp.object_detector_skip_frames = None
    assert wire.initialisation_payload(*args)['object_detector_skip_frames'] is None
