"""CPU: TFLite_Detection_PostProcess with use_regular_nms = true -- the restatement the GPU tests compare against
(tests/regular_nms_ref.py) on hand-worked cases, its class-by-class form against the single greedy selection the kernel runs
(csrc/post_regular.hip), and the model reader: a file that states use_regular_nms with detections_per_class loads and reports the
mode, one without the number (or with a number below 1) is refused by name, a fast-NMS file's options are unchanged."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_nms_ref as R  # noqa: E402


def box(y, x, h=0.2, w=0.2):
    return [y, x, y + h, x + w]


def run(boxes, scores, max_det=10, per_class=100, score_thr=0.1, iou_thr=0.5):
    """Both forms; they must agree.  -> (rows as (class, anchor), scores of the rows, count, full outputs)."""
    a = R.regular_nms(np.array(boxes, np.float32), np.array(scores, np.float32), max_det, per_class, score_thr, iou_thr)
    b = R.regular_nms_single_greedy(np.array(boxes, np.float32), np.array(scores, np.float32), max_det, per_class, score_thr, iou_thr)
    assert a[3] == b[3] and a[4] == b[4]
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    return a[4], list(a[2][:a[3]]), a[3], a


def test_overlapping_boxes_of_different_classes_both_survive():
    boxes = [box(0.1, 0.1), box(0.11, 0.11)]                       # IoU ~ 0.82
    rows, _, n, _ = run(boxes, [[0.9, 0.0], [0.0, 0.8]])
    assert n == 2 and rows == [(0, 0), (1, 1)]
    rows, _, n, _ = run(boxes, [[0.9, 0.0], [0.8, 0.0]])           # the same two boxes in ONE class: the second is suppressed
    assert n == 1 and rows == [(0, 0)]


def test_one_anchor_is_emitted_under_two_classes():
    rows, sc, n, out = run([box(0.1, 0.1), box(0.6, 0.6)], [[0.9, 0.7], [0.2, 0.0]])
    assert rows == [(0, 0), (1, 0), (0, 1)] and sc == [np.float32(0.9), np.float32(0.7), np.float32(0.2)]
    np.testing.assert_array_equal(out[0][0], out[0][1])            # the same box twice
    np.testing.assert_array_equal(out[1][:3], [0, 1, 0])


def test_equal_scores_lower_class_first_then_lower_anchor():
    boxes = [box(0.0, 0.0), box(0.3, 0.3), box(0.6, 0.6)]          # disjoint
    rows, _, _, _ = run(boxes, [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5]])
    assert rows == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    rows, _, _, _ = run(boxes, [[0.5, 0.75], [0.75, 0.5], [0.5, 0.75]], max_det=4)
    assert rows == [(0, 1), (1, 0), (1, 2), (0, 0)]


def test_detections_per_class_caps_a_class():
    boxes = [box(0.0, 0.0), box(0.3, 0.3), box(0.6, 0.6)]
    rows, _, n, _ = run(boxes, [[0.9, 0.3], [0.8, 0.0], [0.7, 0.2]], per_class=1)
    assert n == 2 and rows == [(0, 0), (1, 0)]
    rows, _, n, _ = run(boxes, [[0.9, 0.3], [0.8, 0.0], [0.7, 0.2]], per_class=2)
    assert rows == [(0, 0), (0, 1), (1, 0), (1, 2)]


def test_below_threshold_and_nan_scores_are_skipped():
    boxes = [box(0.0, 0.0), box(0.3, 0.3), box(0.6, 0.6)]
    rows, _, n, _ = run(boxes, [[np.nan, 0.05], [0.09, 0.1], [0.3, np.nan]])
    assert rows == [(0, 2), (1, 1)] and n == 2                     # 0.1 >= 0.1 is a candidate


def test_a_non_positive_area_box_never_suppresses_and_is_never_suppressed():
    flat = [0.1, 0.1, 0.1, 0.3]                                    # zero height
    inverted = [0.3, 0.1, 0.1, 0.3]                                # ymax < ymin
    rows, _, n, _ = run([flat, box(0.1, 0.1), inverted, box(0.1, 0.1)], [[0.9], [0.8], [0.7], [0.6]])
    assert rows == [(0, 0), (0, 1), (0, 2)]                        # only the duplicate of the real box goes


def test_rows_past_the_count_are_zero():
    _, _, n, out = run([box(0.0, 0.0), box(0.5, 0.5)], [[0.9], [0.05]], max_det=5)
    assert n == 1
    assert not out[0][1:].any() and not out[1][1:].any() and not out[2][1:].any()
    _, _, n, out = run([box(0.0, 0.0)], [[0.01]], max_det=3)
    assert n == 0 and not out[0].any() and not out[2].any()


def test_max_detections_cuts_the_merged_list_by_score():
    boxes = [box(0.0, 0.0), box(0.3, 0.3), box(0.6, 0.6)]
    rows, sc, n, _ = run(boxes, [[0.2, 0.9], [0.3, 0.8], [0.4, 0.1]], max_det=3)
    assert n == 3 and rows == [(1, 0), (1, 1), (0, 2)]


def test_single_greedy_selection_equals_the_class_by_class_form():
    """Seeded random cases with scores on a grid of eighths (ties everywhere), some non-positive-area boxes and NaN scores."""
    rng = np.random.default_rng(20)
    exhausted = capped = 0
    for case in range(120):
        A, C = int(rng.integers(65, 130)), int(rng.integers(1, 6))
        yx = rng.random((A, 2)).astype(np.float32) * np.float32(0.7)
        hw = (rng.random((A, 2)).astype(np.float32) * np.float32(0.3) + np.float32(0.02))
        boxes = np.concatenate([yx, yx + hw], axis=1).astype(np.float32)
        flip = rng.random(A) < 0.05
        boxes[flip, 2] = boxes[flip, 0] - np.float32(0.01)
        scores = (rng.integers(0, 9, (A, C)) / 8.0).astype(np.float32)
        scores[rng.random((A, C)) < 0.02] = np.nan
        per_class = int(rng.choice([1, 2, 3, 100]))
        max_det = int(rng.integers(1, 40))
        thr = float(rng.choice([1e-8, 0.3]))
        iou = float(rng.choice([0.3, 0.6, 1.0]))
        a = R.regular_nms(boxes, scores, max_det, per_class, thr, iou)
        b = R.regular_nms_single_greedy(boxes, scores, max_det, per_class, thr, iou)
        assert a[3] == b[3] and a[4] == b[4], case
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y, err_msg=str(case))
        exhausted += a[3] < max_det
        capped += per_class < 100
    assert exhausted > 5 and capped > 20                           # both endings are in the sample


def test_uint8_wrapper_dequantises_like_the_fast_path_oracle():
    """The uint8 wrapper's boxes and per-class scores against oracle/nets_quant.ssd_quant_decode (best class of every anchor)."""
    from oracle import nets_quant
    from deepdish_amd import quantize
    qm = quantize.synthetic_ssd_quant_model(1234)
    rng = np.random.default_rng(1)
    anchors = nets_quant.ssd_anchors(300)
    A = len(anchors)
    box_q, cls_q = rng.integers(0, 256, (A, 4), dtype=np.uint8), rng.integers(0, 256, (A, 91), dtype=np.uint8)
    Lb, Lc, Lo = qm['layers']['box0'], qm['layers']['cls0'], qm['logistic']
    enc, sc = R.dequantise_u8(box_q, cls_q, Lb['out_scale'], Lb['out_zp'], Lc['out_scale'], Lc['out_zp'], Lo['out_scale'], Lo['out_zp'])
    b, s, c, _ = nets_quant.ssd_quant_decode(qm, box_q, cls_q, anchors)
    np.testing.assert_array_equal(R.decode_boxes(enc, anchors), b)
    np.testing.assert_array_equal(sc.max(axis=1), s)
    np.testing.assert_array_equal(sc.argmax(axis=1), c)


# ------------------------------------------------------------------------------------------- the model reader
def _folded_f32():
    from deepdish_amd import nets, quantize
    folded = {}
    for name, kind, w, b, stride, act in quantize.folded_ssd_layers(nets.synthetic_ssd_weights(7)):
        folded[name + '/weights'] = w if kind == 'conv' else w[:, :, :, None]
        folded[name + '/biases'] = b
    return folded


def _models():
    from deepdish_amd import quantize
    from deepdish_amd.tools import tflite_writer
    return [('v1-uint8', quantize.synthetic_ssd_quant_model(1234), tflite_writer.write_ssd_mobilenet, 'uint8'),
            ('v1-f32', _folded_f32(), tflite_writer.write_ssd_mobilenet, 'f32'),
            ('v2-uint8', quantize.synthetic_ssd_v2_quant_model(1234), tflite_writer.write_ssd_mobilenet_v2, 'uint8')]


@pytest.fixture(scope='module')
def models():
    return _models()


def test_a_regular_nms_file_loads_and_reports_mode_and_number(tmp_path, models):
    from deepdish_amd.tools.weights_io import load_ssd_model, ssd_post_options
    for name, model, write, want_kind in models:
        path = str(tmp_path / ('ssd_mobilenet_%s.tflite' % name))
        write(model, path, post=dict(use_regular_nms=True, detections_per_class=100, max_detections=20))
        kind, m = load_ssd_model(path)
        post = ssd_post_options(m)
        assert kind == want_kind, name
        assert post['use_regular_nms'] is True and post['detections_per_class'] == 100 and post['max_detections'] == 20, (name, post)
        assert abs(post['nms_iou_threshold'] - 0.6) < 1e-7 and abs(post['nms_score_threshold'] - 1e-8) < 1e-12


def test_regular_nms_without_a_usable_detections_per_class_is_refused_by_name(tmp_path, models):
    from deepdish_amd.tools import tflite_reader
    from deepdish_amd.tools.weights_io import load_ssd_model
    for name, model, write, _ in models:
        path = str(tmp_path / ('ssd_mobilenet_%s.tflite' % name))
        for post, words in ((dict(use_regular_nms=True), ('use_regular_nms', 'detections_per_class')),
                            (dict(use_regular_nms=True, detections_per_class=0), ('detections_per_class = 0',)),
                            (dict(use_regular_nms=True, detections_per_class=100, max_classes_per_detection=3), ('max_classes_per_detection',)),
                            (dict(use_regular_nms=True, detections_per_class=100, max_detections=100), ('max_detections',))):
            write(model, path, post=post)
            with pytest.raises(tflite_reader.UnsupportedModel) as e:
                load_ssd_model(path)
            for w in words:
                assert w in str(e.value), (name, post, str(e.value))


def test_a_fast_nms_files_options_are_unchanged(tmp_path, models):
    from deepdish_amd.tools.weights_io import load_ssd_model, ssd_post_options
    for name, model, write, _ in models:
        path = str(tmp_path / ('ssd_mobilenet_%s.tflite' % name))
        write(model, path, post=dict(detections_per_class=7))      # stated, but use_regular_nms is false: plays no part
        _, m = load_ssd_model(path)
        assert ssd_post_options(m) == dict(max_detections=10, nms_score_threshold=ssd_post_options(m)['nms_score_threshold'], nms_iou_threshold=ssd_post_options(m)['nms_iou_threshold'])
        assert sorted(ssd_post_options(m)) == ['max_detections', 'nms_iou_threshold', 'nms_score_threshold']
    assert ssd_post_options(models[0][1]) == dict(max_detections=10, nms_score_threshold=1e-8, nms_iou_threshold=0.6)
