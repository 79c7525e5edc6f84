"""CPU: tests/post_ref.py against the oracle functions it is built from, and tests/post_cases.py against the conditions that keep its cases
from being vacuous -- everything tests/test_gpu_post_ops.py relies on, checked against the references alone.

* the tie-defined suppression references equal oracle/deepsort_np.non_max_suppression and oracle/detectors_np.ssd_nms_boxes on tie-free
  inputs at every size the GPU test runs (ssd_nms_boxes walks its pairs in Python: the largest sizes run at the one threshold that leaves it
  the fewest pairs, 0.3);
* the YOLO wrapper is oracle/nets_torch.yolov5_decode whenever `cap` is not exceeded;
* every suppression case of 64 boxes or more keeps and suppresses at least 10 % of its boxes (exempt: identical boxes, threshold 1.0), the
  chains leave every other box; every YOLO launch has passing and failing rows and an image that passes none; every ssd_decode class count
  has a best class in each of its sweeps;
* every ssd_decode score keeps more than its bound between itself and the threshold."""
import os

import numpy as np
import pytest

import post_cases as pc
import post_ref


def _oracle(mode, boxes, thr, keys):
    with np.errstate(divide='ignore', invalid='ignore'):
        return post_ref.NMS_ORACLE[mode](boxes, thr, keys)


@pytest.mark.parametrize('sizes', [[k for k in pc.NMS_SIZES + pc.NMS_NAN_SIZES if k <= 1025]] + [[k] for k in pc.NMS_SIZES if k > 1025], ids=str)
@pytest.mark.parametrize('mode', [0, 1])
def test_tie_defined_suppression_is_the_oracle_on_tie_free_inputs(mode, sizes):
    for k in sizes:
        for thr in pc.NMS_THRS:
            if mode == 1 and k > 129 and thr != 0.3:
                continue
            boxes, keys = pc.nms_case(k, 'tie_free', thr, mode)
            assert len(np.unique(keys)) == k
            assert post_ref.NMS_REF[mode](boxes, thr, keys) == [int(i) for i in _oracle(mode, boxes, thr, keys)], (k, thr)


@pytest.mark.parametrize('mode', [0, 1])
def test_chains_and_zero_areas_are_the_oracle_too(mode):
    """Tie-free as well: the chain and the zero-area cases at the sizes where the oracle's Python loops stay short."""
    for k in (2, 63, 65, 129):
        for thr in pc.NMS_THRS:
            for kind in ('chain', 'zero_area'):
                boxes, keys = pc.nms_case(k, kind, thr, mode)
                assert post_ref.NMS_REF[mode](boxes, thr, keys) == [int(i) for i in _oracle(mode, boxes, thr, keys)], (k, thr, kind)


def test_tie_order_is_key_descending_higher_index_first_nan_largest():
    keys = np.array([1.0, np.nan, 3.0, 1.0, np.nan, -np.inf, 3.0])
    assert list(post_ref.tie_order(keys)) == [4, 1, 6, 2, 3, 0, 5]
    # np.argsort places NaN last, so the reference picks it first
    assert set(np.argsort(keys)[-2:]) == {1, 4}


@pytest.mark.parametrize('mode', [0, 1])
def test_suppression_cases_are_not_vacuous(mode):
    for k in pc.NMS_SIZES:
        for thr in pc.NMS_THRS:
            for kind in pc.NMS_KINDS:
                boxes, keys = pc.nms_case(k, kind, thr, mode)
                keep = post_ref.NMS_REF[mode](boxes, thr, keys)
                assert len(set(keep)) == len(keep) <= k
                if kind == 'chain' and thr < 1.0:
                    order = post_ref.tie_order(keys)
                    assert keep == [int(i) for i in order[::2]], (k, thr)
                if kind == 'identical':
                    assert len(keep) == (k if thr == 1.0 and mode == 0 else 1), (k, thr, len(keep))      # mode 1: the + 1 puts identical boxes above 1
                if k >= 64 and not pc.nms_exempt(kind, thr):
                    assert 0.1 * k <= len(keep) <= 0.9 * k, (k, kind, thr, len(keep))
    for k in pc.NMS_NAN_SIZES:
        for thr in pc.NMS_THRS[:2]:
            boxes, keys = pc.nms_case(k, 'tie_free', thr, mode, nan=True)
            assert np.isnan(keys).sum() >= 2 and not np.isinf(keys).any()
            keep = post_ref.NMS_REF[mode](boxes, thr, keys)
            assert np.isnan(keys[keep[0]]) and keep[0] == np.flatnonzero(np.isnan(keys)).max()


def test_yolo_wrapper_is_the_oracle_and_every_launch_passes_and_fails_rows():
    from oracle import nets_torch
    for n_cls in pc.YOLO_CLASSES:
        for n_rows, batch in pc.yolo_launches(n_cls):
            raw = pc.yolo_raw(n_rows, n_cls, batch)
            counts = []
            for z in range(batch):
                with np.errstate(invalid='ignore'):
                    b, s, c = post_ref.yolo_rows(raw[z], pc.YOLO_THR, *pc.YOLO_STRETCH[:2])
                    ob, os_, oc = nets_torch.yolov5_decode(raw[z], np.float32(pc.YOLO_THR), *pc.YOLO_STRETCH[:2])
                n, (wb, ws, wc) = post_ref.capped((b, s, c), n_rows)
                assert n == len(os_)
                np.testing.assert_array_equal(wb, ob); np.testing.assert_array_equal(ws, os_); np.testing.assert_array_equal(wc, oc)
                n2, (wb, ws, wc) = post_ref.capped((b, s, c), n // 2)
                assert n2 == n and len(ws) == n // 2
                np.testing.assert_array_equal(wb, ob[:n // 2])
                counts.append(n)
            assert 0 < sum(counts) < batch * n_rows, (n_cls, n_rows, batch)
            if batch > 1:
                assert counts[1] == 0 and (len(set(counts)) == 3 or n_rows == 1), counts      # the empty image; a different count per image
            if n_rows >= 7:                                                             # the crafted rows: 0 and 5 pass, 1, 2, 3, 4 and 6 fail
                with np.errstate(invalid='ignore'):
                    prod = raw[0, :7, 5:] * raw[0, :7, 4:5]
                conf = np.take_along_axis(prod, np.argmax(prod, axis=1)[:, None], axis=1)[:, 0]
                assert conf[5] == np.float32(pc.YOLO_THR) and conf[6] == np.nextafter(np.float32(pc.YOLO_THR), np.float32(0))
                assert np.isnan(conf[2:5]).all() and conf[1] == 0 and conf[0] == np.float32(0.75)
                assert np.argmax(prod[0]) == min(3, n_cls - 1) and np.argmax(prod[2]) == n_cls - 1 and np.argmax(prod[3]) == min(3, n_cls - 1)
    imgs, rows, n_cls = pc.YOLO_GRID_STRIDE
    assert imgs * rows > 8192 * 8


def test_select_cases_pass_and_fail_rows_and_the_square_canvas_is_the_stretch():
    g = np.load(os.path.join(pc.GOLDEN, 'letterbox_geometry.npz'))['rows']
    for W, H, (nw, nh) in pc.YOLO_LETTERBOX:
        assert ((g[:, :4] == [W, H, nw, nh]).all(axis=1) & (g[:, 8] == 1)).any(), (W, H)
    for n_rows in pc.YOLO_ROWS:
        for batch in pc.YOLO_BATCHES:
            if n_rows == 1 and batch == 1:
                continue
            boxes, conf, cls = pc.select_inputs(n_rows, batch)
            n = [len(post_ref.select_rows(boxes[z], conf[z], cls[z], pc.YOLO_THR, 640.0, 480.0)[1]) for z in range(batch)]
            assert 0 < sum(n) < batch * n_rows
            a = post_ref.select_rows(boxes[0], conf[0], cls[0], pc.YOLO_THR, 640.0, 640.0)
            b = post_ref.select_rows(boxes[0], conf[0], cls[0], pc.YOLO_THR, *pc.YOLO_SQUARE)
            np.testing.assert_array_equal(a[0], b[0])


def test_select_reference_is_the_decode_reference_on_its_own_rows():
    """select_rows on (first four columns, confidence, class) of a matrix == the decode references, stretch and letterboxed."""
    raw = pc.yolo_raw(1025, 80, 1)[0]
    with np.errstate(invalid='ignore'):
        prod = raw[:, 5:] * raw[:, 4:5]
    cls = np.argmax(prod, axis=1)
    conf = np.take_along_axis(prod, cls[:, None], axis=1)[:, 0]
    for W, H, lb in [pc.YOLO_STRETCH] + pc.YOLO_LETTERBOX:
        with np.errstate(invalid='ignore'):
            want = post_ref.yolo_rows(raw, pc.YOLO_THR, W, H, lb)
        got = post_ref.select_rows(raw[:, :4], conf, cls, pc.YOLO_THR, W, H, lb)
        for w, g_ in zip(want, got):
            np.testing.assert_array_equal(w, g_)


def test_ssd_decode_cases_reach_every_sweep_and_keep_their_distance_from_the_threshold():
    for C in pc.SSD_CLASSES:
        sweeps_seen = set()
        for A in pc.SSD_ANCHORS:
            for batch in pc.SSD_BATCHES:
                raw, anchors = pc.ssd_decode_inputs(A, C, batch)
                r = post_ref.ssd_decode(raw, anchors, pc.SSD_THR)
                assert r['cls'].min() >= 0 and r['cls'].max() <= C - 2
                won = np.isfinite(r['best'])
                here = set((r['cls'][won] // 128).tolist())
                if A * batch >= 16:
                    assert here == set(range(pc.ssd_sweeps(C))), (C, A, batch, here)
                sweeps_seen |= here
                thr = np.float64(np.float32(pc.SSD_THR))
                assert (np.abs(r['score'] - thr) > r['score_bound']).all()
                assert r['passes'].any() and (~r['passes']).any() or A * batch < 16
                assert np.isfinite(r['boxes']).all() and np.isfinite(r['boxes_bound']).all()
                if A >= 16:                                                   # the crafted anchors
                    assert list(r['cls'][0, 1:7]) == [(1 if C > 2 else 0), 0, 0, 0, (C - 2 if C > 2 else 0), r["cls"][0, 6]]
                    assert r['score'][0, 3] == 0 and r['score'][0, 4] == 0 and not won[0, 3] and not won[0, 4]
                    if C > 2:
                        assert won[0, 5] and r['best'][0, 5] == np.float32(1.5)
        assert sweeps_seen == set(range(pc.ssd_sweeps(C))), C


def test_oracle_ssd_postprocess_never_lets_a_nan_logit_win():
    """oracle/nets_torch.ssd_postprocess on the crafted anchors: class ids in range, the all -inf and all-NaN rows class 0 with score 0."""
    from oracle import nets_torch
    raw, anchors = pc.ssd_decode_inputs(16, 18, 1)
    want = post_ref.ssd_decode(raw, anchors, 0.0)
    with np.errstate(all='ignore'):
        ob, oc, os_, n = nets_torch.ssd_postprocess(raw[0], anchors, max_det=16, score_thr=0.0, iou_thr=1.0)
    assert n == 16 and oc.min() >= 0 and oc.max() <= 16
    by_score = {}
    for c, s in zip(oc, os_):
        by_score.setdefault(float(s), set()).add(int(c))
    assert by_score[0.0] == {0}
    got_classes = sorted(int(c) for c in oc)
    assert got_classes == sorted(int(c) for c in want['cls'][0])


def test_finish_reference_pads_where_the_reference_would_index_past_its_scores():
    b, c, s = pc.finish_image(3, 'nan_boxes', 0)
    assert np.isnan(b[:, 3]).any()
    assert post_ref.ssd_finish(b, c, s, pc.FINISH_CONF, pc.FINISH_IOU, *pc.FINISH_SIZE) is not None
    for N in pc.FINISH_MAX_DET:
        for batch in pc.FINISH_BATCHES:
            boxes, cls, scores, kinds = pc.finish_batch(N, batch)
            out = [post_ref.ssd_finish(boxes[z], cls[z], scores[z], pc.FINISH_CONF, pc.FINISH_IOU, *pc.FINISH_SIZE) for z in range(batch)]
            if N == 64 and batch == 5:
                total = [sum(len(v) for v in o.values()) for o in out]
                assert all(0 < t < 64 for t in total), total                  # some rows kept, some dropped or suppressed
                assert len(out[kinds.index('one_class')]) == 1 and len(out[kinds.index('all_classes')]) > 32
