"""TEST INFRASTRUCTURE ONLY -- TFLite_Detection_PostProcess with use_regular_nms = true restated for the tests (the custom op
inside the reference's SSD .tflite graph, tools/ssd_mobilenet.py:100-109 upstream; kernels/detection_postprocess.cc
NonMaxSuppressionMultiClassRegularHelper over NonMaxSuppressionSingleClassHelper).  TensorFlow Lite is absent from this image:
this is written from the op's published behaviour, parity against it is unpinned (as for the fast path in oracle/nets_torch.py).

`regular_nms` is the class-by-class form, written directly from the semantics; `regular_nms_single_greedy` is the one greedy
selection over all (anchor, class) pairs that csrc/post_regular.hip runs -- tests/test_regular_nms_ref.py holds the two
against each other.  The IoU is oracle/nets_torch.ssd_postprocess_decoded's (f32, non-positive area gives 0, no +1)."""
import numpy as np

f = np.float32


def _areas(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def _iou_one_to_many(boxes, area, i, rest):
    """IoU of box i with boxes[rest], f32 -- the expressions of oracle/nets_torch.ssd_postprocess_decoded."""
    y0 = np.maximum(boxes[i, 0], boxes[rest, 0]); x0 = np.maximum(boxes[i, 1], boxes[rest, 1])
    y1 = np.minimum(boxes[i, 2], boxes[rest, 2]); x1 = np.minimum(boxes[i, 3], boxes[rest, 3])
    inter = np.maximum(y1 - y0, f(0)) * np.maximum(x1 - x0, f(0))
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / (area[i] + area[rest] - inter)
    return np.where((area[i] <= 0) | (area[rest] <= 0), f(0), iou)


def _rows(boxes, picked, max_det):
    ob, oc, os_ = np.zeros((max_det, 4), np.float32), np.zeros(max_det, np.float32), np.zeros(max_det, np.float32)
    for j, (s, c, a) in enumerate(picked):
        ob[j], oc[j], os_[j] = boxes[a], c, s
    return ob, oc, os_, len(picked), [(int(c), int(a)) for _, c, a in picked]


def single_class_nms(boxes, area, scores, per_class, score_thr, iou_thr):
    """NonMaxSuppressionSingleClassHelper: candidates score >= threshold (a NaN is none), stable sort by descending score (equal
    scores: lower anchor first), greedy NMS, stop after min(#candidates, detections_per_class) kept.  -> kept anchors in keep order."""
    with np.errstate(invalid='ignore'):
        cand = np.nonzero(scores >= f(score_thr))[0]
    order = cand[np.argsort(-scores[cand], kind='stable')]
    want = min(len(order), per_class)
    alive = np.ones(len(order), dtype=bool)
    kept = []
    for i, a in enumerate(order):
        if len(kept) >= want:
            break
        if not alive[i]:
            continue
        kept.append(int(a))
        rest = order[i + 1:]
        if len(rest):
            alive[i + 1:] &= ~(_iou_one_to_many(boxes, area, a, rest) > f(iou_thr))
    return kept


def regular_nms(boxes, scores, max_det, per_class, score_thr=1e-8, iou_thr=0.6):
    """One image.  boxes f32 [A, 4] (ymin, xmin, ymax, xmax), scores f32 [A, C] (column c = class c, no background column) ->
    (boxes [max_det, 4], classes f32, scores f32, count, [(class, anchor)] of the rows).  Class by class in ascending id; after each
    class its kept rows are merged into the running list by descending score, stably (earlier class first on equal scores, the
    keep order inside a class), and the list is cut to max_detections."""
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    area = _areas(boxes)
    running = []
    for c in range(scores.shape[1]):
        kept = single_class_nms(boxes, area, scores[:, c], per_class, score_thr, iou_thr)
        running = sorted(running + [(scores[a, c], c, a) for a in kept], key=lambda r: -r[0])[:max_det]     # sorted() is stable
    return _rows(boxes, running, max_det)


def regular_nms_single_greedy(boxes, scores, max_det, per_class, score_thr=1e-8, iou_thr=0.6):
    """The same rows as ONE greedy selection over all (anchor, class) pairs: order them by (score descending, class ascending,
    anchor ascending); repeatedly take the best live pair as the next row, kill the live pairs of the same class whose IoU with it
    exceeds the threshold, kill the class once it has detections_per_class rows; stop at max_detections rows or when nothing lives."""
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    area = _areas(boxes)
    with np.errstate(invalid='ignore'):
        live = scores >= f(score_thr)
    per = np.zeros(scores.shape[1], dtype=int)
    picked = []
    while len(picked) < max_det and live.any():
        sc = np.where(live, scores, -np.inf)
        c, a = np.argwhere(sc.T == sc.max())[0]                   # class-major: the lowest class, then the lowest anchor, of the best score
        picked.append((scores[a, c], int(c), int(a)))
        live[a, c] = False
        per[c] += 1
        if per[c] >= per_class:
            live[:, c] = False
        else:
            rest = np.nonzero(live[:, c])[0]
            live[rest[_iou_one_to_many(boxes, area, a, rest) > f(iou_thr)], c] = False
    return _rows(boxes, picked, max_det)


def decode_boxes(enc, anchors):
    """The op's anchor decode (scales 10, 10, 5, 5), f32: the expressions of oracle/nets_torch.ssd_postprocess."""
    enc = np.asarray(enc, dtype=np.float32)
    a = np.asarray(anchors, dtype=np.float32)
    yc = enc[:, 0] / f(10) * a[:, 2] + a[:, 0]
    xc = enc[:, 1] / f(10) * a[:, 3] + a[:, 1]
    hh = f(0.5) * np.exp(enc[:, 2] / f(5)) * a[:, 2]
    hw = f(0.5) * np.exp(enc[:, 3] / f(5)) * a[:, 3]
    return np.stack([yc - hh, xc - hw, yc + hh, xc + hw], axis=1).astype(np.float32)


def regular_nms_raw(raw, anchors, max_det, per_class, score_thr=1e-8, iou_thr=0.6, boxes=None):
    """From the f32 head matrix raw [A, 4 + 1 + C] (column 4 = background): every class logit through the sigmoid first (the op sees
    scores).  boxes: decoded boxes to use instead of this file's own decode (numpy's exp and the device's expf differ in the last bits)."""
    raw = np.asarray(raw, dtype=np.float32)
    sc = (f(1) / (f(1) + np.exp(-raw[:, 5:]))).astype(np.float32)
    return regular_nms(decode_boxes(raw[:, :4], anchors) if boxes is None else boxes, sc, max_det, per_class, score_thr, iou_thr)


def dequantise_u8(box_u8, cls_u8, box_scale, box_zp, cls_scale, cls_zp, out_scale, out_zp):
    """uint8 head tensors of one image -> (box encodings f32 [A, 4], scores f32 [A, C]): oracle/nets_quant.ssd_quant_decode's
    expressions -- scale * (q - zero point), the class bytes through oracle/nets_quant.logistic_table first; column 0 is background."""
    from oracle.nets_quant import logistic_table
    enc = f(box_scale) * (np.asarray(box_u8).astype(np.float32) - f(box_zp))
    tab = logistic_table(cls_scale, cls_zp, out_scale, out_zp)
    sq = tab[np.asarray(cls_u8)[:, 1:]]
    return enc, (f(out_scale) * (sq.astype(np.float32) - f(out_zp))).astype(np.float32)


def regular_nms_u8(qm, box_u8, cls_u8, anchors, max_det, per_class, score_thr=1e-8, iou_thr=0.6, boxes=None):
    """From a quantised model's head tensors (box_u8 [A, 4], cls_u8 [A, 1 + C]); qm: the QModel whose quantisation they carry."""
    Lb, Lc, Lo = qm['layers']['box0'], qm['layers']['cls0'], qm['logistic']
    enc, sc = dequantise_u8(box_u8, cls_u8, Lb['out_scale'], Lb['out_zp'], Lc['out_scale'], Lc['out_zp'], Lo['out_scale'], Lo['out_zp'])
    return regular_nms(decode_boxes(enc, anchors) if boxes is None else boxes, sc, max_det, per_class, score_thr, iou_thr)
