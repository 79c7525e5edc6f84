"""numpy references of the detector post-process (csrc/post.hip) and of the suppression kernels (csrc/nms.hip), one launch at a time.

Nothing is defined twice: the operations are the project's own oracle functions, and this file adds only what they leave open.

* YOLO rows -> (xyxy, conf, cls): oracle/nets_torch.yolov5_decode (tools/yolov5.py:120-131), tests/letterbox_ref.decode for a letterboxed
  frame.  Added here: the capacity contract (out_n counts every passing row, the first `cap` of them are written, nothing behind them) and
  the packed layout of yolo_pack_k.
* Suppression: oracle/deepsort_np.non_max_suppression (mode 0), oracle/detectors_np.ssd_nms_boxes (mode 1),
  oracle/nets_torch.ssd_postprocess_decoded (mode 2, already tie-defined).  The first sorts with an unstable argsort, so its order under
  equal keys is open from 17 rows; `tie_order` is the order csrc/nms.hip documents -- key descending, among equal keys the higher
  original index first, a NaN key as the largest key (np.argsort places it last, the reference picks it first) -- and `nms_mode0` /
  `nms_mode1` run the oracle functions' own overlap expressions, vectorised per pivot (the same IEEE operations per pair), in that order.
  tests/test_post_ref.py proves them identical to the oracle functions on tie-free inputs.
* SSD anchor decode: csrc/ssd_dev.h decode_anchor restated in float64 with a per-element bound (`ssd_decode`).
* SSD finish: oracle/detectors_np.ssd_predict_tail (`ssd_finish`), padded to four rows where the reference itself would index past its
  score vector.
"""
import numpy as np

import letterbox_ref
import net_op_ref
from oracle import deepsort_np, detectors_np, nets_torch      # noqa: F401  (re-exported: the tests name the oracle through this module)

U = net_op_ref.U                  # 2^-24, the unit roundoff of f32


# ------------------------------------------------------------------------------------------------ YOLO
def yolo_rows(raw, thr, img_w, img_h, letterbox=None):
    """One image's passing rows in row order: (boxes f32 [n, 4], conf f32 [n], cls int32 [n]).  letterbox = (net_w, net_h) or None."""
    if letterbox is None:
        b, s, c = nets_torch.yolov5_decode(raw, np.float32(thr), float(img_w), float(img_h))
        return np.asarray(b, np.float32), np.asarray(s, np.float32), np.asarray(c).astype(np.int32)
    b, s, c = letterbox_ref.decode(raw, thr, int(img_w), int(img_h), *letterbox)
    return b, s, c.astype(np.int32)


def select_rows(boxes4, conf, cls, thr, img_w, img_h, letterbox=None):
    """The second half alone on (x, y, w, h) f32 [n, 4], conf f32 [n], cls int32 [n]: rows with conf >= thr in row order; corners formed
    in f32, un-mapped by letterbox_ref.unmap_corners (stretch = offset 0, new = net: the terms are exact and the result is x * W in f64)."""
    boxes4 = np.asarray(boxes4, np.float32)
    conf = np.asarray(conf, np.float32)
    keep = np.where(conf >= np.float32(thr))[0]
    x, y, bw, bh = (boxes4[keep, i] for i in range(4))
    two = np.float32(2)
    with np.errstate(invalid='ignore', over='ignore'):
        x1, y1, x2, y2 = x - bw / two, y - bh / two, x + bw / two, y + bh / two
        if letterbox is None:
            gx = gy = (0, 1, 1)
        else:
            nw, nh, ox, oy = letterbox_ref.geometry(int(img_w), int(img_h), *letterbox)
            gx, gy = (ox, nw, letterbox[0]), (oy, nh, letterbox[1])
        b = np.stack([letterbox_ref.unmap_corners(x1, *gx, img_w), letterbox_ref.unmap_corners(y1, *gy, img_h),
                      letterbox_ref.unmap_corners(x2, *gx, img_w), letterbox_ref.unmap_corners(y2, *gy, img_h)], axis=1)
    return b.reshape(-1, 4), conf[keep], np.asarray(cls, np.int32)[keep]


def capped(rows, cap):
    """The capacity contract around one image's passing rows: -> (out_n, rows written).  out_n is the FULL count."""
    b, s, c = rows
    return len(s), (b[:cap], s[:cap], c[:cap])


def pack(boxes, scores, cls, n_rows, cap):
    """yolo_pack_k: per-image [batch][cap] outputs -> f32 [total][6] rows {x1, y1, x2, y2, score, class bits}, image order x row order, counts
    clipped to cap."""
    out = []
    for z, n in enumerate(n_rows):
        n = min(int(n), cap)
        out.append(np.concatenate([boxes[z, :n], scores[z, :n, None], cls[z, :n, None].astype(np.int32).view(np.float32)], axis=1))
    return np.concatenate(out, axis=0).astype(np.float32).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------ suppression
def tie_order(keys):
    """Pick order of csrc/nms.hip: key descending, equal keys the higher original index first, NaN = the largest key."""
    k = np.asarray(keys, np.float64)
    k = np.where(np.isnan(k), np.inf, k)
    idx = np.arange(len(k))
    return np.lexsort((-idx, -k))


def nms_mode0(boxes_tlwh, max_overlap, keys):
    """deepsort_np.non_max_suppression's statements (preprocessing.py:6-73) with `order` replaced by the tie-defined one."""
    if len(boxes_tlwh) == 0:
        return []
    b = np.asarray(boxes_tlwh).astype(float)
    x1, y1 = b[:, 0], b[:, 1]
    x2, y2 = b[:, 2] + b[:, 0], b[:, 3] + b[:, 1]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = tie_order(keys)[::-1]
    keep = []
    while len(order) > 0:
        i = order[-1]
        rest = order[:-1]
        keep.append(int(i))
        w = np.maximum(0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        order = rest[~((w * h) / area[rest] > max_overlap)]
    return keep


def nms_mode1(boxes_xyxy, iou_threshold, scores):
    """detectors_np.ssd_nms_boxes' statements (ssd_mobilenet.py:59-98) for ONE class, a pivot's pairs at once, in the tie-defined order."""
    b = np.asarray(boxes_xyxy, np.float64)
    left, top = b[:, 0], b[:, 1]
    wid, hei = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    area = wid * hei
    alive = tie_order(scores)
    keep = []
    while len(alive) > 0:
        i, alive = alive[0], alive[1:]
        keep.append(int(i))
        iw = np.maximum(0.0, np.minimum(left[i] + wid[i], left[alive] + wid[alive]) - np.maximum(left[i], left[alive]) + 1)
        ih = np.maximum(0.0, np.minimum(top[i] + hei[i], top[alive] + hei[alive]) - np.maximum(top[i], top[alive]) + 1)
        inter = iw * ih
        with np.errstate(divide='ignore', invalid='ignore'):
            alive = alive[inter / (area[i] + area[alive] - inter) <= iou_threshold]
    return keep


def oracle_mode0(boxes, thr, keys):
    return deepsort_np.non_max_suppression(boxes, thr, keys)


def oracle_mode1(boxes, thr, scores):
    """ssd_nms_boxes for one class -> kept row indices (it returns the rows; the scores are distinct, so they name the rows)."""
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores, np.float64)
    assert len(np.unique(scores)) == len(scores)
    _, _, s = detectors_np.ssd_nms_boxes(boxes, np.zeros(len(boxes)), scores, thr)
    where = {float(v): i for i, v in enumerate(scores)}
    return [where[float(v)] for v in s[0]]


NMS_REF = {0: nms_mode0, 1: nms_mode1}
NMS_ORACLE = {0: oracle_mode0, 1: oracle_mode1}


# ------------------------------------------------------------------------------------------------ SSD decode
def _half_ulp(mag):
    return 0.5 * np.spacing(np.asarray(mag, np.float64).astype(np.float32)).astype(np.float64)


def _expf_allowance(value):
    """The device's expf behind decode_anchor: tests/net_op_ref.py:213 (`16 * U * max(1, |act|)`, term 4 of its docstring) bounds the same
    device exponential with the handful of f32 operations around it; the same figure is used here for the exponential alone and for the
    whole sigmoid."""
    return 16 * U * np.maximum(1.0, np.abs(value))


def ssd_decode(raw, anchors, score_thr):
    """csrc/ssd_dev.h decode_anchor + ssd_decode_k's class scan for raw f32 [..., A, 4 + C], anchors f32 [A, 4] (yc, xc, h, w).
    -> dict: boxes f64 [..., A, 4] with `boxes_bound`, score f64 with `score_bound`, cls int32 (exact), passes bool (score >= thr).

    The bound.  Every operation of decode_anchor is one correctly rounded f32 operation (contraction off) except expf, so an intermediate
    v computed from inputs with error e carries e propagated through the operation plus half an ulp at |v| + e:
        q = r / 10              : half_ulp(q)
        p = q * a_size          : e_q * |a_size| + half_ulp
        c = p + a_centre        : e_p + half_ulp                                  (3 operations)
        t = r / 5               : half_ulp(t)
        E = expf(t)             : exp(t) * expm1(e_t) + the expf allowance
        h = 0.5 * E * a_size    : e_E * |a_size| / 2 + half_ulp                   (0.5 * E is exact)
        box = c -+ h            : e_c + e_h + half_ulp                            (7 rounded operations and one expf per corner)
    and the score 1 / (1 + expf(-best)) is the sigmoid net_op_ref bounds as a whole.
    The class is exact: a strict `>` scan over the same f32 logits in ascending class, so the lowest index wins a tie, a NaN never wins
    and a row no class wins gives class 0 (best = -inf, score 0)."""
    raw = np.asarray(raw, np.float32)
    an = np.asarray(anchors, np.float32).astype(np.float64)
    r = raw[..., :4].astype(np.float64)
    boxes, bnd = np.zeros(r.shape), np.zeros(r.shape)
    for axis in (0, 1):                                              # 0: y / height, 1: x / width
        centre, size = an[:, axis], an[:, 2 + axis]
        q = r[..., axis] / 10.0
        e = _half_ulp(q)
        p = q * size
        e = e * np.abs(size) + _half_ulp(np.abs(p) + e * np.abs(size))
        c = p + centre
        e_c = e + _half_ulp(np.abs(c) + e)
        t = r[..., 2 + axis] / 5.0
        e_t = _half_ulp(t)
        E = np.exp(t)
        e_E = E * np.expm1(e_t) + _expf_allowance(E)
        h = 0.5 * E * size
        e_h = 0.5 * e_E * np.abs(size)
        e_h = e_h + _half_ulp(np.abs(h) + e_h)
        for col, v in ((axis, c - h), (2 + axis, c + h)):
            boxes[..., col] = v
            bnd[..., col] = e_c + e_h + _half_ulp(np.abs(v) + e_c + e_h)
    logits = raw[..., 5:]
    best = np.full(logits.shape[:-1], -np.inf, np.float32)
    cls = np.zeros(logits.shape[:-1], np.int32)
    for c in range(logits.shape[-1]):                                # the sequential strict `>` scan
        with np.errstate(invalid='ignore'):
            win = logits[..., c] > best
        best = np.where(win, logits[..., c], best)
        cls = np.where(win, c, cls).astype(np.int32)
    with np.errstate(over='ignore'):
        score = 1.0 / (1.0 + np.exp(-best.astype(np.float64)))
    return dict(boxes=boxes, boxes_bound=bnd, score=score, score_bound=_expf_allowance(score), cls=cls, best=best,
                passes=score >= np.float64(np.float32(score_thr)))


# ------------------------------------------------------------------------------------------------ SSD finish
FINISH_LABELS = {i: str(i - 1) for i in range(0, 130)}            # label-file line -> text; line id + 1 names class id


def ssd_finish(boxes, cls, scores, confidence, iou_thr, img_w, img_h):
    """detectors_np.ssd_predict_tail on one image's [N] rows -> {class id: [(box tuple, score), ...]} in pick order inside a class.
    The NaN scrub indexes the score vector with the COLUMN of every NaN box element (0..3); with fewer than four rows the reference raises
    an IndexError there.  ssd_finish_k ignores a column that names no row, which is the reference on rows padded to four with scores of 0
    (never selected: confidence > 0)."""
    assert confidence > 0
    boxes, cls, scores = np.asarray(boxes, np.float32), np.asarray(cls, np.float32), np.asarray(scores, np.float32)
    pad = max(0, 4 - len(scores))
    if pad:
        boxes = np.concatenate([boxes, np.zeros((pad, 4), np.float32)])
        cls, scores = np.concatenate([cls, np.zeros(pad, np.float32)]), np.concatenate([scores, np.zeros(pad, np.float32)])
    b, names, s = detectors_np.ssd_predict_tail([boxes, cls, scores, float(len(scores))], FINISH_LABELS, confidence, iou_thr,
                                                original_image_size=(img_w, img_h))
    out = {}
    assert len(names) == len(s)
    for bb, nm, ss in zip(b, names, s):
        out.setdefault(int(nm), []).append((tuple(float(v) for v in bb), float(ss)))
    return out
