"""Seeded, literal cases for the detector post-process and suppression launches (tests/test_gpu_post_ops.py runs them on the device,
tests/test_post_ref.py holds them to the conditions that keep them from being vacuous, on the CPU).  numpy only.

Every shape sits on a loop bound, tail or dispatch edge of csrc/post.hip / csrc/nms.hip; the comment beside each list says which."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# ------------------------------------------------------------------------------------------------ YOLO
# yolo_conf_k: half a wave per row, lane l reads columns l, l + 32, l + 64; a second sweep from column 96.
YOLO_CLASSES = [1,        # 6 columns, most lanes idle
                27,       # 32 columns: exactly one lane row
                28,       # first column of the second lane row
                80,       # the shipped models
                91,       # 96 columns: one full sweep
                92,       # first column of the second sweep (c0 += 96)
                200]
YOLO_ROWS = [1, 7, 1023, 1024, 1025, 2049]      # yolo_compact_k's rounds of 1024 rows
YOLO_BATCHES = [1, 3]
YOLO_THR = 0.25
YOLO_STRETCH = (640.0, 480.0, None)                      # (img_w, img_h, letterbox)
YOLO_LETTERBOX = [(1280, 720, (640, 640)), (48, 64, (640, 640))]            # rows of tests/golden/letterbox_geometry.npz
YOLO_SQUARE = (640, 640, (640, 640))                     # must give the stretch bits
YOLO_GRID_STRIDE = (300, 256, 1)                         # images, rows, classes: 76 800 rows > 8 192 blocks x 8 rows
SENTINEL_F, SENTINEL_I = np.float32(-7777.0), np.int32(-77)


def yolo_launches(n_cls):
    """(n_rows, batch) of one class count.  One row per image cannot both pass and fail, so that shape runs as three images only."""
    return [(r, b) for r in YOLO_ROWS for b in YOLO_BATCHES if not (r == 1 and b == 1)]


def yolo_raw(n_rows, n_cls, batch, seed=0):
    """raw f32 [batch][n_rows][5 + n_cls].  Image z's objectness is scaled so that the images pass different numbers of rows; image 1 of a
    batch passes none.  Image 0 (from 7 rows) carries the crafted rows, see `yolo_crafted`."""
    rng = np.random.default_rng([20261021, n_rows, n_cls, batch, seed])
    raw = rng.random((batch, n_rows, 5 + n_cls), dtype=np.float32)
    raw[..., 4] = np.float32(0.2) + raw[..., 4] * np.float32(0.8)
    raw[..., 5:] *= np.float32(0.6)                                          # no product reaches 0.6 by chance ...
    hot = rng.random((batch, n_rows)) < 0.4
    hc = rng.integers(0, n_cls, (batch, n_rows))
    for z in range(batch):
        rows = np.flatnonzero(hot[z])
        raw[z, rows, 5 + hc[z, rows]] = np.float32(0.7) + rng.random(len(rows), dtype=np.float32) * np.float32(0.3)
        raw[z, :, 4] *= np.float32([1.0, 0.01, 0.6][z % 3])                  # image 1: nothing passes
    if n_rows == 1:
        raw[0, 0, 4], raw[0, 0, 5] = 1.0, 0.9                                # one row: image 0 passes, image 2 fails
        raw[2 % batch, 0, 4] = 0.05 if batch > 1 else raw[0, 0, 4]
    if n_rows >= 7:
        yolo_crafted(raw[0], n_cls)
    return raw


def yolo_crafted(img, n_cls):
    """Rows 0..6 of an image, in place.  thr = YOLO_THR."""
    thr = np.float32(YOLO_THR)
    last = n_cls - 1
    a = min(3, last)
    img[0, 4] = 1.0; img[0, 5:] = 0.1                      # equal best products: classes a and a + 1 (neighbouring lanes), a + 32 (the same
    for c in (a, a + 1, a + 32, a + 96):                   # lane, next load of the sweep) and a + 96 (the next sweep) -- the first wins
        if c <= last:
            img[0, 5 + c] = 0.75
    img[1, 4] = 0.0                                        # objectness 0: every product 0, class 0, fails
    img[2, 4] = 0.0; img[2, 5 + last] = np.inf             # inf * 0 = NaN in the last column: class `last`, confidence NaN, fails
    img[3, 4] = 1.0; img[3, 5 + a] = np.nan                # a NaN product beside larger finite ones and a later NaN: the first NaN's index
    img[3, 5 + last] = np.nan if last > a else img[3, 5 + last]
    img[3, 5] = 0.9 if a > 0 else img[3, 5]
    img[4, :] = np.nan                                     # an all-NaN row: class 0, fails
    img[5, 4] = 1.0; img[5, 5:] = 0.1; img[5, 5 + last] = thr                                  # equal to the threshold bit for bit: passes
    img[6, 4] = 1.0; img[6, 5:] = 0.1; img[6, 5 + last] = np.nextafter(thr, np.float32(0))     # one ulp below: fails


# yolo_compact_k alone (dd_yolov5_select_batch): crafted per-row (x, y, w, h), confidence, class
def select_inputs(n_rows, batch, seed=0):
    rng = np.random.default_rng([20261022, n_rows, batch, seed])
    thr = np.float32(YOLO_THR)
    boxes = rng.random((batch, n_rows, 4), dtype=np.float32)
    conf = rng.random((batch, n_rows), dtype=np.float32)
    cls = rng.integers(0, 1 << 20, (batch, n_rows)).astype(np.int32)
    for z in range(batch):
        conf[z] *= np.float32([1.0, 0.2, 0.5][z % 3])                        # image 1: nothing passes
    if n_rows == 1:
        conf[0, 0] = 0.9
        conf[2 % batch, 0] = 0.1 if batch > 1 else conf[0, 0]
    if n_rows >= 7:
        conf[0, 0] = thr; conf[0, 1] = np.nextafter(thr, np.float32(0)); conf[0, 2] = np.nan; conf[0, 3] = np.inf
        conf[0, n_rows - 1] = 0.99; conf[0, n_rows - 2] = 0.01                # the last rows of the last (partial) round
        boxes[0, 3] = [0.5, 0.5, 0.0, 0.0]                                    # a point
        boxes[0, n_rows - 1] = [0.01, 0.02, 0.5, 0.5]                         # reaches into the padding: negative after the un-mapping
    return boxes, conf, cls


# yolo_pack_k: block z sums min(n_rows[i], cap) over i < z with stride 256 -- a second pass from the 257th image
PACK_BATCHES = [1, 2, 256, 257, 600]
PACK_CAP = 256
PACK_COUNTS = [0, 1, 255, 256, 257]             # 257 > cap: clipped


def pack_inputs(batch):
    rng = np.random.default_rng([20261023, batch])
    counts = np.array([PACK_COUNTS[(z * 3 + batch + 2) % 5] for z in range(batch)], np.int32)
    if batch >= 256:
        counts[rng.permutation(batch)[:batch // 3]] = 600                    # far above cap
    boxes = rng.random((batch, PACK_CAP, 4), dtype=np.float32)
    scores = rng.random((batch, PACK_CAP), dtype=np.float32)
    cls = rng.integers(-2 ** 31, 2 ** 31 - 1, (batch, PACK_CAP)).astype(np.int32)      # any bit pattern, NaN patterns included
    return boxes, scores, cls, counts


# ------------------------------------------------------------------------------------------------ SSD decode
# ssd_decode_k: sixteen lanes per anchor, lane `sub` reads classes 1 + sub + 16 i, 128 classes per sweep (class 0 = background)
SSD_CLASSES = [2,          # one class
               17, 18,     # 16 and 17 classes: last lane of the first sixteen, first lane again
               91,         # the shipped model
               129, 130,   # 128 classes: one full sweep; 129: the first class of the second sweep
               300]        # three sweeps
SSD_ANCHORS = [1, 15, 16, 17, 1917]       # one 16-lane group; partial / full / one more block of 16 anchors
SSD_BATCHES = [1, 3]
SSD_THR = 0.3


def ssd_sweeps(n_classes):
    return (n_classes - 2) // 128 + 1


def ssd_decode_inputs(n_anchors, n_classes, batch):
    """raw f32 [batch][n_anchors][4 + n_classes], anchors f32 [n_anchors][4].  Anchor g (counted over the batch) has its best class planted in
    one sweep after the other; from 16 anchors the first image carries the crafted rows (`ssd_crafted`)."""
    rng = np.random.default_rng([20261024, n_anchors, n_classes, batch])
    raw = (rng.standard_normal((batch, n_anchors, 4 + n_classes)) * 2).astype(np.float32)
    raw[..., :4] = (rng.standard_normal((batch, n_anchors, 4)) * 3).astype(np.float32)
    anchors = np.concatenate([rng.random((n_anchors, 2)), 0.05 + 0.45 * rng.random((n_anchors, 2))], axis=1).astype(np.float32)
    raw[:, np.arange(n_anchors) % 3 == 1, 4:] -= np.float32(8)               # a third of the anchors stay below the threshold
    sw = ssd_sweeps(n_classes)
    flat = raw.reshape(batch * n_anchors, 4 + n_classes)
    for j, g in enumerate(range(0, len(flat), max(1, len(flat) // 64))):
        lo = 1 + 128 * (j % sw)
        c = int(rng.integers(lo, min(lo + 128, n_classes)))
        flat[g, 4 + c] = flat[g, 5:].max() + np.float32(1 + (g % 7) / 8)      # one above the anchor's other logits
    if n_anchors >= 16:
        ssd_crafted(raw[0], n_classes)
    return raw, anchors


def ssd_crafted(img, n_classes):
    """Anchors 1..9 of an image, in place (anchor 0 keeps its planted class)."""
    C = n_classes
    cols = img[:, 4:]
    cols[1, 1:] = -1.0                                     # equal best logits: neighbouring lanes, the same lane's next load, the next
    for c in (2, 3, 2 + 16, 2 + 128, 2 + 256):             # sweeps -- the lowest class wins
        if c < C:
            cols[1, c] = 4.0
    cols[2, 1:] = 2.5                                      # every class equal: class 0 (column 1)
    cols[3, 1:] = -np.inf                                  # no class wins: class 0, score 0
    cols[4, 1:] = np.nan                                   # likewise
    cols[5, 1:] = -3.0; cols[5, 1] = np.nan                # a NaN beside finite logits never wins
    cols[5, C - 1] = 1.5 if C > 2 else cols[5, C - 1]
    cols[6, 0] = 50.0                                      # the background column is no class
    img[7, 2:4] = [40.0, -40.0]                            # expf(8), expf(-8)
    img[8, 2:4] = [-40.0, 40.0]
    img[9, :4] = 0.0                                       # the anchor itself
    cols[7, 1:] = -30.0; cols[8, 1:] = 30.0                # saturated scores


# ------------------------------------------------------------------------------------------------ SSD second stage
# nms_f32_select_batched: PER = 8 up to 2048 boxes, PER = 16 above
SSD_POST = [(65, 1), (65, 64), (2048, 1), (2048, 64), (2049, 1), (2049, 64), (4096, 1), (4096, 64), (2049, 10)]      # (anchors, max_det)


def ssd_post_case(A, max_det, thr=0.4, iou=0.5):
    """Per-anchor arrays as scripts/ssd_post_cases.py crafts them, at another anchor count: clustered boxes, scores at 16 levels (ties),
    a NaN score, a NaN box, degenerate boxes, one score exactly at the threshold.  The f32 path's order is total (bit keys, NaN scores are
    no candidates): this case pins it."""
    rng = np.random.default_rng([20261025, A, max_det])
    centres = rng.random((max(2, A // 12), 4), dtype=np.float32) * np.float32(0.6)
    src = rng.integers(0, len(centres), A)
    cy, cx = centres[src, 0] + np.float32(0.2), centres[src, 1] + np.float32(0.2)
    boxes = np.stack([cy - 0.1, cx - 0.1, cy + 0.1, cx + 0.1], axis=1).astype(np.float32) + rng.random((A, 4), dtype=np.float32) * np.float32(0.03)
    boxes[5] = boxes[4]
    boxes[11, 2] = boxes[11, 0]
    boxes[13, 1] = np.nan
    boxes[17] = boxes[17, [2, 3, 0, 1]]                                       # unordered corners: negative extents, positive area
    score = np.float32(thr) * rng.random(A, dtype=np.float32) * np.float32(0.99)
    m = (A * 2) // 3
    pick = rng.permutation(A)[:m]
    score[pick] = np.float32(thr) + np.floor(rng.random(m) * 16).astype(np.float32) * np.float32((1 - thr) / 16)
    score[pick[0]] = np.float32(thr)
    score[pick[1]] = np.nan
    cls = rng.integers(0, 90, A).astype(np.int32)
    keys = np.where(score >= np.float32(thr), score, np.float32(-1)).astype(np.float32)
    return dict(A=A, boxes=boxes, score=score, cls=cls, keys=keys, max_det=max_det, thr=thr, iou=iou)


# ------------------------------------------------------------------------------------------------ SSD finish
FINISH_MAX_DET = [1, 3, 4, 10, 64]        # the NaN scrub's column index names a row only from 4; lanes go up to 64
FINISH_BATCHES = [1, 5]
FINISH_CONF, FINISH_IOU, FINISH_SIZE = 0.3, 0.5, (300.0, 200.0)
FINISH_KINDS = ['mixed', 'nan_boxes', 'nan_scores', 'one_class', 'all_classes']


def finish_image(N, kind, seed):
    """One image's (boxes f32 [N, 4] ymin xmin ymax xmax normalised, classes f32 [N], scores f32 [N])."""
    rng = np.random.default_rng([20261026, N, seed])
    centres = rng.random((max(1, N // 4), 2)) * 0.6 + 0.2
    src = rng.integers(0, len(centres), N)
    c = centres[src] + rng.random((N, 2)) * 0.04
    half = 0.08 + rng.random((N, 2)) * 0.04
    boxes = np.concatenate([c - half, c + half], axis=1).astype(np.float32)
    n_cls = {'one_class': 1, 'all_classes': N}.get(kind, 3)
    cls = (np.arange(N) % n_cls if kind == 'all_classes' else rng.integers(0, n_cls, N)).astype(np.float32)
    if kind == 'all_classes':
        cls = cls[rng.permutation(N)]
    scores = (0.1 + 0.9 * rng.random(N)).astype(np.float32)
    # equal scores inside a class, groups of at most 16 rows: the reference's sort is stable there, "higher row first"
    lv = np.float32(0.3) + np.floor(rng.random(N) * 4).astype(np.float32) * np.float32(0.125)
    tied = np.arange(N) % 2 == 0 if N <= 32 else (np.arange(N) % 4 == 0)
    scores[tied] = lv[tied]
    if N >= 2:
        scores[N - 1] = np.float32(FINISH_CONF)                               # equal to the confidence in f32: takes part
        scores[0] = np.nextafter(np.float32(FINISH_CONF), np.float32(0)) if N > 4 else scores[0]
    if N >= 6:                                                                # boxes one pixel wide, where the + 1 decides
        x0 = np.float32(0.5)
        for r, dx in ((2, 0.0), (3, 1.0), (4, 2.0)):
            boxes[r] = [0.25, x0 + np.float32(dx / FINISH_SIZE[0]), 0.5, x0 + np.float32((dx + 1) / FINISH_SIZE[0])]
            cls[r], scores[r] = cls[2], np.float32(0.9 - 0.01 * r)
    if kind == 'nan_boxes':                                                   # a NaN in each box column, each in another row (one row when N < 4);
        for col in range(4):                                                  # the column's number is a score index too -- where that row exists
            boxes[(N - 1 - col) % N, col] = np.nan
    if kind == 'nan_scores':
        scores[::3] = np.nan
    return boxes, cls, scores


def finish_batch(N, batch):
    """-> boxes [batch, N, 4], classes, scores [batch, N] and the kinds.  A single image: NaN boxes (at max_det = 3 that is the NaN in column
    3 with no row 3)."""
    kinds = ['nan_boxes'] if batch == 1 else FINISH_KINDS[:batch]
    imgs = [finish_image(N, k, i) for i, k in enumerate(kinds)]
    return tuple(np.stack([im[j] for im in imgs]) for j in range(3)) + (kinds,)


# ------------------------------------------------------------------------------------------------ suppression, f64
# nms_ex: <= 64 one wave; 65 .. 1024 nms_rank_k + nms_lazy_k; from 1025 nms_rank_k + nms_mask_k + nms_scan_k; k % 64 == 1: one box in the last word
NMS_SIZES = [1, 2, 63, 64, 65, 128, 129, 1024, 1025, 4033, 4095, 4096]
NMS_THRS = [0.3, 0.6, 1.0]
NMS_KINDS = ['tie_free', 'levels4', 'levels1', 'identical', 'zero_area', 'chain']
NMS_NAN_SIZES = [5, 64, 65, 1025]
NMS_CAPACITY = 4096
# exempt from "keeps and suppresses at least 10 %": the all-equal boxes (one survivor) and the cases in which nothing can overlap enough --
# threshold 1.0 (mode 0: inter / area never exceeds 1; mode 1: the + 1 lifts the IoU above 1 only for all but identical boxes)
NMS_EXEMPT_KINDS = ('identical',)
NMS_EXEMPT_THR = 1.0
CHAIN_STEP = {(0, 0.3): 45, (0, 0.6): 30, (0, 1.0): 30, (1, 0.3): 45, (1, 0.6): 20, (1, 1.0): 20}      # see nms_case


def _as_mode(x1, y1, w, h, mode):
    """mode 0: tlwh; mode 1: xyxy."""
    return np.stack([x1, y1, w, h] if mode == 0 else [x1, y1, x1 + w, y1 + h], axis=1).astype(np.float64)


def nms_case(k, kind, thr, mode, nan=False):
    """-> (boxes f64 [k, 4], keys f64 [k]).  Clusters of about six near-duplicates (some pairs above 0.6, some between 0.3 and 0.6), rows in
    random order.
    chain: 99 x 99 (mode 1: 100 x 100) boxes on a line, CHAIN_STEP pixels apart, keys descending along it: a box overlaps its successor above
    the threshold and the one after that below it (mode 0: (100 - d) / 100 and (100 - 2 d) / 100; mode 1: (101 - d) 101 / (20000 - (101 - d)
    101)), so the survivors are every other box -- and a suppressed box would suppress its successor if it still counted.
    nan: NaN keys spread over the rows (no +inf among the keys)."""
    rng = np.random.default_rng([20261027, k, NMS_KINDS.index(kind), int(thr * 10), mode, int(nan)])
    n_cl = max(1, k // 6)
    cen = rng.random((n_cl, 2)) * (60.0 * np.sqrt(n_cl))
    src = rng.integers(0, n_cl, k)
    x1 = cen[src, 0] + rng.random(k) * 12
    y1 = cen[src, 1] + rng.random(k) * 12
    w, h = 40 + rng.random(k) * 10, 40 + rng.random(k) * 10
    keys = rng.permutation(k).astype(np.float64) / 7.0 + 0.125                # distinct
    if kind == 'levels4':
        keys = np.floor(rng.random(k) * 4) / 4.0
    elif kind == 'levels1':
        keys = np.full(k, 0.5)
    elif kind == 'identical':
        x1[:], y1[:], w[:], h[:] = 10.0, 20.0, 30.0, 40.0
    elif kind == 'zero_area':                                                 # a third of the boxes are points / lines
        z = rng.random(k) < 0.34
        w[z & (np.arange(k) % 2 == 0)] = 0.0
        h[z] = 0.0
    elif kind == 'chain':
        d = CHAIN_STEP[(mode, thr)]
        pos = rng.permutation(k)                                              # row r sits at place pos[r] of the chain
        x1, y1 = pos * float(d), np.full(k, 5.0)
        w = h = np.full(k, 99.0 if mode == 0 else 100.0)
        keys = (k - pos).astype(np.float64)
    if nan:
        keys = keys.copy()
        keys[rng.permutation(k)[:max(2, k // 4)]] = np.nan
    return _as_mode(x1, y1, w, h, mode), keys


def nms_exempt(kind, thr):
    return kind in NMS_EXEMPT_KINDS or thr == NMS_EXEMPT_THR


# ------------------------------------------------------------------------------------------------ counts
COUNT_SIZES = [1, 63, 64, 65, 1000]       # counts_add_k: blocks of 64


def counts_inputs(n):
    rng = np.random.default_rng([20261028, n])
    a, b, c = (rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64) for _ in range(3))
    a[0], b[0], c[0] = 2 ** 33 + 1, -2 ** 35, -5                                      # above 2^32, and negative
    return a, b, c
