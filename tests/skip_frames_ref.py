"""Test-side restatement of --object-detector-skip-frames N (deepdish.py:892-893,929-938,1003-1014 upstream) on top of the oracle
chain (oracle/deepsort_np, countline_np, image_np, nets_torch): which frames run the detector, and how a skipped frame pairs its own
boxes with the features of the last encoder call (zip() truncation).  Test infrastructure only."""
import numpy as np

from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch


def schedule(n, frames):
    """deepdish.py:892,929-938 -> [True where the detector runs] for `frames` frames counted from the pipeline's start:
    skip_rem starts at 0, a detector run sets it to `n or 0`, a skipped frame decrements it."""
    skip_rem, prev, out = 0, None, []
    for _ in range(frames):
        if skip_rem > 0 and prev is not None:
            skip_rem -= 1
            out.append(False)
        else:
            prev = True
            skip_rem = n or 0
            out.append(True)
    return out


def pair(boxes, labels, scores, features):
    """:1014 -- Detection i takes box i of this frame and feature row i of the last encoder call; zip() stops at the shorter list."""
    return list(zip(boxes, labels, scores, features))


def hygiene(boxes0, labels0, scores0, max_x, max_y, fg_mask=None, ratio=0.25):
    """:940-960; fg_mask = this frame's foreground mask, None = --disable-background-subtraction."""
    boxes, labels, scores = [], [], []
    for (x, y, w, h), lbl, scr in zip(boxes0, labels0, scores0):
        if np.any(np.isnan(np.asarray(boxes0, dtype=np.float64))):
            continue
        x, y = int(np.clip(x, 0, max_x)), int(np.clip(y, 0, max_y))
        w, h = int(np.clip(w, 0, max_x - x)), int(np.clip(h, 0, max_y - y))
        if w * h > 0.9 * max_x * max_y:
            continue
        if fg_mask is None or np.count_nonzero(fg_mask[y:y + h, x:x + w]) >= ratio * w * h:
            boxes.append((x, y, w, h))
            labels.append(lbl)
            scores.append(scr)
    return boxes, labels, scores


def mars_encoder(weights):
    """encoder(frame, boxes) -> features [n, 128]: the oracle's crop + MARS forward (generate_detections.py:40-84,151-177)."""
    def encode(frame, boxes):
        patches = np.stack([image_np.extract_image_patch(frame, np.asarray(b), (64, 32)) for b in boxes])
        return nets_torch.mars_forward(weights, patches)
    return encode


class Stream:
    """One stream of the reference's Pipeline run with --object-detector-skip-frames n: detect_objects :929-960,
    encode_features :988-1014, track_objects :1028-1029 and the count line, over the oracle's tracker and counter."""

    def __init__(self, encode, line, n=None, ratio=0.25, nms_max_overlap=0.6, size=(640, 480), wanted=('person',)):
        self.encode, self.n, self.ratio, self.nms, self.size = encode, n, ratio, nms_max_overlap, size
        self.tracker = ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60)
        self.counter = cl.CountLine(np.asarray(line, dtype=float), wanted)
        self.skip_rem, self.prev_objd, self.prev_features = 0, None, None

    def step(self, frame, detections, fg_mask=None):
        """frame u8 [H, W, 3]; detections = (boxes tlwh, labels, scores), the detector's output on this frame -- not read on a
        skipped frame; fg_mask = this frame's foreground mask (None: background subtraction off).
        -> (skipped, the boxes NMS kept, the Detections handed to the tracker)."""
        if self.skip_rem > 0 and self.prev_objd is not None:                     # :929-932
            boxes0, labels0, scores0 = self.prev_objd
            self.skip_rem -= 1
            skipped = True
        else:                                                                      # :933-938
            boxes0, labels0, scores0 = detections
            self.prev_objd = detections
            self.skip_rem = self.n or 0
            skipped = False
        boxes, labels, scores = hygiene(boxes0, labels0, scores0, self.size[0], self.size[1], fg_mask, self.ratio)
        keep = ds.non_max_suppression(boxes, self.nms, np.asarray(scores, dtype=np.float64))        # :995
        boxes1 = [boxes[i] for i in keep]
        labels1 = [labels[i] for i in keep]
        scores1 = [scores[i] for i in keep]
        if skipped and self.prev_features is not None:                            # :1003-1006
            features = self.prev_features
        else:                                                                      # :1008-1010 (an empty call returns no rows)
            features = self.encode(frame, boxes1) if boxes1 else np.zeros((0, 128), np.float32)
            self.prev_features = features
        dets = [ds.Det(b, l, s, f) for b, l, s, f in pair(boxes1, labels1, scores1, features)]     # :1014
        self.tracker.predict()                                                     # :1028-1029
        self.tracker.update(dets)
        self.counter.step(self.tracker)
        return skipped, boxes1, dets
