"""CPU restatement of the overlay csrc/render.hip paints (numpy + Pillow): the definition the kernel is held to.

What upstream does: deepdish.py:295-408 (the render elements and their do_render), :971-974, :1066-1086, :1122-1134 (where a frame's
elements are made) and :1187-1207 (stable sort by priority, paint with Pillow, RGBA -> BGR).  What is pinned to what:

    base         the BGR frame itself (cleared back buffer + pasted camera image + the final conversion); colours are RGB upstream
    rectangle    Pillow's ImageDraw.rectangle(outline=...), byte for byte (rect_mask; tests/test_render_ref.py checks it against Pillow)
    text         Pillow's ImageDraw.text at the truncated position, byte for byte: the font's coverage mask blended with blend()
    line         this build's own rule (line_mask): a capsule in exact integers, not Pillow's polygon fill
    coordinates  truncated toward zero (np.int32(...) upstream, int() inside Pillow), clamped to COORD_MIN .. COORD_MAX; an element with
                 a non-finite coordinate is skipped

An element here is a tuple whose first two fields are its kind and priority:
    ('line', priority, [x0, y0, x1, y1, ...], width, rgb)      a polyline, painted segment by segment
    ('rect', priority, [x0, y0, x1, y1], rgb)
    ('text', priority, (x, y), string, rgb)
"""
import math

import numpy as np
from PIL import Image, ImageFont

COORD_MIN, COORD_MAX, MAX_SIDE = -8192, 8191, 8192


def default_font(W):
    """deepdish.py:238-247 loads FreeSansBold at int(24 / 640 * W); that file is not shipped, so Pillow's default face at that size."""
    size = max(1, int(24 / 640 * W))
    try:
        return ImageFont.load_default(size=size)
    except (OSError, TypeError, ValueError):      # no FreeType: the bitmap default
        return ImageFont.load_default()


def text_size(font, s):
    """font.getsize(s) of deepdish.py:396-406, which Pillow 10 removed: its deprecation note names getbbox(s)[2:4]."""
    return tuple(int(v) for v in font.getbbox(s)[2:4])


def coords(values):
    """floats -> ints as upstream's np.int32(...) (truncation toward zero), clamped; None when one is not finite."""
    out = []
    for v in values:
        v = float(v)
        if not math.isfinite(v):
            return None
        out.append(min(max(int(v), COORD_MIN), COORD_MAX))
    return out


def rect_mask(H, W, x0, y0, x1, y1):
    """Pixels ImageDraw.rectangle([x0, y0, x1, y1], outline=...) colours (x1 >= x0, y1 >= y0): both horizontal edges, and the vertical edges
    as Pillow draws them -- lines from row y0 + 1 to row y1, which for y1 == y0 run backwards over rows y0 and y0 + 1."""
    yy, xx = np.mgrid[0:H, 0:W]
    ylo, yhi = min(y0 + 1, y1), max(y0 + 1, y1)
    horizontal = ((yy == y0) | (yy == y1)) & (xx >= x0) & (xx <= x1)
    vertical = ((xx == x0) | (xx == x1)) & (yy >= ylo) & (yy <= yhi)
    return horizontal | vertical


def line_mask(H, W, ax, ay, bx, by, w):
    """The capsule of odd width w around segment a-b, in exact integers: with d = b - a, L2 = d.d, t = (p - a).d, c = (p - a) x d, pixel p
    is painted iff  t <= 0: 4 |p - a|^2 <= w^2;  t >= L2: 4 |p - b|^2 <= w^2;  otherwise 4 c^2 <= w^2 L2."""
    assert w % 2 == 1 and 1 <= w <= 15
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    dx, dy = int(bx) - int(ax), int(by) - int(ay)
    L2 = dx * dx + dy * dy
    px, py, qx, qy = xx - ax, yy - ay, xx - bx, yy - by
    t = px * dx + py * dy
    c = px * dy - py * dx
    return np.where(t <= 0, 4 * (px * px + py * py) <= w * w, np.where(t >= L2, 4 * (qx * qx + qy * qy) <= w * w, 4 * c * c <= w * w * L2))


def blend(dst, m, ink):
    """Pillow's paint-through-mask (Paste.c / Draw.c): t = dst (255 - m) + ink m + 128; ((t >> 8) + t) >> 8.  Any integer arrays."""
    t = np.asarray(dst, np.int64) * (255 - np.asarray(m, np.int64)) + np.asarray(ink, np.int64) * m + 128
    return ((t >> 8) + t) >> 8


def text_mask(font, s):
    """-> (coverage u8 [h, w], (off_x, off_y)) as ImageDraw.text obtains it (getmask2, or getmask for a bitmap font), or None when empty."""
    try:
        core, off = font.getmask2(s, 'L')
    except AttributeError:
        core, off = font.getmask(s, 'L'), (0, 0)
    if core.size[0] == 0 or core.size[1] == 0:
        return None
    m = np.array(Image.Image()._new(core).convert('L'))
    return m, (int(off[0]), int(off[1]))


def blit(img, x, y, mask, bgr):
    """mask pasted at (x, y) with ink bgr, clipped to img (u8 [H, W, 3]), in place."""
    H, W = img.shape[:2]
    h, w = mask.shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if x0 >= x1 or y0 >= y1:
        return
    m = mask[y0 - y:y1 - y, x0 - x:x1 - x, None]
    img[y0:y1, x0:x1] = blend(img[y0:y1, x0:x1], m, np.array(bgr)[None, None, :]).astype(np.uint8)


def paint(frame_bgr, elements, font=None):
    """-> the annotated frame, u8 [H, W, 3] BGR: `elements` stably sorted by priority (deepdish.py:1194) and painted in that order."""
    H, W = frame_bgr.shape[:2]
    assert H <= MAX_SIDE and W <= MAX_SIDE
    out = np.array(frame_bgr, dtype=np.uint8, copy=True)
    font = font or default_font(W)
    for e in sorted(elements, key=lambda e: e[1]):
        kind = e[0]
        if kind == 'rect':                                           # deepdish.py:303-305
            c = coords(e[2])
            if c is not None:
                out[rect_mask(H, W, *c)] = e[3][::-1]
        elif kind == 'line':                                         # :335-338; segment by segment, a zero-length one is a disc
            c = coords(e[2])
            if c is not None:
                for i in range(0, len(c) - 3, 2):
                    out[line_mask(H, W, c[i], c[i + 1], c[i + 2], c[i + 3], e[3])] = e[4][::-1]
        elif kind == 'text':                                         # :326
            c = coords(e[2])
            tm = text_mask(font, str(e[3]))
            if c is not None and tm is not None:
                blit(out, c[0] + tm[1][0], c[1] + tm[1][1], tm[0], e[4][::-1])
        else:
            raise ValueError(kind)
    return out


def overlay_elements(W, H, line, tracks, crossings, detections, counters, annotation='label', font=None):
    """The element list of one frame in upstream's insertion order (its priorities then decide the paint order):
    line [x0, y0, x1, y1]; tracks: (track_id, label, tlbr, path [[x, y], ...]) per confirmed track with time_since_update <= 1, in track
    order; crossings: [x0, y0, x1, y1] per crossing of this step; detections: tlbr rows; counters: (label, negcount, poscount) in the
    order of the wanted labels."""
    font = font or default_font(W)
    el = [('line', 2, list(line), 3, (0, 0, 255))]                  # :972 CameraCountLine
    for tid, label, tlbr, path in tracks:
        if len(path) > 1:                                            # :1066-1069 TrackedPath
            el.append(('line', 3, [v for p in path for v in p], 3, (255, 0, 255)))
        txt = str(tid) if annotation == 'id' else (label or '') if annotation == 'label' else ''      # :1080-1085
        el.append(('rect', 6, list(tlbr), (255, 255, 255)))         # :1086 TrackedObject: outline, then text at the box's top-left
        el.append(('text', 6, (tlbr[0], tlbr[1]), txt, (0, 255, 0)))
    for c in crossings:                                              # :1122 TrackedPathIntersection
        el.append(('line', 4, list(c), 5, (0, 0, 255)))
    for d in detections:                                             # :1125-1127 DetectedObject
        el.append(('rect', 5, list(d), (255, 0, 0)))
    cursor = H                                                       # :391-408 CountingStats
    for label, neg, pos in reversed(list(counters)):
        cursor -= text_size(font, str(neg))[1]
        el.append(('text', 10, (0, cursor), str(neg), (255, 0, 0)))
        el.append(('text', 10, ((W - text_size(font, label)[0]) / 2, cursor), label, (0, 255, 0)))
        el.append(('text', 10, (W - text_size(font, str(pos))[0], cursor), str(pos), (0, 0, 255)))
    return el


def paint_records(frame_bgr, records, masks):
    """The same painter over packed records (deepdish_amd/render.py: int32 [k, 8] = kind, four coordinates, arg, ink, 0), in order.
    masks: atlas offset -> coverage u8 [h, w]."""
    H, W = frame_bgr.shape[:2]
    out = np.array(frame_bgr, dtype=np.uint8, copy=True)
    for kind, a, b, c, d, arg, ink, _ in np.asarray(records).reshape(-1, 8).tolist():
        bgr = (ink & 255, (ink >> 8) & 255, (ink >> 16) & 255)
        if kind == 0:
            out[rect_mask(H, W, a, b, c, d)] = bgr
        elif kind == 1:
            out[line_mask(H, W, a, b, c, d, arg)] = bgr
        else:
            assert masks[arg].shape == (d, c)
            blit(out, a, b, masks[arg], bgr)
    return out
