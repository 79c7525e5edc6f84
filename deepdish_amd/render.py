"""Annotated output frames (csrc/render.hip): the reference's overlay (deepdish.py:295-408, 1187-1207) painted over frames in HBM.

A frame's overlay is a list of primitive records, int32 [k, 8], painted in order (a later record overwrites an earlier one):

    rects(tlbr, rgb)                    rectangle outlines, Pillow's ImageDraw.rectangle byte for byte
    lines(a, b, width, rgb)             segments a[i] - b[i]: every pixel within width / 2 of the segment (odd widths 1 .. 15)
    polylines(points, counts, ...)      several polylines at once, segment by segment (round caps close the joints)
    Renderer.text(x, y, string, rgb)    Pillow's ImageDraw.text at the truncated position, byte for byte, through a coverage atlas

Record set 2, which a Renderer(..., records=2) accepts (the default renderer refuses it, as it always has):

    fills(tlbr, rgb)                    filled rectangles, Pillow's ImageDraw.rectangle(fill=...) byte for byte (corners inclusive)
    lines(a, b, width, rgb, even=True)  the same capsule rule for widths 1 .. 15 of either parity

Each returns such an array; np.concatenate them in paint order and hand one array per output frame to Renderer.draw:

    r = Renderer(480, 640)
    prims = np.concatenate([lines([[320, 0]], [[320, 480]], 3, (0, 0, 255)), rects([[10.5, 20, 80, 200]], (255, 255, 255)),
                            r.text(10.5, 20, 'person', (0, 255, 0))])
    out = r.draw(frames_dev, [prims, EMPTY], streams=[2, 0])       # u8 [2, 480, 640, 3] BGR on the device

Coordinates are floats or ints: truncated toward zero (upstream's np.int32(...), Pillow's int()), then clamped to -8192 .. 8191; an
element with a non-finite coordinate is dropped.  Colours are RGB as upstream gives them; the frames are BGR.  overlay_primitives builds
the reference's whole overlay from the state a pipeline keeps (MultiStreamPipeline.render, HotPath.render)."""
import ctypes

import numpy as np

from ._lib import lib, check, P

KIND_RECT, KIND_LINE, KIND_MASK, KIND_FILL = 0, 1, 2, 3
COORD_MIN, COORD_MAX, MAX_SIDE = -8192, 8191, 8192
EMPTY = np.zeros((0, 8), dtype=np.int32)


def ink(rgb):
    r, g, b = (int(v) & 255 for v in rgb)
    return b | (g << 8) | (r << 16)


def _coords(values, ncol):
    """floats [k, ncol] -> (int32 [k, ncol] truncated toward zero and clamped, rows whose values are all finite)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1, ncol)
    ok = np.isfinite(v).all(axis=1)
    return np.clip(np.trunc(np.where(np.isfinite(v), v, 0.0)), COORD_MIN, COORD_MAX).astype(np.int32), ok


def _records(kind, xyxy, arg, rgb):
    out = np.zeros((len(xyxy), 8), dtype=np.int32)
    out[:, 0] = kind
    out[:, 1:5] = xyxy
    out[:, 5] = arg
    out[:, 6] = ink(rgb)
    return out


def rects(tlbr, rgb):
    """Rectangle outlines [x0, y0, x1, y1] (deepdish.py:303-305).  Pillow refuses x1 < x0 or y1 < y0; such a box is dropped here."""
    c, ok = _coords(tlbr, 4)
    ok &= (c[:, 2] >= c[:, 0]) & (c[:, 3] >= c[:, 1])
    return _records(KIND_RECT, c[ok], 0, rgb)


def fills(tlbr, rgb):
    """Filled rectangles [x0, y0, x1, y1], both corners inclusive (deepdish.py:418-420, :437-438).  Pillow refuses x1 < x0 or y1 < y0; such
    a box is dropped here.  Record set 2."""
    c, ok = _coords(tlbr, 4)
    ok &= (c[:, 2] >= c[:, 0]) & (c[:, 3] >= c[:, 1])
    return _records(KIND_FILL, c[ok], 0, rgb)


def _width(width, even=False):
    width = int(width)
    if width < 1 or width > 15 or (width % 2 == 0 and not even):
        raise ValueError('line width %d: %swidths 1 .. 15' % (width, '' if even else 'odd '))
    return width


def lines(a, b, width, rgb, even=False):
    """Segments a[i] - b[i] ([k, 2] each); a zero-length segment is a disc.  even=True: a width of either parity (record set 2)."""
    c, ok = _coords(np.concatenate([np.asarray(a, np.float64).reshape(-1, 2), np.asarray(b, np.float64).reshape(-1, 2)], axis=1), 4)
    return _records(KIND_LINE, c[ok], _width(width, even), rgb)


def polylines(points, counts, width, rgb):
    """points [sum(counts), 2]: polylines of counts[i] points each, behind one another (deepdish.py:335-338 Line.do_render).  A polyline
    with a non-finite coordinate is dropped whole; one of fewer than two points has no segment."""
    c, ok = _coords(points, 2)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    assert counts.sum() == len(c)
    if len(c) < 2:
        return _records(KIND_LINE, np.zeros((0, 4), np.int32), _width(width), rgb)
    owner = np.repeat(np.arange(len(counts)), counts)
    bad = np.bincount(owner, weights=~ok, minlength=len(counts)) > 0
    keep = (owner[:-1] == owner[1:]) & ~bad[owner[:-1]]
    return _records(KIND_LINE, np.concatenate([c[:-1], c[1:]], axis=1)[keep], _width(width), rgb)


def pack(per_frame):
    """list of record arrays, one per output frame -> (records int32 [total, 8], offsets int32 [n + 1])."""
    arrs = [np.asarray(a, dtype=np.int32).reshape(-1, 8) for a in per_frame]
    off = np.zeros(len(arrs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in arrs])
    flat = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if arrs else EMPTY
    return flat, off


def unpack(records, offsets):
    return [records[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def default_font(W):
    """deepdish.py:238-247 loads FreeSansBold at int(24 / 640 * W); that file is not shipped, so Pillow's default face at that size (the
    bitmap default where Pillow has no FreeType)."""
    from PIL import ImageFont
    try:
        return ImageFont.load_default(size=max(1, int(24 / 640 * W)))
    except (OSError, TypeError, ValueError):
        return ImageFont.load_default()


def text_size(font, s):
    """font.getsize(s) as deepdish.py:396-406 calls it; Pillow 10 removed it and names getbbox(s)[2:4] as the replacement."""
    return tuple(int(v) for v in font.getbbox(s)[2:4])


class Renderer:
    """One canvas size, one font, one coverage atlas on the device.  A string is rasterised once (font.getmask2, or getmask for a bitmap
    font, as ImageDraw.text does) and lives in the atlas from then on."""

    def __init__(self, H, W, font=None, context=None, records=1):
        from .runtime import default_context
        self.ctx = context or default_context()
        self.H, self.W = int(H), int(W)
        self.font = font if font is not None else default_font(self.W)
        h = P()
        check(lib().dd_render_create(self.ctx.handle, self.H, self.W, ctypes.byref(h)), 'dd_render_create')
        self._h = h
        self.records = int(records)           # 1: outlines, odd-width lines, masks; 2: fills and even widths too (the top-down view needs them)
        if self.records != 1:
            check(lib().dd_render_record_set(self._h, self.records), 'dd_render_record_set')
        self._strings = {}                 # string -> (atlas offset, w, h, off_x, off_y), or None for a string without a pixel
        self.cache_hits = self.cache_misses = 0

    def __del__(self):
        try:
            if self._h:
                lib().dd_render_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def put_mask(self, mask):
        """u8 [h, w] coverage -> its atlas offset."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        off = ctypes.c_int()
        check(lib().dd_render_put_mask(self._h, P(m.ctypes.data), m.shape[1], m.shape[0], ctypes.byref(off)), 'dd_render_put_mask')
        return off.value

    def _string(self, s):
        if s in self._strings:
            self.cache_hits += 1
            return self._strings[s]
        self.cache_misses += 1
        from PIL import Image
        try:
            core, off = self.font.getmask2(s, 'L')
        except AttributeError:
            core, off = self.font.getmask(s, 'L'), (0, 0)
        entry = None
        if core.size[0] > 0 and core.size[1] > 0:
            m = np.array(Image.Image()._new(core).convert('L'))
            entry = (self.put_mask(m), m.shape[1], m.shape[0], int(off[0]), int(off[1]))
        self._strings[s] = entry
        return entry

    def text(self, x, y, s, rgb):
        """ImageDraw.text((x, y), s, fill=rgb, font=self.font) -> [0 or 1, 8].  The reference passes float positions and FreeType then
        rasterises at the fractional offset; here the position is truncated first."""
        c, ok = _coords([[x, y]], 2)
        entry = self._string(str(s))
        if entry is None or not ok[0]:
            return EMPTY
        off, w, h, ox, oy = entry
        px, py = int(c[0, 0]) + ox, int(c[0, 1]) + oy
        if px >= self.W or py >= self.H or px + w <= 0 or py + h <= 0:      # nothing of it on the canvas
            return EMPTY
        return _records(KIND_MASK, np.array([[px, py, w, h]], dtype=np.int32), off, rgb)

    def draw(self, frames_dev, primitives, streams=None, out=None):
        """frames_dev: u8 [n_frames, H, W, 3] (or [H, W, 3]) BGR torch tensor in HBM; primitives: one record array per output frame;
        streams: the frame each output frame is made from (default: all, in order).  -> u8 [len(streams), H, W, 3] on the device, queued
        on the context's stream (out: a tensor to write instead of a new one; never the frames themselves)."""
        import torch
        if frames_dev.dim() == 3:
            frames_dev = frames_dev[None]
        assert tuple(frames_dev.shape[1:]) == (self.H, self.W, 3) and frames_dev.dtype == torch.uint8 and frames_dev.is_contiguous()
        streams = np.arange(frames_dev.shape[0], dtype=np.int32) if streams is None else np.ascontiguousarray(list(streams), dtype=np.int32)
        if len(primitives) != len(streams):
            raise ValueError('%d record arrays for %d output frames' % (len(primitives), len(streams)))
        recs, off = pack(primitives)
        if out is None:
            out = torch.empty((len(streams), self.H, self.W, 3), dtype=torch.uint8, device=frames_dev.device)
        assert tuple(out.shape) == (len(streams), self.H, self.W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
        check(lib().dd_render_draw(self._h, P(frames_dev.data_ptr()), int(frames_dev.shape[0]), P(streams.ctypes.data), len(streams),
                                   P(recs.ctypes.data) if len(recs) else P(None), P(off.ctypes.data), P(out.data_ptr()), None), 'dd_render_draw')
        return out


def annotation_kind(annotation):
    a = str(annotation).lower()                # deepdish.py:1080-1085 --object-annotation
    if a not in ('label', 'id', 'none'):
        raise ValueError("annotation must be 'label', 'id' or 'none', got %r" % (annotation,))
    return a


def topdown_primitives(view_w, view_h, ground_points, point_counts, scale):
    """The top-down panel of one frame (deepdish.py:410-440): the black panel [0, 0, int(view_w), int(view_h)], then per track its
    marker -- a fill from trunc(q_last - 1) to trunc(q_last + 1) -- and its path, the polyline through trunc(q) in width 2, with
    q = g * scale * (1, -1) + (view_w / 2, view_h) for ground points g (:429; view_w, view_h untruncated there).  Nothing is clipped to
    the panel.  A non-finite ground point drops the marker or the segments that touch it.  -> (panel [1, 8], elements [k, 8])."""
    g = np.asarray(ground_points, dtype=np.float64).reshape(-1, 2)
    counts = np.asarray(point_counts, dtype=np.int64).reshape(-1)
    assert counts.sum() == len(g)
    q = g * np.asarray(scale, dtype=np.float64) * np.array([1.0, -1.0]) + np.array([view_w * 0.5, view_h * 1.0])
    green = (0, 255, 0)
    parts, at = [], 0
    for n in counts:                                                  # per track: the marker lies under the track's own path
        t = q[at:at + n]
        at += n
        if n:
            parts.append(fills(np.concatenate([t[-1] - 1.0, t[-1] + 1.0]), green))
            parts.append(lines(t[:-1], t[1:], 2, green, even=True))
    panel = fills([0, 0, int(view_w), int(view_h)], (0, 0, 0))
    return panel, (np.concatenate(parts, axis=0) if parts else EMPTY)


def overlay_primitives(renderer, line, track_ids, track_labels, track_tlbr, points, point_counts, crossings, det_tlbr, counters,
                       annotation='label', topdown=None):
    """One frame's overlay in the reference's paint order (a stable sort by priority, deepdish.py:1194):
        2  count line, width 3, RGB (0, 0, 255)                                     :354-359, :972
        3  the whole path of every drawn track with >= 2 points, width 3, (255, 0, 255)      :340-345, :1066-1069
        4  this step's crossing segments, width 5, (0, 0, 255)                      :347-352, :1122
        5  the detections given to the tracker, outline (255, 0, 0)                 :295-305, :1125-1127
        6  per track: outline (255, 255, 255), then its text at the top-left, (0, 255, 0)    :307-326, :1086
        9  with topdown: the black panel in the top-left corner                     :410-420
        10 with topdown: per track its marker, then its ground path in width 2, (0, 255, 0)  :422-440, :1088-1097
        10 counters, from the bottom edge up, labels reversed                       :378-408
    topdown = (view_w, view_h, ground_points, scale): the panel's size (W / 4, H / 4 upstream, not truncated), `points` unprojected to
    the ground (GroundPlane.space_from_image) and the metres -> pixels factors; see topdown_primitives.
    track_*: the confirmed tracks with time_since_update <= 1, in track order; points / point_counts: their paths behind one another;
    counters: (label, negcount, poscount) in the order of the wanted labels."""
    annotation = annotation_kind(annotation)
    W, H, font = renderer.W, renderer.H, renderer.font
    track_tlbr = np.asarray(track_tlbr, dtype=np.float64).reshape(-1, 4)
    parts = [lines([line[0:2]], [line[2:4]], 3, (0, 0, 255)),
             polylines(points, point_counts, 3, (255, 0, 255)),
             lines(np.asarray(crossings, np.float64).reshape(-1, 4)[:, :2], np.asarray(crossings, np.float64).reshape(-1, 4)[:, 2:], 5, (0, 0, 255)),
             rects(det_tlbr, (255, 0, 0))]
    for k in range(len(track_tlbr)):                                 # the text of track k lies under the outline of track k + 1
        txt = str(track_ids[k]) if annotation == 'id' else (track_labels[k] or '') if annotation == 'label' else ''
        parts.append(rects(track_tlbr[k], (255, 255, 255)))
        parts.append(renderer.text(track_tlbr[k, 0], track_tlbr[k, 1], txt, (0, 255, 0)))
    if topdown is not None:
        view_w, view_h, ground_points, scale = topdown
        parts.extend(topdown_primitives(view_w, view_h, ground_points, point_counts, scale))
    cursor = H
    for label, neg, pos in reversed(list(counters)):
        cursor -= text_size(font, str(neg))[1]
        parts.append(renderer.text(0, cursor, str(neg), (255, 0, 0)))
        parts.append(renderer.text((W - text_size(font, label)[0]) / 2, cursor, label, (0, 255, 0)))
        parts.append(renderer.text(W - text_size(font, str(pos))[0], cursor, str(pos), (0, 0, 255)))
    return np.concatenate(parts, axis=0)
