"""CPU restatement of the top-down view (numpy + Pillow): the definition csrc/ground_dev.h, csrc/ground.hip and the fill / even-width part
of csrc/render.hip are held to.  It extends tests/render_ref.py by importing it.

What upstream does: deepdish.py:592-611 builds a cameratransform camera (rectilinear projection + spatial orientation) from lens and
mounting data, :1088-1097 sends every drawn track's bottom-centre path through cam.spaceFromImage, :410-440 paints a black panel in the
frame's corner (priority 9) and per track a marker and the ground path in width 2 (priority 10).  cameratransform is not installed
here: the geometry is restated from its published definition and its parity with the package is NOT pinned.

    camera(...)            the 9 doubles of dd_ground_camera: fx, fy, cx, cy, e, cos tilt, sin tilt, cos roll, sin roll
    space_from_image(...)  float64, in the operation order of csrc/ground_dev.h -- one IEEE operation per numpy operation, nothing fused --
                           so the host entry and the kernel must equal it bit for bit:
                               a = (u - cx) / fx              b = -(v - cy) / fy
                               a' = cos r * a - sin r * b     b' = sin r * a + cos r * b
                               den = cos t - sin t * b'
                               X = (e * a') / den             Y = (e * (cos t * b' + sin t)) / den
                           den <= 0 (the ray never reaches the ground), a non-finite input or a non-finite result -> (NaN, NaN).
                           That rule is this build's decision; upstream hands such a pixel to the package unchecked.
    fill_mask(...)         Pillow's ImageDraw.rectangle(xy, fill=ink) with no outline: x0 <= x <= x1, y0 <= y <= y1
    capsule_mask(...)      render_ref.line_mask's rule for a width of either parity (exact integers for any w)
    topdown_elements(...)  the panel, markers and polylines of one frame; element_coords(...) gives them as integer coordinates in paint order
    overlay_elements(...)  render_ref.overlay_elements with them in upstream's place: in front of the counters

New element kinds, beside render_ref's ('line' | 'rect' | 'text'):
    ('fill', priority, [x0, y0, x1, y1], rgb)
    ('segments', priority, [[ax, ay, bx, by], ...], width, rgb)      segments on their own: one with a non-finite end is skipped alone
"""
import math

import numpy as np

import render_ref
from render_ref import COORD_MIN, COORD_MAX, blit, coords, default_font, rect_mask, text_mask      # noqa: F401

CAMERA_DOUBLES = 9
GREEN = (0, 255, 0)


def camera(f_mm, sensor_mm, image, elevation_m, tilt_deg, roll_deg=0.0):
    """-> f64 [9].  math.cos / math.sin are the C library's, as in dd_ground_camera."""
    (sw, sh), (W, H) = sensor_mm, image
    t, r = tilt_deg * (math.pi / 180.0), roll_deg * (math.pi / 180.0)
    return np.array([f_mm / sw * W, f_mm / sh * H, W / 2.0, H / 2.0, elevation_m, math.cos(t), math.sin(t), math.cos(r), math.sin(r)], dtype=np.float64)


def space_from_image(cams, points, cam_index=None):
    """cams f64 [n_cams, 9] (or [9]); points f64 [n, 2]; cam_index int [n] (default: camera 0) -> f64 [n, 2]."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, CAMERA_DOUBLES)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    idx = np.zeros(len(p), dtype=np.int64) if cam_index is None else np.asarray(cam_index, dtype=np.int64)
    assert ((idx >= 0) & (idx < len(cams))).all()
    fx, fy, cx, cy, e, ct, st, cr, sr = (cams[idx, k] for k in range(CAMERA_DOUBLES))
    u, v = p[:, 0], p[:, 1]
    with np.errstate(all='ignore'):
        a = (u - cx) / fx
        b = -(v - cy) / fy
        ar = cr * a - sr * b
        br = sr * a + cr * b
        den = ct - st * br
        x = (e * ar) / den
        y = (e * (ct * br + st)) / den
        ok = np.isfinite(u) & np.isfinite(v) & (den > 0.0) & np.isfinite(x) & np.isfinite(y)
    out = np.full((len(p), 2), np.nan, dtype=np.float64)
    out[ok, 0], out[ok, 1] = x[ok], y[ok]
    return out


def fill_mask(H, W, x0, y0, x1, y1):
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)


def capsule_mask(H, W, ax, ay, bx, by, w):
    """render_ref.line_mask for widths 1 .. 15 of either parity: pixel p is painted iff, with d = b - a, L2 = d.d, t = (p - a).d,
    c = (p - a) x d:  t <= 0: 4 |p - a|^2 <= w^2;  t >= L2: 4 |p - b|^2 <= w^2;  otherwise 4 c^2 <= w^2 L2."""
    assert 1 <= w <= 15
    if w % 2 == 1:
        return render_ref.line_mask(H, W, ax, ay, bx, by, w)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    dx, dy = int(bx) - int(ax), int(by) - int(ay)
    L2 = dx * dx + dy * dy
    px, py, qx, qy = xx - ax, yy - ay, xx - bx, yy - by
    t = px * dx + py * dy
    c = px * dy - py * dx
    return np.where(t <= 0, 4 * (px * px + py * py) <= w * w, np.where(t >= L2, 4 * (qx * qx + qy * qy) <= w * w, 4 * c * c <= w * w * L2))


def topdown_elements(W, H, ground_paths, scale=(1.0, 1.0)):
    """The top-down elements of one frame in upstream's insertion order.  W, H: the frame; ground_paths: per drawn track, in track order,
    its ground path f64 [k, 2] (k >= 1); scale: metres -> pixels.  With (view_w, view_h) = (W / 4, H / 4), NOT truncated (:601, :429):
        q = g * scale * (1, -1) + (view_w / 2, view_h)
        per track  ('fill', 10, trunc(q_last - 1) ++ trunc(q_last + 1), green)            :435-438, width / 2 = 1
                   ('segments', 10, trunc(q[i]) ++ trunc(q[i + 1]) for every i, 2, green) :439-440
        and once   ('fill', 9, [0, 0, int(view_w), int(view_h)], black)                     :414-420
    Coordinates stay floats here; paint() truncates them (toward zero, as np.array(..., dtype=int)), skipping what is not finite."""
    vw, vh = W / 4, H / 4
    el = []
    for g in ground_paths:
        g = np.asarray(g, dtype=np.float64).reshape(-1, 2)
        q = g * np.asarray(scale, dtype=np.float64) * np.array([1.0, -1.0]) + np.array([vw * 0.5, vh * 1.0])
        el.append(('fill', 10, list(q[-1] - 1.0) + list(q[-1] + 1.0), GREEN))
        el.append(('segments', 10, [list(q[i]) + list(q[i + 1]) for i in range(len(q) - 1)], 2, GREEN))
    el.append(('fill', 9, [0, 0, int(vw), int(vh)], (0, 0, 0)))
    return el


def overlay_elements(W, H, line, tracks, crossings, detections, counters, annotation='label', font=None, ground_paths=(), scale=(1.0, 1.0)):
    """render_ref.overlay_elements with the top-down view: upstream appends a track's TopDownObj inside its track loop (:1097), long before
    the counters (:1134 on), and both have priority 10 -- the stable sort keeps the markers and paths UNDER the counters.  So the top-down
    elements are inserted in front of the counters' texts here.  ground_paths: one per track, in track order."""
    base = render_ref.overlay_elements(W, H, line, tracks, crossings, detections, counters, annotation, font=font)
    n = 3 * len(list(counters))
    assert all(e[0] == 'text' and e[1] == 10 for e in base[len(base) - n:])
    return base[:len(base) - n] + topdown_elements(W, H, ground_paths, scale) + base[len(base) - n:]


def element_coords(elements):
    """The fills and segments of `elements` in paint order with integer coordinates, as the painter sees them:
    ('fill', [x0, y0, x1, y1], rgb) and ('segment', [ax, ay, bx, by], width, rgb); dropped ones are left out."""
    out = []
    for e in sorted(elements, key=lambda e: e[1]):
        if e[0] == 'fill':
            c = coords(e[2])
            if c is not None and c[2] >= c[0] and c[3] >= c[1]:
                out.append(('fill', c, e[3]))
        elif e[0] == 'segments':
            for s in e[2]:
                c = coords(s)
                if c is not None:
                    out.append(('segment', c, e[3], e[4]))
    return out


def paint(frame_bgr, elements, font=None):
    """render_ref.paint with the two new element kinds: stable sort by priority, then in order."""
    H, W = frame_bgr.shape[:2]
    out = np.array(frame_bgr, dtype=np.uint8, copy=True)
    font = font or default_font(W)
    for e in sorted(elements, key=lambda e: e[1]):
        if e[0] == 'fill':
            c = coords(e[2])
            if c is not None and c[2] >= c[0] and c[3] >= c[1]:      # Pillow refuses reversed corners; it cannot happen for a marker
                out[fill_mask(H, W, *c)] = e[3][::-1]
        elif e[0] == 'segments':
            for s in e[2]:
                c = coords(s)
                if c is not None:
                    out[capsule_mask(H, W, c[0], c[1], c[2], c[3], e[3])] = e[4][::-1]
        else:
            out = render_ref.paint(out, [e], font=font)
    return out


def paint_records(frame_bgr, records, masks):
    """render_ref.paint_records with kind 3 and lines of either parity."""
    H, W = frame_bgr.shape[:2]
    out = np.array(frame_bgr, dtype=np.uint8, copy=True)
    for kind, a, b, c, d, arg, ink, _ in np.asarray(records).reshape(-1, 8).tolist():
        bgr = (ink & 255, (ink >> 8) & 255, (ink >> 16) & 255)
        if kind == 0:
            out[rect_mask(H, W, a, b, c, d)] = bgr
        elif kind == 1:
            out[capsule_mask(H, W, a, b, c, d, arg)] = bgr
        elif kind == 2:
            assert masks[arg].shape == (d, c)
            blit(out, a, b, masks[arg], bgr)
        elif kind == 3:
            out[fill_mask(H, W, a, b, c, d)] = bgr
        else:
            raise ValueError(kind)
    return out
