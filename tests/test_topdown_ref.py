"""CPU: tests/topdown_ref.py, the definition of the top-down view, held to what it is meant to be -- the geometry to a forward projection
written here from rotation matrices (not from the closed form the ref and the kernel use), the filled rectangle to Pillow byte for
byte, the even-width capsule to the rule in Python integers, the element list to values worked out by hand, the whole frame to Pillow.
deepdish_amd/render.py's record builders are held to the ref's elements here too, without a device."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import render_ref  # noqa: E402
import topdown_ref  # noqa: E402

SENSOR, F_MM = (6.17, 4.55), 3.6                 # fx = 373.4, fy = 379.8 at 640 x 480: fx != fy
TILTS, ROLLS = (0.0, 30.0, 60.0, 85.0), (0.0, 10.0, -10.0)
IMAGES = ((640, 480), (1280, 720))
ELEVATION = 4.0

# The largest relative round-trip error topdown_ref.space_from_image makes on _ground_points() over every camera of
# test_round_trip_through_an_independent_forward_projection, in float64, measured once (see that test's docstring).
MEASURED_ROUND_TRIP = 1.14e-15


def _rx(t):
    """World -> camera for a tilt t: 0 looks straight down, 90 degrees at the horizon towards +Y."""
    c, s = math.cos(t), math.sin(t)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]])


def _rz(r):
    c, s = math.cos(r), math.sin(r)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def _project(cam_args, ground):
    """Forward projection of ground points [n, 2] (Z = 0): p_c = Rz(roll) Rx(tilt) (p - C), the camera looks along -z_c with x_c to the
    right and y_c up; u = cx + fx x_c / (-z_c), v = cy - fy y_c / (-z_c).  -> (pixels [n, 2], depth -z_c [n])."""
    f_mm, (sw, sh), (W, H), e, tilt, roll = cam_args
    fx, fy, cx, cy = f_mm / sw * W, f_mm / sh * H, W / 2, H / 2
    p = np.concatenate([np.asarray(ground, np.float64), np.zeros((len(ground), 1))], axis=1) - np.array([0.0, 0.0, e])
    pc = p @ (_rz(math.radians(roll)) @ _rx(math.radians(tilt))).T
    depth = -pc[:, 2]
    return np.stack([cx + fx * pc[:, 0] / depth, cy - fy * pc[:, 1] / depth], axis=1), depth


def _ground_points():
    x, y = np.meshgrid(np.linspace(-6.0, 6.0, 13), np.linspace(-3.0, 20.0, 24))
    return np.stack([x.ravel() + 0.03125, y.ravel() + 0.0625], axis=1)


def _cameras():
    for image, tilt, roll in itertools.product(IMAGES, TILTS, ROLLS):
        yield (F_MM, SENSOR, image, ELEVATION, tilt, roll)


def _round_trip_errors():
    worst = 0.0
    used = 0
    for args in _cameras():
        g = _ground_points()
        px, depth = _project(args, g)
        front = depth > 0.05 * np.linalg.norm(np.concatenate([g, np.full((len(g), 1), args[3])], axis=1), axis=1)      # well in front of the camera
        back = topdown_ref.space_from_image(topdown_ref.camera(*args), px[front])
        assert np.isfinite(back).all(), args
        err = np.linalg.norm(back - g[front], axis=1) / np.maximum(np.linalg.norm(g[front], axis=1), args[3])
        worst = max(worst, float(err.max()))
        used += int(front.sum())
    return worst, used


def test_round_trip_through_an_independent_forward_projection():
    """Ground points on a 13 x 24 grid over -6 .. 6 m by -3 .. 20 m, projected by _project and unprojected by the ref, come back: for
    tilts 0, 30, 60, 85 degrees x rolls 0, +-10 degrees x a 640 x 480 and a 1280 x 720 camera with fx != fy, points well in front of the
    camera.  The error is |back - p| / max(|p|, elevation).  Measured: the ref's largest error over all 7 152 of them is 1.14e-15 in float64
    (five units in the last place); 16 x that, 1.8e-14, is allowed: head-room for another summation order."""
    worst, used = _round_trip_errors()
    print('largest relative round-trip error %.3g over %d points' % (worst, used))
    assert used > 4000
    assert worst <= 16 * MEASURED_ROUND_TRIP


def test_the_library_s_host_entry_makes_the_same_round_trip():
    """The product's own code (dd_ground_camera + the host path of dd_ground_from_image) under the same check and the same bound."""
    from deepdish_amd.ground import GroundPlane
    worst = 0.0
    for args in _cameras():
        g = _ground_points()
        px, depth = _project(args, g)
        front = depth > 0.05 * np.linalg.norm(np.concatenate([g, np.full((len(g), 1), args[3])], axis=1), axis=1)
        cam = GroundPlane(args[0], sensor_mm=args[1], image=args[2], elevation_m=args[3], tilt_deg=args[4], roll_deg=args[5])
        back = cam.space_from_image(px[front])
        err = np.linalg.norm(back - g[front], axis=1) / np.maximum(np.linalg.norm(g[front], axis=1), args[3])
        worst = max(worst, float(err.max()))
    assert worst <= 16 * MEASURED_ROUND_TRIP


def test_known_values():
    for (W, H), tilt in itertools.product(IMAGES, TILTS):
        cam = topdown_ref.camera(F_MM, SENSOR, (W, H), ELEVATION, tilt)
        got = topdown_ref.space_from_image(cam, [[W / 2, H / 2]])[0]      # the principal point lands at (0, e tan tilt)
        assert abs(got[0]) <= 1e-12 and got[1] == pytest.approx(ELEVATION * math.tan(math.radians(tilt)), rel=1e-12, abs=1e-12)
    cam = topdown_ref.camera(F_MM, SENSOR, (640, 480), ELEVATION, 0.0)
    right, above = topdown_ref.space_from_image(cam, [[400.0, 240.0], [320.0, 100.0]])
    assert right[0] > 0 and right[1] == 0 and above[1] > 0 and above[0] == 0
    assert right[0] == pytest.approx(ELEVATION * 80.0 / (F_MM / SENSOR[0] * 640), rel=1e-14)
    # tilt 60 degrees: the row v = cy - fy tan 30 is the horizon; it and every row above it yield NaN, the rows below it do not
    cam = topdown_ref.camera(F_MM, SENSOR, (640, 480), ELEVATION, 60.0)
    horizon = cam[3] - cam[1] * math.tan(math.radians(30.0))
    assert 0 < horizon < 240
    rows = np.arange(0, 480, dtype=np.float64)
    for u in (0.0, 320.0, 639.0):
        g = topdown_ref.space_from_image(cam, np.stack([np.full(480, u), rows], axis=1))
        assert np.isnan(g[rows <= math.floor(horizon - 1e-9)]).all() and np.isfinite(g[rows >= math.ceil(horizon + 1e-9)]).all()
    assert np.isnan(topdown_ref.space_from_image(cam, [[320.0, horizon]])).all() or topdown_ref.space_from_image(cam, [[320.0, horizon]])[0, 1] > 1e12
    assert np.isnan(topdown_ref.space_from_image(cam, [[320.0, horizon - 1e-6]])).all()
    # the elevation scales X and Y linearly
    pts = np.array([[100.0, 300.0], [500.0, 470.0], [320.0, 200.0]])
    one = topdown_ref.space_from_image(topdown_ref.camera(F_MM, SENSOR, (640, 480), 1.0, 60.0, 10.0), pts)
    eight = topdown_ref.space_from_image(topdown_ref.camera(F_MM, SENSOR, (640, 480), 8.0, 60.0, 10.0), pts)
    np.testing.assert_array_equal(eight, 8.0 * one)                  # a power of two: exactly
    three = topdown_ref.space_from_image(topdown_ref.camera(F_MM, SENSOR, (640, 480), 3.0, 60.0, 10.0), pts)
    np.testing.assert_allclose(three, 3.0 * one, rtol=4e-16)


# ------------------------------------------------------------------ filled rectangle
def _pillow_fill(W, H, box, base=None):
    im = Image.new('L', (W, H), 0) if base is None else base
    ImageDraw.Draw(im).rectangle(list(box), fill=255)
    return np.array(im) == 255


def test_filled_rectangle_equals_pillow():
    """Every box with 0 <= x0 <= x1 < 14 and 0 <= y0 <= y1 < 14 on a 14 x 14 canvas (equal corners included); boxes partly and wholly
    outside; the panel [0, 0, 160, 120] on 640 x 480, which is 161 x 121 pixels."""
    N = 14
    spans = [(a, b) for a in range(N) for b in range(a, N)]
    n = 0
    for (x0, x1), (y0, y1) in itertools.product(spans, repeat=2):
        np.testing.assert_array_equal(topdown_ref.fill_mask(N, N, x0, y0, x1, y1), _pillow_fill(N, N, (x0, y0, x1, y1)), err_msg=str((x0, y0, x1, y1)))
        n += 1
    assert n == 105 * 105
    for box in ((-3, -3, 4, 5), (10, 9, 20, 30), (-5, 4, 30, 6), (5, -9, 6, 40), (-4, -4, 20, 20), (-9, -9, -2, -2), (14, 0, 20, 13), (0, 14, 13, 14),
                (-1, 0, -1, 13), (13, 13, 13, 13), (-2, 13, 0, 15), (20, 20, 30, 30)):
        np.testing.assert_array_equal(topdown_ref.fill_mask(N, N, *box), _pillow_fill(N, N, box), err_msg=str(box))
    panel = topdown_ref.fill_mask(480, 640, 0, 0, 160, 120)
    np.testing.assert_array_equal(panel, _pillow_fill(640, 480, (0, 0, 160, 120)))
    assert int(panel.sum()) == 161 * 121 and panel[120, 160] and not panel[121, 160] and not panel[120, 161]


# ------------------------------------------------------------------ even-width capsule
def _brute(H, W, ax, ay, bx, by, w):
    """The rule, pixel by pixel, in Python integers."""
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        py, qy = y - ay, y - by
        for x in range(W):
            px, qx = x - ax, x - bx
            t = px * dx + py * dy
            if t <= 0:
                out[y, x] = 4 * (px * px + py * py) <= w * w
            elif t >= L2:
                out[y, x] = 4 * (qx * qx + qy * qy) <= w * w
            else:
                c = px * dy - py * dx
                out[y, x] = 4 * c * c <= w * w * L2
    return out


@pytest.mark.parametrize('width', [2, 4, 6])
def test_even_width_capsule_equals_the_rule_in_python_integers(width):
    """Every segment between the points of a 9 x 9 grid (6 561, the zero-length ones included), on an 11 x 11 canvas that leaves a
    one-pixel margin around the grid."""
    N = 11
    grid = list(itertools.product(range(1, 10), repeat=2))
    painted = 0
    for (ax, ay), (bx, by) in itertools.product(grid, repeat=2):
        got = topdown_ref.capsule_mask(N, N, ax, ay, bx, by, width)
        np.testing.assert_array_equal(got, _brute(N, N, ax, ay, bx, by, width), err_msg=str((ax, ay, bx, by)))
        assert got[ay, ax] and got[by, bx]
        painted += int(got.sum())
    assert painted > 0
    # a zero-length segment of width 2 is the centre and its four neighbours: |p - a| <= 1
    disc = topdown_ref.capsule_mask(5, 5, 2, 2, 2, 2, 2)
    assert disc.tolist() == [[False] * 5, [False, False, True, False, False], [False, True, True, True, False], [False, False, True, False, False], [False] * 5]


def test_odd_widths_are_render_ref_s_own():
    for w, seg in itertools.product((1, 3, 5, 15), ((0, 0, 13, 9), (5, 5, 5, 5), (12, 1, -3, 7))):
        np.testing.assert_array_equal(topdown_ref.capsule_mask(14, 14, *seg, w), render_ref.line_mask(14, 14, *seg, w))


def _dilate(m):
    p = np.pad(m, 1)
    return np.any([p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)


def test_width_2_relation_to_pillow_is_measured_not_asserted():
    """As tests/test_render_ref.py does for odd widths: endpoints -2 .. 15 on a 14 x 14 canvas, one segment in five.  Printed: the share
    of the union's pixels on which Pillow's draw.line(width=2) and the rule differ, and how many segments have a Pillow pixel farther
    than one pixel from every pixel of the rule.  README carries the figures; nothing is asserted about them."""
    N = 14
    segs = list(itertools.product(range(-2, 16), repeat=4))[::5]
    differ = union = outside = 0
    for ax, ay, bx, by in segs:
        im = Image.new('L', (N, N), 0)
        ImageDraw.Draw(im).line([ax, ay, bx, by], fill=255, width=2)
        pil = np.array(im) == 255
        rule = topdown_ref.capsule_mask(N, N, ax, ay, bx, by, 2)
        outside += int((pil & ~_dilate(rule)).any())
        differ += int((pil ^ rule).sum())
        union += int((pil | rule).sum())
    print('width 2: the rules differ on %.3f of the union (%d segments); %d segments have a Pillow pixel farther than one pixel from the rule'
          % (differ / union, len(segs), outside))
    assert len(segs) >= 20000 and union > 0


# ------------------------------------------------------------------ the element list
def test_topdown_elements_on_a_hand_made_scene():
    """642 x 482 frame: view = (160.5, 120.5), so q's x offset is 80.25 (not 80) and the panel's corner is (160, 120).
    topdownview_size_m = (20, 10): scale = (160.5 / 20, 120.5 / 10) = (8.025, 12.05).  Three tracks with 1, 2 and 5 ground points, one of
    the five NaN (above the horizon).  Worked out by hand below: q = (80.25 + 8.025 X, 120.5 - 12.05 Y)."""
    W, H = 642, 482
    scale = np.array([W / 4, H / 4]) / np.array([20.0, 10.0])
    assert scale.tolist() == [8.025, 12.05]
    nan = float('nan')
    paths = [[[0.0, 0.0]],                                            # q = (80.25, 120.5)
             [[1.0, 2.0], [-2.0, 4.0]],                               # q = (88.275, 96.4), (64.2, 72.3)
             [[10.0, 1.0], [4.0, 8.0], [nan, nan], [-12.0, 0.5], [-11.0, 11.0]]]      # (160.5, 108.45), (112.35, 24.1), -, (-16.05, 114.475), (-8.025, -12.05)
    el = topdown_ref.topdown_elements(W, H, paths, scale)
    assert [e[0] for e in el] == ['fill', 'segments'] * 3 + ['fill'] and [e[1] for e in el] == [10] * 6 + [9]
    want = [('fill', [0, 0, 160, 120], (0, 0, 0)),
            ('fill', [79, 119, 81, 121], (0, 255, 0)),
            ('fill', [63, 71, 65, 73], (0, 255, 0)), ('segment', [88, 96, 64, 72], 2, (0, 255, 0)),
            ('fill', [-9, -13, -7, -11], (0, 255, 0)),               # trunc(-9.025) = -9, trunc(-7.025) = -7: toward zero
            ('segment', [160, 108, 112, 24], 2, (0, 255, 0)), ('segment', [-16, 114, -8, -12], 2, (0, 255, 0))]
    assert topdown_ref.element_coords(el) == want
    # the untruncated view_w / 2 = 80.25 decides at X = 1.97: 80.25 + 15.809 = 96.06 -> marker 95 .. 97; with 80 it would be 94 .. 96
    el2 = topdown_ref.topdown_elements(W, H, [[[1.97, 0.0]]], scale)
    assert topdown_ref.element_coords(el2)[1] == ('fill', [95, 119, 97, 121], (0, 255, 0))
    # a marker on a NaN head is dropped, the segment into it too
    el3 = topdown_ref.topdown_elements(W, H, [[[1.0, 2.0], [nan, nan]]], scale)
    assert topdown_ref.element_coords(el3) == [want[0]]
    # scale (1, 1) on 640 x 480: q = (80 + X, 120 - Y)
    el4 = topdown_ref.topdown_elements(640, 480, [[[3.5, 2.5]]])
    assert topdown_ref.element_coords(el4) == [('fill', [0, 0, 160, 120], (0, 0, 0)), ('fill', [82, 116, 84, 118], (0, 255, 0))]


def _scene(W, H):
    tracks = [(7, 'person', [30.5, 40.5, 90.0, 200.0], [[60.0, 200.0]]),
              (9, 'person', [300.0, 100.0, 380.0, 300.0], [[330.0, 290.0], [340.0, 300.0]]),
              (12, 'person', [400.0, 50.0, 470.0, 260.0], [[430.0, 250.0], [432.0, 252.0], [433.0, 10.0], [434.0, 258.0], [435.0, 260.0]])]
    return tracks, dict(line=[W // 2, 0, W // 2, H], crossings=[], detections=[[28.0, 38.0, 92.0, 204.0]], counters=[('person', 3, 14)])


def test_paint_order_and_the_product_s_records_equal_the_ref():
    """The whole overlay of a three-track scene with the top-down view, built twice: by the ref (elements, stable sort by priority) and by
    deepdish_amd/render.py (records in paint order, no device needed for the builders).  The panel comes after every track text, the
    markers and paths after the panel and before the counters; the records' integer coordinates equal the ref's."""
    from deepdish_amd import render as rd
    from deepdish_amd.ground import GroundPlane
    W, H = 642, 482
    font = render_ref.default_font(640)
    tracks, rest = _scene(W, H)
    cam = GroundPlane(F_MM, sensor_mm=SENSOR, image=(W, H), elevation_m=ELEVATION, tilt_deg=60.0, roll_deg=2.0)
    ground = [topdown_ref.space_from_image(cam.table, np.array(t[3])) for t in tracks]
    assert np.isnan(ground[2][2]).all() and np.isfinite(ground[2][[0, 1, 3, 4]]).all()      # (433, 10) lies above the horizon
    scale = np.array([W / 4, H / 4]) / np.array([20.0, 10.0])
    el = topdown_ref.overlay_elements(W, H, rest['line'], tracks, rest['crossings'], rest['detections'], rest['counters'], 'label', font=font,
                                      ground_paths=ground, scale=scale)
    order = sorted(el, key=lambda e: e[1])
    kinds = [(e[0], e[1]) for e in order]
    panel_at = kinds.index(('fill', 9))
    assert max(i for i, k in enumerate(kinds) if k[1] == 6) < panel_at < kinds.index(('fill', 10))
    assert max(i for i, k in enumerate(kinds) if k[0] in ('fill', 'segments')) < min(i for i, k in enumerate(kinds) if k == ('text', 10))

    class _Texts:                                                    # Renderer.text without a device: position and string only
        W, H, font = 642, 482, render_ref.default_font(640)

        def text(self, x, y, s, rgb):
            return np.array([[rd.KIND_MASK, int(x), int(y), 0, 0, 0, rd.ink(rgb), 0]], dtype=np.int32)
    pts = np.concatenate([np.array(t[3]) for t in tracks])
    counts = [len(t[3]) for t in tracks]
    recs = rd.overlay_primitives(_Texts(), [W // 2, 0, W // 2, H], [t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks], pts, counts,
                                 np.zeros((0, 4)), [[28.0, 38.0, 92.0, 204.0]], [('person', 3, 14)], 'label',
                                 topdown=(W / 4, H / 4, cam.space_from_image(pts), scale))
    got = [('fill', r[1:5].tolist(), r[6]) if r[0] == rd.KIND_FILL else ('segment', r[1:5].tolist(), int(r[5]), r[6])
           for r in recs if r[0] == rd.KIND_FILL or (r[0] == rd.KIND_LINE and r[5] == 2)]
    want = [(e[0], e[1], rd.ink(e[2])) if e[0] == 'fill' else (e[0], e[1], e[2], rd.ink(e[3])) for e in topdown_ref.element_coords(el)]
    assert got == want and len(want) == 1 + 3 + 1 + 2
    kinds = recs[:, 0].tolist()
    first_fill = kinds.index(rd.KIND_FILL)
    assert recs[first_fill, 1:5].tolist() == [0, 0, 160, 120] and recs[first_fill, 6] == 0
    assert kinds[first_fill - 1] == rd.KIND_MASK and kinds[first_fill - 2] == rd.KIND_RECT                  # after the last track's box and text
    assert kinds[-3:] == [rd.KIND_MASK] * 3 and set(kinds[first_fill:-3]) == {rd.KIND_FILL, rd.KIND_LINE}      # before the counters
    # without topdown the records are the leading and trailing ones of the above
    plain = rd.overlay_primitives(_Texts(), [W // 2, 0, W // 2, H], [t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks], pts, counts,
                                  np.zeros((0, 4)), [[28.0, 38.0, 92.0, 204.0]], [('person', 3, 14)], 'label')
    np.testing.assert_array_equal(plain, np.concatenate([recs[:first_fill], recs[-3:]]))


def test_record_builders():
    from deepdish_amd import render as rd
    f = rd.fills([[10.9, -3.9, 20.2, 5.5], [float('nan'), 0, 1, 1], [-1e9, -1e9, 1e9, 1e9], [5, 5, 4, 9], [3, 3, 3, 3]], (1, 2, 3))
    assert f.tolist() == [[3, 10, -3, 20, 5, 0, 3 | 2 << 8 | 1 << 16, 0], [3, -8192, -8192, 8191, 8191, 0, 3 | 2 << 8 | 1 << 16, 0],
                          [3, 3, 3, 3, 3, 0, 3 | 2 << 8 | 1 << 16, 0]]
    for w in range(1, 16):
        assert rd.lines([[0, 0]], [[5, 5]], w, (0, 0, 0), even=True)[0, 5] == w
    for bad in (0, 16, -2):
        with pytest.raises(ValueError):
            rd.lines([[0, 0]], [[1, 1]], bad, (0, 0, 0), even=True)
    with pytest.raises(ValueError):                                  # without even=True an even width is refused, as before
        rd.lines([[0, 0]], [[1, 1]], 2, (0, 0, 0))
    panel, rest = rd.topdown_primitives(160.0, 120.0, np.zeros((0, 2)), [], (1.0, 1.0))
    assert panel.tolist() == [[3, 0, 0, 160, 120, 0, 0, 0]] and len(rest) == 0


def test_whole_frame_equals_pillow_when_no_path_has_two_points():
    """Pillow draws everything but lines.  A scene whose tracks all have one-point paths (and a zero-length count line, which the capsule
    rule and nothing else paints, left out): outlines, texts, panel, markers and counters by ImageDraw calls in priority order."""
    W, H = 320, 240
    font = render_ref.default_font(W)
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    tracks = [(1, 'person', [20.5, 30.5, 70.0, 150.0], [[45.0, 150.0]]), (2, 'person', [10.0, 5.0, 90.0, 60.0], [[50.0, 60.0]]),
              (3, 'bicycle', [200.0, 100.0, 260.0, 200.0], [[230.0, 200.0]])]
    cam = topdown_ref.camera(F_MM, SENSOR, (W, H), ELEVATION, 40.0)
    ground = [topdown_ref.space_from_image(cam, np.array(t[3])) for t in tracks]
    assert all(np.isfinite(g).all() for g in ground)
    scale = np.array([W / 4, H / 4]) / np.array([20.0, 10.0])
    allel = [e for e in topdown_ref.overlay_elements(W, H, [0, 0, 0, 0], tracks, [], [[18.0, 28.0, 72.0, 152.0]], [('person', 2, 5)], 'label', font=font,
                                                     ground_paths=ground, scale=scale) if e[0] != 'line']
    got = topdown_ref.paint(frame, allel, font=font)
    im = Image.fromarray(np.ascontiguousarray(frame[..., ::-1]), 'RGB')
    d = ImageDraw.Draw(im)
    for e in sorted(allel, key=lambda e: e[1]):
        if e[0] == 'rect':
            d.rectangle([int(v) for v in e[2]], outline=e[3])
        elif e[0] == 'text':
            d.text((int(e[2][0]), int(e[2][1])), e[3], fill=e[4], font=font)
        elif e[0] == 'fill':
            d.rectangle([int(v) for v in e[2]], fill=e[3])
        else:
            assert e[0] == 'segments' and e[2] == []
    np.testing.assert_array_equal(got[..., ::-1], np.array(im))
    inside = got[:61, :81]
    assert (inside == 0).all(axis=-1).sum() > 60 * 80 * 0.9 and ((inside == (0, 255, 0)).all(axis=-1)).sum() >= 9      # a black panel with green markers
