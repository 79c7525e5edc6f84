"""CPU: tests/render_ref.py (the definition csrc/render.hip is held to) against Pillow, and the record packing of deepdish_amd/render.py.

Rectangles, the mask blend and text are Pillow's, byte for byte.  Lines are this build's own capsule rule: every pixel Pillow's draw.line
colours lies within one pixel (Chebyshev) of a pixel the rule colours; the reverse does not hold (round caps, clipping) and is not asserted."""
import itertools
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import render_ref  # noqa: E402

STRINGS = ('person', '12', 'bicycle 7', '')


def test_rectangle_outline_equals_pillow():
    """Every box with corners in -2 .. 9 on an 8 x 8 canvas, x1 >= x0 and y1 >= y0, the degenerate ones included."""
    n = 0
    for x0, y0 in itertools.product(range(-2, 10), repeat=2):
        for x1, y1 in itertools.product(range(x0, 10), range(y0, 10)):
            im = Image.new('L', (8, 8), 0)
            ImageDraw.Draw(im).rectangle([x0, y0, x1, y1], outline=255)
            np.testing.assert_array_equal(render_ref.rect_mask(8, 8, x0, y0, x1, y1), np.array(im) == 255, err_msg=str((x0, y0, x1, y1)))
            n += 1
    assert n == 78 * 78
    assert render_ref.rect_mask(8, 8, 5, 5, 5, 5).sum() == 2 and render_ref.rect_mask(8, 8, 5, 5, 6, 5).sum() == 4


def test_blend_equals_pillow_for_every_dst_mask_ink():
    """All 256^3 (dst, mask, ink) through ImageDraw.bitmap: one 256 x 256 (mask across, dst down) image per ink."""
    dst, m = np.mgrid[0:256, 0:256]
    mask = Image.fromarray(m.astype(np.uint8), 'L')
    for ink in range(256):
        im = Image.fromarray(dst.astype(np.uint8), 'L')
        ImageDraw.Draw(im).bitmap((0, 0), mask, fill=ink)
        np.testing.assert_array_equal(render_ref.blend(dst, m, ink), np.array(im), err_msg='ink %d' % ink)


@pytest.mark.parametrize('mode', ['RGB', 'RGBA'])
def test_text_equals_pillow(mode):
    """Default font; inside, at negative offsets, clipped at the right and bottom edges.  RGBA with alpha 255 is the reference's buffer."""
    W, H = 160, 48
    font = render_ref.default_font(640)
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)           # RGB
    painted = 0
    for s in STRINGS:
        for x, y in ((10, 8), (-7, -5), (W - 20, 10), (30, H - 16), (W - 8, H - 14), (-400, 5)):
            if mode == 'RGB':
                im = Image.fromarray(base, 'RGB')
            else:
                im = Image.fromarray(np.dstack([base, np.full((H, W, 1), 255, np.uint8)]), 'RGBA')
            ImageDraw.Draw(im).text((x, y), s, fill=(10, 250, 130), font=font)
            want = np.array(im)[..., :3]
            got = render_ref.paint(base[..., ::-1], [('text', 6, (x, y), s, (10, 250, 130))], font=font)[..., ::-1]
            np.testing.assert_array_equal(got, want, err_msg=repr((s, x, y)))
            painted += int((want != base).any())
    assert painted == 15                                           # every string but the empty one, everywhere but at x = -400


def test_text_position_is_truncated_toward_zero():
    font = render_ref.default_font(640)
    base = np.zeros((40, 120, 3), np.uint8)
    a = render_ref.paint(base, [('text', 6, (3.9, -2.7), 'person', (255, 255, 255))], font=font)
    b = render_ref.paint(base, [('text', 6, (3, -2), 'person', (255, 255, 255))], font=font)
    np.testing.assert_array_equal(a, b)
    assert a.any()
    np.testing.assert_array_equal(render_ref.paint(base, [('text', 6, (float('nan'), 2), 'person', (255, 255, 255))], font=font), base)


def _dilate(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


@pytest.mark.parametrize('width', [1, 3, 5, 7])
def test_every_pillow_line_pixel_is_within_one_pixel_of_the_rule(width):
    """Endpoints -2 .. 15 on a 14 x 14 canvas, one segment in five.  The share of the union's pixels on which the two rules differ is
    printed, not asserted."""
    N = 14
    segs = list(itertools.product(range(-2, 16), repeat=4))[::5]
    assert len(segs) >= 20000
    differ = union = 0
    for ax, ay, bx, by in segs:
        im = Image.new('L', (N, N), 0)
        ImageDraw.Draw(im).line([ax, ay, bx, by], fill=255, width=width)
        pil = np.array(im) == 255
        rule = render_ref.line_mask(N, N, ax, ay, bx, by, width)
        assert not (pil & ~_dilate(rule)).any(), (ax, ay, bx, by)
        differ += int((pil ^ rule).sum())
        union += int((pil | rule).sum())
    print('width %d: the rules differ on %.3f of the union (%d segments)' % (width, differ / union, len(segs)))


def test_line_rule_against_python_integers_at_the_coordinate_limits():
    """Coordinates at +-8191 / -8192: the int64 arithmetic of line_mask against the same rule in Python's unbounded integers."""
    def brute(H, W, ax, ay, bx, by, w, pixels):
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        out = []
        for (x, y) in pixels:
            px, py = x - ax, y - ay
            t = px * dx + py * dy
            if t <= 0:
                out.append(4 * (px * px + py * py) <= w * w)
            elif t >= L2:
                out.append(4 * ((x - bx) ** 2 + (y - by) ** 2) <= w * w)
            else:
                out.append(4 * (px * dy - py * dx) ** 2 <= w * w * L2)
        return out
    H = W = 24
    rng = np.random.default_rng(3)
    pixels = [(int(x), int(y)) for x, y in rng.integers(0, 24, (60, 2))] + [(0, 0), (23, 23), (0, 23), (23, 0), (11, 12), (12, 11)]
    cases = [(-8192, -8192, 8191, 8191), (8191, -8192, -8192, 8191), (-8192, 11, 8191, 12), (12, -8192, 11, 8191), (8191, 8191, 8191, 8191),
             (-8192, -8191, 8191, 8190), (0, 0, 8191, 8191), (-8192, 5, 5, 5), (3, 3, 3, 3), (8191, 0, 0, 8191), (-8192, 8191, 23, 0)]
    painted = 0
    for (ax, ay, bx, by), w in itertools.product(cases, (1, 3, 7, 15)):
        m = render_ref.line_mask(H, W, ax, ay, bx, by, w)
        want = brute(H, W, ax, ay, bx, by, w, pixels)
        assert [bool(m[y, x]) for x, y in pixels] == want, (ax, ay, bx, by, w)
        painted += int(m.sum())
    assert painted > 500


def test_composition_equals_pillow_calls_in_priority_order():
    """A hand-made element set, inserted out of priority order: the painted frame equals the same elements drawn with Pillow calls in
    priority order (stable), the line rule substituted for draw.line."""
    W, H = 96, 64
    font = render_ref.default_font(640)
    rng = np.random.default_rng(9)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)           # BGR
    el = [('text', 10, (0, 50.0), '3', (255, 0, 0)),
          ('rect', 6, [20.7, 10.2, 60.9, 50.5], (255, 255, 255)),
          ('text', 6, (20.7, 10.2), 'person', (0, 255, 0)),
          ('rect', 6, [22.0, 12.0, 70.0, 40.0], (255, 255, 255)),     # painted over the first track's text
          ('text', 6, (22.0, 12.0), 'bicycle 7', (0, 255, 0)),
          ('line', 4, [30.5, 40.5, 52.2, 44.9], 5, (0, 0, 255)),
          ('rect', 5, [18, 8, 58, 52], (255, 0, 0)),
          ('line', 3, [10.0, 60.0, 25.5, 45.5, 30.5, 40.5, 52.2, 44.9], 3, (255, 0, 255)),
          ('line', 2, [48, 0, 48, 64], 3, (0, 0, 255)),
          ('rect', 5, [float('nan'), 8, 58, 52], (9, 9, 9)),          # skipped
          ('rect', 5, [-5.5, -3.5, 200.0, 9000.0], (255, 0, 0))]
    got = render_ref.paint(frame, el, font=font)
    im = Image.fromarray(np.ascontiguousarray(frame[..., ::-1]), 'RGB')
    for e in sorted(el, key=lambda e: e[1]):
        draw = ImageDraw.Draw(im)
        c = render_ref.coords(e[2])
        if c is None:
            continue
        if e[0] == 'rect':
            draw.rectangle(c, outline=e[3])
        elif e[0] == 'text':
            draw.text((c[0], c[1]), e[3], fill=e[4], font=font)
        else:
            a = np.array(im)
            for i in range(0, len(c) - 3, 2):
                a[render_ref.line_mask(H, W, c[i], c[i + 1], c[i + 2], c[i + 3], e[3])] = e[4]
            im = Image.fromarray(a, 'RGB')
    np.testing.assert_array_equal(got[..., ::-1], np.array(im))
    # the order matters: the same elements with the priorities of the two track boxes' group and the detections swapped differ
    swapped = [(e[0], {5: 6, 6: 5}.get(e[1], e[1])) + e[2:] for e in el]
    assert (render_ref.paint(frame, swapped, font=font) != got).any()


def test_overlay_elements_follow_the_reference_s_layout():
    font = render_ref.default_font(640)
    el = render_ref.overlay_elements(640, 480, [320, 0, 320, 480], [(7, 'person', [10.5, 20.5, 50.0, 90.0], [[30, 90], [32, 92], [35, 95]]),
                                                                      (9, 'person', [100, 20, 150, 90], [[125, 90]])],
                                     [[32, 92, 35, 95]], [[11, 21, 51, 91]], [('person', 2, 5), ('car', 0, 1)], annotation='id', font=font)
    kinds = [(e[0], e[1]) for e in el]
    assert kinds == [('line', 2), ('line', 3), ('rect', 6), ('text', 6), ('rect', 6), ('text', 6), ('line', 4), ('rect', 5)] + [('text', 10)] * 6
    assert [e[3] for e in el if e[:2] == ('text', 6)] == ['7', '9']
    texts = [e for e in el if e[1] == 10]
    assert [t[3] for t in texts] == ['0', 'car', '1', '2', 'person', '5']          # labels reversed, cursor going up
    h0 = render_ref.text_size(font, '0')[1]
    assert texts[0][2] == (0, 480 - h0) and texts[3][2][1] == 480 - h0 - render_ref.text_size(font, '2')[1]
    assert texts[1][2][0] == (640 - render_ref.text_size(font, 'car')[0]) / 2 and texts[2][2][0] == 640 - render_ref.text_size(font, '1')[0]


def test_record_packing_without_a_device():
    """deepdish_amd/render.py: floats are truncated toward zero and clamped, non-finite elements dropped, polylines split into segments,
    and pack / unpack are inverse."""
    from deepdish_amd import render as rd
    r = rd.rects([[10.9, -3.9, 20.2, 5.5], [float('inf'), 0, 1, 1], [-1e9, -1e9, 1e9, 1e9], [5, 5, 4, 9]], (1, 2, 3))
    assert r.tolist() == [[0, 10, -3, 20, 5, 0, 3 | 2 << 8 | 1 << 16, 0], [0, -8192, -8192, 8191, 8191, 0, 3 | 2 << 8 | 1 << 16, 0]]
    pts = [[0.5, 0.5], [3.9, 4.1], [7, 7],   [1, 1],   [2, 2], [float('nan'), 3], [4, 4],   [9.9, 9.9], [-9.9, -9.9]]
    seg = rd.polylines(pts, [3, 1, 3, 2], 3, (255, 0, 255))
    assert seg[:, 1:6].tolist() == [[0, 0, 3, 4, 3], [3, 4, 7, 7, 3], [9, 9, -9, -9, 3]]
    assert (seg[:, 0] == rd.KIND_LINE).all() and (seg[:, 6] == (255 | 255 << 16)).all()
    assert len(rd.polylines(np.zeros((0, 2)), [], 3, (0, 0, 0))) == 0 and len(rd.polylines([[1, 1]], [1], 3, (0, 0, 0))) == 0
    ln = rd.lines([[1.5, 2.5]], [[1.5, 2.5]], 5, (0, 0, 255))
    assert ln.tolist() == [[1, 1, 2, 1, 2, 5, 255, 0]]
    for bad in (0, 2, 17, -1):
        with pytest.raises(ValueError):
            rd.lines([[0, 0]], [[1, 1]], bad, (0, 0, 0))
    flat, off = rd.pack([r, rd.EMPTY, seg, ln])
    assert flat.dtype == np.int32 and flat.flags.c_contiguous and off.tolist() == [0, 2, 2, 5, 6]
    back = rd.unpack(flat, off)
    for a, b in zip(back, [r, rd.EMPTY, seg, ln]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        rd.annotation_kind('both')
    assert rd.annotation_kind('ID') == 'id'
