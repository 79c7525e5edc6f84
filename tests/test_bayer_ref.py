"""CPU: the numpy restatement of the 8-bit Bayer / monochrome -> BGR converter (tests/bayer_ref.py) against a per-pixel scalar loop written
straight from the rule's sentences, the identities the rule implies, one hand-computed frame, and the C ABI of the conversion and of the
ring that takes such frames: entries bound and exported, bad arguments answered with a code and a message that names the function and the
argument -- without a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bayer_ref  # noqa: E402

PATTERNS = bayer_ref.PATTERNS
SHAPES = [(3, 3), (4, 4), (5, 7), (18, 3), (3, 18)]             # (W, H)


def _scalar(m, pattern):
    """The rule, one pixel at a time."""
    H, W = m.shape
    m = m.astype(int)
    block = pattern[6:]
    colour = lambda x, y: block[(y & 1) * 2 + (x & 1)]
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            cx, cy = min(max(x, 1), W - 2), min(max(y, 1), H - 2)
            here = colour(cx, cy)
            n, s, w, e = m[cy - 1, cx], m[cy + 1, cx], m[cy, cx - 1], m[cy, cx + 1]
            v = {}
            if here in 'rb':
                v[here] = m[cy, cx]
                v['g'] = (n + s + w + e + 2) >> 2
                v['b' if here == 'r' else 'r'] = (m[cy - 1, cx - 1] + m[cy - 1, cx + 1] + m[cy + 1, cx - 1] + m[cy + 1, cx + 1] + 2) >> 2
            else:
                v['g'] = m[cy, cx]
                v[colour(cx - 1, cy)] = (w + e + 1) >> 1
                v[colour(cx, cy - 1)] = (n + s + 1) >> 1
            out[y, x] = (v['b'], v['g'], v['r'])
    return out


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H', SHAPES)
def test_ref_equals_the_scalar_loop(pattern, W, H):
    rng = np.random.default_rng(W * 100 + H)
    for m in (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.choice(np.array([0, 1, 254, 255], np.uint8), (H, W))):
        got = bayer_ref.bayer_to_bgr(m, H, W, pattern)
        assert got.shape == (H, W, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, _scalar(m, pattern))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H', SHAPES)
def test_flat_colour_and_to_bayer_round_trip(pattern, W, H):
    """A mosaic of a constant colour comes back as that colour everywhere; synth.to_bayer makes that mosaic."""
    from deepdish_amd.synth import to_bayer
    bgr = (201, 14, 77)
    mosaic = to_bayer(np.broadcast_to(np.array(bgr, np.uint8), (H, W, 3)), pattern)
    assert mosaic.shape == (H, W) and mosaic.dtype == np.uint8
    col = bayer_ref.site_colours(pattern, H, W)
    for k, ch in enumerate('bgr'):
        assert (mosaic[col == ch] == bgr[k]).all()
    assert (bayer_ref.bayer_to_bgr(mosaic, H, W, pattern) == np.array(bgr, np.uint8)).all()


@pytest.mark.parametrize('pattern', PATTERNS)
def test_ramp_is_exact_in_the_interior(pattern):
    """Each channel a ramp with even steps per pixel: every average the rule takes is the value at the site itself."""
    from deepdish_amd.synth import to_bayer
    H, W = 7, 10
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([10 + 4 * x + 2 * y, 200 - 2 * x - 6 * y, 3 + 2 * x + 8 * y], axis=-1).astype(np.uint8)
    got = bayer_ref.bayer_to_bgr(to_bayer(img, pattern), H, W, pattern)
    np.testing.assert_array_equal(got[1:-1, 1:-1], img[1:-1, 1:-1])


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H', SHAPES)
def test_border_repeats_its_inner_neighbour(pattern, W, H):
    m = np.random.default_rng(7).integers(0, 256, (H, W), dtype=np.uint8)
    got = bayer_ref.bayer_to_bgr(m, H, W, pattern)
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[-1], got[-2])
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    np.testing.assert_array_equal(got[:, -1], got[:, -2])


@pytest.mark.parametrize('W,H', SHAPES)
def test_patterns_are_tied_to_each_other(W, H):
    """Swapping R and B in the filter swaps them in the picture; dropping the first column or row of an RGGB mosaic leaves a GRBG / GBRG one,
    away from the border (whose ring sits one pixel further in after the drop)."""
    m = np.random.default_rng(W + 31 * H).integers(0, 256, (H, W), dtype=np.uint8)
    ref = bayer_ref.bayer_to_bgr
    np.testing.assert_array_equal(ref(m, H, W, 'bayer_rggb'), ref(m, H, W, 'bayer_bggr')[..., ::-1])
    np.testing.assert_array_equal(ref(m, H, W, 'bayer_grbg'), ref(m, H, W, 'bayer_gbrg')[..., ::-1])
    if W >= 4:
        np.testing.assert_array_equal(ref(np.ascontiguousarray(m[:, 1:]), H, W - 1, 'bayer_grbg')[1:-1, 1:-1], ref(m, H, W, 'bayer_rggb')[1:-1, 2:-1])
    if H >= 4:
        np.testing.assert_array_equal(ref(np.ascontiguousarray(m[1:]), H - 1, W, 'bayer_gbrg')[1:-1, 1:-1], ref(m, H, W, 'bayer_rggb')[2:-1, 1:-1])


def test_hand_computed_frame():
    """RGGB, 4 x 4.  Sites: row 0 R G R G, row 1 G B G B, row 2 R G R G, row 3 G B G B.
    D(1, 1), a B site 64:  G = (200 + 18 + 33 + 250 + 2) >> 2 = 125, R = (12 + 7 + 101 + 77 + 2) >> 2 = 49
    D(2, 1), G 250 on a blue row:  B = (64 + 5 + 1) >> 1 = 35, R = (7 + 77 + 1) >> 1 = 42
    D(1, 2), G 18 on a red row:  R = (101 + 77 + 1) >> 1 = 89, B = (64 + 222 + 1) >> 1 = 143
    D(2, 2), an R site 77:  G = (250 + 41 + 18 + 140 + 2) >> 2 = 112, B = (64 + 5 + 222 + 3 + 2) >> 2 = 74"""
    m = np.array([[12, 200, 7, 90], [33, 64, 250, 5], [101, 18, 77, 140], [9, 222, 41, 3]], np.uint8)
    d11, d21, d12, d22 = (64, 125, 49), (35, 250, 42), (143, 18, 89), (74, 112, 77)
    want = np.array([[d11, d11, d21, d21], [d11, d11, d21, d21], [d12, d12, d22, d22], [d12, d12, d22, d22]], np.uint8)
    np.testing.assert_array_equal(bayer_ref.bayer_to_bgr(m, 4, 4, 'bayer_rggb'), want)


def test_pitch_and_gray():
    m = np.random.default_rng(5).integers(0, 256, (5, 9), dtype=np.uint8)
    for pattern in PATTERNS:
        np.testing.assert_array_equal(bayer_ref.bayer_to_bgr(m.reshape(-1), 5, 7, pattern, pitch=9),
                                      bayer_ref.bayer_to_bgr(np.ascontiguousarray(m[:, :7]), 5, 7, pattern))
    g = bayer_ref.raw8_to_bgr(m.reshape(-1), 5, 7, 'gray', pitch=9)
    assert g.shape == (5, 7, 3)
    for c in range(3):
        np.testing.assert_array_equal(g[..., c], m[:, :7])
    assert bayer_ref.raw8_to_bgr(np.array([9], np.uint8), 1, 1, 'gray').tolist() == [[[9, 9, 9]]]


def test_to_gray_keeps_grey_levels():
    """synth.to_gray's weights sum to 2^14: a grey pixel keeps its level; pure colours give BT.601's luma.  It pins nothing."""
    from deepdish_amd.synth import to_gray
    lv = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(to_gray(np.repeat(lv[None, :, None], 3, axis=2)), lv[None])
    assert to_gray(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() == [[29, 150, 76]]
    with pytest.raises(ValueError, match='nope'):
        from deepdish_amd.synth import to_bayer
        to_bayer(np.zeros((4, 4, 3), np.uint8), 'nope')


def test_symbols_declared_bound_and_exported():
    from deepdish_amd._lib import lib, MISSING, SIGNATURES, LIB_PATH
    l = lib()
    assert MISSING == []
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'deepdish_hip.h')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dd_[a-z0-9_]+)', out))
    for name in ('dd_raw8_to_bgr', 'dd_ingest_create_raw8'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in SIGNATURES and hasattr(l, name) and name in exported, name


def test_bad_arguments_are_codes_without_a_device():
    """The checks come before any use of ctx (NULL here); each message names the function and the argument."""
    from deepdish_amd._lib import lib
    l = lib()
    W = 640
    for args, what in [((1, 480, W, 5, 0, 0), b'layout 5'), ((1, 480, W, 11, 0, 0), b'layout 11'), ((1, 480, 2, 6, 0, 0), b'W 2'),
                       ((1, 2, W, 9, 0, 0), b'H 2'), ((1, 0, W, 10, 0, 0), b'H 0'), ((1, 480, W, 7, W - 2, 0), b'pitch 638'),
                       ((70000, 480, W, 8, 0, 0), b'batch 70000'), ((1, 480, W, 6, 0, W * 479), b'frame_stride')]:
        assert l.dd_raw8_to_bgr(None, None, *args, None, None) < 0, what
        msg = l.dd_last_error()
        assert b'dd_raw8_to_bgr' in msg and what in msg, msg
    assert l.dd_raw8_to_bgr(None, None, 1, 2, 2, 10, 0, 0, None, None) < 0          # gray may be that small: the NULL context is what is refused
    assert b'NULL ctx' in l.dd_last_error()
    for args, what in [((480, W, 480, W, 0, 5), b'layout 5'), ((480, W, 480, W, 0, 11), b'layout 11'), ((480, 2, 480, W, 0, 6), b'src_w 2'),
                       ((2, W, 480, W, 1, 9), b'src_h 2')]:
        assert l.dd_ingest_create_raw8(None, 2, 1, *args, None) < 0, what
        msg = l.dd_last_error()
        assert b'dd_ingest_create_raw8' in msg and what in msg, msg
    assert l.dd_ingest_create_raw8(None, 2, 1, 2, 2, 2, 2, 0, 10, None) < 0
    assert b'dd_ingest_create_raw8' in l.dd_last_error()
    assert l.dd_ingest_create_format(None, 2, 1, 480, W, 480, W, 0, 6, None) < 0     # the raw8 codes stay refused by the entry that never took them
    assert b'dd_ingest_create_format' in l.dd_last_error()


def test_pixel_format_names():
    from deepdish_amd.ingest import PIXEL_FORMATS
    assert [PIXEL_FORMATS['bayer_' + p] for p in ('rggb', 'grbg', 'gbrg', 'bggr')] == [6, 7, 8, 9]
    assert PIXEL_FORMATS['gray'] == 10 and 'grey' not in PIXEL_FORMATS
