"""CPU: the numpy restatement of the packed 4:2:2 (YUY2 / UYVY) -> BGR decoder (tests/yuv422_ref.py) at hand-written frames and against
the 4:2:0 definition already pinned, and the C ABI of the conversion: the entry point bound and exported, bad arguments answered with a
code and a message that names the function and the argument -- without a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402
import yuv422_ref  # noqa: E402

# a 4 x 1 frame: pixel x -> (Y, U, V); pixels 0, 1 share the first macropixel's chroma, pixels 2, 3 the second's
PIXELS = [(81, 90, 240), (145, 90, 240), (41, 240, 110), (235, 240, 110)]
FRAMES = {'yuy2': [81, 90, 145, 240, 41, 240, 235, 110], 'uyvy': [90, 81, 240, 145, 240, 41, 110, 235]}


@pytest.mark.parametrize('order', yuv422_ref.ORDERS)
def test_anchor_frame(order):
    got = yuv422_ref.yuv422_to_bgr(np.array(FRAMES[order], np.uint8), 1, 4, order)
    assert got.shape == (1, 4, 3) and got.dtype == np.uint8
    for x, (y, u, v) in enumerate(PIXELS):
        np.testing.assert_array_equal(got[0, x], yuv_ref.yuv_to_bgr(y, u, v), err_msg='pixel %d' % x)
    assert tuple(got[0, 0]) == (0, 0, 254)                       # (81, 90, 240) is test_yuv_ref's red anchor


@pytest.mark.parametrize('order', yuv422_ref.ORDERS)
def test_pitch_skips_the_padding(order):
    """Two rows with pitch 2 W + 3: the second row starts at the pitch, the padding bytes are never read as samples."""
    row = FRAMES[order]
    buf = np.array(row + [7, 7, 7] + row[4:] + row[:4], np.uint8)
    got = yuv422_ref.yuv422_to_bgr(buf, 2, 4, order, pitch=11)
    want = [yuv_ref.yuv_to_bgr(*p) for p in PIXELS]
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want[2:] + want[:2])


@pytest.mark.parametrize('order', yuv422_ref.ORDERS)
def test_agrees_with_the_420_definition(order):
    """A packed 6 x 4 frame whose rows 2k and 2k + 1 carry equal chroma is the NV12 frame with those samples: same picture under
    yuv_ref.yuv420_to_bgr.  Ties the new definition to the one already pinned."""
    rng = np.random.default_rng(422)
    H, W = 4, 6
    Y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    U, V = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)
    packed = np.empty((H, W, 2), np.uint8)
    luma, chroma = (0, 1) if order == 'yuy2' else (1, 0)
    packed[..., luma] = Y
    packed[:, 0::2, chroma], packed[:, 1::2, chroma] = np.repeat(U, 2, axis=0), np.repeat(V, 2, axis=0)
    nv12 = np.concatenate([Y.ravel(), np.stack([U, V], -1).ravel()])
    np.testing.assert_array_equal(yuv422_ref.yuv422_to_bgr(packed, H, W, order), yuv_ref.yuv420_to_bgr(nv12, H, W, 'nv12'))


def test_symbol_bound_and_exported():
    from deepdish_amd._lib import lib, MISSING, SIGNATURES, LIB_PATH
    l = lib()
    assert MISSING == []
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dd_[a-z0-9_]+)', out))
    assert 'dd_yuv422_to_bgr' in SIGNATURES and hasattr(l, 'dd_yuv422_to_bgr') and 'dd_yuv422_to_bgr' in exported


def test_bad_arguments_are_codes_without_a_device():
    """The checks come before any use of ctx (NULL here): order 6, W 641 and pitch 2 W - 2 each name the function and the argument."""
    from deepdish_amd._lib import lib
    l = lib()
    W = 640
    for args, what in [((1, 480, W, 6, 0, 0), b'order 6'), ((1, 480, 641, 4, 0, 0), b'W 641'),
                       ((1, 480, W, 5, 2 * W - 2, 0), b'pitch %d' % (2 * W - 2)), ((1, 0, W, 4, 0, 0), b'H 0')]:
        assert l.dd_yuv422_to_bgr(None, None, *args, None, None) < 0, what
        msg = l.dd_last_error()
        assert b'dd_yuv422_to_bgr' in msg and what in msg, msg
    assert l.dd_ingest_create_format(None, 2, 1, 2, 2, 2, 2, 0, 4, None) < 0
    assert b'dd_ingest_create_format' in l.dd_last_error()


def test_pixel_format_names():
    from deepdish_amd.ingest import PIXEL_FORMATS
    assert PIXEL_FORMATS['yuy2'] == 4 and PIXEL_FORMATS['uyvy'] == 5 and 'yuyv' not in PIXEL_FORMATS


def test_to_yuv422_round_trip_is_close():
    """The synthetic forward transform is a sane BT.601 one: flat colours survive the round trip through the decoder within 3 levels,
    by the bound argued in test_yuv_ref.py::test_to_yuv420_round_trip_is_close (each of Y, U, V rounded by at most 0.5, gains 1.164 and
    2.018: a channel moves by less than 2.1 before its own rounding).  It pins nothing.  An odd height is allowed."""
    from deepdish_amd.synth import to_yuv422
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 256, (6, 3), dtype=np.uint8)
    for order in yuv422_ref.ORDERS:
        for c in cols:
            frame = np.broadcast_to(c, (3, 6, 3)).copy()
            yuv = to_yuv422(frame, order)
            assert yuv.shape == (3, 6, 2) and yuv.dtype == np.uint8
            back = yuv422_ref.yuv422_to_bgr(yuv, 3, 6, order)
            assert np.abs(back.astype(int) - frame.astype(int)).max() <= 3, (order, c, back[0, 0])
    with pytest.raises(ValueError, match='even width'):
        to_yuv422(np.zeros((2, 5, 3), np.uint8), 'yuy2')
