"""CPU: the numpy restatement of the NV12 / I420 -> BGR decoder (tests/yuv_ref.py) at its anchor values, and the C ABI of the
conversion: both entry points bound and exported, bad arguments answered with a code and a message that names the function."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402

# (Y, U, V) -> (B, G, R)
ANCHORS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254)),
           ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((255, 255, 255), (255, 125, 255)),
           ((0, 0, 0), (0, 154, 0))]


def test_anchor_values():
    for (y, u, v), bgr in ANCHORS:
        assert tuple(int(c) for c in yuv_ref.yuv_to_bgr(y, u, v)) == bgr, (y, u, v)


def test_layouts_read_the_same_samples():
    """A 4x2 frame written in both layouts decodes to the same picture, the chroma of pixel (x, y) being that of block (x >> 1, y >> 1)."""
    Y = np.array([[16, 81, 145, 41], [235, 255, 0, 100]], np.uint8)
    U, V = np.array([[90, 240]], np.uint8), np.array([[240, 110]], np.uint8)
    nv12 = np.concatenate([Y.ravel(), np.stack([U, V], -1).ravel()])
    i420 = np.concatenate([Y.ravel(), U.ravel(), V.ravel()])
    a = yuv_ref.yuv420_to_bgr(nv12, 2, 4, 'nv12')
    np.testing.assert_array_equal(a, yuv_ref.yuv420_to_bgr(i420, 2, 4, 'i420'))
    assert a.shape == (2, 4, 3)
    for y in range(2):
        for x in range(4):
            np.testing.assert_array_equal(a[y, x], yuv_ref.yuv_to_bgr(Y[y, x], U[0, x >> 1], V[0, x >> 1]))
    assert tuple(a[0, 1]) == (0, 0, 254)


def test_symbols_bound_and_exported():
    from deepdish_amd._lib import lib, MISSING, SIGNATURES, LIB_PATH
    l = lib()
    assert MISSING == []
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dd_[a-z0-9_]+)', out))
    for name in ('dd_yuv420_to_bgr', 'dd_ingest_create_format'):
        assert name in SIGNATURES and hasattr(l, name) and name in exported, name


def test_bad_arguments_are_codes_that_name_the_function():
    from deepdish_amd._lib import lib
    l = lib()
    assert l.dd_yuv420_to_bgr(None, None, 1, 2, 2, 1, 0, 0, 0, None, None) < 0
    assert b'dd_yuv420_to_bgr' in l.dd_last_error()
    assert l.dd_ingest_create_format(None, 2, 1, 2, 2, 2, 2, 0, 1, None) < 0
    assert b'dd_ingest_create_format' in l.dd_last_error()


def test_to_yuv420_round_trip_is_close():
    """The synthetic forward transform is a sane BT.601 one: flat colours survive the round trip through the decoder within a few levels
    (it pins nothing).  Bound: each of Y, U, V is rounded by at most 0.5 and the decoder's largest gains are 1.164 (Y) and 2.018 (U into B),
    so a channel moves by at most 0.5 * (1.164 + 2.018) + 0.5 < 2.1 before its own rounding: 3 levels."""
    from deepdish_amd.synth import to_yuv420
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 256, (6, 3), dtype=np.uint8)
    for layout in ('nv12', 'i420'):
        for c in cols:
            frame = np.broadcast_to(c, (4, 6, 3)).copy()
            yuv = to_yuv420(frame, layout)
            assert yuv.shape == (6, 6) and yuv.dtype == np.uint8
            back = yuv_ref.yuv420_to_bgr(yuv, 4, 6, layout)
            assert np.abs(back.astype(int) - frame.astype(int)).max() <= 3, (layout, c, back[0, 0])
