"""CPU: the letterbox geometry, the launch plan and the box un-mapping, without a device.

* dd_letterbox_geometry and tests/letterbox_ref.geometry against tests/golden/letterbox_geometry.npz, which scripts/make_golden_letterbox.py
  read off the reference's own letterbox_image (yolo3/utils.py:18-28): every W, H in 2..120 into 64 x 64, the geometries the GPU tests run,
  common camera sizes into 640 x 640 and 416 x 416, and rows where Pillow refuses the resize.
* dd_resize_lanczos_letterbox_plan answers with no context: 0 where neither axis is resampled, 1 (one launch through LDS) for every small
  geometry and for 1280 x 720 -> 640 x 640, 2 for 4096 x 48 -> 2048 x 32.  That last one is a 2:1 reduction whose vertical windows are 12
  rows; the canvas is 2048 pixels wide, the smallest power of two at which 12 rows of the band (12 x 6 144 = 73 728 B) no longer fit
  letterbox_lanczos_k's 65 536-byte LDS budget (1 024 wide: 36 864 B, one launch).
* The un-mapping with off = 0, new = net is x * W bit for bit (what the stretch decode stores)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import letterbox_ref  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'letterbox_geometry.npz')
SMALL = [(96, 54, 64, 64), (54, 96, 64, 64), (33, 17, 64, 64), (49, 7, 64, 64), (70, 50, 64, 48), (200, 120, 96, 96)]      # (W, H, w, h)
COPIES = [(640, 480, 640, 640), (64, 48, 64, 64)]
TWO_LAUNCH = (4096, 48, 2048, 32)


def _geometry(W, H, w, h):
    from deepdish_amd._lib import lib
    out = [ctypes.c_int(-7) for _ in range(4)]
    rc = lib().dd_letterbox_geometry(W, H, w, h, *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def _plan(W, H, w, h, src_c=3, swap_rb=1, batch=1):
    from deepdish_amd._lib import lib
    path, rows = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib().dd_resize_lanczos_letterbox_plan(None, H, W, src_c, swap_rb, h, w, batch, ctypes.byref(path), ctypes.byref(rows))
    return rc, path.value, rows.value


def test_geometry_equals_the_reference_letterbox_image():
    from deepdish_amd._lib import lib
    rows = np.load(GOLDEN)['rows']
    assert rows.dtype == np.int32 and rows.shape[1] == 9 and len(rows) >= 119 * 119 + 20
    assert (rows[:, 8] == 0).sum() >= 3
    for W, H, w, h, new_w, new_h, off_x, off_y, valid in rows.tolist():
        rc, got = _geometry(W, H, w, h)
        if valid:
            assert rc == 0 and got == (new_w, new_h, off_x, off_y), (W, H, w, h)
            assert letterbox_ref.geometry(W, H, w, h) == (new_w, new_h, off_x, off_y), (W, H, w, h)
        else:
            assert rc < 0 and got == (-7, -7, -7, -7), (W, H, w, h)
            assert b'dd_letterbox_geometry' in lib().dd_last_error()
            with pytest.raises(ValueError):
                letterbox_ref.geometry(W, H, w, h)


def test_the_truncation_is_the_reference_s():
    """49 x 7 into 64 x 64: 49 * (64 / 49) is just below 64 in f64, so the picture is 63 wide; 2 x 161 leaves no picture at all."""
    assert _geometry(49, 7, 64, 64) == (0, (63, 9, 0, 27))
    assert _geometry(640, 480, 640, 640) == (0, (640, 480, 0, 80))
    assert _geometry(1280, 720, 640, 640) == (0, (640, 360, 0, 140))
    assert _geometry(2, 161, 64, 64)[0] < 0
    assert _geometry(0, 10, 64, 64)[0] < 0


def test_plan_answers_without_a_device():
    for g in COPIES:
        rc, path, rows = _plan(*g)
        assert (rc, path) == (0, 0) and rows >= 1, g
    for g in SMALL + [(1280, 720, 640, 640)]:
        rc, path, rows = _plan(*g)
        assert (rc, path) == (0, 1) and rows >= 1, g
        assert letterbox_ref.one_row_window_bytes(*g) <= letterbox_ref.LDS_BUDGET
    assert _plan(200, 120, 96, 96)[2] < 57                         # the 57 picture rows take several bands
    rc, path, rows = _plan(*TWO_LAUNCH)
    assert (rc, path) == (0, 2) and rows >= 1
    assert letterbox_ref.one_row_window_bytes(*TWO_LAUNCH) == 12 * 6144 > letterbox_ref.LDS_BUDGET
    assert letterbox_ref.one_row_window_bytes(2048, 48, 1024, 32) == 12 * 3072 and _plan(2048, 48, 1024, 32)[1] == 1
    assert _plan(3840, 2160, 640, 640)[1] == 2                     # 36 rows of 1 920 bytes
    for form in ((3, 0), (4, 0), (4, 1)):                          # the channel form does not change the decision
        assert _plan(1280, 720, 640, 640, *form)[:2] == (0, 1)
    assert _plan(1280, 720, 640, 640, batch=1536)[:2] == (0, 1)


def test_plan_errors_are_codes():
    from deepdish_amd._lib import lib
    assert _plan(2, 161, 64, 64)[0] < 0                            # no picture
    assert _plan(96, 54, 64, 64, src_c=2)[0] < 0
    assert b'src_c' in lib().dd_last_error()
    assert lib().dd_resize_lanczos_letterbox(None, None, 1, 54, 96, 3, 1, None, 64, 64, 114, None) < 0
    assert lib().dd_yolov5_decode_letterbox(None, None, 1, 80, 0.25, 640, 480, 640, 640, None, None, None, 0, None, None) < 0
    assert lib().dd_pipeline_detector_letterbox(None, 114) < 0


def test_unmapping_without_a_letterbox_is_the_stretch_product():
    """off = 0 and new = net: (x - 0) / 1 * W in f64, rounded to f32 -- the stretch decode's (float)((double)x * (double)W), bitwise."""
    rng = np.random.default_rng(12)
    x = np.concatenate([rng.uniform(-0.5, 1.5, 9000), rng.standard_normal(1000) * 1e3]).astype(np.float32)
    for size, net in ((640, 640), (480, 640), (1280, 416), (7, 64)):
        got = letterbox_ref.unmap_corners(x, 0, net, net, size)
        want = (x.astype(np.float64) * np.float64(size)).astype(np.float32)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_unmapping_puts_the_picture_s_corners_on_the_frame_s():
    """The canvas-normalised corners of the pasted picture map to (0, 0) and (W, H) up to the f32 rounding of the inputs."""
    for (W, H, w, h) in SMALL + [(1280, 720, 640, 640), (640, 480, 640, 640)]:
        new_w, new_h, off_x, off_y = letterbox_ref.geometry(W, H, w, h)
        xs = letterbox_ref.unmap_corners(np.float32([off_x / w, (off_x + new_w) / w]), off_x, new_w, w, W)
        ys = letterbox_ref.unmap_corners(np.float32([off_y / h, (off_y + new_h) / h]), off_y, new_h, h, H)
        np.testing.assert_allclose(xs, [0, W], atol=W * 2.0 ** -22)
        np.testing.assert_allclose(ys, [0, H], atol=H * 2.0 ** -22)


def test_python_options_are_checked_before_anything_is_built():
    from deepdish_amd.tools.yolov5 import letterbox_pad
    assert letterbox_pad(False) is None and letterbox_pad(True) == 114 and letterbox_pad(128) == 128 and letterbox_pad(0) == 0
    for bad in (256, -1, 'yes', 1.5):
        with pytest.raises(ValueError):
            letterbox_pad(bad)
