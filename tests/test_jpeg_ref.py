"""CPU: tests/jpeg_ref.py -- the definition the JPEG kernel is held to -- against Pillow's encoder, whole files, byte for byte; the
header dd_jpeg_header builds, dd_jpeg_plan and the argument refusals, none of which needs a device; wire.mjpeg_part."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_ref  # noqa: E402
from jpeg_cases import CASES, QUALITIES, frame, rows  # noqa: E402


def pillow(bgr, quality, restart_rows):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), 'RGB').save(f, 'JPEG', quality=quality, subsampling='4:2:0', restart_marker_rows=restart_rows)
    return f.getvalue()


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d-q%d-r%d-%s' % c)
def test_reference_equals_pillow(case):
    H, W, q, r, kind = case
    bgr = frame(H, W, kind)
    assert jpeg_ref.encode(bgr, q, rows(H, r)) == pillow(bgr, q, rows(H, r))


def test_reference_equals_pillow_at_480x640():
    bgr = frame(480, 640, 'smooth')
    got = jpeg_ref.encode(bgr, 95, 1)
    assert got == pillow(bgr, 95, 1)
    assert len(got) < 480 * 640 * 3 // 10


def test_every_quality():
    """A seeded 32 x 48 noise frame at every quality: every scaled table, so every divisor the quantiser can meet at that base entry."""
    bgr = frame(32, 48, 'noise', seed=5)
    for q in QUALITIES:
        assert jpeg_ref.encode(bgr, q, 1) == pillow(bgr, q, 1), 'quality %d' % q


def test_restart_counter_wraps():
    data = jpeg_ref.encode(frame(160, 32, 'noise'), 95, 1)
    scan = data[len(jpeg_ref.header(160, 32, 95, 1)):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (k & 7) for k in range(9)]


def test_checker_at_quality_100_exercises_stuffing():
    bgr = frame(32, 48, 'checker')
    data, info = jpeg_ref.encode_info(bgr, 100, 1)
    assert data == pillow(bgr, 100, 1)
    assert b'\xff\x00' in info['scan']


def test_noise_at_quality_10_emits_zrl():
    bgr = frame(48, 64, 'noise')
    data, info = jpeg_ref.encode_info(bgr, 10, 1)
    assert data == pillow(bgr, 10, 1)
    assert info['zrl'] >= 1


def test_mjpeg_part_is_the_reference_s_literal():
    from deepdish_amd import wire
    jpg = jpeg_ref.encode(frame(8, 8, 'smooth'))
    assert wire.mjpeg_part(jpg) == b'--frame\r\nContent-Type: image/jpeg\r\n\r\n' + jpg + b'\r\n'
    assert wire.mjpeg_part(bytearray(b'\xff\xd8\xff\xd9')) == b'--frame\r\nContent-Type: image/jpeg\r\n\r\n\xff\xd8\xff\xd9\r\n'


# ------------------------------------------------------------------ the library, without a device
@pytest.mark.parametrize('H,W,q,r', [(480, 640, 95, 1), (33, 47, 50, 1), (1, 1, 1, 1), (720, 1280, 100, 3), (32, 48, 75, 2)])
def test_header_equals_pillow_up_to_the_scan(H, W, q, r):
    from deepdish_amd import jpeg
    head = jpeg.header(H, W, q, r)
    assert head == jpeg_ref.header(H, W, q, r)
    ref = pillow(np.zeros((H, W, 3), np.uint8), q, r)
    assert ref[:len(head)] == head and head[-14:-12] == b'\xff\xda'
    markers, i = [], 2
    while i < len(head):
        markers.append(head[i + 1])
        i += 2 + int.from_bytes(head[i + 2:i + 4], 'big')
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]


def test_every_quality_s_header():
    from deepdish_amd import jpeg
    for q in QUALITIES:
        assert jpeg.header(32, 48, q, 1) == jpeg_ref.header(32, 48, q, 1), 'quality %d' % q


def test_plan_answers_without_a_device():
    from deepdish_amd import jpeg
    assert jpeg.plan(480, 640) == jpeg.PATH_LDS and jpeg.plan(720, 1280) == jpeg.PATH_LDS and jpeg.plan(1080, 1920) == jpeg.PATH_LDS
    assert jpeg.plan(1, 1) == jpeg.PATH_LDS
    assert jpeg.plan(480, 640, 2) == jpeg.PATH_LDS and jpeg.plan(480, 640, 30) == jpeg.PATH_STREAM
    assert jpeg.plan(16, 2048) == jpeg.PATH_LDS and jpeg.plan(16, 2049) == jpeg.PATH_STREAM        # 128 MCUs in an interval: the most LDS holds
    assert jpeg.plan(2064, 16, 128) == jpeg.PATH_LDS and jpeg.plan(2064, 16, 129) == jpeg.PATH_STREAM
    assert jpeg.plan(2048, 16, 1000) == jpeg.PATH_LDS                                               # no more rows than the frame has


def test_argument_refusals():
    from deepdish_amd._lib import lib, DeepDishHipError
    from deepdish_amd import jpeg
    h, path = ctypes.c_void_p(), ctypes.c_int()
    for H, W, q, r, word in ((0, 16, 95, 1, b'h, w'), (16, 8193, 95, 1, b'h, w'), (8193, 16, 95, 1, b'h, w'), (16, 16, 0, 1, b'quality'),
                             (16, 16, 101, 1, b'quality'), (16, 16, 95, 0, b'restart_rows'), (8192, 8192, 95, 128, b'restart_rows')):
        assert lib().dd_jpeg_create(None, H, W, q, r, ctypes.byref(h)) == -1, (H, W, q, r)
        msg = lib().dd_last_error()
        assert b'dd_jpeg_create' in msg and word in msg, msg
    assert lib().dd_jpeg_create(None, 8192, 8192, 95, 127, ctypes.byref(h)) == 0                    # 127 * 512 = 65024 MCUs: allowed
    n = ctypes.c_int()
    buf = (ctypes.c_uint8 * 16)()
    assert lib().dd_jpeg_header(h, buf, 16, ctypes.byref(n)) == -4 and n.value == len(jpeg_ref.header(8192, 8192, 95, 127))
    assert lib().dd_jpeg_encode(h, 1, 1, 1, 100, 1, None) == -3 and b'context' in lib().dd_last_error()      # no context: header only
    assert lib().dd_jpeg_destroy(h) == 0
    assert lib().dd_jpeg_plan(16, 16, 0, ctypes.byref(path)) == -1 and b'restart_rows' in lib().dd_last_error()
    assert lib().dd_jpeg_plan(16, 0, 1, ctypes.byref(path)) == -1 and lib().dd_jpeg_plan(16, 16, 1, None) == -1
    with pytest.raises(DeepDishHipError, match='quality'):
        jpeg.header(16, 16, quality=0)
    with pytest.raises(ValueError):
        jpeg_ref.encode(np.zeros((16, 16, 3), np.uint8), quality=0)
    with pytest.raises(ValueError):
        jpeg_ref.encode(np.zeros((16, 16, 3), np.uint8), restart_rows=0)
