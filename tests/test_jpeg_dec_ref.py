"""CPU: tests/jpeg_dec_ref.py, the definition of the JPEG decoder, against Pillow (libjpeg-turbo) -- Image.open(f).convert('RGB') with the
channels swapped, byte for byte: every accepted sampling, restart layout and table kind, at sizes below, at and across an MCU, on noise
and on a ramp, from quality 20 to 100; and the files this build's own encoder writes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, own_file, pillow_decode, pillow_file, picture  # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (15, 31), (49, 7), (3, 5), (40, 56), (2, 17)]
LAYOUTS = [('none', False), ('none', True), ('mcu1', False), ('mcu3', False), ('row1', False)]


@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_equals_pillow(H, W):
    n = 0
    for kind in ('noise', 'ramp'):
        for q in (20, 95, 100):
            for sampling in SAMPLINGS:
                for restart, optimize in LAYOUTS:
                    data = pillow_file(H, W, kind, q, sampling, restart, optimize)
                    got = jpeg_dec_ref.decode(data)
                    assert got.shape == (H, W, 3) and got.dtype == np.uint8
                    assert np.array_equal(got, pillow_decode(data)), (kind, q, sampling, restart, optimize)
                    n += 1
    assert n == 120


def test_both_orientations_of_the_narrow_sizes():
    """A down-sampled width of 1 and 2 (libjpeg replicates there instead of filtering) and of 3, either way up."""
    for H, W in ((5, 3), (17, 2), (33, 17), (7, 49), (4, 4), (6, 5)):
        for sampling in SAMPLINGS:
            data = pillow_file(H, W, 'noise', 95, sampling)
            assert np.array_equal(jpeg_dec_ref.decode(data), pillow_decode(data)), (H, W, sampling)


@pytest.mark.parametrize('H,W,q,r', [(33, 47, 95, 1), (40, 56, 50, 2), (16, 16, 100, 1), (160, 32, 75, 1), (1, 1, 95, 1)])
def test_own_encoder_files(H, W, q, r):
    data = own_file(H, W, 'noise', q, r)
    assert np.array_equal(jpeg_dec_ref.decode(data), pillow_decode(data))


def test_one_component_gives_equal_channels():
    out = jpeg_dec_ref.decode(pillow_file(17, 33, 'noise', 95, 'L'))
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()


def test_coefficients_round_trip_through_the_encoder_definition():
    """jpeg_ref.coefficients (the encoder's) and jpeg_dec_ref.coefficients (the decoder's) of the same file are the same numbers."""
    import jpeg_ref
    bgr = picture(33, 47, 'noise', 3)
    enc = jpeg_ref.coefficients(bgr, 95)                                  # [mh, mw, 6, 64] zigzag
    dec = jpeg_dec_ref.coefficients(jpeg_ref.encode(bgr, 95, 1))          # [blocks, 64] natural
    assert np.array_equal(enc.reshape(-1, 64), dec.astype(np.int64)[:, jpeg_ref.ZIGZAG])


def test_refusals_and_damage_raise_value_error():
    good = pillow_file(40, 56, 'noise', 95, '4:2:0', 'mcu3')
    with pytest.raises(ValueError, match='progressive'):
        jpeg_dec_ref.decode(pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True))
    sos = jpeg_dec_ref.parse(good)['scan_offset']
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(good[:sos + (len(good) - sos) * 6 // 10])
    with pytest.raises(ValueError, match='truncated'):
        jpeg_dec_ref.decode(good[:sos - 3])
    i = good.index(b'\xff\xd1', sos)
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(good[:i] + good[i + 2:])
