"""GPU: the JPEG decoder at 1/2, 1/4 and 1/8 scale (csrc/jpeg_dec.hip, jpeg_pixels_scaled_k / jpeg_planes_scaled_k) held to
tests/jpeg_scaled_ref.py, which tests/test_jpeg_scaled_ref.py holds to Pillow -- equality everywhere.  The files and sizes are that
test's: every sampling, quality 50 and 95, optimised and standard tables, no restart markers, one MCU and one MCU row, at exact MCUs,
odd sides, a 4:2:2 chroma width <= 2 and the one-MCU frame; then the widths at which a band leaves LDS, many files in one call, and bad
files between good ones.  Frames land in sentinel-filled buffers between guards.  The damaged file is one the host check
(scripts/jpeg_decode_check.cpp) decodes under the sanitizers first; nothing is looped or retried on the card."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'scripts'))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import own_file, pillow_file  # noqa: E402
from jpeg_dec_cases import reference as full_reference  # noqa: E402
from jpeg_scaled_cases import SCALES, files, pairs, reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
LUMA = {'4:2:0': (3, 2, 2), '4:2:2': (3, 2, 1), '4:4:4': (3, 1, 1), 'L': (1, 1, 1)}


@functools.lru_cache(maxsize=None)
def _decoder(H, W, s, max_frames=64):
    from deepdish_amd.jpeg import JpegDecoder
    dec = JpegDecoder(H, W, max_frames=max_frames, scale=s)
    assert (dec.out_H, dec.out_W) == (-(-H // s), -(-W // s))
    return dec


def _decode(dec, data, shift=0):
    """Into the head of a sentinel-filled buffer that would hold the frames at full size, between two guards -> (status [n], frames
    [n, out_H, out_W, 3]).  Everything behind the last scaled frame must stay as it was.  shift: bytes off a dword boundary."""
    import torch
    n, size, room = len(data), dec.out_H * dec.out_W * 3, len(data) * dec.H * dec.W * 3
    buf = torch.full((GUARD + shift + room + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
    out = buf[GUARD + shift:GUARD + shift + n * size].view(n, dec.out_H, dec.out_W, 3)
    got, _ = dec.decode(data, out=out, status=st[GUARD:GUARD + n])
    assert tuple(got.shape) == (n, dec.out_H, dec.out_W, 3)
    dec.ctx.sync()
    host, sth = dec.ctx.to_host(buf), dec.ctx.to_host(st)
    assert (host[:GUARD + shift] == SENTINEL).all(), 'bytes before the first frame were written'
    assert (host[GUARD + shift + n * size:] == SENTINEL).all(), 'bytes behind the last scaled frame were written'
    assert (sth[:GUARD] == -7).all() and (sth[GUARD + n:] == -7).all(), 'a status outside the batch was written'
    return sth[GUARD:GUARD + n], host[GUARD + shift:GUARD + shift + n * size].reshape(n, dec.out_H, dec.out_W, 3)


def _check(dec, data, shift=0):
    status, frames = _decode(dec, data, shift)
    assert status.tolist() == [0] * len(data)
    for i, d in enumerate(data):
        assert np.array_equal(frames[i], reference(d, dec.scale)), 'frame %d differs from jpeg_scaled_ref at 1/%d' % (i, dec.scale)
    return frames


# ------------------------------------------------------------------ the ref test's files and sizes
@pytest.mark.parametrize('hw,s', pairs(), ids=lambda v: str(v).replace(' ', ''))
def test_files_and_sizes(hw, s):
    """48 files in one call: the four samplings, two qualities, both table kinds and three restart layouts as neighbours."""
    H, W = hw
    data = files(H, W)
    assert len(data) == 48
    _check(_decoder(H, W, s), data)


@pytest.mark.parametrize('s', SCALES)
def test_neighbours_that_differ_in_everything(s):
    """Samplings and restart layouts mixed in one call (intervals that straddle MCU rows, this build's own encoder among them); the same
    call once more into frames off a dword boundary, where rows of a multiple of four pixels must not be stored as dwords."""
    data = [pillow_file(40, 64, 'noise', 95, '4:2:0', 'mcu3'), pillow_file(40, 64, 'ramp', 20, '4:4:4', 'none', True), pillow_file(40, 64, 'noise', 100, 'L', 'row1'),
            own_file(40, 64, 'noise', 50, 2), pillow_file(40, 64, 'noise', 1, '4:2:2', 'mcu1', True), pillow_file(40, 64, 'ramp', 75, '4:2:0', 'none'),
            pillow_file(40, 64, 'noise', 95, '4:2:2', 'row1', seed=4)]
    dec = _decoder(40, 64, s)
    assert dec.out_W % 4 == 0
    a = _check(dec, data)
    b = _check(dec, data, shift=1)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ where a band leaves LDS
def test_a_width_that_leaves_lds_at_full_size_stays_there_at_half():
    """2 600 x 16, 4:2:0: 26 bytes of LDS per padded luma column at full size, 12 at half size."""
    from deepdish_amd import jpeg
    H, W = 16, 2600
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:0'])[0] == jpeg.DEC_PATH_PLANES
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:0'], scale=1)[0] == jpeg.DEC_PATH_PLANES
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:0'], scale=2) == (jpeg.DEC_PATH_LDS, 8, 1)
    data = [pillow_file(H, W, 'ramp', 95, '4:2:0'), pillow_file(H, W, 'noise', 50, '4:2:0', 'row1')]
    status, frames = _decode(_decoder(H, W, 1, 2), data)
    assert status.tolist() == [0, 0]
    for i, d in enumerate(data):
        assert np.array_equal(frames[i], full_reference(d))
    _check(_decoder(H, W, 2, 2), data)


def test_the_widest_frame_at_half_size():
    """8 192 x 8: a 4:2:0 band is still too wide for LDS at half size and goes through the HBM planes; its 4:2:2 and greyscale
    neighbours of the same call stay in LDS."""
    from deepdish_amd import jpeg
    H, W = 8, 8192
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:0'], scale=2)[0] == jpeg.DEC_PATH_PLANES
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:2'], scale=2)[0] == jpeg.DEC_PATH_LDS
    assert jpeg.decoder_plan(H, W, *LUMA['4:2:0'], scale=4)[0] == jpeg.DEC_PATH_LDS
    data = [pillow_file(H, W, 'ramp', 95, '4:2:0'), pillow_file(H, W, 'ramp', 50, '4:2:2', 'row1'), pillow_file(H, W, 'noise', 50, '4:2:0', 'row1'),
            pillow_file(H, W, 'ramp', 95, 'L')]
    _check(_decoder(H, W, 2, 4), data)


# ------------------------------------------------------------------ many files
def test_64_files_in_one_call_equal_each_decoded_alone():
    H, W, s = 37, 53, 2
    data = files(H, W) + [pillow_file(H, W, 'noise', 75, smp, 'mcu3', seed=k) for k, smp in enumerate(['4:2:0', '4:2:2', '4:4:4', 'L'] * 4)]
    assert len(data) == 64
    dec = _decoder(H, W, s)
    together = _check(dec, data)
    for i, d in enumerate(data):
        status, alone = _decode(dec, [d])
        assert status.tolist() == [0] and np.array_equal(alone[0], together[i]), 'file %d decodes differently alone' % i


# ------------------------------------------------------------------ bad files between good ones
@pytest.mark.parametrize('s', SCALES)
def test_refused_foreign_and_truncated_files_between_good_ones(s):
    """The status contract is the full-size decoder's: a progressive file (ST_HEADER), a file of another size (ST_SIZE, judged against
    the size the files must state, not the scaled one) and an empty one leave their frames untouched; a file cut in mid-scan (one the
    host check decodes under the sanitizers) reports ST_DATA; the good frames are exact; nothing is written behind the scaled frames."""
    from deepdish_amd import jpeg
    import make_jpeg_corpus
    good, damaged = make_jpeg_corpus.damaged_for_the_card()
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(damaged['cut'])
    H, W = 40, 56
    other = pillow_file(H, W, 'ramp', 50, '4:2:2', 'row1')
    scaled_size = pillow_file(-(-H // s), -(-W // s), 'noise', 95, '4:2:0')
    data = [good, pillow_file(H, W, 'noise', 95, '4:2:0', progressive=True), other, scaled_size, damaged['cut'], b'', pillow_file(H, W, 'noise', 95, '4:4:4')]
    status, frames = _decode(_decoder(H, W, s), data)
    assert status.tolist() == [0, jpeg.ST_HEADER, 0, jpeg.ST_SIZE, jpeg.ST_DATA, jpeg.ST_NO_FRAME, 0]
    for i in (0, 2, 6):
        assert np.array_equal(frames[i], reference(data[i], s)), 'good frame %d' % i
    for i in (1, 3, 5):
        assert (frames[i] == SENTINEL).all(), 'frame %d was written' % i


# ------------------------------------------------------------------ the argument
def test_a_scale_that_is_none_of_1_2_4_8_raises():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError, lib
    for bad in (3, 0, 16, -2):
        with pytest.raises(DeepDishHipError, match=r'scale %d ' % bad):
            jpeg.JpegDecoder(16, 16, scale=bad)
        with pytest.raises(DeepDishHipError, match=r'scale %d ' % bad):
            jpeg.decoder_plan(16, 16, scale=bad)
    assert b'1, 2, 4, 8' in lib().dd_last_error()
    with pytest.raises(ValueError):
        jpeg.JpegDecoder(16, 16, scale=2.0)


def test_scale_1_is_the_decoder_without_the_argument():
    import torch
    from deepdish_amd import jpeg
    H, W = 37, 53
    data = files(H, W)[:16]
    a, b = jpeg.JpegDecoder(H, W, max_frames=16), jpeg.JpegDecoder(H, W, max_frames=16, scale=1)
    assert (a.out_H, a.out_W, b.out_H, b.out_W) == (H, W, H, W)
    fa, sa = a.decode(data)
    fb, sb = b.decode(data)
    a.ctx.sync()
    assert tuple(fb.shape) == (16, H, W, 3) and torch.equal(fa, fb) and torch.equal(sa, sb) and sa.tolist() == [0] * 16
    assert jpeg.decoder_plan(H, W, scale=1) == jpeg.decoder_plan(H, W)


def test_draft_scale_is_the_refs():
    import jpeg_scaled_ref
    from deepdish_amd import jpeg
    for src in ((1920, 1080), (1280, 720), (640, 480), (64, 48), (3840, 2160), (17, 9)):
        for want in ((640, 480), (300, 300), (640, 640), (32, 24), (20, 15), (1, 1), (5000, 4000), src):
            assert jpeg.draft_scale(src, want) == jpeg_scaled_ref.draft_scale(src, want)
