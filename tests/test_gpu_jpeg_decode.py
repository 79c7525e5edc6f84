"""GPU: the JPEG decoder (csrc/jpeg_dec.hip) held to tests/jpeg_dec_ref.py -- equality everywhere, and with Pillow directly where Pillow
wrote the file.  The shapes are the smallest at which each part can go wrong: frames below, at and across an MCU; several bands of
jpeg_pixels_k (the chroma rows it takes from the bands above and below); every restart layout; tables that are not Annex K's; batches
whose neighbours differ in everything; both plan paths at the width where they meet.  Frames and statuses land in sentinel-guarded
buffers.  Damaged files are the three the host check (scripts/jpeg_decode_check.cpp) decodes under the sanitizers first; nothing is
looped or retried on the card."""
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
from jpeg_dec_cases import SAMPLINGS, own_file, picture, pillow_decode, pillow_file, reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
LUMA = {'4:2:0': (3, 2, 2), '4:2:2': (3, 2, 1), '4:4:4': (3, 1, 1), 'L': (1, 1, 1)}


@functools.lru_cache(maxsize=None)
def _decoder(H, W, max_frames=32):
    from deepdish_amd.jpeg import JpegDecoder
    return JpegDecoder(H, W, max_frames=max_frames)


def _decode(dec, files, shift=0):
    """dd_jpegdec_decode into sentinel-filled frames and statuses between two guards -> (status [n], frames [n, H, W, 3]).  shift: bytes by
    which the frames start off a dword boundary."""
    import torch
    n, size = len(files), dec.H * dec.W * 3
    buf = torch.full((GUARD + shift + n * size + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
    out = buf[GUARD + shift:GUARD + shift + n * size].view(n, dec.H, dec.W, 3)
    dec.decode(files, out=out, status=st[GUARD:GUARD + n])
    dec.ctx.sync()
    host, sth = dec.ctx.to_host(buf), dec.ctx.to_host(st)
    assert (host[:GUARD + shift] == SENTINEL).all(), 'bytes before the first frame were written'
    assert (host[GUARD + shift + n * size:] == SENTINEL).all(), 'bytes behind the last frame were written'
    assert (sth[:GUARD] == -7).all() and (sth[GUARD + n:] == -7).all(), 'a status outside the batch was written'
    return sth[GUARD:GUARD + n], host[GUARD + shift:GUARD + shift + n * size].reshape(n, dec.H, dec.W, 3)


def _check(dec, files, pillow=True, shift=0):
    status, frames = _decode(dec, files, shift)
    assert status.tolist() == [0] * len(files)
    for i, data in enumerate(files):
        assert np.array_equal(frames[i], reference(data)), 'frame %d differs from jpeg_dec_ref' % i
        if pillow:
            assert np.array_equal(frames[i], pillow_decode(data)), 'frame %d differs from Pillow' % i


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize('H,W', [(1, 1), (8, 8), (16, 16), (17, 33), (15, 31), (49, 7), (2, 17), (96, 64)], ids=lambda v: str(v))
def test_geometry(H, W):
    """Every sampling, on noise and on a ramp, at qualities 1, 50, 95 and 100 (quality 100 on noise: 16-bit codes, ZRL runs, the largest
    coefficients and the range-limit edges): 32 files in one call."""
    from deepdish_amd import jpeg
    if (H, W) == (96, 64):
        for s in SAMPLINGS:
            path, rows, bands = jpeg.decoder_plan(H, W, *LUMA[s])
            assert path == jpeg.DEC_PATH_LDS and bands >= 3 and rows * bands >= H
    files = [pillow_file(H, W, kind, q, s) for s in SAMPLINGS for kind in ('noise', 'ramp') for q in (1, 50, 95, 100)]
    assert len(files) == 32
    _check(_decoder(H, W), files)


def test_frames_off_a_dword_boundary():
    """Rows of a multiple of four pixels are stored as dwords only when the output allows it."""
    _check(_decoder(16, 16), [pillow_file(16, 16, 'noise', 95, s) for s in SAMPLINGS], shift=1)


# ------------------------------------------------------------------ restart layouts
@pytest.mark.parametrize('sampling', ['4:2:0', '4:2:2'])
def test_restart_layouts(sampling):
    """40 x 56: none; every MCU (12 or 20 intervals: the RSTn numbering wraps past 7); every 3 MCUs (intervals that straddle MCU rows); one
    MCU row."""
    files = [pillow_file(40, 56, 'noise', 95, sampling, r) for r in ('none', 'mcu1', 'mcu3', 'row1')]
    assert [jpeg_dec_ref.parse(f)['n_intervals'] for f in files] == ([1, 12, 4, 3] if sampling == '4:2:0' else [1, 20, 7, 5])
    _check(_decoder(40, 56), files)


def test_many_lanes_of_a_wave():
    """jpeg_entropy_k with 64 intervals to a wave (what a call of very many intervals gets; DD_JPEGDEC_LANES is read when a decoder is
    created): 7 files of 12 and 20 intervals, 108 lanes in two waves."""
    from deepdish_amd.jpeg import JpegDecoder
    files = [pillow_file(40, 56, 'noise', 95, s, 'mcu1', seed=k) for k, s in enumerate(['4:2:0', '4:2:2', '4:2:0', '4:2:2', '4:2:0', '4:2:2', '4:2:0'])]
    keep = os.environ.get('DD_JPEGDEC_LANES')
    os.environ['DD_JPEGDEC_LANES'] = '64'
    try:
        dec = JpegDecoder(40, 56, max_frames=7)
    finally:
        if keep is None:
            del os.environ['DD_JPEGDEC_LANES']
        else:
            os.environ['DD_JPEGDEC_LANES'] = keep
    _check(dec, files)


# ------------------------------------------------------------------ tables
def test_optimised_tables():
    files = [pillow_file(40, 56, kind, q, s, optimize=True) for s in SAMPLINGS for kind, q in (('noise', 100), ('ramp', 20))]
    assert jpeg_dec_ref.parse(files[0])['huff'] != jpeg_dec_ref.parse(pillow_file(40, 56, 'noise', 100, '4:2:0'))['huff']
    _check(_decoder(40, 56), files)


def test_neighbours_that_differ_in_everything():
    files = [pillow_file(40, 56, 'noise', 95, '4:2:0', 'mcu3'), pillow_file(40, 56, 'ramp', 20, '4:4:4', 'none', True), pillow_file(40, 56, 'noise', 100, 'L', 'row1'),
             own_file(40, 56, 'noise', 50, 2), pillow_file(40, 56, 'noise', 1, '4:2:2', 'mcu1', True), pillow_file(40, 56, 'ramp', 75, '4:2:0', 'none'),
             pillow_file(40, 56, 'noise', 95, '4:2:2', 'row1', seed=4)]
    assert len(files) == 7
    _check(_decoder(40, 56), files)


# ------------------------------------------------------------------ other
@pytest.mark.parametrize('sampling,H,W', [('4:2:0', 17, 2513), ('4:4:4', 9, 2729)])
def test_plan_paths_where_they_meet(sampling, H, W):
    """The narrowest frame whose band does not fit in LDS takes its planes through HBM; one pixel narrower stays in LDS.  Two bands: the
    4:2:0 filter reads the other band's chroma row from the planes there and from a block transformed again here."""
    from deepdish_amd import jpeg
    assert jpeg.decoder_plan(H, W, *LUMA[sampling])[0] == jpeg.DEC_PATH_PLANES
    assert jpeg.decoder_plan(H, W - 1, *LUMA[sampling])[0] == jpeg.DEC_PATH_LDS
    for w in (W, W - 1):
        _check(_decoder(H, w, 2), [pillow_file(H, w, 'ramp', 95, sampling), pillow_file(H, w, 'noise', 50, sampling, 'row1')])


def test_paths_mixed_in_one_call():
    """A greyscale file (LDS) between two 4:2:0 files (planes) of the same size."""
    H, W = 17, 2513
    _check(_decoder(H, W, 3), [pillow_file(H, W, 'ramp', 95, '4:2:0'), pillow_file(H, W, 'ramp', 95, 'L'), pillow_file(H, W, 'noise', 50, '4:2:0', 'row1')])


@pytest.mark.parametrize('H,W,kind', [(33, 47, 'noise'), (480, 640, 'scene')])
def test_round_trip_through_the_encoder(H, W, kind):
    from deepdish_amd.jpeg import JpegEncoder
    enc = JpegEncoder(H, W)
    files = enc.encode_to_host(enc.ctx.to_device(np.ascontiguousarray(picture(H, W, kind))[None]))
    assert files == [own_file(H, W, kind, 95, 1)]
    _check(_decoder(H, W, 4), files)


def test_four_frames_of_480x640():
    """Rendered-looking scenes: two without restart markers (one lane decodes the whole file) and two with an interval per MCU row."""
    files = [pillow_file(480, 640, 'scene', 95, '4:2:0', 'none', seed=0), pillow_file(480, 640, 'scene', 75, '4:2:0', 'row1', seed=1),
             pillow_file(480, 640, 'scene', 75, '4:2:2', 'none', seed=2), own_file(480, 640, 'scene', 95, 1, seed=3)]
    assert [jpeg_dec_ref.parse(f)['n_intervals'] for f in files] == [1, 30, 1, 30]
    _check(_decoder(480, 640, 4), files)


def test_status_of_refused_and_foreign_files():
    """A progressive file, a file of another size and an empty one between good frames: their statuses, their frames untouched."""
    from deepdish_amd import jpeg
    good = [pillow_file(40, 56, 'noise', 95, '4:2:0', seed=k) for k in range(2)]
    files = [good[0], pillow_file(40, 56, 'noise', 95, '4:2:0', progressive=True), pillow_file(16, 16, 'noise', 95, '4:2:0'), b'', good[1]]
    status, frames = _decode(_decoder(40, 56), files)
    assert status.tolist() == [0, jpeg.ST_HEADER, jpeg.ST_SIZE, jpeg.ST_NO_FRAME, 0]
    assert np.array_equal(frames[0], reference(good[0])) and np.array_equal(frames[4], reference(good[1]))
    assert (frames[1:4] == SENTINEL).all()


# ------------------------------------------------------------------ damaged input
@pytest.mark.parametrize('which', ['cut', 'replaced', 'rst_removed'])
def test_damaged_file_between_two_good_frames(which):
    """Only files the host check has decoded under the sanitizers with the same code (scripts/make_jpeg_corpus.py lists them).  The
    damaged frame reports a status; its neighbours are exact; the guards hold."""
    from deepdish_amd import jpeg
    import make_jpeg_corpus
    good, damaged = make_jpeg_corpus.damaged_for_the_card()
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(damaged[which])
    other = pillow_file(40, 56, 'ramp', 50, '4:2:2', 'row1')
    status, frames = _decode(_decoder(40, 56), [good, damaged[which], other])
    assert status.tolist() == [0, jpeg.ST_DATA, 0]
    assert np.array_equal(frames[0], reference(good)) and np.array_equal(frames[2], reference(other))
