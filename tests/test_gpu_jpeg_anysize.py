"""GPU: files of any size up to the decoder's, each at its own scale (JpegDecoder(H, W, any_size=True); jpeg_pixels_any_k<S> and
jpeg_planes_any_k<S> in csrc/jpeg_dec.hip), held to tests/jpeg_dec_ref.py, tests/jpeg_scaled_ref.py, tests/jpeg_prog_ref.py and to Pillow --
equality everywhere.  One decoder of at most 64 x 48 (w x h) takes, in one call, frames below, at and across an MCU, lopsided ones both
ways round, the largest it accepts, every sampling and restart layout, two files that are too large, a refused header and an empty file.
Every frame is the top-left rectangle of its slot; every other byte of the slot, and the guards around the batch, must still hold the
sentinel.  No damaged entropy data here: the card only sees damaged files a host program has decoded first."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_dec_ref  # noqa: E402
import jpeg_prog_cases  # noqa: E402
import jpeg_scaled_cases  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_decode, pillow_file, reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
MAX_H, MAX_W = 48, 64
# (height, width): the issue's 8x8, 16x16, 17x9, 33x16, 16x5, 3x40, 40x3, 1x1 and the largest accepted
SIZES = [(8, 8), (16, 16), (17, 9), (33, 16), (16, 5), (3, 40), (40, 3), (1, 1), (MAX_H, MAX_W)]
RESTARTS = ('none', 'mcu1', 'row1')


def _good_files(progressive=()):
    """13 files: the sizes with sampling and restart layout cycling, then 37 wide x 48 high in all four samplings.  progressive: indices
    written as progressive files instead."""
    out = []
    for k, (H, W) in enumerate(SIZES):
        out.append(pillow_file(H, W, 'noise' if k % 2 == 0 else 'ramp', (95, 50, 100)[k % 3], SAMPLINGS[k % 4], RESTARTS[k % 3], progressive=k in progressive))
    for k, s in enumerate(SAMPLINGS):
        out.append(pillow_file(48, 37, 'noise', 95, s, RESTARTS[(k + 1) % 3], progressive=len(out) in progressive))
    return out


@functools.lru_cache(maxsize=None)
def _decoder(H=MAX_H, W=MAX_W, max_frames=32, **kw):
    from deepdish_amd.jpeg import JpegDecoder
    return JpegDecoder(H, W, max_frames=max_frames, any_size=True, **kw)


def _decode(dec, files, scales=None, shift=0):
    """Into sentinel-filled slots and statuses between two guards -> (status [n], slots [n, out_H, out_W, 3])."""
    import torch
    n, size = len(files), dec.out_H * dec.out_W * 3
    buf = torch.full((GUARD + shift + n * size + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
    out = buf[GUARD + shift:GUARD + shift + n * size].view(n, dec.out_H, dec.out_W, 3)
    dec.decode(files, out=out, status=st[GUARD:GUARD + n], scales=scales)
    dec.ctx.sync()
    host, sth = dec.ctx.to_host(buf), dec.ctx.to_host(st)
    assert (host[:GUARD + shift] == SENTINEL).all(), 'bytes before the first slot were written'
    assert (host[GUARD + shift + n * size:] == SENTINEL).all(), 'bytes behind the last slot were written'
    assert (sth[:GUARD] == -7).all() and (sth[GUARD + n:] == -7).all(), 'a status outside the batch was written'
    return sth[GUARD:GUARD + n], host[GUARD + shift:GUARD + shift + n * size].reshape(n, dec.out_H, dec.out_W, 3)


def _expect(dec, frames):
    """Slots of sentinel with frame i (None: nothing) in the top-left corner of slot i."""
    want = np.full((len(frames), dec.out_H, dec.out_W, 3), SENTINEL, np.uint8)
    for i, f in enumerate(frames):
        if f is not None:
            want[i, :f.shape[0], :f.shape[1]] = f
    return want


def _same(got, want):
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), 'slot %d differs (frame or sentinel)' % i


def _ref(data, s=1):
    return reference(data) if s == 1 else jpeg_scaled_cases.reference(data, s)


def test_the_files_cover_what_they_should():
    files = _good_files()
    heads = [jpeg_dec_ref.parse(f) for f in files]
    assert [(h['height'], h['width']) for h in heads] == SIZES + [(48, 37)] * 4
    assert {(h['ncomp'], h['hmax'], h['vmax']) for h in heads[:9]} == {(3, 2, 2), (3, 2, 1), (3, 1, 1), (1, 1, 1)}
    assert {(h['ncomp'], h['hmax'], h['vmax']) for h in heads[9:]} == {(3, 2, 2), (3, 2, 1), (3, 1, 1), (1, 1, 1)}
    assert {0, 1}.issubset({h['restart_interval'] for h in heads}) and any(h['restart_interval'] == h['mcus_x'] > 1 for h in heads)


@pytest.mark.parametrize('shift', [0, 1], ids=['dword-aligned', 'off-a-dword'])
def test_mixed_sizes_in_one_call(shift):
    """The rectangles equal jpeg_dec_ref and Pillow; 65 x 48 and 64 x 49 are ST_SIZE, a progressive file is ST_HEADER on this decoder and
    an empty one ST_NO_FRAME, all four slots untouched; their neighbours are exact."""
    from deepdish_amd import jpeg
    good = _good_files()
    files = good[:4] + [pillow_file(48, 65, 'noise', 95, '4:2:0')] + good[4:8] + [pillow_file(40, 56, 'noise', 95, '4:2:0', progressive=True), b''] + good[8:] \
        + [pillow_file(49, 64, 'ramp', 95, '4:4:4')]
    bad = {4: jpeg.ST_SIZE, 9: jpeg.ST_HEADER, 10: jpeg.ST_NO_FRAME, len(files) - 1: jpeg.ST_SIZE}
    dec = _decoder()
    assert (dec.out_H, dec.out_W) == (MAX_H, MAX_W)
    status, slots = _decode(dec, files, shift=shift)
    assert status.tolist() == [bad.get(i, 0) for i in range(len(files))]
    _same(slots, _expect(dec, [None if i in bad else reference(f) for i, f in enumerate(files)]))
    for i, f in enumerate(files):
        if i not in bad:
            h, w = reference(f).shape[:2]
            assert np.array_equal(slots[i, :h, :w], pillow_decode(f)), 'frame %d differs from Pillow' % i


def test_a_file_too_large_names_both_sizes():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import lib
    dec = _decoder()
    status, slots = _decode(dec, [pillow_file(48, 65, 'noise', 95, '4:2:0')])
    assert status.tolist() == [jpeg.ST_SIZE] and (slots == SENTINEL).all()
    msg = lib().dd_last_error().decode()
    assert '65 x 48' in msg and '64 x 48' in msg


@pytest.mark.parametrize('own', [1, 2])
def test_a_scale_per_file(own):
    """The same files with scales cycling 1, 2, 4, 8 (2, 4, 8 on a decoder whose own scale is 2: smaller slots) against jpeg_scaled_ref."""
    files = _good_files()
    cycle = (1, 2, 4, 8) if own == 1 else (2, 4, 8)
    scales = [cycle[i % len(cycle)] for i in range(len(files))]
    dec = _decoder(scale=own)
    assert (dec.out_H, dec.out_W) == (-(-MAX_H // own), -(-MAX_W // own))
    status, slots = _decode(dec, files, scales=scales)
    assert status.tolist() == [0] * len(files)
    want = [_ref(f, s) for f, s in zip(files, scales)]
    for f, s, w in zip(files, scales, want):
        h = jpeg_dec_ref.parse(f)
        assert w.shape == (-(-h['height'] // s), -(-h['width'] // s), 3)
    _same(slots, _expect(dec, want))
    # every scale on the two files that fill the slot, and no scales at all: the decoder's own for every file
    big = [files[8], files[9]]
    for s in cycle:
        status, slots = _decode(dec, big, scales=[s, s])
        assert status.tolist() == [0, 0]
        _same(slots, _expect(dec, [_ref(f, s) for f in big]))
    status, slots = _decode(dec, big)
    _same(slots, _expect(dec, [_ref(f, own) for f in big]))


def test_a_scale_below_the_decoders_own_is_refused():
    from deepdish_amd._lib import DeepDishHipError
    files = _good_files()[:2]
    for dec, scales in ((_decoder(scale=2), [2, 1]), (_decoder(), [1, 3]), (_decoder(scale=4), [2, 4])):
        with pytest.raises(DeepDishHipError, match=r'\(-1\).*scale') as e:
            _decode(dec, files, scales=scales)
        assert 'file %d' % (1 if scales[1] in (1, 3) else 0) in str(e.value)
    with pytest.raises(DeepDishHipError, match=r'\(-3\).*ANY_SIZE'):
        from deepdish_amd.jpeg import JpegDecoder
        _decode(JpegDecoder(16, 16), [pillow_file(16, 16, 'noise', 95, '4:2:0')], scales=[1])


def test_progressive_twins_beside_baseline_files():
    files = _good_files(progressive=(2, 8, 9))
    assert [jpeg_dec_ref.parse(f)['sof'] if i not in (2, 8, 9) else 0xC2 for i, f in enumerate(files)].count(0xC2) == 3
    dec = _decoder(progressive=True)
    status, slots = _decode(dec, files)
    assert status.tolist() == [0] * len(files)
    want = [jpeg_prog_cases.reference(f) if i in (2, 8, 9) else reference(f) for i, f in enumerate(files)]
    _same(slots, _expect(dec, want))
    for i in (2, 8, 9):
        assert np.array_equal(want[i], pillow_decode(files[i]))
    scales = [(2, 4, 8, 1)[i % 4] for i in range(len(files))]
    status, slots = _decode(dec, files, scales=scales)
    assert status.tolist() == [0] * len(files)
    _same(slots, _expect(dec, [jpeg_prog_cases.reference(f, s) if i in (2, 8, 9) else _ref(f, s) for i, (f, s) in enumerate(zip(files, scales))]))


def test_split_routes_the_long_marker_less_file():
    files = [pillow_file(1, 1, 'noise', 95, '4:2:0'), pillow_file(MAX_H, MAX_W, 'noise', 95, '4:2:0'), pillow_file(8, 8, 'ramp', 50, 'L'),
             pillow_file(48, 37, 'noise', 95, '4:2:2'), pillow_file(17, 9, 'noise', 95, '4:4:4', 'mcu1')]
    scans = [jpeg_dec_ref.parse(f) for f in files]
    routed = sum(h['n_intervals'] == 1 and h['scan_length'] > 64 for h in scans)
    assert scans[1]['scan_length'] > 64 and scans[0]['scan_length'] <= 64 and scans[2]['scan_length'] <= 64 and routed >= 2
    dec = _decoder(split=True)
    status, slots = _decode(dec, files)
    assert status.tolist() == [0] * len(files)
    _same(slots, _expect(dec, [reference(f) for f in files]))
    stats = dec.split_stats()
    assert stats['files'] == routed and stats['subsequences'] > stats['files']


@pytest.mark.parametrize('max_h', [16, 17])
def test_planes_and_lds_in_one_call(max_h):
    """A decoder as wide as the narrowest 4:2:0 frame whose band does not fit in LDS at scale 1: a file of that width takes its planes
    through HBM (at 17 rows: two bands, the h2v2 filter reading the other band's chroma row from the planes), a 16 x 16 file beside it
    stays in LDS, and at scale 2 both do."""
    from deepdish_amd import jpeg
    W = 2400
    while jpeg.decoder_plan(max_h, W, 3, 2, 2)[0] == jpeg.DEC_PATH_LDS:
        W += 1
    assert 2500 < W < 2560 and jpeg.decoder_plan(max_h, W - 1, 3, 2, 2)[0] == jpeg.DEC_PATH_LDS
    assert jpeg.decoder_plan(16, 16, 3, 2, 2)[0] == jpeg.DEC_PATH_LDS and jpeg.decoder_plan(max_h, W, 3, 2, 2, scale=2)[0] == jpeg.DEC_PATH_LDS
    files = [pillow_file(max_h, W, 'ramp', 95, '4:2:0'), pillow_file(16, 16, 'noise', 95, '4:2:0'), pillow_file(max_h, W, 'noise', 50, '4:2:0', 'row1')]
    dec = _decoder(max_h, W, 3)
    status, slots = _decode(dec, files)
    assert status.tolist() == [0, 0, 0]
    _same(slots, _expect(dec, [reference(f) for f in files]))
    status, slots = _decode(dec, files, scales=[1, 2, 2])
    assert status.tolist() == [0, 0, 0]
    _same(slots, _expect(dec, [_ref(f, s) for f, s in zip(files, (1, 2, 2))]))
