"""GPU: marker-less files decoded by many lanes (JpegDecoder(..., split=True); jpeg_split_entropy_k in csrc/jpeg_dec.hip, jpd_decode_span in
csrc/jpeg_dec_dev.h) held to tests/jpeg_dec_ref.py and to Pillow -- equality everywhere, statuses exact.  The shapes are the smallest at
which the rounds can go wrong: scans shorter than a subsequence (the old kernel), files that never fall into step (as many rounds as
subsequences), stuffed bytes on, before and behind a subsequence boundary, blocks longer than two subsequences, neighbours that take the
other kernels in the same call.  The subsequence size is read when a decoder is made (DD_JPEGDEC_SPLIT_BYTES).  Frames and statuses land in
sentinel-guarded buffers.  The two damaged files are ones the host check (scripts/jpeg_split_check.cpp) decodes under the sanitizers first;
nothing is looped or retried on the card."""
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
import jpeg_scaled_cases  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, own_file, pillow_decode, pillow_file, reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
DEFAULT_B = 64          # a scan longer than this is split when DD_JPEGDEC_SPLIT_BYTES is not set (the subsequences may then be larger)


@functools.lru_cache(maxsize=None)
def _decoder(H, W, B=None, max_frames=32, scale=1, progressive=False, split=True):
    """A decoder whose subsequences are B bytes (None: the default)."""
    from deepdish_amd.jpeg import JpegDecoder
    keep = os.environ.pop('DD_JPEGDEC_SPLIT_BYTES', None)
    if B is not None:
        os.environ['DD_JPEGDEC_SPLIT_BYTES'] = str(B)
    try:
        return JpegDecoder(H, W, max_frames=max_frames, scale=scale, progressive=progressive, split=split)
    finally:
        os.environ.pop('DD_JPEGDEC_SPLIT_BYTES', None)
        if keep is not None:
            os.environ['DD_JPEGDEC_SPLIT_BYTES'] = keep


def _decode(dec, files):
    """dd_jpegdec_decode into sentinel-filled frames and statuses between two guards -> (status [n], frames [n, out_H, out_W, 3])."""
    import torch
    n, size = len(files), dec.out_H * dec.out_W * 3
    buf = torch.full((GUARD + n * size + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
    out = buf[GUARD:GUARD + n * size].view(n, dec.out_H, dec.out_W, 3)
    dec.decode(files, out=out, status=st[GUARD:GUARD + n])
    dec.ctx.sync()
    host, sth = dec.ctx.to_host(buf), dec.ctx.to_host(st)
    assert (host[:GUARD] == SENTINEL).all(), 'bytes before the first frame were written'
    assert (host[GUARD + n * size:] == SENTINEL).all(), 'bytes behind the last frame were written'
    assert (sth[:GUARD] == -7).all() and (sth[GUARD + n:] == -7).all(), 'a status outside the batch was written'
    return sth[GUARD:GUARD + n], host[GUARD:GUARD + n * size].reshape(n, dec.out_H, dec.out_W, 3)


def _scan(data):
    h = jpeg_dec_ref.parse(data)
    return h, bytes(data)[h['scan_offset']:]


def _eligible(files, B):
    """How many of the files the host routes to jpeg_split_entropy_k: baseline, one restart interval, a scan longer than B."""
    n = 0
    for f in files:
        try:
            h, scan = _scan(f)
        except Exception:
            continue
        n += h['n_intervals'] == 1 and len(scan) > B
    return n


def _n_sub(data, B):
    return -(-len(_scan(data)[1]) // B)


def _check(dec, files, B, pillow=True):
    status, frames = _decode(dec, files)
    assert status.tolist() == [0] * len(files)
    for i, data in enumerate(files):
        assert np.array_equal(frames[i], reference(data)), 'frame %d differs from jpeg_dec_ref' % i
        if pillow:
            assert np.array_equal(frames[i], pillow_decode(data)), 'frame %d differs from Pillow' % i
    stats = dec.split_stats()
    assert stats['files'] == _eligible(files, B)
    if stats['files']:
        assert stats['subsequences'] >= stats['files'] and stats['lane_decodes'] >= stats['subsequences'] and stats['max_rounds'] >= 2
    else:
        assert stats == {'files': 0, 'subsequences': 0, 'max_rounds': 0, 'lane_decodes': 0}
    return stats


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize('B', [16, None], ids=['B16', 'Bdefault'])
@pytest.mark.parametrize('H,W', [(1, 1), (8, 8), (16, 16), (17, 33), (49, 7), (96, 64)], ids=lambda v: str(v))
def test_geometry(H, W, B):
    """test_gpu_jpeg_decode.test_geometry's 32 files, all without restart markers.  The 1 x 1 files have scans of a few bytes and all take
    the old kernel, as do the ramps of 8 x 8 (their noise at high quality is longer than a subsequence: both kernels in one call); every
    96 x 64 file is split."""
    files = [pillow_file(H, W, kind, q, s) for s in SAMPLINGS for kind in ('noise', 'ramp') for q in (1, 50, 95, 100)]
    assert len(files) == 32
    stats = _check(_decoder(H, W, B), files, B or DEFAULT_B)
    if (H, W) == (1, 1):
        assert max(len(_scan(f)[1]) for f in files) <= 16 and stats['files'] == 0
    if (H, W) == (8, 8):
        assert 0 < stats['files'] < 32
    if (H, W) == (96, 64):
        assert stats['files'] == 32


# ------------------------------------------------------------------ the rounds
@pytest.mark.parametrize('B', [16, 32])
def test_files_that_do_not_fall_into_step(B):
    """Noise at high quality: blocks without EOB, so a lane that starts from a guess stays out of step and the truth travels one
    subsequence a round.  The rounds stay within their bound, n_sub + 1."""
    for (H, W), q, s in (((40, 56), 95, '4:2:0'), ((96, 64), 100, '4:4:4')):
        data = pillow_file(H, W, 'noise', q, s)
        stats = _check(_decoder(H, W, B), [data], B)
        assert stats['files'] == 1
        assert 1 < stats['max_rounds'] <= _n_sub(data, B) + 1, stats
        assert stats['subsequences'] <= _n_sub(data, B)


@pytest.mark.parametrize('B', [16, 128])
def test_stuffed_bytes_on_subsequence_boundaries(B):
    """96 x 64 noise at quality 100, 4:4:4: its FF 00 pairs meet the boundaries in all three ways -- a boundary between the FF and its 00, a
    boundary on the FF, a boundary directly behind the pair -- at both sizes."""
    data = pillow_file(96, 64, 'noise', 100, '4:4:4')
    _, scan = _scan(data)
    pairs = [p for p in range(len(scan) - 1) if scan[p] == 0xFF and scan[p + 1] == 0]
    between = sum((p + 1) % B == 0 for p in pairs)
    on = sum(p % B == 0 for p in pairs)
    behind = sum((p + 2) % B == 0 for p in pairs)
    print('FF 00 pairs %d; boundaries between %d, on the FF %d, behind the pair %d' % (len(pairs), between, on, behind))
    assert len(pairs) >= 100 and between >= 1 and on >= 1 and behind >= 1
    _check(_decoder(96, 64, B), [data, pillow_file(96, 64, 'noise', 100, '4:4:4', seed=1)], B)


def test_a_subsequence_in_which_no_block_begins():
    """A block of the quality-100 file is longer than two 16-byte subsequences, so one of them lies wholly inside it and owns no block:
    every non-zero AC coefficient costs its category's bits and a code of at least two."""
    data = pillow_file(96, 64, 'noise', 100, '4:4:4')
    coef = jpeg_dec_ref.coefficients(data).astype(np.int64)
    ac = np.abs(coef[:, 1:])
    category = np.where(ac > 0, np.floor(np.log2(np.maximum(ac, 1))) + 1, 0)
    least_bits = (category + 2 * (ac > 0)).sum(axis=1)
    assert least_bits.max() > 2 * 16 * 8
    _check(_decoder(96, 64, 16), [data], 16)


# ------------------------------------------------------------------ routing
def test_every_route_in_one_call():
    """A split file, files with real restart intervals, a greyscale split file, a file of this build's encoder, a progressive file, an
    empty one and one of another size, in one call on a decoder made with both options."""
    from deepdish_amd import jpeg
    from jpeg_prog_cases import reference as prog_reference
    files = [pillow_file(40, 56, 'noise', 95, '4:2:0', 'none'), pillow_file(40, 56, 'noise', 95, '4:2:2', 'row1'), pillow_file(40, 56, 'ramp', 50, '4:4:4', 'mcu1'),
             pillow_file(40, 56, 'noise', 95, 'L', 'none'), own_file(40, 56, 'noise', 50, 2), pillow_file(40, 56, 'noise', 95, '4:2:0', 'row1', progressive=True), b'',
             pillow_file(16, 16, 'noise', 95, '4:2:0')]
    assert [jpeg_dec_ref.parse(f)['n_intervals'] for f in files[:5]] == [1, 5, 35, 1, 2]
    dec = _decoder(40, 56, None, 8, 1, True)
    status, frames = _decode(dec, files)
    assert status.tolist() == [0, 0, 0, 0, 0, 0, jpeg.ST_NO_FRAME, jpeg.ST_SIZE]
    for i in range(5):
        assert np.array_equal(frames[i], reference(files[i])), 'frame %d differs from jpeg_dec_ref' % i
    assert np.array_equal(frames[5], prog_reference(files[5])) and np.array_equal(frames[5], pillow_decode(files[5]))
    assert (frames[6:] == SENTINEL).all()
    assert dec.split_stats()['files'] == 2


@pytest.mark.parametrize('s', [2, 8])
@pytest.mark.parametrize('H,W', [(37, 53), (33, 16)], ids=lambda v: str(v))
def test_scales(H, W, s):
    """The scaled pixel kernels behind the split entropy stage: tests/jpeg_scaled_cases.py's 48 files, a third of them marker-less."""
    files = jpeg_scaled_cases.files(H, W)
    dec = _decoder(H, W, None, 64, s)
    status, frames = _decode(dec, files)
    assert status.tolist() == [0] * len(files)
    for i, d in enumerate(files):
        assert np.array_equal(frames[i], jpeg_scaled_cases.reference(d, s)), 'frame %d differs from jpeg_scaled_ref at 1/%d' % (i, s)
    assert dec.split_stats()['files'] == _eligible(files, DEFAULT_B) >= 8


def test_two_frames_of_480x640():
    """Rendered-looking scenes without restart markers, the workload's size, at the default subsequence size."""
    files = [pillow_file(480, 640, 'scene', 75, '4:2:0', 'none', seed=5), pillow_file(480, 640, 'scene', 95, '4:2:2', 'none', seed=6)]
    stats = _check(_decoder(480, 640, None, 2), files, DEFAULT_B)
    assert stats['files'] == 2 and stats['max_rounds'] <= max(_n_sub(f, DEFAULT_B) for f in files) + 1
    print(stats)


# ------------------------------------------------------------------ damaged input
@pytest.mark.parametrize('which', ['cut', 'replaced'])
def test_damaged_file_between_two_good_frames(which):
    """Only files the host check has decoded under the sanitizers with the same code (scripts/make_jpeg_split_corpus.py lists them).  The
    damaged frame reports a status; its neighbours are exact; the guards hold."""
    from deepdish_amd import jpeg
    import make_jpeg_split_corpus
    good, damaged = make_jpeg_split_corpus.damaged_for_the_card()
    assert jpeg_dec_ref.parse(damaged[which])['n_intervals'] == 1
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(damaged[which])
    other = pillow_file(40, 56, 'ramp', 50, '4:2:2', 'none')
    dec = _decoder(40, 56)
    status, frames = _decode(dec, [good, damaged[which], other])
    assert status.tolist() == [0, jpeg.ST_DATA, 0]
    assert np.array_equal(frames[0], reference(good)) and np.array_equal(frames[2], reference(other))
    assert dec.split_stats()['files'] == 3


# ------------------------------------------------------------------ the default
def test_a_decoder_without_the_option_is_untouched():
    files = [pillow_file(40, 56, 'noise', 95, '4:2:0', 'none'), pillow_file(40, 56, 'noise', 95, '4:2:2', 'row1'), pillow_file(40, 56, 'noise', 100, '4:4:4', 'none')]
    plain = _decoder(40, 56, None, 32, 1, False, False)
    assert plain.split is False and plain.split_stats() == {'files': 0, 'subsequences': 0, 'max_rounds': 0, 'lane_decodes': 0}
    status, frames = _decode(plain, files)
    assert status.tolist() == [0, 0, 0]
    assert plain.split_stats() == {'files': 0, 'subsequences': 0, 'max_rounds': 0, 'lane_decodes': 0}
    status2, frames2 = _decode(_decoder(40, 56), files)
    assert status2.tolist() == [0, 0, 0] and np.array_equal(frames, frames2)
    for i, d in enumerate(files):
        assert np.array_equal(frames[i], reference(d))


def test_a_subsequence_size_that_is_no_power_of_two_is_refused():
    from deepdish_amd._lib import DeepDishHipError
    for bad in ('100', '8', '8192', 'x'):
        with pytest.raises(DeepDishHipError, match='DD_JPEGDEC_SPLIT_BYTES=' + bad):
            _decoder(16, 16, bad)
