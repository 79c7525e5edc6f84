"""GPU: JpegDecoder(..., progressive=True) (jpeg_prog_markers_k, jpeg_prog_entropy_k and the unchanged pixel kernels of csrc/jpeg_dec.hip)
held to tests/jpeg_prog_ref.py -- equality everywhere, no tolerance.  Pillow's own progressive files over the ref's grid; the scripts
Pillow cannot write (tests/jpeg_prog_writer.py, (a) .. (e)); the smallest shapes at which each path can go wrong (8 x 8: one block;
16 x 5 and 3 x 40: component grids smaller than the MCU grid, where a scan of one component walks another raster; 37 x 53 at 4:2:0; a
file wide enough for the HBM-planes path); scales 2, 4 and 8; a call that mixes baseline and progressive files of all four samplings.
Frames and statuses land in sentinel-guarded buffers.  Damaged files are those scripts/jpeg_prog_check.cpp decodes under the sanitizers
first (tests/test_jpeg_prog_host.py); nothing is looped or retried on the card."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_prog_ref  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_decode, pillow_file  # noqa: E402
from jpeg_prog_cases import SIZES, WRITER_SIZES, damaged_for_the_card, long_eobrun, pillow_grid, reference, writer_grid, written  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5


@functools.lru_cache(maxsize=None)
def _decoder(H, W, max_frames=32, scale=1):
    from deepdish_amd.jpeg import JpegDecoder
    return JpegDecoder(H, W, max_frames=max_frames, scale=scale, progressive=True)


def _decode(dec, files):
    """dd_jpegdec_decode into sentinel-filled frames and statuses between two guards -> (status [n], frames [n, out_H, out_W, 3])."""
    import torch
    n, size = len(files), dec.out_H * dec.out_W * 3
    buf = torch.full((GUARD + n * size + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
    dec.decode(files, out=buf[GUARD:GUARD + n * size].view(n, dec.out_H, dec.out_W, 3), status=st[GUARD:GUARD + n])
    dec.ctx.sync()
    host, sth = dec.ctx.to_host(buf), dec.ctx.to_host(st)
    assert (host[:GUARD] == SENTINEL).all(), 'bytes before the first frame were written'
    assert (host[GUARD + n * size:] == SENTINEL).all(), 'bytes behind the last frame were written'
    assert (sth[:GUARD] == -7).all() and (sth[GUARD + n:] == -7).all(), 'a status outside the batch was written'
    return sth[GUARD:GUARD + n], host[GUARD:GUARD + n * size].reshape(n, dec.out_H, dec.out_W, 3)


def _check(dec, files, pillow=False):
    status, frames = _decode(dec, files)
    assert status.tolist() == [0] * len(files)
    for i, data in enumerate(files):
        assert np.array_equal(frames[i], reference(data, dec.scale)), 'frame %d differs from jpeg_prog_ref' % i
        if pillow:
            assert np.array_equal(frames[i], pillow_decode(data)), 'frame %d differs from Pillow' % i


@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_pillow_grid(H, W):
    """Pillow's progressive files: one component and 4:4:4 / 4:2:2 / 4:2:0, quality 50 and 95, no restart, an interval per MCU and per MCU
    row (whose DRI differs from scan to scan): 24 files in one call, three levels."""
    files = pillow_grid(H, W)
    assert len(files) == 24 and all(jpeg_prog_ref.parse(f)['n_levels'] == 3 for f in files)
    _check(_decoder(H, W), files, pillow=True)


@pytest.mark.parametrize('H,W', WRITER_SIZES, ids=lambda v: str(v))
def test_writer_scripts(H, W):
    """(a) spectral selection only, (b) narrow bands, (c) Al = 3 refined a bit per scan (four levels), (d) DC scans one component at a
    time: 16 files in one call, with table slots that change from scan to scan, shared tables, and EOB runs cut at 5 blocks."""
    files = [d for d, _ in writer_grid(H, W)]
    assert len(files) == 16 and {jpeg_prog_ref.parse(f)['n_levels'] for f in files} == {1, 2, 4}
    status, frames = _decode(_decoder(H, W), files)
    assert status.tolist() == [0] * 16
    for i, (data, base) in enumerate(writer_grid(H, W)):
        assert np.array_equal(frames[i], reference(data)) and np.array_equal(frames[i], pillow_decode(base)), i


def test_an_eob_run_longer_than_one_symbol_carries():
    """(e): 33 024 blocks without an AC coefficient; every AC scan is one lane's EOB run, cut by the writer at 32 767."""
    data, base = long_eobrun()
    status, frames = _decode(_decoder(1032, 2048, 1), [data])
    assert status.tolist() == [0]
    assert np.array_equal(frames[0], reference(data)) and np.array_equal(frames[0], pillow_decode(base))


def test_a_band_too_wide_for_lds():
    """17 x 2513 at 4:2:0 takes its planes through HBM (tests/test_gpu_jpeg_decode.py finds that width): a progressive file, its baseline
    twin and a greyscale progressive file (LDS) in one call."""
    from deepdish_amd import jpeg
    H, W = 17, 2513
    assert jpeg.decoder_plan(H, W, 3, 2, 2)[0] == jpeg.DEC_PATH_PLANES and jpeg.decoder_plan(H, W, 1, 1, 1)[0] == jpeg.DEC_PATH_LDS
    _check(_decoder(H, W, 3), [pillow_file(H, W, 'noise', 50, '4:2:0', 'row1', progressive=True), pillow_file(H, W, 'noise', 50, '4:2:0', 'row1'),
                               pillow_file(H, W, 'ramp', 95, 'L', progressive=True)], pillow=True)


@pytest.mark.parametrize('scale', [2, 4, 8])
@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_scaled(H, W, scale):
    """The scaled pixel kernels read the same coefficients: every sampling of Pillow's grid and one scripted file of each."""
    files = pillow_grid(H, W)[::2] + [written(H, W, s, 'deep', 3)[0] for s in SAMPLINGS]
    dec = _decoder(H, W, 16, scale)
    assert (dec.out_H, dec.out_W) == (-(-H // scale), -(-W // scale))
    _check(dec, files)


def test_baseline_and_progressive_files_of_every_sampling_in_one_call():
    """jpeg_entropy_k and jpeg_prog_entropy_k fill the coefficients of neighbouring frames of one call."""
    H, W = 40, 56
    files = []
    for k, s in enumerate(SAMPLINGS):
        files += [pillow_file(H, W, 'noise', 95, s, ('mcu3', 'none', 'row1', 'mcu1')[k]), pillow_file(H, W, 'noise', 95, s, ('row1', 'mcu1', 'none', 'row1')[k], progressive=True),
                  written(H, W, s, ('narrow', 'dc_each', 'deep', 'spectral')[k], k)[0]]
    assert len(files) == 12
    _check(_decoder(H, W), files)
    _check(_decoder(H, W), files[::-1])
    prog = ['scans' in jpeg_prog_ref.parse(f) for f in files]
    assert sum(prog) == 8
    _check(_decoder(H, W), [f for f, p in zip(files, prog) if not p])          # baseline files alone on such a decoder
    _check(_decoder(H, W), [f for f, p in zip(files, prog) if p])              # progressive files alone: no baseline interval at all


def test_many_lanes_of_a_wave():
    """jpeg_prog_entropy_k with 64 lanes to a wave (DD_JPEGDEC_LANES is read when a decoder is created): files with an interval per MCU,
    several waves a level, lanes of different scans and files side by side."""
    from deepdish_amd.jpeg import JpegDecoder
    files = [pillow_file(40, 56, 'noise', 95, s, 'mcu1', seed=k, progressive=True) for k, s in enumerate(['4:2:0', '4:2:2', '4:4:4', 'L', '4:2:0', '4:2:2', '4:2:0'])]
    keep = os.environ.get('DD_JPEGDEC_LANES')
    os.environ['DD_JPEGDEC_LANES'] = '64'
    try:
        dec = JpegDecoder(40, 56, max_frames=7, progressive=True)
    finally:
        if keep is None:
            del os.environ['DD_JPEGDEC_LANES']
        else:
            os.environ['DD_JPEGDEC_LANES'] = keep
    _check(dec, files, pillow=True)


def test_status_contract():
    """A file cut inside its last scan and one with a byte of a refinement scan replaced (ST_DATA), a file cut in mid-script and a script
    that lacks its last scan (ST_HEADER: an incomplete progressive file is refused), a file of another size (ST_SIZE) and an empty entry
    (ST_NO_FRAME) stand between good frames.  An empty entry lies in front of and behind every file, so every frame has a guard band of a
    whole frame, which must stay untouched; the good frames are exact."""
    from deepdish_amd import jpeg
    good, bad = damaged_for_the_card()
    for name in ('cut_last_scan', 'replaced_in_refinement'):
        with pytest.raises(ValueError, match='corrupt'):
            jpeg_prog_ref.decode(bad[name])
    for name in ('cut_mid_script', 'incomplete_script'):
        with pytest.raises(ValueError, match='^incomplete'):
            jpeg_prog_ref.decode(bad[name])
    goods = [good, pillow_file(40, 56, 'ramp', 50, '4:2:2', 'row1', progressive=True), written(40, 56, '4:4:4', 'deep', 3)[0], pillow_file(40, 56, 'noise', 95, '4:2:0', 'mcu3'),
             pillow_file(40, 56, 'noise', 50, 'L', progressive=True)]
    entries = [(goods[0], 0), (bad['cut_last_scan'], jpeg.ST_DATA), (goods[1], 0), (bad['replaced_in_refinement'], jpeg.ST_DATA), (goods[2], 0),
               (bad['cut_mid_script'], jpeg.ST_HEADER), (pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True), jpeg.ST_SIZE), (goods[3], 0),
               (bad['incomplete_script'], jpeg.ST_HEADER), (goods[4], 0)]
    files, want = [b''], [jpeg.ST_NO_FRAME]
    for data, st in entries:
        files += [data, b'']
        want += [st, jpeg.ST_NO_FRAME]
    status, frames = _decode(_decoder(40, 56), files)
    assert status.tolist() == want
    for i, (data, st) in enumerate(zip(files, want)):
        if st == 0:
            assert np.array_equal(frames[i], reference(data)), i
        elif st != jpeg.ST_DATA:
            assert (frames[i] == SENTINEL).all(), 'frame %d (status %d) was written' % (i, st)


def test_without_the_option_nothing_changes():
    """A decoder made as before refuses a progressive file as before; the option is a keyword the parent commit does not know."""
    from deepdish_amd import jpeg
    base, prog = pillow_file(40, 56, 'noise', 95, '4:2:0'), pillow_file(40, 56, 'noise', 95, '4:2:0', progressive=True)
    dec = jpeg.JpegDecoder(40, 56, max_frames=2)
    assert dec.progressive is False
    frames, status = dec.decode([prog, base])
    dec.ctx.sync()
    assert dec.ctx.to_host(status).tolist() == [jpeg.ST_HEADER, 0]
    assert np.array_equal(dec.ctx.to_host(frames)[1], reference(base))
