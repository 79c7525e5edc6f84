"""CPU: tests/jpeg_prog_ref.py, the definition of progressive decoding, held to Pillow (libjpeg-turbo) byte for byte --
Image.open(f).convert('RGB') with the channels swapped, and im.draft(...) at scales 2, 4 and 8 -- on Pillow's own progressive files
(libjpeg's default script) over the baseline ref's grid, and on the scripts Pillow cannot write, from tests/jpeg_prog_writer.py.  The
writer is validated first: every file it writes must decode in Pillow to exactly the pixels of the baseline file it came from."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_dec_ref  # noqa: E402
import jpeg_prog_ref  # noqa: E402
import jpeg_prog_writer  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_decode, pillow_file  # noqa: E402
from jpeg_prog_cases import (SIZES, WRITER_SIZES, damaged_for_the_card, long_eobrun, pillow_grid, reference, refused, writer_grid,  # noqa: E402
                             written)
from jpeg_scaled_cases import pairs  # noqa: E402


def _pillow_draft(data, H, W, s):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft(im.mode, (W // s, H // s))
    assert im.size == (-(-W // s), -(-H // s)), 'Pillow chose another scale'
    return np.asarray(im.convert('RGB'))[..., ::-1]


@pytest.mark.parametrize('sampling', SAMPLINGS)
@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_ref_equals_pillow(H, W, sampling):
    """One component and 4:4:4 / 4:2:2 / 4:2:0; quality 50 and 95; no restart, an interval per MCU and per MCU row (whose DRI differs from
    scan to scan); full size and every scale Pillow's draft can be asked for."""
    scales = [s for (hw, s) in pairs() if hw == (H, W)]
    files = pillow_grid(H, W, sampling)
    assert len(files) == 6
    for data in files:
        got = reference(data)
        assert got.shape == (H, W, 3) and got.dtype == np.uint8
        assert np.array_equal(got, pillow_decode(data))
        for s in scales:
            assert np.array_equal(reference(data, s), _pillow_draft(data, H, W, s)), 'scale 1/%d differs from Pillow' % s


def test_progressive_and_baseline_of_one_picture_decode_alike():
    """The premise of the design: the same picture saved with progressive=True and without gives the same pixels and, where both files
    cover a block, the same coefficients."""
    for sampling in SAMPLINGS:
        a, b = pillow_file(37, 53, 'noise', 95, sampling), pillow_file(37, 53, 'noise', 95, sampling, progressive=True)
        assert np.array_equal(jpeg_dec_ref.decode(a), reference(b))
        h = jpeg_prog_ref.parse(b)
        ca, cb = jpeg_dec_ref.coefficients(a), jpeg_prog_ref.coefficients(b)
        for c, (_, hs, vs, _) in enumerate(h['comps']):
            bw, bh = -(-(-(-53 * hs // h['hmax'])) // 8), -(-(-(-37 * vs // h['vmax'])) // 8)
            at = [jpeg_prog_ref.block_index(h, c, x, y) for y in range(bh) for x in range(bw)]
            assert np.array_equal(ca[at], cb[at])


def test_the_default_script_is_three_levels():
    h = jpeg_prog_ref.parse(pillow_file(37, 53, 'noise', 95, '4:2:0', 'row1', progressive=True))
    assert [s['level'] for s in h['scans']] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and h['n_levels'] == 3
    assert [s['restart_interval'] for s in h['scans']] == [4, 7, 4, 4, 7, 7, 4, 4, 4, 7]          # re-read per scan: MCUs, or the component's blocks
    assert len(jpeg_prog_ref.parse(pillow_file(16, 16, 'noise', 95, 'L', progressive=True))['scans']) == 6


@pytest.mark.parametrize('H,W', WRITER_SIZES, ids=lambda v: str(v))
def test_writer_scripts(H, W):
    """(a) spectral selection only, (b) narrow bands, (c) Al = 3 refined bit by bit, (d) DC scans one component at a time: Pillow first,
    then the ref."""
    files = writer_grid(H, W)
    assert len(files) == 16
    for data, base in files:
        want = pillow_decode(base)
        assert np.array_equal(pillow_decode(data), want), 'the writer wrote a file Pillow reads otherwise'
        assert np.array_equal(reference(data), want)
    for s in [s for (hw, s) in pairs() if hw == (H, W)]:
        for data, base in files[::5]:
            assert np.array_equal(reference(data, s), _pillow_draft(base, H, W, s))


def test_writer_default_script_is_pillows_pixels():
    for sampling in SAMPLINGS:
        data, base = written(37, 53, sampling, 'default', 0)
        assert np.array_equal(pillow_decode(data), pillow_decode(base)) and np.array_equal(reference(data), pillow_decode(base))


def test_an_eob_run_longer_than_one_symbol_carries():
    """(e)"""
    data, base = long_eobrun()
    h = jpeg_prog_ref.parse(data)
    assert h['scans'][1]['units'] == 33024 > 32767 and h['scans'][1]['n_intervals'] == 1
    want = pillow_decode(base)
    assert np.array_equal(pillow_decode(data), want)
    assert np.array_equal(reference(data), want)


def test_refused_scripts_raise_with_the_reasons_word():
    for name, (data, word) in refused().items():
        with pytest.raises(ValueError, match='^' + word):
            jpeg_prog_ref.parse(data)
    assert {w for _, w in refused().values()} == set(jpeg_prog_ref.REFUSALS)


def test_damage_raises_corrupt():
    good, bad = damaged_for_the_card()
    assert np.array_equal(reference(good), pillow_decode(good))
    with pytest.raises(ValueError, match='^incomplete'):
        jpeg_prog_ref.decode(bad['cut_mid_script'])
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_prog_ref.decode(bad['cut_last_scan'])
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_prog_ref.decode(bad['replaced_in_refinement'])


def test_a_baseline_file_goes_to_the_baseline_ref():
    data = pillow_file(17, 9, 'noise', 95, '4:2:0', 'mcu1')
    assert 'scans' not in jpeg_prog_ref.parse(data)
    assert np.array_equal(jpeg_prog_ref.decode(data), jpeg_dec_ref.decode(data)) and np.array_equal(jpeg_prog_ref.decode(data, 2), reference(data, 2))
