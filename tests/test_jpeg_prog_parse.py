"""CPU: deepdish_amd.jpeg.parse(file, progressive=True) -- dd_jpeg_parse_scans (csrc/jpeg_parse.h) through the C ABI, no device -- against
tests/jpeg_prog_ref.parse: the frame, every scan's parameters, byte range, geometry, restart interval, level and tables; every refused
script by its reason's word; and the default, which refuses a progressive file exactly as before."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_prog_ref  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_file  # noqa: E402
from jpeg_prog_cases import damaged_for_the_card, long_eobrun, pillow_grid, refused, writer_grid  # noqa: E402


def _same(got, want):
    for k in ('height', 'width', 'ncomp', 'sof', 'hmax', 'vmax', 'mcus_x', 'mcus_y', 'blocks_per_mcu'):
        assert got[k] == want[k], k
    assert got['sof'] == 0xC2 and got['n_intervals'] == 0 and got['huff'] == {}
    assert got['comps'] == [c[1:] for c in want['comps']]
    for t, q in want['quant'].items():
        assert np.array_equal(got['quant'][t], q)
    assert len(got['scans']) == len(want['scans']) and got['n_levels'] == want['n_levels'] and got['n_tables'] == want['n_tables']
    for g, w in zip(got['scans'], want['scans']):
        for k in ('comps', 'ss', 'se', 'ah', 'al', 'restart_interval', 'n_intervals', 'level'):
            assert g[k] == w[k], k
        assert (g['offset'], g['offset'] + g['length']) == (w['start'], w['end'])
        assert (g['blocks_x'], g['blocks_y']) == (w['bw'], w['bh'])
        if w['ss'] == 0 and w['ah'] == 0:
            assert g['dc'] == [(t[1], t[2]) for t in w['dc']]
        if w['ss'] > 0:
            assert g['ac'] == (w['ac'][0][1], w['ac'][0][2])


@pytest.mark.parametrize('H,W', [(8, 8), (16, 5), (3, 40), (37, 53)], ids=lambda v: str(v))
def test_scan_records_equal_the_ref(H, W):
    from deepdish_amd import jpeg
    for data in pillow_grid(H, W) + [d for d, _ in writer_grid(H, W)]:
        _same(jpeg.parse(data, progressive=True), jpeg_prog_ref.parse(data))


def test_the_default_script_is_three_levels_and_dri_is_read_per_scan():
    from deepdish_amd import jpeg
    h = jpeg.parse(pillow_file(37, 53, 'noise', 95, '4:2:0', 'row1', progressive=True), progressive=True)
    assert [s['level'] for s in h['scans']] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and h['n_levels'] == 3
    assert [s['restart_interval'] for s in h['scans']] == [4, 7, 4, 4, 7, 7, 4, 4, 4, 7]
    assert [(s['blocks_x'], s['blocks_y']) for s in h['scans'][:3]] == [(4, 3), (7, 5), (4, 3)]          # MCUs; luma's own blocks; chroma's
    e = jpeg.parse(long_eobrun()[0], progressive=True)
    assert e['scans'][1]['blocks_x'] * e['scans'][1]['blocks_y'] == 33024


def test_a_baseline_file_parses_as_without_the_option():
    from deepdish_amd import jpeg
    for sampling in SAMPLINGS:
        data = pillow_file(17, 33, 'noise', 95, sampling, 'mcu3')
        a, b = jpeg.parse(data), jpeg.parse(data, progressive=True)
        assert a.keys() == b.keys() and 'scans' not in b
        assert all(np.array_equal(a[k][t], b[k][t]) for k in ('quant',) for t in a[k]) and all(a[k] == b[k] for k in a if k != 'quant')


def test_every_refused_property_has_its_own_reason():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    seen = set()
    for name, (data, word) in refused().items():
        with pytest.raises(DeepDishHipError) as e:
            jpeg.parse(data, progressive=True)
        assert e.value.reason == word and e.value.code == jpeg.E_FORMAT, name
        assert 'dd_jpeg_parse' in str(e.value)
        seen.add(word)
    assert seen == {'progressive', 'ac_components', 'ac_before_dc', 'first_ah', 'refinement', 'incomplete', 'capacity'}
    with pytest.raises(DeepDishHipError, match='incomplete progressive file is refused') as e:
        jpeg.parse(damaged_for_the_card()[1]['cut_mid_script'], progressive=True)
    assert e.value.reason == 'incomplete'
    # what baseline refuses stays refused, by the same name
    for sof, word in ((0xC3, 'lossless'), (0xC9, 'arithmetic'), (0xCA, 'arithmetic')):
        good = pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True)
        i = good.index(b'\xff\xc2')
        with pytest.raises(DeepDishHipError) as e:
            jpeg.parse(good[:i] + bytes([0xFF, sof]) + good[i + 2:], progressive=True)
        assert e.value.reason == word
    # a baseline frame whose scan states progressive parameters is no progressive file
    base = bytearray(pillow_file(16, 16, 'noise', 95, 'L'))
    sos = base.index(b'\xff\xda')
    base[sos + 8] = 5
    with pytest.raises(DeepDishHipError) as e:
        jpeg.parse(bytes(base), progressive=True)
    assert e.value.reason == 'progressive'


def test_cut_at_every_length_never_reads_past_the_end():
    """Every prefix of a progressive file parses or is refused with a reason; a prefix that parses holds all ten scans."""
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    good = pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True)
    ok = 0
    for n in range(len(good)):
        try:
            h = jpeg.parse(good[:n], progressive=True)
            assert len(h['scans']) == 10
            ok += 1
        except DeepDishHipError as e:
            assert e.reason in ('truncated', 'incomplete', 'segment'), (n, e.reason)
    assert 0 < ok < 200


def test_without_the_option_a_progressive_file_is_refused_as_before():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    with pytest.raises(DeepDishHipError) as e:
        jpeg.parse(pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True))
    assert e.value.reason == 'progressive' and 'SOF2' in str(e.value)
