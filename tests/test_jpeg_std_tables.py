"""CPU: the default Huffman tables (DD_JPEGDEC_STD_TABLES; csrc/jpeg_parse.h jpd_huffman_std) through ctypes, without a device.  Pillow
writes files with the standard tables; tests/jpeg_std_cases.strip removes them table by table -- all, chroma only, luma only, DC0 only,
AC0 + DC1 -- which is what a UVC camera in MJPG mode sends.  First Pillow itself (libjpeg-turbo's jstdhuff.c) must decode every stripped
file to the pixels of the untouched one; then parse(f, std_tables=True) must give the untouched file's four tables field for field, look-up
form included, parse(f) must refuse as ever, and tests/jpeg_dec_ref.py on that record must give the untouched file's pixels.  Equality
everywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import pillow_decode, reference  # noqa: E402
from jpeg_std_cases import SAMPLINGS, SIZES, VARIANTS, referenced, standard_file, strip  # noqa: E402

CASES = [(s, H, W, v) for s in SAMPLINGS for (H, W) in SIZES for v in VARIANTS]


def _info(data, flags):
    from deepdish_amd import jpeg
    from deepdish_amd._lib import lib
    info = jpeg.JpegInfo()
    rc = lib().dd_jpeg_parse_flags(data, len(data), flags, ctypes.byref(info), None)
    return rc, info


def _ref_header(rec):
    """A record of deepdish_amd.jpeg.parse as the dict tests/jpeg_dec_ref.parse gives."""
    h = dict(rec)
    h['comps'] = [(c + 1,) + tuple(comp) for c, comp in enumerate(rec['comps'])]
    h['adobe_transform'] = None
    return h


def test_pillow_decodes_every_stripped_file_to_the_same_pixels():
    """The premise: libjpeg-turbo fills the undefined slots with the Annex K.3 tables."""
    for s, H, W, v in CASES:
        whole = standard_file(H, W, s)
        f = strip(whole, VARIANTS[v])
        assert (len(f) < len(whole)) == bool(referenced(s, VARIANTS[v])), (s, H, W, v)
        assert np.array_equal(pillow_decode(f), pillow_decode(whole)), (s, H, W, v)


def test_the_flagged_parser_gives_the_unstripped_files_tables_field_for_field():
    from deepdish_amd import jpeg
    for s, H, W, v in CASES:
        whole = standard_file(H, W, s)
        f = strip(whole, VARIANTS[v])
        rc_w, want = _info(whole, 0)
        rc, got = _info(f, jpeg.DEC_STD_TABLES)
        assert rc_w == 0 and rc == 0, (s, H, W, v)
        for t in range(4):
            assert bytes(got.huff[t]) == bytes(want.huff[t]), (s, H, W, v, t)          # bits, vals, look, maxcode, valoff, nvals, defined
        assert got.scan_length == want.scan_length and got.scan_offset == want.scan_offset - (len(whole) - len(f))
        rec, rec_w = jpeg.parse(f, std_tables=True), jpeg.parse(whole)
        assert rec['huff'] == rec_w['huff'] and rec['td'] == rec_w['td'] and rec['ta'] == rec_w['ta']
        assert sorted(rec['huff']) == ([(0, 0), (1, 0)] if s == 'L' else [(0, 0), (0, 1), (1, 0), (1, 1)])


def test_a_defined_slot_is_left_as_the_file_defines_it():
    """Optimised tables in the file, the chroma ones stripped: luma stays the file's own, chroma becomes Annex K's."""
    from deepdish_amd import jpeg
    from jpeg_dec_cases import pillow_file
    whole = pillow_file(40, 56, 'noise', 75, '4:2:0', optimize=True)
    std = jpeg.parse(standard_file(40, 56, '4:2:0'))['huff']
    own = jpeg.parse(whole)['huff']
    assert own[(0, 0)] != std[(0, 0)] and own[(1, 0)] != std[(1, 0)]
    got = jpeg.parse(strip(whole, VARIANTS['chroma']), std_tables=True)['huff']
    assert got[(0, 0)] == own[(0, 0)] and got[(1, 0)] == own[(1, 0)] and got[(0, 1)] == std[(0, 1)] and got[(1, 1)] == std[(1, 1)]


def test_without_the_flag_the_stripped_file_is_refused_as_ever():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    for s, H, W, v in CASES:
        f = strip(standard_file(H, W, s), VARIANTS[v])
        if not referenced(s, VARIANTS[v]):
            assert jpeg.parse(f)['height'] == H          # a greyscale file never had the chroma tables
            continue
        with pytest.raises(DeepDishHipError, match='does not define') as e:
            jpeg.parse(f)
        assert e.value.reason == 'undefined' and e.value.code == jpeg.E_FORMAT
        with pytest.raises(DeepDishHipError) as e:
            jpeg.parse(f, progressive=True)
        assert e.value.reason == 'undefined'


def test_a_stripped_progressive_file_is_refused_as_ever():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    whole = standard_file(40, 56, '4:2:0', progressive=True)
    assert jpeg.parse(whole, progressive=True, std_tables=True)['sof'] == 0xC2
    f = strip(whole, VARIANTS['all'])
    assert len(f) < len(whole)
    for kw in ({'progressive': True}, {'progressive': True, 'std_tables': True}):
        with pytest.raises(DeepDishHipError) as e:
            jpeg.parse(f, **kw)
        assert e.value.reason == 'undefined', kw
    for kw in ({}, {'std_tables': True}):
        with pytest.raises(DeepDishHipError) as e:
            jpeg.parse(f, **kw)
        assert e.value.reason == 'progressive', kw


def test_a_scan_that_references_table_id_2_is_refused_as_ever():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    whole = standard_file(40, 56, '4:2:0')
    for f, kws in ((whole, ({}, {'std_tables': True})), (strip(whole, VARIANTS['all']), ({'std_tables': True},)), (strip(whole, VARIANTS['chroma']), ({'std_tables': True},))):
        sos = jpeg.parse(f, std_tables=True)['scan_offset']
        assert f[sos - 14:sos - 12] == b'\xff\xda' and f[sos - 6] == 0x11          # the SOS segment: the Cb component reads DC 1 / AC 1
        for patch in (0x21, 0x12):
            g = bytearray(f)
            g[sos - 6] = patch
            for kw in kws:
                with pytest.raises(DeepDishHipError, match='0 and 1 only') as e:
                    jpeg.parse(bytes(g), **kw)
                assert e.value.reason == 'huffman'


def test_an_unknown_flag_is_refused():
    from deepdish_amd._lib import lib
    data = standard_file(16, 16, '4:2:0')
    assert _info(data, 1)[0] == -1 and b'flags' in lib().dd_last_error()


def test_jpeg_dec_ref_on_the_record_gives_the_unstripped_files_pixels(monkeypatch):
    from deepdish_amd import jpeg
    for s, H, W, v in CASES:
        if (H, W) == (40, 56) and v not in ('all', 'ac0_dc1'):
            continue                                       # the reference decoder is slow: the larger size with two variants only
        whole = standard_file(H, W, s, restart='mcu3' if v == 'luma' else 'none')
        f = strip(whole, VARIANTS[v])
        header = _ref_header(jpeg.parse(f, std_tables=True))
        monkeypatch.setattr(jpeg_dec_ref, 'parse', lambda data, header=header: header)
        got = jpeg_dec_ref.decode(f)
        monkeypatch.undo()
        assert np.array_equal(got, reference(whole)), (s, H, W, v)
        assert np.array_equal(got, pillow_decode(f)), (s, H, W, v)
