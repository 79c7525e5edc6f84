"""CPU: dd_jpeg_parse (csrc/jpeg_parse.h) through ctypes, without a device: its fields against tests/jpeg_dec_ref.parse for files of every
accepted kind, and every refusal by its code, its reason and a word of its message.  Pillow writes the progressive and the CMYK file; the
other refusals are bytes patched into a good header; a header cut at every length is refused, never accepted and never a crash."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_file, picture  # noqa: E402

E_FORMAT = -5


def _same(data):
    from deepdish_amd import jpeg
    got, want = jpeg.parse(data), jpeg_dec_ref.parse(data)
    for k in ('height', 'width', 'ncomp', 'sof', 'hmax', 'vmax', 'mcus_x', 'mcus_y', 'blocks_per_mcu', 'restart_interval', 'n_intervals', 'scan_offset',
              'scan_length', 'td', 'ta'):
        assert got[k] == want[k], k
    assert got['comps'] == [c[1:] for c in want['comps']]
    assert sorted(got['quant']) == sorted(want['quant']) and all(np.array_equal(got['quant'][t], want['quant'][t]) for t in want['quant'])
    assert got['huff'] == want['huff']
    return got


def test_fields_of_every_accepted_kind():
    for sampling in SAMPLINGS:
        for restart, optimize in (('none', False), ('mcu3', False), ('row1', True)):
            for H, W in ((1, 1), (17, 33), (40, 56)):
                got = _same(pillow_file(H, W, 'noise', 95, sampling, restart, optimize))
                assert (got['height'], got['width']) == (H, W) and got['ncomp'] == (1 if sampling == 'L' else 3)
    got = _same(pillow_file(40, 56, 'noise', 50, '4:2:0', 'mcu3'))
    assert got['restart_interval'] == 3 and got['n_intervals'] == 4 and got['blocks_per_mcu'] == 6 and (got['mcus_x'], got['mcus_y']) == (4, 3)
    assert _same(pillow_file(40, 56, 'noise', 50, '4:2:2'))['comps'][0] == (2, 1, 0)


def test_fields_of_this_builds_own_header():
    from deepdish_amd import jpeg
    for H, W, q, r in ((480, 640, 95, 1), (33, 47, 20, 2), (8192, 8192, 100, 127)):
        got = _same(jpeg.header(H, W, q, r))
        assert got['scan_length'] == 0 and got['restart_interval'] == r * ((W + 15) // 16) and got['comps'] == [(2, 2, 0), (1, 1, 1), (1, 1, 1)]


def _lookup_tables_decode_every_code(info, t):
    """The kernel's look-up form against Annex C's code assignment."""
    h = info.huff[t]
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(h.bits[l - 1]):
            if l <= 8:
                for j in range(1 << (8 - l)):
                    assert h.look[(code << (8 - l)) + j] == (l << 8) | h.vals[k]
            else:
                assert code <= h.maxcode[l] and h.vals[h.valoff[l] + code] == h.vals[k]
            code += 1
            k += 1
        if not h.bits[l - 1]:
            assert h.maxcode[l] == -1
        code <<= 1
    assert k == h.nvals


def test_lookup_form_of_annex_k_and_optimised_tables():
    import ctypes
    from deepdish_amd import jpeg
    from deepdish_amd._lib import lib
    for data in (pillow_file(40, 56, 'noise', 100, '4:2:0'), pillow_file(40, 56, 'noise', 100, '4:2:0', optimize=True), pillow_file(17, 33, 'ramp', 20, 'L', optimize=True)):
        info = jpeg.JpegInfo()
        assert lib().dd_jpeg_parse(data, len(data), ctypes.byref(info)) == 0
        for t in range(4):
            if info.huff[t].defined:
                _lookup_tables_decode_every_code(info, t)
        covered = sum(1 for e in info.huff[2].look if e)
        assert 0 < covered <= 256


def _refused(data, reason, word):
    import ctypes
    from deepdish_amd import jpeg
    from deepdish_amd._lib import lib
    info = jpeg.JpegInfo()
    rc = lib().dd_jpeg_parse(bytes(data), len(data), ctypes.byref(info))
    msg = lib().dd_last_error().decode()
    assert rc == E_FORMAT, (rc, msg)
    assert jpeg.REASONS[info.reason] == reason, (jpeg.REASONS[info.reason], msg)
    assert word in msg and 'dd_jpeg_parse' in msg, msg
    with pytest.raises(ValueError):
        jpeg_dec_ref.parse(bytes(data))


def _segments(data):
    """marker -> offset of its 0xFF, for the segments in front of the scan."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        out.setdefault(data[i + 1], i)
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    out[0xDA] = i
    return out


def _patch(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


GOOD = pillow_file(16, 16, 'noise', 95, '4:2:0')
GREY = pillow_file(16, 16, 'noise', 95, 'L')


def test_refusals_pillow_writes():
    from PIL import Image
    _refused(pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True), 'progressive', 'progressive')
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(picture(16, 16, 'noise'))).convert('CMYK').save(f, 'JPEG')
    _refused(f.getvalue(), 'components', '4 components')


def test_refusals_by_patched_bytes():
    seg = _segments(GOOD)
    sof, dqt, dht, sos, app0 = seg[0xC0], seg[0xDB], seg[0xC4], seg[0xDA], seg[0xE0]
    _refused(_patch(GOOD, sof + 1, 0xC2), 'progressive', 'progressive')
    _refused(_patch(GOOD, sof + 1, 0xC9), 'arithmetic', 'arithmetic')
    _refused(_patch(GOOD, sof + 1, 0xC3), 'lossless', 'lossless')
    _refused(_patch(GOOD, sof + 4, 12), 'precision', '12-bit')
    _refused(_patch(GOOD, dqt + 4, 0x10), 'precision', '16-bit quant')
    _refused(_patch(GOOD, sof + 11, 0x12), 'sampling', 'sampling')                 # 4:4:0
    _refused(_patch(GOOD, sof + 11, 0x41), 'sampling', 'sampling')                 # 4:1:1
    _refused(_patch(GOOD, sof + 14, 0x22), 'sampling', 'sampling')                 # chroma as wide as luma, both doubled
    _refused(_patch(GOOD, sof + 12, 3), 'undefined', 'does not define')            # luma's quant table: one the file does not hold
    _refused(_patch(GREY, _segments(GREY)[0xDA] + 6, 0x11), 'undefined', 'does not define')        # a greyscale file holds tables 0 only
    _refused(_patch(GOOD, sos + 6, 0x20), 'huffman', 'Huffman tables')             # DC table 2
    _refused(_patch(_patch(GOOD, sof + 5, 0), sof + 6, 0), 'size', 'size')         # H = 0
    _refused(_patch(_patch(GOOD, sof + 7, 0), sof + 8, 0), 'size', 'size')         # W = 0
    _refused(_patch(_patch(GOOD, sof + 5, 0x20), sof + 6, 1), 'size', '8193')      # H = 8193
    _refused(_patch(GOOD, dht + 5, 3), 'huffman', 'over-subscribes')               # three codes of one bit
    many = bytearray(GOOD)
    many[dht + 5:dht + 21] = bytes([0] * 14 + [255, 255])
    _refused(many, 'huffman', '510 symbols')
    _refused(_patch(_patch(GOOD, app0 + 2, 0xFF), app0 + 3, 0xFF), 'truncated', 'past the file')
    _refused(_patch(GOOD, sos + 11, 1), 'progressive', 'Ss 1')                 # Ss
    _refused(_patch(GOOD, sos + 12, 5), 'progressive', 'Se 5')
    _refused(_patch(GOOD, sos + 13, 0x10), 'progressive', 'Ah/Al')
    one = GOOD[:sos] + bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0]) + GOOD[jpeg_dec_ref.parse(GOOD)['scan_offset']:]
    _refused(one, 'scans', 'several scans')
    adobe = GOOD[:sos] + bytes([0xFF, 0xEE, 0, 14]) + b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 0]) + GOOD[sos:]
    _refused(adobe, 'components', 'Adobe transform 0')
    from deepdish_amd import jpeg
    ycc = GOOD[:sos] + bytes([0xFF, 0xEE, 0, 14]) + b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 1]) + GOOD[sos:]
    assert jpeg.parse(ycc)['height'] == 16                                          # transform 1 is YCbCr
    _refused(b'\x89PNG\r\n\x1a\n' + GOOD, 'truncated', 'SOI')


def test_a_header_cut_at_every_length_is_refused():
    """Every length from 0 up to the SOS segment's last byte but one.  (At the SOS segment's end the header is whole: the parser accepts
    it with a scan of 0 bytes, and the decode then reports DD_JPEG_ST_DATA.)"""
    import ctypes
    from deepdish_amd import jpeg
    from deepdish_amd._lib import lib
    end = jpeg_dec_ref.parse(GOOD)['scan_offset']
    info = jpeg.JpegInfo()
    for n in range(end):
        cut = GOOD[:n]
        assert lib().dd_jpeg_parse(cut, n, ctypes.byref(info)) == E_FORMAT, n
        assert jpeg.REASONS[info.reason] == 'truncated' and b'dd_jpeg_parse' in lib().dd_last_error(), n
    assert lib().dd_jpeg_parse(GOOD[:end], end, ctypes.byref(info)) == 0 and info.scan_length == 0
    assert lib().dd_jpeg_parse(None, 0, ctypes.byref(info)) == -1


def test_parse_raises_with_the_reason():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    with pytest.raises(DeepDishHipError, match='progressive') as e:
        jpeg.parse(pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True))
    assert e.value.reason == 'progressive' and e.value.code == E_FORMAT
