"""Every route of the JPEG decoder's call plan (csrc/jpeg_dec_plan.h) in one call.  One decoder of at most 2528 x 48 (w x h) with all four
options -- progressive, split, any_size, std_tables -- at scale 1 takes nine files at once: a 4:2:0 baseline file with a restart interval per
MCU (one lane per interval), a marker-less 4:4:4 file longer than a subsequence (the split kernel), a progressive 4:2:2 file (a launch per
level), a greyscale file, a 4:2:0 file without its DHT segment, a 2528 x 16 4:2:0 file whose band does not fit in LDS (the planes path), an
empty file, a file whose header is refused and a file taller than the decoder; the per-file scales are 1, 2, 4 and 8.  Every good frame
equals tests/jpeg_dec_ref.py, jpeg_scaled_ref.py or jpeg_prog_ref.py byte for byte in the top-left corner of its slot and every other
byte of every slot keeps its sentinel.  The first test needs no GPU: it holds the files to the routes named, so that the second cannot
quietly run everything down one path."""
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
from jpeg_dec_cases import pillow_file, reference  # noqa: E402
from jpeg_std_cases import VARIANTS, standard_file, strip  # noqa: E402

MAX_H, MAX_W = 48, 2528
SPLIT_BYTES = 64                                        # the decoder's subsequence size when DD_JPEGDEC_SPLIT_BYTES is not set


def _refused_header(data):
    """The file with its SOF0 segment stating 12 bits a sample."""
    at = data.index(b'\xff\xc0')
    assert data[at + 4] == 8
    return data[:at + 4] + b'\x0c' + data[at + 5:]


def _call():
    """-> [(name, file, scale, reference frame or None)], in the order of the call."""
    whole = standard_file(17, 33, '4:2:0', restart='mcu1')
    dri = pillow_file(33, 40, 'noise', 95, '4:2:0', 'mcu1')
    split = pillow_file(17, 24, 'noise', 95, '4:4:4')
    prog = pillow_file(40, 56, 'ramp', 95, '4:2:2', progressive=True)
    grey = pillow_file(16, 5, 'noise', 50, 'L', 'row1')
    wide = pillow_file(16, MAX_W, 'ramp', 95, '4:2:0', 'mcu1')
    return [('dri', dri, 2, jpeg_scaled_cases.reference(dri, 2)),
            ('split', split, 4, jpeg_scaled_cases.reference(split, 4)),
            ('empty', b'', 1, None),
            ('progressive', prog, 8, jpeg_prog_cases.reference(prog, 8)),
            ('grey', grey, 1, reference(grey)),
            ('header', _refused_header(pillow_file(16, 16, 'noise', 95, '4:2:0')), 2, None),
            ('no dht', strip(whole, VARIANTS['all']), 2, jpeg_scaled_cases.reference(whole, 2)),
            ('wide', wide, 1, reference(wide)),
            ('tall', pillow_file(MAX_H + 1, 16, 'ramp', 95, '4:4:4'), 4, None)]


def test_the_files_take_the_routes_named():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    call = {name: (f, s) for name, f, s, _ in _call()}
    head = {name: jpeg_dec_ref.parse(call[name][0]) for name in ('dri', 'split', 'grey', 'wide')}
    head['no dht'] = jpeg.parse(call['no dht'][0], std_tables=True)
    assert {s for name, (f, s) in call.items() if name in head or name == 'progressive'} == {1, 2, 4, 8} and call['wide'][1] == 1
    assert [(head[k]['ncomp'], head[k]['hmax'], head[k]['vmax']) for k in ('dri', 'split', 'grey', 'no dht', 'wide')] == [(3, 2, 2), (3, 1, 1), (1, 1, 1), (3, 2, 2), (3, 2, 2)]
    # one lane per restart interval for all but the split file, which is the only baseline file that is one interval longer than a subsequence
    assert head['dri']['restart_interval'] == 1 and head['dri']['n_intervals'] == head['dri']['mcus_x'] * head['dri']['mcus_y'] > 1
    assert head['split']['n_intervals'] == 1 and head['split']['scan_length'] > SPLIT_BYTES
    assert [k for k, h in head.items() if h['n_intervals'] == 1 and h['scan_length'] > SPLIT_BYTES] == ['split']
    # a launch per level
    p = jpeg.parse(call['progressive'][0], progressive=True)
    assert p['sof'] == 0xC2 and (p['hmax'], p['vmax']) == (2, 1) and p['n_levels'] >= 2
    # no DHT segment: refused without the standard tables
    with pytest.raises(DeepDishHipError) as e:
        jpeg.parse(call['no dht'][0])
    assert e.value.reason == 'undefined'
    # the planes path for the wide file alone, at the narrowest width that takes it
    assert (head['wide']['height'], head['wide']['width']) == (16, MAX_W)
    assert jpeg.decoder_plan(16, MAX_W, 3, 2, 2)[0] == jpeg.DEC_PATH_PLANES and jpeg.decoder_plan(16, MAX_W - 16, 3, 2, 2)[0] == jpeg.DEC_PATH_LDS
    for k in ('dri', 'split', 'grey', 'no dht'):
        h = head[k]
        assert jpeg.decoder_plan(h['height'], h['width'], h['ncomp'], h['hmax'], h['vmax'], scale=call[k][1])[0] == jpeg.DEC_PATH_LDS
    assert jpeg.decoder_plan(p['height'], p['width'], 3, 2, 1, scale=8)[0] == jpeg.DEC_PATH_LDS
    # the three that must not decode
    with pytest.raises(DeepDishHipError):
        jpeg.parse(call['header'][0], progressive=True, std_tables=True)
    assert jpeg_dec_ref.parse(call['tall'][0])['height'] == MAX_H + 1 and call['empty'][0] == b''


@pytest.mark.gpu
def test_every_route_in_one_call():
    from deepdish_amd import jpeg
    from test_gpu_jpeg_anysize import SENTINEL, _decode, _expect, _same
    call = _call()
    dec = jpeg.JpegDecoder(MAX_H, MAX_W, max_frames=len(call), progressive=True, split=True, any_size=True, std_tables=True)
    assert (dec.out_H, dec.out_W) == (MAX_H, MAX_W)
    dec.profile(True)
    status, slots = _decode(dec, [f for _, f, _, _ in call], scales=[s for _, _, s, _ in call])
    bad = {'empty': jpeg.ST_NO_FRAME, 'header': jpeg.ST_HEADER, 'tall': jpeg.ST_SIZE}
    assert status.tolist() == [bad.get(name, jpeg.ST_OK) for name, _, _, _ in call]
    for (name, f, s, want), slot in zip(call, slots):
        if want is None:
            assert (slot == SENTINEL).all(), name
        else:
            h, w = (jpeg.parse(f, progressive=True, std_tables=True)[k] for k in ('height', 'width'))
            assert want.shape == (-(-h // s), -(-w // s), 3), name
    _same(slots, _expect(dec, [want for _, _, _, want in call]))
    assert dec.split_stats()['files'] == 1
    assert len(dec.level_ms()) == jpeg.parse(call[3][1], progressive=True)['n_levels']
