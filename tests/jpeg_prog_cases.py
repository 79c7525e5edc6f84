"""Files shared by the progressive decoder's tests: tests/test_jpeg_prog_ref.py (jpeg_prog_ref and jpeg_prog_writer against Pillow),
tests/test_jpeg_prog_host.py with scripts/make_jpeg_prog_corpus.py (the parser and the shared statements under the sanitizers),
tests/test_gpu_jpeg_progressive.py and tests/test_gpu_ingest_jpeg_progressive.py (the kernels against jpeg_prog_ref).  All are written at
test time, by Pillow and by jpeg_prog_writer, from seeded pictures."""
import functools
import io

import numpy as np

import jpeg_prog_ref
import jpeg_prog_writer
from jpeg_dec_cases import SAMPLINGS, pillow_file
from jpeg_scaled_cases import SIZES              # 8x8, 16x16, 17x9, 37x53, 33x16, 16x5, 3x40 and their transposes

QUALITIES = (50, 95)
RESTARTS = ('none', 'mcu1', 'row1')
WRITER_SIZES = [(8, 8), (16, 5), (3, 40), (37, 53), (64, 64)]
WRITER_SCRIPTS = ('spectral', 'narrow', 'deep', 'dc_each')            # (a) .. (d) of jpeg_prog_writer


def pillow_grid(H, W, sampling=None):
    """Pillow's own progressive files (libjpeg's default script): 6 a sampling, noise and ramp in turn."""
    out = []
    for smp in ([sampling] if sampling else SAMPLINGS):
        for q in QUALITIES:
            for r in RESTARTS:
                out.append(pillow_file(H, W, 'ramp' if len(out) % 2 else 'noise', q, smp, r, progressive=True))
    return out


@functools.lru_cache(maxsize=None)
def written(H, W, sampling, script, restart=0, eob_cap=0x7FFF, tables='scan', quality=95):
    """-> (the progressive file, the baseline file it came from)."""
    base = pillow_file(H, W, 'noise', quality, sampling)
    sc = [s + (restart,) for s in jpeg_prog_writer.SCRIPTS[script](1 if sampling == 'L' else 3)]
    return jpeg_prog_writer.write(base, sc, eob_cap, tables), base


def writer_grid(H, W):
    """Scripts (a) .. (d) over every sampling: no restart and table slots that change, an interval of 3 units and shared tables, an interval
    of 1 with EOB runs cut at 5 blocks."""
    out = []
    for smp in SAMPLINGS:
        for script in WRITER_SCRIPTS:
            k = len(out) % 3
            out.append(written(H, W, smp, script, (0, 3, 1)[k], (0x7FFF, 0x7FFF, 5)[k], ('scan', 'shared', 'scan')[k]))
    return out


@functools.lru_cache(maxsize=None)
def long_eobrun():
    """(e): a flat grey 1032 x 2048 picture, 33 024 blocks with no AC coefficient at all: every AC scan is one EOB run longer than the
    32 767 blocks one EOBn symbol can carry, so the writer has to cut it.  -> (progressive, baseline)"""
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.full((1032, 2048), 77, np.uint8)).save(f, 'JPEG', quality=75)
    base = f.getvalue()
    return jpeg_prog_writer.write(base, jpeg_prog_writer.script_default(1)), base


@functools.lru_cache(maxsize=None)
def reference(data, s=1):
    """jpeg_prog_ref.decode, computed once per file and scale and left unchanged."""
    out = jpeg_prog_ref.decode(data, s)
    out.setflags(write=False)
    return out


def refused():
    """name -> (file, the reason's word): one script for every property the parser refuses by name."""
    base = pillow_file(16, 16, 'noise', 95, '4:2:0')
    grey = pillow_file(16, 16, 'noise', 95, 'L')
    w = jpeg_prog_writer.write
    all_c = (0, 1, 2)
    ac = [((c,), 1, 63, 0, 0) for c in range(3)]
    good = w(base, jpeg_prog_writer.script_default(3))
    sof = good.index(b'\xff\xc2')
    out = {
        'sof6': (good[:sof] + b'\xff\xc6' + good[sof + 2:], 'progressive'),
        'ac_two_components': (w(base, [(all_c, 0, 0, 0, 0), ((1, 2), 1, 63, 0, 0), ((0,), 1, 63, 0, 0)]), 'ac_components'),
        'ac_before_dc': (w(base, [((0,), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]), 'ac_before_dc'),
        'first_scan_with_ah': (w(base, [(all_c, 0, 0, 1, 0)] + ac), 'first_ah'),
        'first_ac_scan_with_ah': (w(base, [(all_c, 0, 0, 0, 0), ((0,), 1, 63, 2, 1)] + ac), 'first_ah'),
        'refinement_skips_a_bit': (w(base, [(all_c, 0, 0, 0, 2), (all_c, 0, 0, 2, 0)] + ac), 'refinement'),
        'refinement_of_another_bit': (w(base, [(all_c, 0, 0, 0, 2), (all_c, 0, 0, 1, 0)] + ac), 'refinement'),
        'band_sent_twice': (w(base, [(all_c, 0, 0, 0, 0)] + ac + [((0,), 1, 5, 0, 0)]), 'refinement'),
        'band_at_two_bits': (w(base, [(all_c, 0, 0, 0, 0), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 0), ((0,), 1, 63, 1, 0)] + ac[1:]), 'refinement'),
        'last_scan_missing': (w(base, jpeg_prog_writer.script_default(3)[:-1]), 'incomplete'),
        'a_component_without_ac': (w(base, [(all_c, 0, 0, 0, 0)] + ac[:2]), 'incomplete'),
        'too_many_tables': (w(grey, [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)]), 'capacity'),
        'too_many_scans': (w(base, [(all_c, 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(3) for k in range(1, 64)], tables='shared'), 'capacity'),
    }
    return out


def damaged_for_the_card():
    """-> (good, {name: file}): a 40 x 56 4:2:0 file of libjpeg's default script with an interval per MCU row, cut in the middle of its
    sixth scan's bytes (the scans behind it are gone: an incomplete script, refused on the host), cut inside its last scan (every scan is
    there: damaged data), and with a byte of its first AC refinement scan replaced by one that keeps the byte count and makes no marker;
    and a whole file of that size whose script lacks its last scan.
    scripts/make_jpeg_prog_corpus.py takes each through the host program before the card sees it."""
    good = pillow_file(40, 56, 'noise', 95, '4:2:0', 'row1', progressive=True)
    scans = jpeg_prog_ref.parse(good)['scans']
    mid = scans[5]
    assert mid['ss'] > 0 and mid['ah'] > 0
    last = scans[-1]
    pos = (mid['start'] + mid['end']) // 2
    while good[pos - 1] == 0xFF or good[pos] == 0xFF or good[pos] ^ 0x5A == 0xFF:
        pos += 1
    assert pos < mid['end']
    short = jpeg_prog_writer.write(pillow_file(40, 56, 'noise', 95, '4:2:0'), jpeg_prog_writer.script_default(3)[:-1])
    return good, {'cut_mid_script': good[:pos], 'cut_last_scan': good[:(last['start'] + last['end']) // 2],
                  'replaced_in_refinement': good[:pos] + bytes([good[pos] ^ 0x5A]) + good[pos + 1:], 'incomplete_script': short}
