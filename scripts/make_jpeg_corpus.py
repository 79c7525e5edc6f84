"""The corpus scripts/jpeg_decode_check.cpp reads: python scripts/make_jpeg_corpus.py DIR [--replacements N]

Pillow and tests/jpeg_ref.py write the files, with fixed seeds:
  - valid files of every accepted kind (4:2:0, 4:2:2, 4:4:4, greyscale; optimised tables; restart markers), each with NAME.coef, the raw
    int16 dump of tests/jpeg_dec_ref.coefficients;
  - a 16 x 16 and a 40 x 56 file truncated at every byte length;
  - N (default 2000) seeded single-byte replacements in each of the two, in the scan and in the header.
DIR/index.txt lists them.  test ids for the card (tests/test_gpu_jpeg_decode.py) come from `damaged_for_the_card`."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import jpeg_dec_ref  # noqa: E402
import jpeg_ref  # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (15, 31), (49, 7), (3, 5), (40, 56), (2, 17)]
SAMPLINGS = ['4:2:0', '4:2:2', '4:4:4', 'L']
RESTARTS = [{}, {'restart_marker_blocks': 1}, {'restart_marker_blocks': 3}, {'restart_marker_rows': 1}]


def picture(H, W, kind, seed=0):
    if kind == 'noise':
        return np.random.default_rng(H * 8209 + W * 17 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 7 + y * 3 + seed) % 256, (x * 2 + y * 5) % 256, (x + y) * 255 // max(1, H + W - 2)], axis=-1).astype(np.uint8)


def pillow_file(bgr, quality, sampling, optimize=False, **restart):
    from PIL import Image
    f = io.BytesIO()
    if sampling == 'L':
        Image.fromarray(np.ascontiguousarray(bgr[..., 1])).save(f, 'JPEG', quality=quality, optimize=optimize, **restart)
    else:
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(f, 'JPEG', quality=quality, subsampling=sampling, optimize=optimize, **restart)
    return f.getvalue()


def valid_files():
    k = 0
    for H, W in SIZES:
        for kind in ('noise', 'ramp'):
            for sampling in SAMPLINGS:
                q = (20, 95, 100)[k % 3]
                yield 'v%03d' % k, pillow_file(picture(H, W, kind), q, sampling, optimize=k % 5 == 0, **RESTARTS[k % 4])
                k += 1
    for H, W, q, r in ((33, 47, 95, 1), (40, 56, 50, 2), (16, 16, 100, 1)):
        yield 'v%03d' % k, jpeg_ref.encode(picture(H, W, 'noise', 7), q, r)
        k += 1


def victims():
    return [('a', pillow_file(picture(16, 16, 'noise'), 95, '4:2:0')),
            ('b', pillow_file(picture(40, 56, 'noise'), 95, '4:2:0', restart_marker_blocks=3))]


def damaged_for_the_card():
    """The three damaged files the GPU tests decode, each after this corpus has taken it through the host program: the 40 x 56 file cut
    at 60 % of its scan; with a byte in mid-scan replaced by 0xFF in front of a byte that makes a marker of it; with its second RST
    marker removed."""
    good = victims()[1][1]
    sos = jpeg_dec_ref.parse(good)['scan_offset']
    cut = good[:sos + (len(good) - sos) * 6 // 10]
    pos = sos + (len(good) - sos) // 2
    while good[pos - 1] == 0xFF or good[pos] == 0xFF or good[pos + 1] == 0 or 0xD0 <= good[pos + 1] <= 0xD7 or good[pos + 1] == 0xFF:
        pos += 1
    replaced = good[:pos] + b'\xff' + good[pos + 1:]
    i = good.index(b'\xff\xd1', sos)
    return good, {'cut': cut, 'replaced': replaced, 'rst_removed': good[:i] + good[i + 2:]}


def damaged_files(replacements):
    for name, data in damaged_for_the_card()[1].items():
        yield 'card_' + name, data
    for tag, good in victims():
        for n in range(len(good)):
            yield 't%s%05d' % (tag, n), good[:n]
        sos = jpeg_dec_ref.parse(good)['scan_offset']
        rng = np.random.default_rng(len(good))
        for i in range(replacements):
            pos = int(rng.integers(sos, len(good))) if i % 2 == 0 else int(rng.integers(0, sos))
            bad = bytearray(good)
            bad[pos] = int(rng.integers(0, 256))
            yield 'r%s%05d' % (tag, i), bytes(bad)


def write(directory, replacements=2000):
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, data in valid_files():
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        jpeg_dec_ref.coefficients(data).astype('<i2').tofile(os.path.join(directory, name + '.coef'))
        lines.append('valid ' + name)
    for name, data in damaged_files(replacements):
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('damaged ' + name)
    open(os.path.join(directory, 'index.txt'), 'w').write('\n'.join(lines) + '\n')
    return len(lines)


if __name__ == '__main__':
    n = int(sys.argv[sys.argv.index('--replacements') + 1]) if '--replacements' in sys.argv else 2000
    print('%d files' % write(sys.argv[1], n))
