"""The corpus scripts/jpeg_split_check.cpp reads: python scripts/make_jpeg_split_corpus.py DIR [--replacements N]

Pillow writes the files, with fixed seeds, all without restart markers -- one entropy-coded segment each, what jpeg_split_entropy_k takes:
  - valid files: four samplings x noise / ramp x quality 1, 50, 95, 100 at 16 x 16, 17 x 33, 49 x 7, 40 x 56 and 96 x 64, with the standard
    and with optimised tables (noise at quality 100 has blocks without EOB that are longer than two 16-byte subsequences, and hardly ever
    falls into step);
  - a 16 x 16 and a 40 x 56 file cut at every byte length;
  - N (default 3000) seeded single-byte replacements over the two, three in four of them in the scan.
DIR/index.txt lists them.  The damaged files the card sees (tests/test_gpu_jpeg_split.py) come from `damaged_for_the_card`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import pillow_file  # noqa: E402

SIZES = [(16, 16), (17, 33), (49, 7), (40, 56), (96, 64)]
SAMPLINGS = ['4:2:0', '4:2:2', '4:4:4', 'L']
QUALITIES = [1, 50, 95, 100]


def valid_files():
    k = 0
    for H, W in SIZES:
        for kind in ('noise', 'ramp'):
            for sampling in SAMPLINGS:
                for q in QUALITIES:
                    for optimize in (False, True):
                        yield 'v%03d' % k, pillow_file(H, W, kind, q, sampling, 'none', optimize)
                        k += 1


def victims():
    return [('a', pillow_file(16, 16, 'noise', 95, '4:2:0')), ('b', pillow_file(40, 56, 'noise', 95, '4:2:0'))]


def damaged_for_the_card():
    """The two damaged files the GPU test decodes, each after this corpus has taken it through the host program: the marker-less 40 x 56
    file cut at 60 % of its scan, and with a byte in mid-scan replaced by 0xFF in front of a byte that makes a marker of it, so that the
    data ends there."""
    good = victims()[1][1]
    sos = jpeg_dec_ref.parse(good)['scan_offset']
    cut = good[:sos + (len(good) - sos) * 6 // 10]
    pos = sos + (len(good) - sos) // 2
    while good[pos - 1] == 0xFF or good[pos] == 0xFF or good[pos + 1] == 0 or 0xD0 <= good[pos + 1] <= 0xD7 or good[pos + 1] == 0xFF:
        pos += 1
    return good, {'cut': cut, 'replaced': good[:pos] + b'\xff' + good[pos + 1:]}


def damaged_files(replacements):
    for name, data in damaged_for_the_card()[1].items():
        yield 'card_' + name, data
    for v, (tag, good) in enumerate(victims()):
        for n in range(len(good)):
            yield 't%s%05d' % (tag, n), good[:n]
        sos = jpeg_dec_ref.parse(good)['scan_offset']
        rng = np.random.default_rng(len(good))
        for i in range(v, replacements, 2):
            pos = int(rng.integers(sos, len(good))) if i % 4 else int(rng.integers(0, sos))
            bad = bytearray(good)
            bad[pos] = int(rng.integers(0, 256))
            yield 'r%s%05d' % (tag, i), bytes(bad)


def write(directory, replacements=3000):
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, data in valid_files():
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('valid ' + name)
    for name, data in damaged_files(replacements):
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('damaged ' + name)
    open(os.path.join(directory, 'index.txt'), 'w').write('\n'.join(lines) + '\n')
    return len(lines)


if __name__ == '__main__':
    n = int(sys.argv[sys.argv.index('--replacements') + 1]) if '--replacements' in sys.argv else 3000
    print('%d files' % write(sys.argv[1], n))
