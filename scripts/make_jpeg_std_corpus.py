"""The corpus scripts/jpeg_std_tables_check.cpp reads: python scripts/make_jpeg_std_corpus.py DIR [--replacements N]

Files without their DHT tables (tests/jpeg_std_cases.py: Pillow's files with the standard tables, stripped table by table), with fixed seeds:
  - every sampling x four sizes x (all, chroma only, luma only, DC0 only, AC0 + DC1), each with NAME.coef, the raw int16 dump of
    tests/jpeg_dec_ref.coefficients of the file it was stripped from: the default tables must decode to exactly those;
  - a 16 x 16 file without any table and a 40 x 56 file without its chroma tables, truncated at every byte length;
  - N (default 2000) seeded single-byte replacements in each of the two, in the scan and in the header.
DIR/index.txt lists them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import jpeg_dec_ref  # noqa: E402
from jpeg_std_cases import SAMPLINGS, SIZES, VARIANTS, standard_file, strip  # noqa: E402


def valid_files():
    k = 0
    for s in SAMPLINGS:
        for H, W in SIZES:
            for v in VARIANTS:
                whole = standard_file(H, W, s, 'noise' if k % 2 == 0 else 'ramp', ('none', 'mcu1', 'mcu3', 'row1')[k % 4])
                yield 'v%03d' % k, strip(whole, VARIANTS[v]), whole
                k += 1


def victims():
    return [('a', strip(standard_file(16, 16, '4:2:0'), VARIANTS['all'])), ('b', strip(standard_file(40, 56, '4:2:0', restart='mcu3'), VARIANTS['chroma']))]


def damaged_files(replacements):
    for tag, good in victims():
        for n in range(len(good)):
            yield 't%s%05d' % (tag, n), good[:n]
        sos = len(good) - jpeg_dec_ref.parse(standard_file(*((16, 16, '4:2:0') if tag == 'a' else (40, 56, '4:2:0', 'noise', 'mcu3'))))['scan_length']
        rng = np.random.default_rng(len(good))
        for i in range(replacements):
            pos = int(rng.integers(sos, len(good))) if i % 2 == 0 else int(rng.integers(0, sos))
            bad = bytearray(good)
            bad[pos] = int(rng.integers(0, 256))
            yield 'r%s%05d' % (tag, i), bytes(bad)


def write(directory, replacements=2000):
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, data, whole in valid_files():
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        jpeg_dec_ref.coefficients(whole).astype('<i2').tofile(os.path.join(directory, name + '.coef'))
        lines.append('valid ' + name)
    for name, data in damaged_files(replacements):
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('damaged ' + name)
    open(os.path.join(directory, 'index.txt'), 'w').write('\n'.join(lines) + '\n')
    return len(lines)


if __name__ == '__main__':
    n = int(sys.argv[sys.argv.index('--replacements') + 1]) if '--replacements' in sys.argv else 2000
    print('%d files' % write(sys.argv[1], n))
