"""The corpus scripts/jpeg_prog_check.cpp reads: python scripts/make_jpeg_prog_corpus.py DIR [--replacements N]

Pillow and tests/jpeg_prog_writer.py write the files, with fixed seeds (tests/jpeg_prog_cases.py):
  - valid progressive files: Pillow's own (libjpeg's default script) of every sampling and restart layout at the sizes where a scan of one
    component walks another grid than the MCUs, the writer's scripts (a) .. (d), the long EOB run (e), and two baseline files; each with
    NAME.coef, the raw int16 dump of tests/jpeg_prog_ref.coefficients;
  - the damaged files the GPU tests decode, a 16 x 16 and a 40 x 56 progressive file cut at every byte length, and N (default 1500) seeded
    single-byte replacements in each of the two, in the scans and in the headers between them;
  - one file for every property the parser refuses by name, with the reason's number.
DIR/index.txt lists them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import jpeg_prog_cases  # noqa: E402
import jpeg_prog_ref  # noqa: E402
from jpeg_dec_cases import pillow_file  # noqa: E402

REASON = {'progressive': 2, 'ac_components': 13, 'ac_before_dc': 14, 'first_ah': 15, 'refinement': 16, 'incomplete': 17, 'capacity': 18}


def valid_files():
    k = 0
    for H, W in ((8, 8), (16, 5), (3, 40), (37, 53), (17, 9)):
        for data in jpeg_prog_cases.pillow_grid(H, W):
            yield 'p%03d' % k, data
            k += 1
    for H, W in ((16, 5), (37, 53)):
        for data, _ in jpeg_prog_cases.writer_grid(H, W):
            yield 'w%03d' % k, data
            k += 1
    yield 'eobrun', jpeg_prog_cases.long_eobrun()[0]
    yield 'base0', pillow_file(37, 53, 'noise', 95, '4:2:0', 'mcu3')
    yield 'base1', pillow_file(16, 16, 'ramp', 50, 'L')


def victims():
    return [('a', pillow_file(16, 16, 'noise', 95, '4:2:0', progressive=True)), ('b', jpeg_prog_cases.damaged_for_the_card()[0])]


def damaged_files(replacements):
    for name, data in jpeg_prog_cases.damaged_for_the_card()[1].items():
        yield 'card_' + name, data
    for tag, good in victims():
        for n in range(len(good)):
            yield 't%s%05d' % (tag, n), good[:n]
        rng = np.random.default_rng(len(good))
        for i in range(replacements):
            bad = bytearray(good)
            bad[int(rng.integers(0, len(good)))] = int(rng.integers(0, 256))
            yield 'r%s%05d' % (tag, i), bytes(bad)


def write(directory, replacements=1500):
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, data in valid_files():
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        jpeg_prog_ref.coefficients(data).astype('<i2').tofile(os.path.join(directory, name + '.coef'))
        lines.append('valid ' + name)
    for name, data in damaged_files(replacements):
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('damaged ' + name)
    for name, (data, word) in jpeg_prog_cases.refused().items():
        open(os.path.join(directory, name + '.jpg'), 'wb').write(data)
        lines.append('refused %s %d' % (name, REASON[word]))
    open(os.path.join(directory, 'index.txt'), 'w').write('\n'.join(lines) + '\n')
    return len(lines)


if __name__ == '__main__':
    n = int(sys.argv[sys.argv.index('--replacements') + 1]) if '--replacements' in sys.argv else 1500
    print('%d files' % write(sys.argv[1], n))
