"""CPU: builds scripts/jpeg_split_check.cpp -- the very span decoder and bit reader jpeg_split_entropy_k runs (csrc/jpeg_dec_dev.h), under
the kernel's rounds emulated on the host -- with the address and undefined-behaviour sanitizers, as a stand-alone program, and runs it over
the corpus scripts/make_jpeg_split_corpus.py writes: 320 valid marker-less files, two files cut at every byte length and 3 000 seeded
single-byte replacements.  At subsequences of 16, 32 and 128 bytes, with the lanes in three orders, every file must give the sequential
decoder's status and, where that is OK, its coefficients, within subsequences + 1 rounds.  Skipped where no C++ compiler is present."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_host_check_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'jpeg_split_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'jpeg_split_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    corpus = str(tmp_path / 'corpus')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_jpeg_split_corpus.py'), corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr
    m = re.search(r'(\d+) valid and (\d+) damaged files .* (\d+) split decodes agree with the sequential decoder: status 0 for (\d+), data (\d+)', r.stdout)
    assert m, r.stdout
    valid, damaged, runs, ok, data = (int(v) for v in m.groups())
    assert valid == 320 and damaged > 6000 and ok >= 9 * 300 and data > 0 and runs == ok + data
