"""CPU: builds scripts/jpeg_std_tables_check.cpp -- the header parser with DD_JPEGDEC_STD_TABLES and the very interval loop the kernels run
(csrc/jpeg_parse.h, csrc/jpeg_dec_dev.h) -- with the address and undefined-behaviour sanitizers, as a stand-alone program, and runs it over
the corpus scripts/make_jpeg_std_corpus.py writes: every sampling and size without all, the chroma, the luma, the DC0 or the AC0 + DC1
tables against tests/jpeg_dec_ref.coefficients of the untouched file, two stripped files cut at every byte length, and 2 000 seeded
single-byte replacements in each.  Nothing is loaded into Python.  Skipped where no C++ compiler is present."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'jpeg_std_tables_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'jpeg_std_tables_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    corpus = str(tmp_path / 'corpus')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_jpeg_std_corpus.py'), corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'stripped files decoded to the expected coefficients' in r.stdout and 'ERROR' not in r.stderr
