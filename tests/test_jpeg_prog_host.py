"""CPU: builds scripts/jpeg_prog_check.cpp -- jpd_parse_scans and the very statements jpeg_prog_entropy_k runs (csrc/jpeg_parse.h,
csrc/jpeg_dec_dev.h) -- with the address and undefined-behaviour sanitizers, as a stand-alone program with nothing preloaded, and runs
it over the corpus scripts/make_jpeg_prog_corpus.py writes: valid files of Pillow's and of the writer's scripts against
tests/jpeg_prog_ref.coefficients, two progressive files cut at every byte length, 1 500 seeded single-byte replacements in each, the
damaged files the GPU tests use, and one script for every property the parser refuses by name.  Skipped where no C++ compiler is present."""
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
    exe = str(tmp_path / 'jpeg_prog_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'jpeg_prog_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    corpus = str(tmp_path / 'corpus')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_jpeg_prog_corpus.py'), corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'valid files decoded to the expected coefficients' in r.stdout and '13 scripts refused by name' in r.stdout and 'ERROR' not in r.stderr
