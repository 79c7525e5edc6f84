"""CPU: builds scripts/snapshot_check.cpp -- the writer, parser and validator of the stream-snapshot blob (csrc/snapshot_fmt.h, no HIP) --
with the address and undefined-behaviour sanitizers, as a stand-alone program, and runs it: blobs written from plain structs (0 tracks;
galleries of 0, 1, 31, 32, 33, 64 and 65 rows; a wrapped budget ring; deleted tracks with paths; with and without background; three
entries) must parse and write back to the same bytes; two blobs cut at every byte length and 3 000 seeded single-byte replacements must
each be refused or validate to a state whose every index is in range, and never be read out of bounds.  Skipped where no C++ compiler
is present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snapshot_blob_check_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'snapshot_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'snapshot_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr
    m = re.search(r'(\d+) blobs round-trip; (\d+) cut blobs refused, (\d+) accepted; (\d+) replacements refused, (\d+) accepted; '
                  r'(\d+) of 1000 in the header refused, (\d+) of 1000 in the galleries accepted', r.stdout)
    assert m, r.stdout
    blobs, cut_refused, cut_accepted, rep_refused, rep_accepted, head_refused, gallery_accepted = (int(v) for v in m.groups())
    assert blobs == 6
    assert cut_accepted == 0 and cut_refused > 3000           # every proper prefix of a blob is refused
    assert rep_refused + rep_accepted == 3000
    # the validator has teeth -- every byte of the header and the entry table is checked -- and is no checksum: a gallery value is data
    # the pipeline may hold, accepted with every index still in range
    assert head_refused == 1000 and gallery_accepted == 1000
