"""CPU: builds scripts/gate_plan_check.cpp -- the motion gate's index arithmetic as csrc/pipeline.hip runs it (csrc/host_phases.h:
plan_skip, gate_streams, GateStats, pair_counts, feature_row_table) -- with the address and undefined-behaviour sanitizers, as a
stand-alone program, and runs it over a few thousand seeded sequences of presence lists, counts and thresholds, S = 1 .. 9.  dl, the row
offsets, the store of retained rows and the statistics must equal a direct restatement per stream.  Skipped where no C++ compiler is present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_plan_host_check_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'gate_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'gate_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr
    m = re.search(r'(\d+) sequences, (\d+) steps \((\d+) without a stream, (\d+) with every stream gated, (\d+) with none\), (\d+) gated stream-steps, '
                  r'(\d+) checks, (\d+) differ', r.stdout)
    assert m, r.stdout
    seqs, steps, empty, all_gated, none_gated, gated, checks, differ = (int(v) for v in m.groups())
    assert seqs >= 2000 and steps >= 4 * seqs and empty > 0 and all_gated > 0 and none_gated > 0 and gated > 0
    assert checks > 20 * steps and differ == 0
