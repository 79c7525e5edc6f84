"""CPU: builds scripts/jpeg_plan_check.cpp -- the very call plan jpegdec_launch runs over the records before it queues anything
(csrc/jpeg_dec_plan.h jd_plan_call and its helpers) -- with the address and undefined-behaviour sanitizers, as a stand-alone program, and
runs it over records forged in memory: every path, scale and route, dead records between live ones, and every check that refuses a call,
each failing alone.  Every case must give the outcome recorded from the planning loop before it was taken out of jpegdec_launch: every
field the plan fills, the call's numbers, and for a refused call the error code and the message.  Skipped where no C++ compiler is present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_host_check_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'jpeg_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'jpeg_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr
    m = re.search(r'(\d+) plans, (\d+) differ from the recorded outcomes', r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 36 and int(m.group(2)) == 0
