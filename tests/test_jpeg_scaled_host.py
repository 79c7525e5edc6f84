"""CPU: builds scripts/jpeg_scaled_check.cpp -- the reduced transforms and the plane-size function the scaled kernels run
(csrc/jpeg_dec_dev.h: jpd_idct4, jpd_idct2, jpd_idct1, jpd_plane) -- with the address and undefined-behaviour sanitizers, as a stand-alone
program, and holds what it writes to tests/jpeg_scaled_ref.py, equal everywhere: random blocks of every magnitude, blocks without AC terms,
every coefficient at +-2047 under a quantiser of 255, the int16 limits, and blocks that are non-zero only in row or column 4, which the
4 x 4 transform must not read.  Skipped where no C++ compiler is present."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import jpeg_scaled_ref  # noqa: E402


def _blocks():
    """-> (coef i16 [k, 64], quant u16 [k, 64]) natural order."""
    rng = np.random.default_rng(18)
    coef, quant = [], []

    def add(c, q):
        coef.append(np.asarray(c, np.int16).reshape(64))
        quant.append(np.asarray(q, np.uint16).reshape(64))

    for k in range(600):                                            # what files hold: a few large low-frequency terms, sparse tails
        bound = (4, 32, 256, 2047)[k % 4]
        c = rng.integers(-bound, bound + 1, (8, 8))
        if k % 3:
            c[rng.random((8, 8)) < 0.7] = 0
        add(c, rng.integers(1, (16, 256)[k % 2], 64))
    for dc in (-2047, -1024, -1, 0, 1, 3, 4, 5, 1024, 2047):        # no AC term at all: libjpeg's short cuts must equal the full pass
        c = np.zeros((8, 8), np.int64)
        c[0, 0] = dc
        add(c, np.full(64, (1, 16, 255)[abs(dc) % 3]))
    for sign in (1, -1):                                            # the extremes: +-2047 * 255 in every term, alternating, one at a time
        add(np.full(64, sign * 2047), np.full(64, 255))
        add(sign * 2047 * (1 - 2 * (np.indices((8, 8)).sum(0) & 1)), np.full(64, 255))
        for i in (0, 1, 8, 9, 27, 63):
            c = np.zeros(64, np.int64)
            c[i] = sign * 2047
            add(c, np.full(64, 255))
        add(np.full(64, sign * 32767 if sign > 0 else -32768), np.full(64, 255))          # what a hostile file can hold
    for k in range(8):                                              # only row 4, only column 4, and both
        c = np.zeros((8, 8), np.int64)
        if k % 3 != 1:
            c[4, :] = rng.integers(-2047, 2048, 8)
        if k % 3 != 0:
            c[:, 4] = rng.integers(-2047, 2048, 8)
        add(c, rng.integers(1, 256, 64))
    return np.stack(coef), np.stack(quant)


QUERIES = [(h, w, hs, vs, hmax, vmax, s) for (h, w) in ((1, 1), (16, 5), (37, 53), (480, 640), (1080, 1920), (8192, 8192), (17, 8191))
           for (hs, vs, hmax, vmax) in ((1, 1, 1, 1), (2, 2, 2, 2), (1, 1, 2, 2), (2, 1, 2, 1), (1, 1, 2, 1)) for s in (1, 2, 4, 8)]


def test_reduced_transforms_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'jpeg_scaled_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'scripts', 'jpeg_scaled_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and 'sanitizer' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    coef, quant = _blocks()
    sizes = (4, 2, 1)
    rec = bytearray(np.int32(3 * len(coef)).tobytes())
    for n in sizes:
        for c, q in zip(coef, quant):
            rec += np.int32(n).tobytes() + c.astype('<i2').tobytes() + q.astype('<u2').tobytes()
    rec += np.int32(len(QUERIES)).tobytes() + np.asarray(QUERIES, '<i4').tobytes()
    src, dst = tmp_path / 'in.bin', tmp_path / 'out.bin'
    src.write_bytes(bytes(rec))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '%d blocks' % (3 * len(coef)) in r.stdout and 'ERROR' not in r.stderr
    got = np.frombuffer(dst.read_bytes(), np.uint8)
    at = 0
    for n in sizes:
        want = np.concatenate([jpeg_scaled_ref.idct_reduced(c[None], q.astype(np.int64), n) for c, q in zip(coef, quant)])
        have = got[at:at + want.size].reshape(want.shape)
        bad = np.nonzero((have != want).reshape(len(coef), -1).any(1))[0]
        assert bad.size == 0, 'the %d x %d transform differs from the ref in blocks %s' % (n, n, bad[:8].tolist())
        at += want.size
    # the 4 x 4 transform does not read term 4: the last eight blocks give what an all-zero block gives
    four = got[:16 * len(coef)].reshape(len(coef), 16)
    assert (four[-8:] == 128).all()
    planes = np.frombuffer(got[at:].tobytes(), '<i4').reshape(-1, 3)
    assert len(planes) == len(QUERIES)
    for (h, w, hs, vs, hmax, vmax, s), p in zip(QUERIES, planes):
        assert tuple(p) == jpeg_scaled_ref.plane_size(h, w, hs, vs, hmax, vmax, s), (h, w, hs, vs, hmax, vmax, s)
