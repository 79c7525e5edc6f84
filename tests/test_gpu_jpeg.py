"""GPU: the JPEG encoder (csrc/jpeg.hip) from the kernel to the pipelines, held to tests/jpeg_ref.py -- whole files, equality everywhere.

A workgroup codes one restart interval and lays its bits into an 8 KiB window of LDS, 256 threads wide: the shapes below cover one and
several windows per interval, one and several intervals per workgroup row count, both kernel paths, frames smaller than an MCU and
frames that are no multiple of 8 or 16 either way.  Outputs land in sentinel-guarded slots."""
import functools
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_ref  # noqa: E402
from jpeg_cases import CASES, QUALITIES, frame, rows  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
E_CAPACITY = -4
# beyond the shared list: three windows in an LDS-resident interval; two MCU rows per interval with a shorter last one; the streaming
# path at its smallest shapes either way, and with several intervals of several windows
GPU_CASES = CASES + [(32, 1000, 100, 1, 'noise'), (72, 256, 95, 2, 'noise'), (16, 2049, 95, 1, 'noise'), (2064, 16, 95, 0, 'smooth'),
                     (40, 2070, 95, 1, 'noise')]


@functools.lru_cache(maxsize=None)
def _reference(H, W, kind, seed, quality, restart_rows):
    return jpeg_ref.encode(frame(H, W, kind, seed), quality, restart_rows)


def _three(H, W, kind):
    """Three different frames led by the case's own."""
    if kind in ('noise', 'smooth'):
        return [(kind, 0), (kind, 1), (kind, 2)]
    return [(kind, 0), ('noise', 1), ('smooth', 2)]


@functools.lru_cache(maxsize=None)
def _encoder(H, W, quality, restart_rows):
    from deepdish_amd.jpeg import JpegEncoder
    return JpegEncoder(H, W, quality=quality, restart_rows=restart_rows)


def _encode(enc, frames, cap=None):
    """dd_jpeg_encode into sentinel-filled slots [n][cap] between two guards -> (return code, files or None, lengths).  Behind every file
    its slot must still hold the sentinel, and a file that does not fit must leave its whole slot untouched."""
    import torch
    from deepdish_amd._lib import lib, P
    frames = np.ascontiguousarray(frames)
    n = len(frames)
    cap = enc.default_capacity if cap is None else cap
    pitch = cap
    buf = torch.full((GUARD + n * pitch + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    lengths = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    dev = enc.ctx.to_device(frames)
    torch.cuda.synchronize()
    rc = lib().dd_jpeg_encode(enc._h, P(dev.data_ptr()), n, P(buf.data_ptr() + GUARD), pitch, P(lengths.data_ptr()), None)
    host, lens = enc.ctx.to_host(buf), enc.ctx.to_host(lengths)
    assert (host[:GUARD] == SENTINEL).all(), 'bytes before the first slot were written'
    assert (host[GUARD + n * pitch:] == SENTINEL).all(), 'bytes behind the last slot were written'
    slots = host[GUARD:GUARD + n * pitch].reshape(n, pitch)
    files = []
    for i in range(n):
        used = int(lens[i]) if lens[i] <= pitch else 0
        assert (slots[i, used:] == SENTINEL).all(), 'frame %d: bytes behind its file were written' % i
        files.append(slots[i, :used].tobytes() if lens[i] <= pitch else None)
    return rc, files, lens


@pytest.mark.parametrize('case', GPU_CASES, ids=lambda c: '%dx%d-q%d-r%d-%s' % c)
def test_kernel_equals_reference_alone_and_in_a_batch(case):
    H, W, q, r, kind = case
    r = rows(H, r)
    enc = _encoder(H, W, q, r)
    three = _three(H, W, kind)
    want = [_reference(H, W, k, s, q, r) for k, s in three]
    assert len(set(want)) == 3
    rc, files, lens = _encode(enc, [frame(H, W, k, s) for k, s in three])
    assert rc == 0 and [int(v) for v in lens] == [len(w) for w in want]
    for i in range(3):
        assert files[i] == want[i], 'frame %d of the batch' % i
        rc1, alone, _ = _encode(enc, [frame(H, W, *three[i])])
        assert rc1 == 0 and alone[0] == want[i], 'frame %d alone' % i


def test_lengths_that_differ_widely_inside_one_launch():
    H, W = 96, 128
    kinds = [('noise', 0), ('zero', 0), ('smooth', 0)]
    want = [_reference(H, W, k, s, 95, 1) for k, s in kinds]
    assert len(want[0]) > 8 * len(want[1])
    rc, files, _ = _encode(_encoder(H, W, 95, 1), [frame(H, W, k, s) for k, s in kinds])
    assert rc == 0 and files == want


def test_every_quality():
    """Every scaled quantisation table: the reciprocal division against the reference's true division."""
    bgr = frame(32, 48, 'noise', 5)
    for q in QUALITIES:
        rc, files, _ = _encode(_encoder(32, 48, q, 1), [bgr])
        assert rc == 0 and files[0] == jpeg_ref.encode(bgr, q, 1), 'quality %d' % q


def test_two_frames_of_480x640():
    H, W = 480, 640
    kinds = [('smooth', 0), ('smooth', 1)]
    rc, files, _ = _encode(_encoder(H, W, 95, 1), [frame(H, W, k, s) for k, s in kinds])
    assert rc == 0
    for i, (k, s) in enumerate(kinds):
        assert files[i] == _reference(H, W, k, s, 95, 1), 'frame %d' % i


@pytest.mark.parametrize('H,W,r,path', [(1, 1, 1, 0), (16, 2048, 1, 0), (16, 2049, 1, 1), (2064, 16, 129, 1)])
def test_each_plan_path_at_its_smallest_shape(H, W, r, path):
    from deepdish_amd import jpeg
    assert jpeg.plan(H, W, r) == path
    enc = _encoder(H, W, 95, r)
    assert enc.path == path
    bgr = frame(H, W, 'noise', 3)
    rc, files, _ = _encode(enc, [bgr])
    assert rc == 0 and files[0] == jpeg_ref.encode(bgr, 95, r)


def test_capacity_contract():
    """A slot smaller than one of three files: DD_E_CAPACITY, all three lengths true, the two that fit intact, and not a byte outside
    (_encode checks every guard; the file that does not fit leaves its slot untouched)."""
    H, W = 96, 128
    kinds = [('smooth', 0), ('noise', 0), ('zero', 0)]
    want = [_reference(H, W, k, s, 95, 1) for k, s in kinds]
    cap = len(want[0]) + 100
    assert len(want[1]) > cap and len(want[2]) < cap
    enc = _encoder(H, W, 95, 1)
    rc, files, lens = _encode(enc, [frame(H, W, k, s) for k, s in kinds], cap=cap)
    assert rc == E_CAPACITY
    assert [int(v) for v in lens] == [len(w) for w in want]
    assert files[0] == want[0] and files[2] == want[2] and files[1] is None
    from deepdish_amd._lib import lib
    assert b'dd_jpeg_encode' in lib().dd_last_error() and b'frame 1' in lib().dd_last_error()


def test_encode_to_host_retries_the_frame_that_overflows():
    H, W = 96, 128
    enc = _encoder(H, W, 95, 1)
    kinds = [('smooth', 0), ('noise', 0), ('zero', 0)]
    dev = enc.ctx.to_device(np.stack([frame(H, W, k, s) for k, s in kinds]))
    want = [_reference(H, W, k, s, 95, 1) for k, s in kinds]
    assert enc.encode_to_host(dev) == want
    keep = enc.default_capacity
    try:
        enc.default_capacity = len(want[0]) + 10
        assert enc.encode_to_host(dev) == want
    finally:
        enc.default_capacity = keep
    out, lengths = enc.encode(dev)
    assert tuple(out.shape) == (3, H * W * 3 + 1024) and [int(v) for v in enc.ctx.to_host(lengths)] == [len(w) for w in want]
    assert enc.ctx.to_host(out)[1, :len(want[1])].tobytes() == want[1]
    from deepdish_amd._lib import DeepDishHipError
    with pytest.raises(DeepDishHipError, match='frame 1 is %d bytes' % len(want[1])):
        enc.encode(dev, capacity=len(want[0]) + 10)


def test_a_file_decodes():
    Image = pytest.importorskip('PIL.Image')
    H, W = 50, 70
    bgr = frame(H, W, 'smooth')
    rc, files, _ = _encode(_encoder(H, W, 95, 1), [bgr])
    im = Image.open(io.BytesIO(files[0]))
    im.load()
    assert im.size == (W, H) and im.mode == 'RGB'
    assert np.abs(np.asarray(im).astype(int)[..., ::-1] - bgr).mean() < 8


# ------------------------------------------------------------------ pipelines
PIPE_S, PIPE_W, PIPE_H = 2, 128, 96


def _boxes(z, f):
    return [(float(22 + 6 * f + 3 * z), float(8 + 28 * k), 14.0, 24.0) for k in range(3)]


def test_render_jpeg_equals_the_reference_of_render():
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    mp = MultiStreamPipeline(PIPE_S, input_size=(PIPE_W, PIPE_H), run_detector=False)
    hps = [HotPath(input_size=(PIPE_W, PIPE_H), run_detector=False) for _ in range(PIPE_S)]
    for f in range(4):
        frames = np.stack([frame(PIPE_H, PIPE_W, 'noise', 10 * f + z) for z in range(PIPE_S)])
        dev = ctx.to_device(frames)
        per = [(_boxes(z, f), ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(PIPE_S)]
        mp.step(dev, mp.pack_injected(per))
        for z, hp in enumerate(hps):
            hp.step(dev[z], injected=per[z])
    rendered = ctx.to_host(mp.render(dev))
    assert (rendered != frames).any()
    files = mp.render_jpeg(dev)
    assert files == [jpeg_ref.encode(rendered[z], 95, 1) for z in range(PIPE_S)]
    assert mp.render_jpeg(dev, streams=[1], annotation='id', quality=60) == [jpeg_ref.encode(ctx.to_host(mp.render(dev, streams=[1], annotation='id'))[0], 60, 1)]
    assert len(mp._jpeg_encoders) == 2 and mp.render_jpeg(dev) == files and len(mp._jpeg_encoders) == 2
    for z, hp in enumerate(hps):
        one = hp.render_jpeg(dev[z])
        assert isinstance(one, bytes) and one == jpeg_ref.encode(ctx.to_host(hp.render(dev[z]))[0], 95, 1)
        assert hp.render_jpeg(dev[z], annotation='none', quality=30) == jpeg_ref.encode(ctx.to_host(hp.render(dev[z], annotation='none'))[0], 30, 1)
