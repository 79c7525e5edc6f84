"""GPU: JPEG slots of the ingest ring (csrc/ingest.hip, csrc/jpeg_dec.hip).  What a consumer acquires is, bit for bit, what a BGR ring gives
when it is fed tests/jpeg_dec_ref.decode's pixels through the same crop_resize launch; every stream carries a status, and a stream
without a frame, with a file of another size or refused costs the others nothing.  BGR and NV12 rings of the same process behave as
before."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from jpeg_dec_cases import own_file, pillow_file, reference  # noqa: E402

pytestmark = pytest.mark.gpu

S, W, H = 3, 48, 32
E_CAPACITY = -4
ARENA = S * (W * H * 3 + 1024)            # noise at quality 95 is larger than the default arena's eighth of the raw bytes


def _read(ctx, addr, shape):
    """Device bytes at `addr` -> numpy (after the context's stream has drained)."""
    import torch
    ctx.sync()
    out = torch.empty(shape, dtype=torch.uint8, device=f'cuda:{ctx.device}')
    hip = ctypes.CDLL('libamdhip64.so')
    rc = hip.hipMemcpy(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(addr), ctypes.c_size_t(int(np.prod(shape))), 3)      # device -> device
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _files(step):
    """Streams that differ in sampling, tables and restart interval, and from step to step."""
    return [pillow_file(H, W, 'noise', 95, '4:2:0', 'row1', seed=10 * step), pillow_file(H, W, 'ramp', 50, '4:4:4', 'none', True, seed=10 * step + 1),
            own_file(H, W, 'noise', 75, 1, seed=10 * step + 2)]


@pytest.mark.parametrize('flip,dst', [(False, None), (True, (24, 24))], ids=['plain', 'flip-resize'])
def test_ring_equals_a_bgr_ring_fed_with_the_reference(flip, dst):
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    out_shape = (S, (dst or (W, H))[1], (dst or (W, H))[0], 3)
    ring = FrameIngest(S, (W, H), dst, slots=2, flip=flip, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    raw = FrameIngest(S, (W, H), dst, slots=2, flip=flip, context=ring.ctx)
    with pytest.raises(ValueError, match='put'):
        ring.host(0)
    want = []
    for step in range(2):
        for z, data in enumerate(_files(step)):
            raw.host(step)[z] = reference(data)
        raw.submit(step)
        want.append(_read(raw.ctx, raw.acquire(step), out_shape))
        raw.release(step)
    # slot 0 is submitted and held; slot 1 is filled, submitted and acquired meanwhile
    for z, data in enumerate(_files(0)):
        ring.put(0, z, data)
    ring.submit(0)
    first = ring.acquire(0)
    for z, data in reversed(list(enumerate(_files(1)))):
        ring.put(1, z, data)
    ring.submit(1)
    got1 = _read(ring.ctx, ring.acquire(1), out_shape)
    got0 = _read(ring.ctx, first, out_shape)
    assert ring.status(0).tolist() == [0, 0, 0] and ring.status(1).tolist() == [0, 0, 0]
    np.testing.assert_array_equal(got0, want[0])
    np.testing.assert_array_equal(got1, want[1])
    if not flip:
        np.testing.assert_array_equal(got0, np.stack([reference(d) for d in _files(0)]))
    ring.release(0)
    ring.release(1)
    # the slot again: stream 1 gets no file, stream 2 one of another size; stream 0 is what it would have been
    ring.put(0, 0, _files(1)[0])
    ring.put(0, 2, pillow_file(32, 32, 'noise', 95, '4:2:0'))
    ring.submit(0)
    got = _read(ring.ctx, ring.acquire(0), out_shape)
    assert ring.status(0).tolist() == [0, jpeg.ST_NO_FRAME, jpeg.ST_SIZE]
    np.testing.assert_array_equal(got[0], want[1][0])
    ring.release(0)
    assert ring.frames(0).shape == out_shape


def test_a_refused_file_and_a_submit_without_a_put():
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    ring = FrameIngest(S, (W, H), slots=2, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    files = _files(0)
    ring.put(0, 0, files[0])
    ring.put(0, 1, pillow_file(H, W, 'noise', 95, '4:2:0', progressive=True))
    ring.put(0, 2, files[2])
    ring.put(0, 2, files[1])                              # a second put for a stream replaces the first
    ring.submit(0)
    got = _read(ring.ctx, ring.acquire(0), (S, H, W, 3))
    assert ring.status(0).tolist() == [0, jpeg.ST_HEADER, 0]
    np.testing.assert_array_equal(got[0], reference(files[0]))
    np.testing.assert_array_equal(got[2], reference(files[1]))
    ring.release(0)
    ring.submit(1)
    ring.acquire(1)
    assert ring.status(1).tolist() == [jpeg.ST_NO_FRAME] * S
    ring.release(1)


def test_an_arena_too_small():
    from deepdish_amd._lib import DeepDishHipError, lib
    from deepdish_amd.ingest import FrameIngest
    files = _files(0)
    ring = FrameIngest(S, (W, H), slots=1, pixel_format='jpeg', jpeg_slot_bytes=((len(files[0]) + 63) & ~63) + len(files[1]) - 1)
    ring.put(0, 0, files[0])
    with pytest.raises(DeepDishHipError, match=r'\(-4\)'):
        ring.put(0, 1, files[1])
    assert b'dd_ingest_jpeg_put' in lib().dd_last_error()
    assert FrameIngest(S, (W, H), slots=1, pixel_format='jpeg').jpeg_slot_bytes == S * W * H * 3 // 8


def test_bgr_and_nv12_rings_of_the_same_process_are_unchanged():
    import yuv_ref
    from deepdish_amd.ingest import FrameIngest
    jring = FrameIngest(S, (W, H), slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    jring.put(0, 0, _files(0)[0])
    jring.submit(0)
    rng = np.random.default_rng(5)
    bgr = FrameIngest(S, (W, H), slots=1, context=jring.ctx)
    frames = rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    bgr.host(0)[...] = frames
    bgr.submit(0)
    np.testing.assert_array_equal(_read(bgr.ctx, bgr.acquire(0), (S, H, W, 3)), frames)
    nv = FrameIngest(S, (W, H), slots=1, context=jring.ctx, pixel_format='nv12')
    yuv = rng.integers(0, 256, (S, H * 3 // 2, W), dtype=np.uint8)
    nv.host(0)[...] = yuv
    nv.submit(0)
    np.testing.assert_array_equal(_read(nv.ctx, nv.acquire(0), (S, H, W, 3)), np.stack([yuv_ref.yuv420_to_bgr(y, H, W, 'nv12') for y in yuv]))
    from deepdish_amd._lib import DeepDishHipError
    with pytest.raises(DeepDishHipError, match='JPEG'):
        bgr.status(0)
    with pytest.raises(DeepDishHipError, match='JPEG'):
        bgr.put(0, 0, _files(0)[0])


PIPE_S, PIPE_W, PIPE_H = 2, 128, 96


def _boxes(z, f):
    return [(float(22 + 6 * f + 3 * z), float(8 + 28 * k), 14.0, 24.0) for k in range(3)]


def test_ring_feeds_the_pipeline():
    """MultiStreamPipeline.step on ring.frames(slot) of a JPEG ring: the track tables of the same pixels uploaded raw."""
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    F = 4
    files = [[pillow_file(PIPE_H, PIPE_W, 'scene', 90, '4:2:0', 'row1' if z else 'none', seed=10 * f + z) for z in range(PIPE_S)] for f in range(F)]
    tables = []
    for mode in ('raw', 'ring'):
        mp = MultiStreamPipeline(PIPE_S, input_size=(PIPE_W, PIPE_H), run_detector=False)
        ring = FrameIngest(PIPE_S, (PIPE_W, PIPE_H), slots=2, context=mp.ctx, pixel_format='jpeg', jpeg_slot_bytes=PIPE_S * PIPE_W * PIPE_H) if mode == 'ring' else None
        for f in range(F):
            per = [(_boxes(z, f), ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(PIPE_S)]
            if ring is None:
                mp.step(torch.from_numpy(np.stack([reference(d) for d in files[f]])).cuda(), mp.pack_injected(per))
            else:
                for z in range(PIPE_S):
                    ring.put(f % 2, z, files[f][z])
                ring.submit(f % 2)
                mp.step(ring.frames(f % 2), mp.pack_injected(per))
                ring.release(f % 2)
                assert ring.status(f % 2).tolist() == [0, 0]
        tables.append([mp.tracker(z).table() for z in range(PIPE_S)])
    for z in range(PIPE_S):
        assert len(tables[0][z][0]) > 0
        np.testing.assert_array_equal(tables[0][z][0], tables[1][z][0])
        np.testing.assert_array_equal(tables[0][z][1], tables[1][z][1])
