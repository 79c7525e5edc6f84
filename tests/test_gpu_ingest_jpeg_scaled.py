"""GPU: JPEG slots of the ingest ring decoding at 1/2, 1/4 or 1/8 scale (csrc/ingest.hip, csrc/jpeg_dec.hip).  What a consumer acquires
is tests/jpeg_scaled_ref.decode's frame where the scaled size is the ring's output size, and otherwise, bit for bit, what a BGR ring of
the scaled size gives when it is fed that frame through the same crop_resize launch.  src_size stays what a file must state; a stream
without a file leaves its frame alone; 'auto' is Pillow's draft rule."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_scaled_ref  # noqa: E402
from jpeg_dec_cases import own_file, pillow_file  # noqa: E402
from jpeg_scaled_cases import reference  # noqa: E402

pytestmark = pytest.mark.gpu

S, W, H = 3, 64, 48
ARENA = S * (W * H * 3 + 1024)


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
    return [pillow_file(H, W, 'noise', 95, '4:2:0', 'row1', seed=10 * step), pillow_file(H, W, 'ramp', 50, '4:2:2', 'none', True, seed=10 * step + 1),
            own_file(H, W, 'noise', 75, 1, seed=10 * step + 2)]


def _submit(ring, slot, data, shape, skip=()):
    for z, d in enumerate(data):
        if z not in skip:
            ring.put(slot, z, d)
    ring.submit(slot)
    got = _read(ring.ctx, ring.acquire(slot), shape)
    status = ring.status(slot).tolist()
    ring.release(slot)
    return got, status


def test_half_scale_straight_into_the_slot():
    """64 x 48 files, jpeg_scale=2, dst_size=(32, 24): no resize launch, the slot holds the decoder's frames."""
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    ring = FrameIngest(S, (W, H), (32, 24), slots=2, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale=2)
    assert ring.jpeg_scale == 2
    shape = (S, 24, 32, 3)
    for step in range(2):
        got, status = _submit(ring, step, _files(step), shape)
        assert status == [0, 0, 0]
        np.testing.assert_array_equal(got, np.stack([reference(d, 2) for d in _files(step)]))
    # slot 0 again: stream 1 gets no file and keeps the frame it had; stream 2 gets a file of the scaled size, which is not the size
    # the ring's files must state
    before = np.stack([reference(d, 2) for d in _files(0)])
    got, status = _submit(ring, 0, [_files(1)[0], None, pillow_file(24, 32, 'noise', 95, '4:2:0')], shape, skip=(1,))
    assert status == [0, jpeg.ST_NO_FRAME, jpeg.ST_SIZE]
    np.testing.assert_array_equal(got[0], reference(_files(1)[0], 2))
    np.testing.assert_array_equal(got[1], before[1])
    np.testing.assert_array_equal(got[2], before[2])
    assert ring.frames(0).shape == shape


@pytest.mark.parametrize('flip,dst', [(False, (20, 15)), (True, (20, 15)), (True, (32, 24))], ids=['resize', 'flip-resize', 'flip'])
def test_half_scale_then_the_rings_own_transform(flip, dst):
    """The decoder's frames go through the staging buffer and the ring's crop_resize launch: what a 'bgr' ring of 32 x 24 gives for the
    ref's frames."""
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    shape = (S, dst[1], dst[0], 3)
    ring = FrameIngest(S, (W, H), dst, slots=2, flip=flip, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale=2)
    raw = FrameIngest(S, (32, 24), dst, slots=2, flip=flip, context=ring.ctx, pixel_format='bgr')
    want = []
    for step in range(2):
        for z, d in enumerate(_files(step)):
            raw.host(step)[z] = reference(d, 2)
        raw.submit(step)
        want.append(_read(raw.ctx, raw.acquire(step), shape))
        raw.release(step)
    assert not np.array_equal(want[0], want[1])
    for step in range(2):
        got, status = _submit(ring, step, _files(step), shape)
        assert status == [0, 0, 0]
        np.testing.assert_array_equal(got, want[step])
    # stream 1 without a file: its staged frame is left alone, so the slot shows that frame (step 1's) again
    got, status = _submit(ring, 0, _files(0), shape, skip=(1,))
    assert status == [0, jpeg.ST_NO_FRAME, 0]
    np.testing.assert_array_equal(got[0], want[0][0])
    np.testing.assert_array_equal(got[1], want[1][1])
    np.testing.assert_array_equal(got[2], want[0][2])


@pytest.mark.parametrize('dst,scale', [((20, 15), 2), ((16, 12), 4), ((8, 6), 8), ((9, 6), 4), ((64, 48), 1), ((100, 80), 1)], ids=lambda v: str(v).replace(' ', ''))
def test_auto_is_the_draft_rule(dst, scale):
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    assert jpeg_scaled_ref.draft_scale((W, H), dst) == scale and jpeg.draft_scale((W, H), dst) == scale
    ring = FrameIngest(S, (W, H), dst, slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale='auto')
    assert ring.jpeg_scale == scale
    if (-(-W // scale), -(-H // scale)) == dst:                  # decoded straight into the slot: the ref's frames at the scale 'auto' picked
        got, status = _submit(ring, 0, _files(0), (S, dst[1], dst[0], 3))
        assert status == [0, 0, 0]
        np.testing.assert_array_equal(got, np.stack([reference(d, scale) for d in _files(0)]))


def test_only_a_jpeg_ring_takes_a_scale():
    from deepdish_amd.ingest import FrameIngest
    for fmt in ('nv12', 'bgr', 'yuy2'):
        with pytest.raises(ValueError, match='jpeg_scale'):
            FrameIngest(S, (W, H), slots=1, pixel_format=fmt, jpeg_scale=2)
    with pytest.raises(ValueError, match='jpeg_scale'):
        FrameIngest(S, (W, H), slots=1, pixel_format='nv12', jpeg_scale='auto')
    with pytest.raises(ValueError, match='jpeg_scale 3'):
        FrameIngest(S, (W, H), slots=1, pixel_format='jpeg', jpeg_scale=3)
    nv = FrameIngest(S, (W, H), slots=1, pixel_format='nv12')              # the default is accepted everywhere
    assert nv.jpeg_scale == 1
