"""GPU: JPEG slots of the ingest ring with the split entropy stage (FrameIngest(..., pixel_format='jpeg', jpeg_split=True); csrc/ingest.hip
hands the flag to csrc/jpeg_dec.hip).  What a consumer acquires is, bit for bit, what a ring made without the option gives for the same
files -- decoded straight into the slot, and through the staging buffer and the ring's crop_resize launch -- with the same statuses and
the same present(slot)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import pillow_file, reference  # noqa: E402

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
    """A marker-less file (split), a file with an interval per MCU row (not split), and a third stream that gets nothing."""
    return [pillow_file(H, W, 'noise', 95, '4:2:0', 'none', seed=10 * step), pillow_file(H, W, 'noise', 75, '4:2:2', 'row1', seed=10 * step + 1), None]


def _submit(ring, slot, data, shape):
    for z, d in enumerate(data):
        if d is not None:
            ring.put(slot, z, d)
    ring.submit(slot)
    got = _read(ring.ctx, ring.acquire(slot), shape)
    status, present = ring.status(slot).tolist(), ring.present(slot).tolist()
    ring.release(slot)
    return got, status, present


@pytest.mark.parametrize('flip,dst', [(False, (W, H)), (True, (40, 30))], ids=['straight-into-the-slot', 'flip-resize-through-staging'])
def test_a_split_ring_gives_the_default_rings_frames(flip, dst):
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    assert [jpeg_dec_ref.parse(f)['n_intervals'] for f in _files(0)[:2]] == [1, 6]
    assert len(_files(0)[0]) - jpeg_dec_ref.parse(_files(0)[0])['scan_offset'] > 128
    ring = FrameIngest(S, (W, H), dst, slots=2, flip=flip, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_split=True)
    plain = FrameIngest(S, (W, H), dst, slots=2, flip=flip, context=ring.ctx, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    assert ring.jpeg_split is True and plain.jpeg_split is False
    shape = (S, dst[1], dst[0], 3)
    for step in range(2):
        want, want_status, want_present = _submit(plain, step, _files(step), shape)
        got, status, present = _submit(ring, step, _files(step), shape)
        assert status == want_status == [0, 0, jpeg.ST_NO_FRAME]
        assert present == want_present == [1, 1, 0]
        np.testing.assert_array_equal(got[:2], want[:2])
        if not flip and dst == (W, H):
            np.testing.assert_array_equal(got[:2], np.stack([reference(d) for d in _files(step)[:2]]))
