"""GPU: JPEG slots of the ingest ring that take files of any size up to src_size (FrameIngest(..., pixel_format='jpeg', jpeg_any_size=True);
csrc/ingest.hip builds one crop box per stream from its record).  A ring of 8 streams, at most 64 x 48, dst 20 x 12: what a consumer
acquires for stream z is, bit for bit, what an ordinary ring built for z's file size with the same jpeg_scale, flip and dst gives for the
same file -- the pattern of tests/test_gpu_ingest_jpeg_split.py.  source_sizes, status and present are as the files imply; a camera that
changes its mode between two submits is followed; the slot masks a MultiStreamPipeline's step; and with jpeg_std_tables=True a file without
its DHT tables gives the frame of the file it was stripped from."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from jpeg_dec_cases import pillow_file, reference  # noqa: E402
from jpeg_std_cases import VARIANTS, standard_file, strip  # noqa: E402

pytestmark = pytest.mark.gpu

S, MAX_W, MAX_H, DST = 8, 64, 48, (20, 12)
ARENA = S * (MAX_W * MAX_H * 3 + 1024)
# (width, height) per stream: the largest accepted, twice dst, dst itself, an odd size, a sliver, one pixel, one too large, nothing
SIZES = [(64, 48), (40, 24), (20, 12), (17, 9), (3, 40), (1, 1), (65, 48), None]
SAMPLINGS = ['4:2:0', '4:2:2', '4:4:4', 'L', '4:2:0', '4:2:2', '4:2:0', '4:4:4']


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


def _files(step, sizes=SIZES):
    return [None if wh is None else pillow_file(wh[1], wh[0], 'noise' if z % 2 else 'ramp', 90, SAMPLINGS[z], ('none', 'row1')[z % 2], seed=10 * step + z)
            for z, wh in enumerate(sizes)]


def _submit(ring, slot, data, n=S):
    for z, d in enumerate(data):
        if d is not None:
            ring.put(slot, z, d)
    ring.submit(slot)
    got = _read(ring.ctx, ring.acquire(slot), (n, DST[1], DST[0], 3))
    status, present = ring.status(slot).tolist(), ring.present(slot).tolist()
    ring.release(slot)
    return got, status, present


def _ordinary(ctx, wh, data, flip, scale):
    """What a ring built for this one file's size gives for it."""
    from deepdish_amd.ingest import FrameIngest
    one = FrameIngest(1, wh, DST, slots=1, flip=flip, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale=scale)
    got, status, present = _submit(one, 0, [data], 1)
    assert status == [0] and present == [1]
    return got[0], one.jpeg_scale


def _check(ring, slot, sizes, step, flip, scale):
    from deepdish_amd import jpeg
    data = _files(step, sizes)
    got, status, present = _submit(ring, slot, data)
    ok = [wh is not None and wh[0] <= MAX_W and wh[1] <= MAX_H for wh in sizes]
    assert status == [0 if k else (jpeg.ST_NO_FRAME if wh is None else jpeg.ST_SIZE) for k, wh in zip(ok, sizes)]
    assert present == [int(k) for k in ok]
    sizes_got = ring.source_sizes(slot).tolist()
    for z, wh in enumerate(sizes):
        if wh is None:
            assert sizes_got[z] == [0, 0, 0]
            continue
        s = jpeg.draft_scale(wh, DST) if scale == 'auto' else scale
        assert sizes_got[z] == [wh[0], wh[1], s], z
        if ok[z]:
            want, s_one = _ordinary(ring.ctx, wh, data[z], flip, scale)
            assert s_one == s
            np.testing.assert_array_equal(got[z], want, err_msg='stream %d, %d x %d' % (z, wh[0], wh[1]))
    return got, data


@pytest.mark.parametrize('flip,scale', [(False, 'auto'), (True, 'auto'), (False, 2), (False, 1)], ids=['auto', 'auto-flip', 'scale2', 'scale1'])
def test_every_stream_equals_a_ring_of_its_own_size(flip, scale):
    """At scale 1 the 40 x 24 file takes crop_resize's 2 x INTER_AREA shortcut; with 'auto' it decodes at 1/2 straight to dst's size."""
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    ring = FrameIngest(S, (MAX_W, MAX_H), DST, slots=2, flip=flip, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_any_size=True, jpeg_scale=scale)
    assert ring.jpeg_any_size is True and ring.jpeg_scale_auto is (scale == 'auto') and ring.jpeg_scale == (1 if scale == 'auto' else scale)
    got, data = _check(ring, 0, SIZES, 0, flip, scale)
    if scale == 'auto' and not flip:
        assert jpeg.draft_scale((40, 24), DST) == 2 and jpeg.draft_scale((64, 48), DST) == 2 and jpeg.draft_scale((20, 12), DST) == 1
        np.testing.assert_array_equal(got[2], reference(data[2]))                      # a file of dst's own size arrives as it was decoded
    # the camera of stream 0 changes its mode, the missing one appears, the one that was too large goes missing: the same slot again, then the other
    changed = [(17, 9)] + SIZES[1:6] + [None, (33, 16)]
    _check(ring, 0, changed, 1, flip, scale)
    _check(ring, 1, SIZES, 2, flip, scale)


def test_refusals_and_the_default_ring():
    from deepdish_amd import jpeg
    from deepdish_amd._lib import DeepDishHipError
    from deepdish_amd.ingest import FrameIngest
    for fmt in ('nv12', 'bgr'):
        with pytest.raises(ValueError, match='jpeg_any_size'):
            FrameIngest(S, (MAX_W, MAX_H), slots=1, pixel_format=fmt, jpeg_any_size=True)
        with pytest.raises(ValueError, match='jpeg_std_tables'):
            FrameIngest(S, (MAX_W, MAX_H), slots=1, pixel_format=fmt, jpeg_std_tables=True)
    plain = FrameIngest(2, (MAX_W, MAX_H), DST, slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale='auto')
    assert plain.jpeg_any_size is False and plain.jpeg_scale_auto is False and plain.jpeg_scale == 2          # 'auto' without any_size: one scale from src_size
    got, status, present = _submit(plain, 0, _files(0)[:2], 2)
    assert status == [0, jpeg.ST_SIZE] and present == [1, 0]                                # the old size test
    with pytest.raises(DeepDishHipError, match=r'\(-3\)'):
        plain.source_sizes(0)


def test_the_slot_masks_a_pipelines_step():
    """Two steps of the ring's frames with present=ring.present(slot): the absent streams never advance, the present ones end with the
    tracks and counts of single pipelines fed the same frames."""
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    mp = MultiStreamPipeline(S, input_size=DST, run_detector=False, encoder_max_batch=64)
    one = [MultiStreamPipeline(1, input_size=DST, run_detector=False, encoder_max_batch=64) for _ in range(S)]
    ring = FrameIngest(S, (MAX_W, MAX_H), DST, slots=2, context=mp.ctx, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_any_size=True, jpeg_scale='auto')
    for f in range(2):
        per = [([(float(1 + 6 * k + f), 1.0, 5.0, 10.0) for k in range(3)], ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(S)]
        for z, d in enumerate(_files(f)):
            if d is not None:
                ring.put(f, z, d)
        ring.submit(f)
        frames, present = ring.frames(f), ring.present(f)
        assert present.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
        host = _read(ring.ctx, frames.data_ptr(), frames.shape)
        mp.step(frames, mp.pack_injected(per), present=present)
        ring.release(f)
        for z in range(S):
            if present[z]:
                one[z].step(torch.from_numpy(host[z][None].copy()).cuda(), one[z].pack_injected([per[z]]))
    assert mp.frames_seen().tolist() == [2, 2, 2, 2, 2, 2, 0, 0]
    assert mp.present_stats()['masked_steps'] == 2 and mp.present_stats()['streams_stepped'] == 12
    for z in range(6):
        (ia, ma), (ib, mb) = mp.tracker(z).table(), one[z].tracker(0).table()
        assert len(ia) > 0
        np.testing.assert_array_equal(ia, ib, err_msg='stream %d' % z)
        np.testing.assert_array_equal(ma, mb, err_msg='stream %d' % z)
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
    for z in (6, 7):
        assert len(mp.tracker(z).table()[0]) == 0


def test_std_tables_on_the_ring():
    """A file without its DHT tables in stream 1: with jpeg_std_tables=True its frame is that of the file it was stripped from, on an
    any-size ring and on an ordinary one; without the flag it is ST_HEADER and its neighbours are untouched by that."""
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    whole = [standard_file(24, 40, '4:2:0', seed=1), standard_file(24, 40, '4:2:2', seed=2), standard_file(24, 40, 'L', seed=3)]
    bare = [whole[0], strip(whole[1], VARIANTS['all']), strip(whole[2], VARIANTS['ac0_dc1'])]
    assert len(bare[1]) < len(whole[1]) and len(bare[2]) < len(whole[2])
    kw = dict(slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    n = len(whole)
    for any_size, src in ((True, (MAX_W, MAX_H)), (False, (40, 24))):
        ring = FrameIngest(n, src, DST, jpeg_any_size=any_size, jpeg_std_tables=True, **kw)
        want, status, _ = _submit(ring, 0, whole, n)
        assert status == [0, 0, 0]
        got, status, present = _submit(ring, 0, bare, n)
        assert status == [0, 0, 0] and present == [1, 1, 1]
        np.testing.assert_array_equal(got, want)
        off = FrameIngest(n, src, DST, context=ring.ctx, jpeg_any_size=any_size, **kw)
        got, status, present = _submit(off, 0, bare, n)
        assert status == [0, jpeg.ST_HEADER, jpeg.ST_HEADER] and present == [1, 0, 0]
        np.testing.assert_array_equal(got[0], want[0])
    # straight into the slot, no resize: the reference's pixels
    ring = FrameIngest(n, (40, 24), slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_std_tables=True)
    for z, d in enumerate(bare):
        ring.put(0, z, d)
    ring.submit(0)
    got = _read(ring.ctx, ring.acquire(0), (n, 24, 40, 3))
    assert ring.status(0).tolist() == [0, 0, 0]
    np.testing.assert_array_equal(got, np.stack([reference(d) for d in whole]))
