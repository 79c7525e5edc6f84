"""GPU: JPEG slots of the ingest ring taking progressive files (FrameIngest(..., pixel_format='jpeg', jpeg_progressive=True);
csrc/ingest.hip, csrc/jpeg_dec.hip).  What a consumer acquires is tests/jpeg_prog_ref.decode's frame where no transform is asked, and
otherwise, bit for bit, what a BGR ring of the decoded size gives when it is fed that frame through the same crop_resize launch -- the
ring's existing oracle.  'auto' is Pillow's draft rule; a ring made without the option refuses such files as before; and a progressive
ring drives a pipeline's presence mask through present(slot).  The damaged file is one scripts/jpeg_prog_check.cpp decodes first."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_prog_ref  # noqa: E402
from jpeg_dec_cases import own_file, pillow_file  # noqa: E402
from jpeg_prog_cases import damaged_for_the_card, reference, written  # noqa: E402

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
    """A Pillow progressive file with an interval per MCU row, a scripted 4:2:2 file (Al = 3 refined bit by bit) and a baseline file of
    this build's own encoder; they differ from step to step."""
    return [pillow_file(H, W, 'noise', 95, '4:2:0', 'row1', seed=10 * step, progressive=True), written(H, W, '4:2:2', 'deep', 3 * step, quality=50 + 45 * step)[0],
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


def test_straight_into_the_slot():
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    assert ['scans' in jpeg_prog_ref.parse(f) for f in _files(0)] == [True, True, False]
    ring = FrameIngest(S, (W, H), slots=2, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_progressive=True)
    assert ring.jpeg_progressive is True and ring.jpeg_scale == 1
    shape = (S, H, W, 3)
    for step in range(2):
        got, status = _submit(ring, step, _files(step), shape)
        assert status == [0, 0, 0]
        np.testing.assert_array_equal(got, np.stack([reference(d) for d in _files(step)]))
    # slot 0 again: stream 1 gets no file and keeps the frame it had; stream 2 gets a progressive file of another size
    before = np.stack([reference(d) for d in _files(0)])
    got, status = _submit(ring, 0, [_files(1)[0], None, pillow_file(24, 32, 'noise', 95, '4:2:0', progressive=True)], shape, skip=(1,))
    assert status == [0, jpeg.ST_NO_FRAME, jpeg.ST_SIZE]
    assert ring.present(0).tolist() == [1, 0, 0]
    np.testing.assert_array_equal(got[0], reference(_files(1)[0]))
    np.testing.assert_array_equal(got[1], before[1])
    np.testing.assert_array_equal(got[2], before[2])


@pytest.mark.parametrize('flip,dst,scale', [(False, (40, 30), 1), (True, (64, 48), 1), (True, (20, 15), 2), (False, (32, 24), 'auto')], ids=['resize', 'flip', 'half-flip-resize', 'auto'])
def test_the_rings_own_transform_and_scales(flip, dst, scale):
    """Decoded at full size, or at the scale asked for or picked by the draft rule, then through the staging buffer and the ring's
    crop_resize launch where flip or resize is asked: what a 'bgr' ring of the decoded size gives for the ref's frames."""
    from deepdish_amd.ingest import FrameIngest
    ring = FrameIngest(S, (W, H), dst, slots=2, flip=flip, pixel_format='jpeg', jpeg_slot_bytes=ARENA, jpeg_scale=scale, jpeg_progressive=True)
    s = ring.jpeg_scale
    assert s == (2 if scale == 'auto' else scale)
    jw, jh = -(-W // s), -(-H // s)
    shape = (S, dst[1], dst[0], 3)
    raw = FrameIngest(S, (jw, jh), dst, slots=2, flip=flip, context=ring.ctx, pixel_format='bgr')
    for step in range(2):
        for z, d in enumerate(_files(step)):
            raw.host(step)[z] = reference(d, s)
        raw.submit(step)
        want = _read(raw.ctx, raw.acquire(step), shape)
        raw.release(step)
        if (jw, jh) == dst and not flip:
            np.testing.assert_array_equal(want, np.stack([reference(d, s) for d in _files(step)]))
        got, status = _submit(ring, step, _files(step), shape)
        assert status == [0, 0, 0]
        np.testing.assert_array_equal(got, want)


def test_a_ring_without_the_option_refuses_as_before():
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    ring = FrameIngest(S, (W, H), slots=1, pixel_format='jpeg', jpeg_slot_bytes=ARENA)
    assert ring.jpeg_progressive is False
    got, status = _submit(ring, 0, _files(0), (S, H, W, 3))
    assert status == [jpeg.ST_HEADER, jpeg.ST_HEADER, 0] and ring.present(0).tolist() == [0, 0, 1]
    np.testing.assert_array_equal(got[2], reference(_files(0)[2]))
    for fmt in ('nv12', 'bgr'):
        with pytest.raises(ValueError, match='jpeg_progressive'):
            FrameIngest(S, (W, H), slots=1, pixel_format=fmt, jpeg_progressive=True)


def test_a_progressive_ring_masks_the_pipelines_step():
    """present(slot) follows from the status as before: a stream whose progressive file is missing, cut inside its last scan (ST_DATA) or
    cut in mid-script (ST_HEADER) is absent from that step, and its tracks and counts are those of a run that never saw those frames."""
    import torch
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    PW, PH, F = 56, 40, 6
    _, damaged = damaged_for_the_card()
    files = [[pillow_file(PH, PW, 'scene', 90, ('4:2:0', '4:2:2', '4:4:4')[z], 'row1' if z else 'none', seed=10 * f + z, progressive=True) for z in range(S)] for f in range(F)]
    bad = {1: None, 2: damaged['cut_last_scan'], 4: damaged['cut_mid_script']}          # step -> what stream 1 gets
    want_status = {1: jpeg.ST_NO_FRAME, 2: jpeg.ST_DATA, 4: jpeg.ST_HEADER}
    mp = MultiStreamPipeline(S, input_size=(PW, PH), run_detector=False, encoder_max_batch=64)
    ring = FrameIngest(S, (PW, PH), slots=2, context=mp.ctx, pixel_format='jpeg', jpeg_slot_bytes=S * PW * PH * 3, jpeg_progressive=True)
    one = [MultiStreamPipeline(1, input_size=(PW, PH), run_detector=False, encoder_max_batch=64) for _ in range(S)]
    for f in range(F):
        slot = f % 2
        per = [([(float(4 + 3 * f + z), float(2 + 12 * k), 10.0, 12.0) for k in range(3)], ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(S)]
        for z in range(S):
            data = bad[f] if (z == 1 and f in bad) else files[f][z]
            if data is not None:
                ring.put(slot, z, data)
        ring.submit(slot)
        frames, present, status = ring.frames(slot), ring.present(slot), ring.status(slot)
        assert status.tolist() == [0, want_status.get(f, 0), 0] and present.tolist() == (status == 0).astype(int).tolist()
        mp.step(frames, mp.pack_injected(per), present=present)
        ring.release(slot)
        for z in range(S):
            if present[z]:
                one[z].step(torch.from_numpy(reference(files[f][z])[None].copy()).cuda(), one[z].pack_injected([per[z]]))
    assert mp.frames_seen().tolist() == [F, F - 3, F]
    for z in range(S):
        (ia, ma), (ib, mb) = mp.tracker(z).table(), one[z].tracker(0).table()
        assert len(ia) > 0
        np.testing.assert_array_equal(ia, ib, err_msg='stream %d' % z)
        np.testing.assert_array_equal(ma, mb, err_msg='stream %d' % z)
        np.testing.assert_array_equal(mp.counts()[z], one[z].counts()[0])
