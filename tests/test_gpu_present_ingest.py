"""GPU: a JPEG ingest ring drives the pipeline's presence mask.  FrameIngest.present(slot) is status(slot) == 0; a stream whose file is
missing or cut short is absent from that step, and its tracks and counts are those of a run that never saw those frames.  The cut file is
the one the host decode check (scripts/jpeg_decode_check.cpp) decodes first; nothing is looped or retried on the card."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'scripts'))

import jpeg_dec_ref  # noqa: E402
from jpeg_dec_cases import pillow_file, reference  # noqa: E402

pytestmark = pytest.mark.gpu

S, W, H, F = 3, 56, 40, 6                # 40 x 56: the size of the damaged files the host check has decoded


def _boxes(z, f):
    return [(float(4 + 3 * f + z), float(2 + 12 * k), 10.0, 12.0) for k in range(3)]


def test_ring_status_masks_the_step():
    import torch
    import make_jpeg_corpus
    from deepdish_amd import jpeg
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    _, damaged = make_jpeg_corpus.damaged_for_the_card()
    with pytest.raises(ValueError, match='corrupt'):
        jpeg_dec_ref.decode(damaged['cut'])
    files = [[pillow_file(H, W, 'scene', 90, '4:2:0', 'row1' if z else 'none', seed=10 * f + z) for z in range(S)] for f in range(F)]
    missing, cut = (1, 4), 2                                # steps on which stream 1 gets no file / the file cut short
    mp = MultiStreamPipeline(S, input_size=(W, H), run_detector=False, encoder_max_batch=64)
    ring = FrameIngest(S, (W, H), slots=2, context=mp.ctx, pixel_format='jpeg', jpeg_slot_bytes=S * W * H * 3)
    one = [MultiStreamPipeline(1, input_size=(W, H), run_detector=False, encoder_max_batch=64) for _ in range(S)]
    assert FrameIngest(S, (W, H), slots=2, context=mp.ctx).present(0).tolist() == [1] * S          # a raw ring: every stream, always
    for f in range(F):
        slot = f % 2
        per = [(_boxes(z, f), ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(S)]
        for z in range(S):
            if z == 1 and f in missing:
                continue
            ring.put(slot, z, damaged['cut'] if (z == 1 and f == cut) else files[f][z])
        ring.submit(slot)
        frames = ring.frames(slot)
        present = ring.present(slot)
        status = ring.status(slot)
        assert present.dtype == np.uint8 and present.tolist() == (status == 0).astype(int).tolist()
        assert status.tolist() == [0, jpeg.ST_NO_FRAME if f in missing else jpeg.ST_DATA if f == cut else 0, 0]
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
