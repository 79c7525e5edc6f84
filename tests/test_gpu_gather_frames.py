"""GPU: dd_gather_frames (csrc/gather.hip, frames_gather_k) against numpy indexing -- equality.  Frame sizes that take the 16-byte, the
dword and the byte path (by their size, and by a base that is off by one byte), n = 0, 1 and all, the bytes around the destination
untouched, and a source frame that starts past 2^31 bytes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A


def _gather(src_t, src_off, n_src, fb, idx, dst_t, dst_off):
    from deepdish_amd._lib import lib
    from deepdish_amd.runtime import default_context
    ix = np.ascontiguousarray(idx, dtype=np.int32)
    torch.cuda.synchronize()                 # the tensors were filled on torch's stream, the gather runs on the context's
    return lib().dd_gather_frames(default_context().handle, ctypes.c_void_p(src_t.data_ptr() + src_off), n_src, fb,
                                  ix.ctypes.data_as(ctypes.c_void_p), len(ix), ctypes.c_void_p(dst_t.data_ptr() + dst_off), None)


@pytest.mark.parametrize('fb', [3, 100, 105, 768, 921600])           # 100: a multiple of 4 and not of 16 -- the dword path at any dword base
@pytest.mark.parametrize('shift', [(0, 0), (1, 0), (0, 1), (1, 1), (4, 4)], ids=['aligned', 'src+1', 'dst+1', 'both+1', 'both+4'])
def test_gather_equals_numpy_indexing(fb, shift):
    S = 5
    rng = np.random.default_rng(fb + 7 * shift[0] + 13 * shift[1])
    src = rng.integers(0, 256, (S, fb), dtype=np.uint8)
    src_t = torch.zeros(S * fb + 16, dtype=torch.uint8, device='cuda')
    src_t[shift[0]:shift[0] + S * fb] = torch.from_numpy(src.reshape(-1)).cuda()
    for idx in ([], [0], [4], [1, 3], [0, 2, 3, 4], list(range(S))):
        dst_t = torch.full((GUARD + S * fb + GUARD + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert _gather(src_t, shift[0], S, fb, idx, dst_t, GUARD + shift[1]) == 0
        torch.cuda.synchronize()
        got = dst_t.cpu().numpy()
        a, b = GUARD + shift[1], GUARD + shift[1] + len(idx) * fb
        np.testing.assert_array_equal(got[a:b].reshape(len(idx), fb), src[idx], err_msg='idx %r' % (idx,))
        assert (got[:a] == SENTINEL).all() and (got[b:] == SENTINEL).all(), 'bytes outside the %d gathered frames were written' % len(idx)


def test_bad_lists_are_refused_on_the_host():
    from deepdish_amd._lib import lib
    t = torch.zeros(4 * 16, dtype=torch.uint8, device='cuda')
    d = torch.zeros(4 * 16, dtype=torch.uint8, device='cuda')
    for idx in ([1, 1], [2, 1], [0, 4], [-1, 2], [0, 1, 2, 3, 3]):
        assert _gather(t, 0, 4, 16, idx, d, 0) == -1, idx
        assert b'dd_gather_frames' in lib().dd_last_error()
    assert _gather(t, 0, 4, 0, [0], d, 0) == -1


def test_a_source_offset_past_2_to_the_31_bytes():
    """Stream 2 400 of 640 x 480 frames starts 2.2e9 bytes into the batch: the allocation is left uninitialised, only that frame is written."""
    fb, z = 640 * 480 * 3, 2400
    assert z * fb > 2 ** 31
    src_t = torch.empty((z + 1) * fb, dtype=torch.uint8, device='cuda')
    frame = torch.from_numpy(np.random.default_rng(3).integers(0, 256, fb, dtype=np.uint8)).cuda()
    src_t[z * fb:] = frame
    first = src_t[:fb].clone()
    dst_t = torch.full((2 * fb + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    assert _gather(src_t, 0, z + 1, fb, [0, z], dst_t, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst_t[fb:2 * fb], frame) and torch.equal(dst_t[:fb], first)
    assert bool((dst_t[2 * fb:] == SENTINEL).all())
