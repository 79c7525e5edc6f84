"""GPU: 8-bit Bayer mosaics and monochrome frames through the stand-alone converter (csrc/bayer.hip, dd_raw8_to_bgr) against
tests/bayer_ref.py -- equality only.  Every call converts three frames into the middle of a sentinel-filled buffer that must stay intact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import bayer_ref  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = bayer_ref.PATTERNS
S = 3
LEAD = 64          # the output starts this far into a fresh allocation: 16-byte aligned, as a fresh source tensor is


def _takes_wide(W, pitch=0, frame_stride=0):
    """The host's choice (ddk::raw8_to_bgr) for 16-byte aligned base addresses: 16 pixels per lane when W, the pitch and the frame stride
    are multiples of 16, else a lane per pixel."""
    assert LEAD % 16 == 0
    return W % 16 == 0 and (pitch or W) % 16 == 0 and frame_stride % 16 == 0


def _convert(raw, H, W, layout, n, **kw):
    """raw (flat u8) -> BGR through raw8_to_bgr, written into the middle of a sentinel-filled buffer that must stay intact around it."""
    import torch
    from deepdish_amd.ingest import raw8_to_bgr
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    tail, nb = 256, n * H * W * 3
    buf = torch.full((LEAD + nb + tail,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    out = buf[LEAD:LEAD + nb].view(n, H, W, 3)
    src = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()                                      # the upload ran on torch's stream, the conversion runs on the context's
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    r = raw8_to_bgr(src, H, W, layout, out=out, context=ctx, **kw)
    assert r is out
    ctx.sync()
    host = buf.cpu().numpy()
    assert (host[:LEAD] == 0xA5).all() and (host[LEAD + nb:] == 0xA5).all(), 'bytes outside the frames were written'
    return host[LEAD:LEAD + nb].reshape(n, H, W, 3)


DENSE = [(3, 3), (4, 3), (3, 4), (5, 7), (18, 5), (70, 34), (16, 3), (32, 4), (640, 480)]
GRAY = [(1, 1), (17, 3), (16, 1), (640, 480)]


def test_dense_cases_cover_both_kernels():
    """(16, 3) is the smallest frame the wide kernel takes (one lane a row pair, both edge clamps in it; with S = 3 the frame stride 48 keeps
    every frame 16-byte aligned), (32, 4) puts two lanes in a row, so a halo byte crosses a lane boundary, and has one row pair that is
    all interior rows' neighbours; (640, 480) runs it over many workgroups.  The others can only take the narrow one.  Gray: (16, 1) and
    (640, 480) wide, (1, 1) and (17, 3) narrow."""
    wide = [c for c in DENSE if _takes_wide(c[0], 0, c[0] * c[1])]
    assert wide == [(16, 3), (32, 4), (640, 480)]
    assert [c for c in DENSE if c not in wide] == [(3, 3), (4, 3), (3, 4), (5, 7), (18, 5), (70, 34)]
    assert [c for c in GRAY if _takes_wide(c[0], 0, c[0] * c[1])] == [(16, 1), (640, 480)]
    assert not _takes_wide(14) and _takes_wide(16) and not _takes_wide(16, 30) and not _takes_wide(16, 32, 40)
    assert not _takes_wide(70, 84, 84 * 34 + 33) and _takes_wide(640, 672, 672 * 480 + 64)


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H', DENSE)
def test_converter_vs_ref(pattern, W, H):
    raw = np.random.default_rng(W * 1000 + H).integers(0, 256, (S, H, W), dtype=np.uint8)
    got = _convert(raw.reshape(-1), H, W, pattern, S)
    for z in range(S):
        np.testing.assert_array_equal(got[z], bayer_ref.bayer_to_bgr(raw[z], H, W, pattern))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H,pad,fs_extra,wide', [(70, 34, 14, 33, False), (640, 480, 32, 64, True)])
def test_converter_padded_surfaces(pattern, W, H, pad, fs_extra, wide):
    """pitch = W + pad with the next frame further away than dense: W + 14 with an odd frame stride takes the narrow kernel, 640 + 32 with
    16-byte multiples everywhere the wide one."""
    pitch = W + pad
    stride = pitch * H + fs_extra
    assert _takes_wide(W, pitch, stride) == wide
    raw = np.random.default_rng(11 + W).integers(0, 256, S * stride, dtype=np.uint8)
    got = _convert(raw, H, W, pattern, S, pitch=pitch, frame_stride=stride)
    for z in range(S):
        np.testing.assert_array_equal(got[z], bayer_ref.bayer_to_bgr(raw[z * stride:(z + 1) * stride], H, W, pattern, pitch))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H', [(32, 4), (70, 34)])
def test_extremes(pattern, W, H):
    """Bytes drawn only from {0, 1, 254, 255}: every sum meets its carry and rounding corners ((a + b + c + d + 2) >> 2 is not two nested
    rounded averages).  One wide shape, one narrow."""
    raw = np.random.default_rng(W + H).choice(np.array([0, 1, 254, 255], np.uint8), (S, H, W))
    got = _convert(raw.reshape(-1), H, W, pattern, S)
    for z in range(S):
        np.testing.assert_array_equal(got[z], bayer_ref.bayer_to_bgr(raw[z], H, W, pattern))


@pytest.mark.parametrize('W,H', GRAY)
def test_gray_vs_ref(W, H):
    raw = np.random.default_rng(W * 1000 + H).integers(0, 256, (S, H, W), dtype=np.uint8)
    got = _convert(raw.reshape(-1), H, W, 'gray', S)
    for z in range(S):
        np.testing.assert_array_equal(got[z], bayer_ref.gray_to_bgr(raw[z], H, W))


def test_gray_padded_surface():
    W, H, pitch = 17, 3, 23
    stride = pitch * H + 5
    raw = np.random.default_rng(17).integers(0, 256, S * stride, dtype=np.uint8)
    got = _convert(raw, H, W, 'gray', S, pitch=pitch, frame_stride=stride)
    for z in range(S):
        np.testing.assert_array_equal(got[z], bayer_ref.gray_to_bgr(raw[z * stride:(z + 1) * stride], H, W, pitch))


@pytest.mark.parametrize('layout', ['bayer_grbg', 'gray'])
def test_an_output_offset_past_2_to_the_31_bytes(layout):
    """Frame 2 400 of 640 x 480 is written 2.2e9 bytes into the output: both allocations are left uninitialised but for frames 0 and
    2 400 of the source and a guard behind the output; only those two frames are read back."""
    import torch
    from deepdish_amd.ingest import raw8_to_bgr
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    H, W, z = 480, 640, 2400
    fb = H * W
    assert z * fb * 3 > 2 ** 31
    frames = np.random.default_rng(31).integers(0, 256, (2, H, W), dtype=np.uint8)
    src = torch.empty((z + 1) * fb, dtype=torch.uint8, device='cuda')
    src[:fb] = torch.from_numpy(frames[0].reshape(-1)).cuda()
    src[z * fb:] = torch.from_numpy(frames[1].reshape(-1)).cuda()
    buf = torch.empty((z + 1) * fb * 3 + 256, dtype=torch.uint8, device='cuda')
    buf[(z + 1) * fb * 3:] = 0xA5
    torch.cuda.synchronize()
    out = buf[:(z + 1) * fb * 3].view(z + 1, H, W, 3)
    assert raw8_to_bgr(src, H, W, layout, out=out, context=ctx) is out
    ctx.sync()
    np.testing.assert_array_equal(out[0].cpu().numpy(), bayer_ref.raw8_to_bgr(frames[0], H, W, layout))
    np.testing.assert_array_equal(out[z].cpu().numpy(), bayer_ref.raw8_to_bgr(frames[1], H, W, layout))
    assert bool((buf[(z + 1) * fb * 3:] == 0xA5).all())


def test_python_refusals():
    import torch
    from deepdish_amd.ingest import raw8_to_bgr
    src = torch.zeros(16, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='rggb'):
        raw8_to_bgr(src, 4, 4, 'rggb')
    with pytest.raises(ValueError, match='2x4'):
        raw8_to_bgr(src, 4, 2, 'bayer_rggb')
    with pytest.raises(ValueError, match='src holds 16 bytes'):
        raw8_to_bgr(src, 5, 4, 'gray', out=torch.empty((1, 5, 4, 3), dtype=torch.uint8, device='cuda'))
    assert raw8_to_bgr(src, 4, 4, 'gray').shape == (1, 4, 4, 3)
