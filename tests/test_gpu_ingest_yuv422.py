"""GPU: packed 4:2:2 (YUY2 / UYVY) frames through the converter (csrc/yuv.hip) and the ingest ring, against tests/yuv422_ref.py --
equality only.  The ring's flip + resize is held to the oracle's restatement of cv2 INTER_LINEAR applied to the converted frame (OpenCV
itself is absent: unpinned), once fused (one launch) and once, in a fresh child process with DD_INGEST_YUV_FUSED=0, as convert + resize.

Run as a script (`python tests/test_gpu_ingest_yuv422.py out.npz`) this file is that child: it pushes every ring case through a
FrameIngest and saves what came out."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import yuv_ref  # noqa: E402
import yuv422_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = yuv422_ref.ORDERS
S = 3
# the geometries of test_gpu_ingest_yuv.py, plus one with an odd source height (4:2:2 has no vertical sub-sampling)
RING_GEOMETRIES = [((1280, 720), (640, 480), False), ((1280, 960), (640, 480), True), ((480, 360), (640, 480), True),
                   ((640, 480), (640, 480), False), ((640, 480), (640, 480), True), ((70, 34), (30, 22), True),
                   ((70, 33), (30, 22), True)]
RING_CASES = [(order,) + g for order in ORDERS for g in RING_GEOMETRIES]


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


def _ring_input(i):
    _, src, _, _ = RING_CASES[i]
    return np.random.default_rng(422 + i).integers(0, 256, (S, src[1], src[0], 2), dtype=np.uint8)


def _run_ring(i):
    from deepdish_amd.ingest import FrameIngest
    order, src, dst, flip = RING_CASES[i]
    ing = FrameIngest(S, src, dst, slots=2, flip=flip, pixel_format=order)
    ing.host(1)[...] = _ring_input(i)
    ing.submit(1)
    got = _read(ing.ctx, ing.acquire(1), (S, dst[1], dst[0], 3))
    ing.release(1)
    return got


# ------------------------------------------------------------------ converter vs yuv422_ref
LEAD = 64          # the output starts this far into a fresh allocation: 16-byte aligned, as a fresh source tensor is


def _takes_wide(W, pitch=0, frame_stride=0):
    """The host's choice (ddk::yuv422_to_bgr) for 16-byte aligned base addresses: 16 pixels per lane when W, the pitch and the frame
    stride are multiples of 16, else a lane per macropixel."""
    assert LEAD % 16 == 0
    return W % 16 == 0 and (pitch or 2 * W) % 16 == 0 and frame_stride % 16 == 0


def _convert(raw, H, W, order, n, **kw):
    """raw (flat u8) -> BGR through yuv422_to_bgr, written into the middle of a sentinel-filled buffer that must stay intact around it."""
    import torch
    from deepdish_amd.ingest import yuv422_to_bgr
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    tail, nb = 256, n * H * W * 3
    buf = torch.full((LEAD + nb + tail,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    out = buf[LEAD:LEAD + nb].view(n, H, W, 3)
    src = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()                                      # the upload ran on torch's stream, the conversion runs on the context's
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    r = yuv422_to_bgr(src, H, W, order, out=out, context=ctx, **kw)
    assert r is out
    ctx.sync()
    host = buf.cpu().numpy()
    assert (host[:LEAD] == 0xA5).all() and (host[LEAD + nb:] == 0xA5).all(), 'bytes outside the frames were written'
    return host[LEAD:LEAD + nb].reshape(n, H, W, 3)


DENSE = [(2, 1), (18, 3), (70, 34), (640, 480), (16, 1)]


def test_dense_cases_cover_both_kernels():
    """(16, 1) is the smallest frame the wide kernel takes (one lane, one row; with S = 3 the frame stride 32 keeps every frame 16-byte
    aligned) and (640, 480) runs it over many workgroups; (2, 1), (18, 3) and (70, 34) can only take the narrow one."""
    wide = [c for c in DENSE if _takes_wide(c[0], 0, 2 * c[0] * c[1])]
    assert wide == [(640, 480), (16, 1)]
    assert [c for c in DENSE if c not in wide] == [(2, 1), (18, 3), (70, 34)]
    assert not _takes_wide(14) and _takes_wide(16) and not _takes_wide(16, 34) and not _takes_wide(16, 48, 40)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('W,H', DENSE)
def test_converter_vs_ref(order, W, H):
    """Random bytes, dense frames: (2, 1) one macropixel and an odd height, (18, 3) the narrow kernel with an odd row count, (70, 34) the
    narrow kernel over more than one workgroup, (640, 480) the wide kernel, (16, 1) the smallest frame that takes it."""
    raw = np.random.default_rng(W * 1000 + H).integers(0, 256, (S, H, W, 2), dtype=np.uint8)
    got = _convert(raw.reshape(-1), H, W, order, S)
    for z in range(S):
        np.testing.assert_array_equal(got[z], yuv422_ref.yuv422_to_bgr(raw[z], H, W, order))


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('W,H,pad,fs_extra,wide', [(70, 34, 14, 33, False), (640, 480, 32, 64, True)])
def test_converter_padded_surfaces(order, W, H, pad, fs_extra, wide):
    """pitch = 2 W + pad with the next frame further away than dense: padded surfaces.  2 W + 14 with an odd frame stride takes the
    narrow kernel, 1280 + 32 with 16-byte multiples everywhere the wide one."""
    pitch = 2 * W + pad
    stride = pitch * H + fs_extra
    assert _takes_wide(W, pitch, stride) == wide
    raw = np.random.default_rng(11 + W).integers(0, 256, S * stride, dtype=np.uint8)
    got = _convert(raw, H, W, order, S, pitch=pitch, frame_stride=stride)
    for z in range(S):
        np.testing.assert_array_equal(got[z], yuv422_ref.yuv422_to_bgr(raw[z * stride:(z + 1) * stride], H, W, order, pitch))


@pytest.fixture(scope='module')
def every_triple():
    """One 4096 x 4096 frame whose macropixels enumerate all 2^24 (Y, U, V) triples, each exactly once: macropixel k = y * 2048 + mx has
    U = k & 255, V = (k >> 8) & 255, Y0 = 2 ((k >> 16) & 127), Y1 = Y0 + 1.  -> (Y [4096, 4096], U, V [4096, 2048], the reference's BGR)."""
    k = np.arange(4096 * 2048, dtype=np.int64).reshape(4096, 2048)
    U, V = (k & 255).astype(np.uint8), ((k >> 8) & 255).astype(np.uint8)
    Y = np.empty((4096, 4096), np.uint8)
    Y[:, 0::2] = (2 * ((k >> 16) & 127)).astype(np.uint8)
    Y[:, 1::2] = Y[:, 0::2] + 1
    want = yuv_ref.yuv_to_bgr(Y, np.repeat(U, 2, axis=1), np.repeat(V, 2, axis=1))
    return Y, U, V, want


@pytest.mark.parametrize('order', ORDERS)
def test_every_input_once(order, every_triple):
    Y, U, V, want = every_triple
    raw = np.empty((4096, 4096, 2), np.uint8)
    luma, chroma = (0, 1) if order == 'yuy2' else (1, 0)
    raw[..., luma] = Y
    raw[:, 0::2, chroma], raw[:, 1::2, chroma] = U, V
    got = _convert(raw.reshape(-1), 4096, 4096, order, 1)
    assert np.array_equal(got[0], want)


# ------------------------------------------------------------------ the ring
@pytest.fixture(scope='module')
def two_launch_outputs(tmp_path_factory):
    """Every ring case once more in ONE fresh child process with DD_INGEST_YUV_FUSED=0 (read when a ring is created)."""
    path = str(tmp_path_factory.mktemp('yuv422') / 'two_launch.npz')
    env = dict(os.environ, DD_INGEST_YUV_FUSED='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(path) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize('i', range(len(RING_CASES)), ids=['%s-%dx%d-%dx%d-%s' % (c[0], *c[1], *c[2], 'flip' if c[3] else 'noflip') for c in RING_CASES])
def test_ring_flip_resize_vs_oracle(i, two_launch_outputs):
    from oracle import image_np
    order, src, dst, flip = RING_CASES[i]
    raw = _ring_input(i)
    assert os.environ.get('DD_INGEST_YUV_FUSED', '1') != '0'
    got = _run_ring(i)
    for z in range(S):
        img = yuv422_ref.yuv422_to_bgr(raw[z], src[1], src[0], order)
        if flip:
            img = img[::-1]                                       # convert, then cv2.flip(frame, 0), deepdish.py:864
        want = image_np.resize_linear_u8(np.ascontiguousarray(img), dst[0], dst[1]) if src != dst else img
        np.testing.assert_array_equal(got[z], want)
    np.testing.assert_array_equal(two_launch_outputs['case%d' % i], got)


@pytest.mark.parametrize('order', ORDERS)
def test_ring_feeds_the_pipeline(order):
    """The look-ahead loop of test_gpu_ingest_yuv.py::test_ring_feeds_the_pipeline with packed 4:2:2 slots: the detector's own rows
    (uint8 synthetic SSD, every label wanted), the tracks and the counts are those of a run that is handed yuv422_ref's BGR of the same
    buffers."""
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import DEFAULT_LABELS
    from deepdish_amd.synth import Scene, to_yuv422
    F = 7
    labels = [l.strip() for l in open(DEFAULT_LABELS)][1:]
    wanted = [l for l in labels if l and l != '???']
    scenes = [Scene(seed=40 + z, n_obj=6, n_frames=F) for z in range(S)]
    yuv = [np.stack([to_yuv422(sc.frame(f), order) for sc in scenes]) for f in range(F)]
    bgr = [np.stack([yuv422_ref.yuv422_to_bgr(y, 480, 640, order) for y in fr]) for fr in yuv]
    res = []
    for mode in ('direct', 'ring'):
        mp = MultiStreamPipeline(S, model='synthetic-ssd_mobilenet_v1-uint8', wanted_labels=wanted)
        rows = []
        if mode == 'direct':
            dev = [torch.from_numpy(fr).cuda() for fr in bgr]
            for f in range(F):
                mp.step(dev[f], None, dev[f + 1] if f + 1 < F else None)
                rows.append([mp.detections(z) for z in range(S)])
        else:
            ing = FrameIngest(S, (640, 480), slots=F, context=mp.ctx, pixel_format=order)
            assert ing.host(0).shape == (S, 480, 640, 2)
            for f in range(F):
                ing.host(f)[...] = yuv[f]
            ing.submit(0)
            for f in range(F):
                if f + 1 < F:
                    ing.submit(f + 1)
                nxt = ing.frames(f + 1, stream=mp.detector_stream()) if f + 1 < F else None
                mp.step(ing.frames(f), None, nxt)
                ing.release(f)
                rows.append([mp.detections(z) for z in range(S)])
        res.append((rows, [mp.tracker(z).table() for z in range(S)], mp.counts()))
    n_rows = 0
    for f in range(F):
        for z in range(S):
            a, b = res[0][0][f][z], res[1][0][f][z]
            assert list(a[1]) == list(b[1])
            np.testing.assert_array_equal(np.asarray(a[0], np.float64), np.asarray(b[0], np.float64))
            np.testing.assert_array_equal(np.asarray(a[2], np.float64), np.asarray(b[2], np.float64))
            n_rows += len(a[1])
    assert n_rows > 0
    for z in range(S):
        np.testing.assert_array_equal(res[0][1][z][0], res[1][1][z][0])
        np.testing.assert_array_equal(res[0][1][z][1], res[1][1][z][1])
    np.testing.assert_array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize('order', ORDERS)
def test_slot_size(order):
    from deepdish_amd.ingest import FrameIngest
    H, W = 33, 70
    ing = FrameIngest(S, (W, H), slots=2, pixel_format=order)
    for slot in range(2):
        assert ing.host(slot).nbytes == S * H * W * 2
        assert ing.host(slot).shape == (S, H, W, 2)
    assert ing.frames(0).shape == (S, H, W, 3)


def test_bad_arguments_raise_before_anything_is_allocated():
    from deepdish_amd._lib import lib, P
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.runtime import default_context
    with pytest.raises(ValueError, match='yuyv') as e:
        FrameIngest(S, (640, 480), pixel_format='yuyv')
    assert "'yuy2'" in str(e.value)                               # the spelling to use
    with pytest.raises(ValueError, match='641'):
        FrameIngest(S, (641, 480), pixel_format='yuy2')
    assert FrameIngest(S, (640, 479), pixel_format='uyvy').host(0).shape == (S, 479, 640, 2)
    # the C entry itself: a code, the message names the value, and no handle comes back
    ctx = default_context()
    h = P()
    assert lib().dd_ingest_create_format(ctx.handle, 2, S, 480, 641, 480, 641, 0, 4, ctypes.byref(h)) < 0
    assert b'src_w 641' in lib().dd_last_error() and not h.value
    assert lib().dd_ingest_create_format(ctx.handle, 2, S, 480, 640, 480, 640, 0, 6, ctypes.byref(h)) < 0
    assert b'pixel_format 6' in lib().dd_last_error() and not h.value
    assert lib().dd_ingest_create_format(ctx.handle, 2, S, 480, 640, 480, 640, 0, 3, ctypes.byref(h)) < 0
    assert b'pixel_format 3' in lib().dd_last_error() and not h.value
    assert lib().dd_yuv422_to_bgr(ctx.handle, None, 1, 480, 640, 6, 0, 0, None, None) < 0
    assert b'order 6' in lib().dd_last_error()
    assert lib().dd_yuv422_to_bgr(ctx.handle, None, 1, 480, 640, 4, 1278, 0, None, None) < 0
    assert b'pitch 1278' in lib().dd_last_error()


if __name__ == '__main__':
    np.savez(sys.argv[1], **{'case%d' % i: _run_ring(i) for i in range(len(RING_CASES))})
