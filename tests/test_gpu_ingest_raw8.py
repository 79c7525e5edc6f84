"""GPU: 8-bit Bayer mosaics and monochrome frames through the ingest ring (dd_ingest_create_raw8, csrc/bayer.hip) against tests/bayer_ref.py --
equality only.  The ring's flip + resize is held to the oracle's restatement of cv2 INTER_LINEAR applied to the converted frame (OpenCV
itself is absent: unpinned), once fused (one launch) and once, in a fresh child process with DD_INGEST_YUV_FUSED=0, as convert + resize.

Run as a script (`python tests/test_gpu_ingest_raw8.py out.npz`) this file is that child: it pushes every ring case through a
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
import bayer_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = bayer_ref.LAYOUTS
S = 3
# the geometries of test_gpu_ingest_yuv422.py, plus the smallest mosaic stretched
RING_GEOMETRIES = [((1280, 720), (640, 480), False), ((1280, 960), (640, 480), True), ((480, 360), (640, 480), True),
                   ((640, 480), (640, 480), False), ((640, 480), (640, 480), True), ((70, 34), (30, 22), True),
                   ((70, 33), (30, 22), True), ((3, 3), (5, 4), False)]
RING_CASES = [(layout,) + g for layout in LAYOUTS for g in RING_GEOMETRIES]


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
    return np.random.default_rng(808 + i).integers(0, 256, (S, src[1], src[0]), dtype=np.uint8)


def _run_ring(i):
    from deepdish_amd.ingest import FrameIngest
    layout, src, dst, flip = RING_CASES[i]
    ing = FrameIngest(S, src, dst, slots=2, flip=flip, pixel_format=layout)
    ing.host(1)[...] = _ring_input(i)
    ing.submit(1)
    got = _read(ing.ctx, ing.acquire(1), (S, dst[1], dst[0], 3))
    ing.release(1)
    return got


@pytest.fixture(scope='module')
def two_launch_outputs(tmp_path_factory):
    """Every ring case once more in ONE fresh child process with DD_INGEST_YUV_FUSED=0 (read when a ring is created)."""
    path = str(tmp_path_factory.mktemp('raw8') / 'two_launch.npz')
    env = dict(os.environ, DD_INGEST_YUV_FUSED='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(path) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize('i', range(len(RING_CASES)), ids=['%s-%dx%d-%dx%d-%s' % (c[0], *c[1], *c[2], 'flip' if c[3] else 'noflip') for c in RING_CASES])
def test_ring_flip_resize_vs_oracle(i, two_launch_outputs):
    from oracle import image_np
    layout, src, dst, flip = RING_CASES[i]
    raw = _ring_input(i)
    assert os.environ.get('DD_INGEST_YUV_FUSED', '1') != '0'
    got = _run_ring(i)
    for z in range(S):
        img = bayer_ref.raw8_to_bgr(raw[z], src[1], src[0], layout)
        if flip:
            img = img[::-1]                                       # convert, then cv2.flip(frame, 0), deepdish.py:864
        want = image_np.resize_linear_u8(np.ascontiguousarray(img), dst[0], dst[1]) if src != dst else img
        np.testing.assert_array_equal(got[z], want)
    np.testing.assert_array_equal(two_launch_outputs['case%d' % i], got)


@pytest.mark.parametrize('layout', ['bayer_gbrg', 'gray'])
def test_ring_feeds_the_pipeline(layout):
    """The look-ahead loop of test_gpu_ingest_yuv422.py::test_ring_feeds_the_pipeline with raw 8-bit slots: the detector's own rows (uint8
    synthetic SSD, every label wanted), the tracks and the counts are those of a run that is handed bayer_ref's BGR of the same buffers."""
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import DEFAULT_LABELS
    from deepdish_amd.synth import Scene, to_bayer, to_gray
    F = 7
    labels = [l.strip() for l in open(DEFAULT_LABELS)][1:]
    wanted = [l for l in labels if l and l != '???']
    scenes = [Scene(seed=40 + z, n_obj=6, n_frames=F) for z in range(S)]
    sample = to_gray if layout == 'gray' else (lambda f: to_bayer(f, layout))
    raw = [np.stack([sample(sc.frame(f)) for sc in scenes]) for f in range(F)]
    bgr = [np.stack([bayer_ref.raw8_to_bgr(y, 480, 640, layout) for y in fr]) for fr in raw]
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
            ing = FrameIngest(S, (640, 480), slots=F, context=mp.ctx, pixel_format=layout)
            assert ing.host(0).shape == (S, 480, 640)
            assert ing.present(0).tolist() == [1] * S
            for f in range(F):
                ing.host(f)[...] = raw[f]
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


@pytest.mark.parametrize('layout', LAYOUTS)
def test_slot_size(layout):
    from deepdish_amd.ingest import FrameIngest
    H, W = 33, 70
    ing = FrameIngest(S, (W, H), slots=2, pixel_format=layout)
    for slot in range(2):
        assert ing.host(slot).nbytes == S * H * W
        assert ing.host(slot).shape == (S, H, W)
    assert ing.frames(0).shape == (S, H, W, 3)
    assert ing.present(0).tolist() == [1] * S


def test_bad_arguments_raise_before_anything_is_allocated():
    from deepdish_amd._lib import lib, P, DeepDishHipError
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.runtime import default_context
    with pytest.raises(ValueError, match='grey') as e:
        FrameIngest(S, (640, 480), pixel_format='grey')
    assert "'gray'" in str(e.value) and 'is none of' in str(e.value) and "'bayer_rggb'" in str(e.value)
    with pytest.raises(ValueError, match='2x480'):
        FrameIngest(S, (2, 480), pixel_format='bayer_rggb')
    with pytest.raises(ValueError, match='640x2'):
        FrameIngest(S, (640, 2), pixel_format='bayer_bggr')
    assert FrameIngest(S, (2, 1), pixel_format='gray').host(0).shape == (S, 1, 2)
    for kw in ({'jpeg_scale': 2}, {'jpeg_progressive': True}, {'jpeg_split': True}, {'jpeg_any_size': True}, {'jpeg_std_tables': True}):
        for layout in ('bayer_rggb', 'gray'):
            with pytest.raises(ValueError, match=list(kw)[0]):
                FrameIngest(S, (640, 480), pixel_format=layout, **kw)
    # the C entries themselves: a code, the message names the value, and no handle comes back
    ctx = default_context()
    h = P()
    assert lib().dd_ingest_create_raw8(ctx.handle, 2, S, 480, 640, 480, 640, 0, 5, ctypes.byref(h)) < 0
    assert b'layout 5' in lib().dd_last_error() and not h.value
    assert lib().dd_ingest_create_raw8(ctx.handle, 2, S, 480, 2, 480, 640, 0, 7, ctypes.byref(h)) < 0
    assert b'src_w 2' in lib().dd_last_error() and not h.value
    for code in range(6, 12):                                     # the entry that never took them refuses them with the words it always had
        assert lib().dd_ingest_create_format(ctx.handle, 2, S, 480, 640, 480, 640, 0, code, ctypes.byref(h)) < 0
        assert b'dd_ingest_create_format: pixel_format %d is none of 0 (BGR), 1 (NV12), 2 (I420), 4 (YUY2), 5 (UYVY)' % code in lib().dd_last_error()
        assert not h.value
    # a raw8 ring holds no files: status and put are state errors
    ing = FrameIngest(S, (16, 8), pixel_format='gray')
    with pytest.raises(DeepDishHipError):
        ing.status(0)
    assert b'does not hold JPEG files' in lib().dd_last_error()
    with pytest.raises(DeepDishHipError):
        ing.put(0, 0, b'\xff\xd8')
    assert b'does not hold JPEG files' in lib().dd_last_error()


if __name__ == '__main__':
    np.savez(sys.argv[1], **{'case%d' % i: _run_ring(i) for i in range(len(RING_CASES))})
