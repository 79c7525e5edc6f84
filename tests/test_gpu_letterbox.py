"""GPU: letterboxed YOLOv5 input (csrc/letterbox.hip) and the box un-mapping (csrc/post.hip), from the kernels to the pipelines.

Pixels are held to Pillow (tests/letterbox_ref.canvas: Image.new + resize(LANCZOS) + paste), the geometry to the reference's
letterbox_image (tests/test_letterbox_ref.py), the boxes to tests/letterbox_ref.decode -- equality everywhere.  The frames are the three
of tests/test_gpu_lanczos_paths.py (noise, all 255, a 0 / 255 checkerboard in cells of 3 rows x 5 pixels); outputs land in
sentinel-guarded buffers.

DD_LETTERBOX_FUSED and DD_YOLO_DEC are read once per process, so those forms run in a child: this file as a script,
`python tests/test_gpu_letterbox.py out.npz pixels|pipeline`, runs the named job under whatever the environment sets and saves the results."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import letterbox_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LEAD, TAIL = 64, 256                                               # guard bytes around the output (LEAD keeps its 64-byte alignment)
ALL_FORMS = ((3, 0), (3, 1), (4, 0), (4, 1))                       # (src_c, swap_rb): RGB, BGR, RGBA, BGRA
PADS = (114, 0)
# (W, H, w, h, batch, path, forms)
GEOMETRIES = [
    (96, 54, 64, 64, 3, 1, ALL_FORMS),                             # 64 x 36, 14 rows of padding above and below
    (54, 96, 64, 64, 3, 1, ((3, 1),)),                             # 36 x 64, padding left and right
    (64, 48, 64, 64, 3, 0, ((3, 1),)),                             # copy only
    (33, 17, 64, 64, 3, 1, ((3, 1),)),                             # upscale to 64 x 32
    (49, 7, 64, 64, 3, 1, ((3, 1),)),                              # 63 x 9: a one-column right pad, odd offset 27
    (70, 50, 64, 48, 3, 1, ((3, 1),)),                             # 64 x 45: 1 row above, 2 below
    (200, 120, 96, 96, 3, 1, ((3, 1),)),                           # 57 picture rows: several bands, the last partial
    (1280, 720, 640, 640, 2, 1, ((3, 1),)),
]
CASES = [g[:6] + f for g in GEOMETRIES for f in g[6]]
CASE_IDS = ['%dx%d-%dx%d-b%d-path%d-c%d-swap%d' % c for c in CASES]
CHILD_CASES = [c for c in CASES if c[:4] in ((96, 54, 64, 64), (54, 96, 64, 64), (64, 48, 64, 64)) and c[6:] == (3, 1)]
TWO_LAUNCH = (4096, 48, 2048, 32, 1, 2, 3, 1)                      # tests/test_letterbox_ref.py: 12 rows x 6 144 B exceed the LDS budget


# ------------------------------------------------------------------ pixels
@functools.lru_cache(maxsize=None)
def _rgb(H, W, batch):
    """The RGB view of a geometry's frames: noise, all 255, a checkerboard of 0 / 255 in cells of 3 rows x 5 pixels."""
    f = np.random.default_rng(H * 10007 + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    f[1] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    f[2] = (((yy // 3 + xx // 5) & 1) * 255).astype(np.uint8)[..., None]
    f = f[:batch]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(W, H, w, h, batch, pad):
    out = np.stack([letterbox_ref.canvas(fr, w, h, pad) for fr in _rgb(H, W, batch)])
    out.setflags(write=False)
    return out


def _source(H, W, batch, src_c, swap_rb):
    rgb = _rgb(H, W, batch)
    px = rgb[..., ::-1] if swap_rb else rgb
    if src_c == 4:                                                 # a fourth channel of noise: it must be ignored
        px = np.concatenate([px, np.random.default_rng(H + W).integers(0, 256, (batch, H, W, 1), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(px)


def _plan(W, H, w, h, src_c, swap_rb, batch):
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context
    path, rows = ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib().dd_resize_lanczos_letterbox_plan(default_context().handle, H, W, src_c, swap_rb, h, w, batch, ctypes.byref(path), ctypes.byref(rows)))
    return path.value, rows.value


def _letterbox(case, pad):
    """-> (path, canvases u8 [batch, h, w, 3]); the guard bytes around the output are checked."""
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context
    W, H, w, h, batch, _, src_c, swap_rb = case
    ctx = default_context()
    src = ctx.to_device(_source(H, W, batch, src_c, swap_rb))
    nb = batch * h * w * 3
    buf = torch.full((LEAD + nb + TAIL,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()                                       # the fill ran on torch's stream, the launch runs on the context's
    path = _plan(W, H, w, h, src_c, swap_rb, batch)[0]
    check(lib().dd_resize_lanczos_letterbox(ctx.handle, ctypes.c_void_p(src.data_ptr()), batch, H, W, src_c, swap_rb,
                                            ctypes.c_void_p(buf.data_ptr() + LEAD), h, w, pad, None), 'dd_resize_lanczos_letterbox')
    host = ctx.to_host(buf)
    assert (host[:LEAD] == 0xA5).all() and (host[LEAD + nb:] == 0xA5).all(), 'bytes outside the canvases were written'
    return path, host[LEAD:LEAD + nb].reshape(batch, h, w, 3)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_canvas_equals_pillow(case, pad):
    W, H, w, h, batch, want_path = case[:6]
    path, got = _letterbox(case, pad)
    assert path == want_path, 'the geometry no longer takes the path this row is here for'
    want = _want(W, H, w, h, batch, pad)
    for i in range(batch):
        np.testing.assert_array_equal(got[i], want[i], err_msg='frame %d' % i)


def test_two_launch_geometry_in_process():
    """4096 x 48 into 2048 x 32: the vertical window of one canvas row does not fit the LDS budget, so the dense horizontal pass writes the
    context's scratch and letterbox_v_pad_k does the rest."""
    W, H, w, h, batch = TWO_LAUNCH[:5]
    path, got = _letterbox(TWO_LAUNCH, 114)
    assert path == 2
    np.testing.assert_array_equal(got, _want(W, H, w, h, batch, 114))


def test_two_launch_form_in_a_child_process(tmp_path):
    """DD_LETTERBOX_FUSED=0: the same bytes from the two-launch form (a copy-only geometry stays path 0 and runs letterbox_v_pad_k alone)."""
    out = str(tmp_path / 'child.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, 'pixels'], env=dict(os.environ, DD_LETTERBOX_FUSED='0'),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as z:
        for i, case in enumerate(CHILD_CASES):
            W, H, w, h, batch, path = case[:6]
            assert int(z['path%d' % i]) == (2 if path == 1 else 0), case
            np.testing.assert_array_equal(z['out%d' % i], _want(W, H, w, h, batch, 114), err_msg=str(case))


# ------------------------------------------------------------------ boxes
ROWS, N_CLS, DECODE_THR = 2100, 80, 0.1                            # more than two 1 024-row passes of yolo_compact_k


@functools.lru_cache(maxsize=None)
def _raw():
    """A head tensor as SURVEY section 8(d) draws it: xywh U(0, 1), objectness and classes Beta(0.5, 4)."""
    rng = np.random.default_rng(85)
    raw = np.concatenate([rng.uniform(0, 1, (ROWS, 4)), rng.beta(0.5, 4.0, (ROWS, 1 + N_CLS))], axis=1).astype(np.float32)
    raw.setflags(write=False)
    return raw


def _decode(entry, *geom):
    """dd_yolov5_decode (geom = img_w, img_h as floats) or dd_yolov5_decode_letterbox (img_w, img_h, net_w, net_h) on _raw()."""
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context, ptr
    ctx = default_context()
    raw = ctx.to_device(_raw())
    boxes, scores = ctx.empty((ROWS, 4), torch.float32), ctx.empty((ROWS,), torch.float32)
    cls, n = ctx.empty((ROWS,), torch.int32), ctx.empty((1,), torch.int32)
    check(getattr(lib(), entry)(ctx.handle, ptr(raw), ROWS, N_CLS, DECODE_THR, *geom, ptr(boxes), ptr(scores), ptr(cls), ROWS, ptr(n), None), entry)
    k = int(ctx.to_host(n)[0])
    return ctx.to_host(boxes)[:k], ctx.to_host(scores)[:k], ctx.to_host(cls)[:k]


@pytest.mark.parametrize('geom', [(640, 480, 640, 640), (1280, 720, 640, 640), (49, 7, 64, 64)], ids=lambda g: '%dx%d-%dx%d' % g)
def test_decode_unmaps_boxes_as_the_restatement(geom):
    want_b, want_s, want_c = letterbox_ref.decode(_raw(), DECODE_THR, *geom)
    keep = np.zeros(ROWS, bool)
    prod = _raw()[:, 5:] * _raw()[:, 4:5]
    keep[prod.max(axis=1) >= np.float32(DECODE_THR)] = True
    assert len(want_s) == keep.sum() >= 50
    assert all(keep[i:i + 64].any() for i in range(0, ROWS, 64)), 'a wave without a passing row'
    got_b, got_s, got_c = _decode('dd_yolov5_decode_letterbox', *geom)
    np.testing.assert_array_equal(got_s, want_s)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_b.view(np.uint32), want_b.view(np.uint32))
    assert (got_b < 0).any(), 'no box reaches into the padding'


def test_decode_of_a_square_frame_is_the_stretch_decode():
    a = _decode('dd_yolov5_decode_letterbox', 640, 640, 640, 640)
    b = _decode('dd_yolov5_decode', 640.0, 640.0)
    assert len(a[1]) >= 50
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------ plugin
def _wanted():
    from deepdish_amd.pipeline import DEFAULT_YOLO_LABELS
    return sorted({l.strip() for l in open(DEFAULT_YOLO_LABELS)})


@functools.lru_cache(maxsize=None)
def _detector():
    from deepdish_amd.tools.yolov5 import YOLOV5
    from deepdish_amd.pipeline import DEFAULT_YOLO_LABELS
    return YOLOV5(wanted_labels=_wanted(), model_file='synthetic-yolov5s', label_file=DEFAULT_YOLO_LABELS, letterbox=True)


def _scene_frame(seed, f=0):
    from deepdish_amd.synth import Scene
    return Scene(seed=seed, n_obj=8, n_frames=4).frame(f)          # BGR u8 [480, 640, 3]


def _tlwh(boxes):
    out = np.array(boxes, dtype=np.float32).reshape(-1, 4).copy()
    out[:, 2] = boxes[:, 2] - boxes[:, 0]                          # f32, tools/yolov5.py:140-142
    out[:, 3] = boxes[:, 3] - boxes[:, 1]
    return out


def test_plugin_letterboxes_its_input_and_unmaps_its_boxes():
    det = _detector()
    assert det.letterbox == 114
    bgr = _scene_frame(3)
    rgba = np.concatenate([bgr[..., ::-1], np.full(bgr.shape[:2] + (1,), 255, np.uint8)], axis=-1)      # RGBA in, no swap
    boxes, labels, scores = det.detect_image(rgba)
    np.testing.assert_array_equal(det.ctx.to_host(det._resized)[0], letterbox_ref.canvas(bgr[..., ::-1], 640, 640, 114))
    raw = np.asarray(det.net.read(), dtype=np.float32).reshape(-1, 5 + det.n_cls)
    want_b, want_s, want_c = letterbox_ref.decode(raw, det.score_threshold, 640, 480, 640, 640)
    assert len(want_s) > 0 and len(scores) == len(want_s)          # every label is wanted
    np.testing.assert_array_equal(np.array(boxes, dtype=np.float32).view(np.uint32), _tlwh(want_b).view(np.uint32))
    np.testing.assert_array_equal(np.array(scores, dtype=np.float32), want_s)
    assert labels == [det.labels[int(c)] for c in want_c]
    # BGR frame on the device: the same picture, the same answer
    b2, l2, s2 = det.detect_frame_device(det.ctx.to_device(bgr), 480, 640)
    assert l2 == labels
    np.testing.assert_array_equal(np.array(b2, dtype=np.float32), np.array(boxes, dtype=np.float32))


def test_plugin_on_a_square_image_is_the_stretch_plugin():
    """A 640 x 640 image fills the canvas: no resample, no padding, and the un-mapping is x * W -- the stretch plugin's bits.  The image is
    a synthetic scene with its top rows repeated below it (noise alone leaves the synthetic weights nothing above the default threshold),
    and the threshold is lowered for the call so that the compared result is not empty."""
    det = _detector()
    bgr = _scene_frame(5)
    img = np.ascontiguousarray(np.concatenate([bgr, bgr[:160]], axis=0)[..., [2, 1, 0, 0]])      # RGBA [640, 640, 4]; the fourth channel is ignored
    assert img.shape == (640, 640, 4)
    thr = det.score_threshold
    try:
        det.score_threshold = 0.08                                # the f32 oracle forward has ~280 rows of this image above it, none above 0.25
        a = det.detect_image(img)
        det.letterbox = None                                       # the reference's stretch (letterbox=False)
        b = det.detect_image(img)
    finally:
        det.letterbox, det.score_threshold = 114, thr
    assert len(a[1]) > 0 and a[1] == b[1]
    np.testing.assert_array_equal(np.array(a[0], dtype=np.float32).view(np.uint32), np.array(b[0], dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(np.array(a[2], dtype=np.float32), np.array(b[2], dtype=np.float32))


# ------------------------------------------------------------------ pipeline
PIPE_S, PIPE_W, PIPE_H = 3, 128, 96


@functools.lru_cache(maxsize=None)
def _pipe_frames():
    """Two steps of three 128 x 96 BGR frames: every fifth pixel of synthetic 640 x 480 scenes."""
    f = np.stack([np.stack([np.ascontiguousarray(_scene_frame(3 + z, step)[::5, ::5]) for z in range(PIPE_S)]) for step in range(2)])
    assert f.shape == (2, PIPE_S, PIPE_H, PIPE_W, 3)
    f.setflags(write=False)
    return f


def _run_pipeline():
    """-> per step, per stream (boxes tlwh f64, labels, scores f64) of dd_pipeline_detections; and the code of a late option call."""
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import default_context
    mp = MultiStreamPipeline(PIPE_S, 'synthetic-yolov5s', input_size=(PIPE_W, PIPE_H), wanted_labels=_wanted(), detector_letterbox=True,
                             run_detector=True)
    ctx = default_context()
    frames = [ctx.to_device(f) for f in _pipe_frames()]
    res = []
    mp.step(frames[0], frames_next=frames[1])                      # the second step's detector run is queued ahead
    res.append([mp.detections(z) for z in range(PIPE_S)])
    mp.step(frames[1])
    res.append([mp.detections(z) for z in range(PIPE_S)])
    late = lib().dd_pipeline_detector_letterbox(mp._h, 114)
    return res, late, lib().dd_last_error()


@functools.lru_cache(maxsize=None)
def _plugin_on_pipe_frames():
    det = _detector()
    return [[det.detect_frame_device(det.ctx.to_device(fr), PIPE_H, PIPE_W) for fr in step] for step in _pipe_frames()]


def _same_detections(got, want, where):
    gb, gl, gs = got
    wb, wl, ws = want
    assert list(gl) == list(wl), where
    np.testing.assert_array_equal(np.asarray(gb, np.float64).reshape(-1, 4), np.array(wb, dtype=np.float64).reshape(-1, 4), err_msg=where)
    np.testing.assert_array_equal(np.asarray(gs, np.float64), np.array(ws, dtype=np.float64), err_msg=where)


def test_pipeline_detections_equal_the_plugin_s():
    res, late, msg = _run_pipeline()
    want = _plugin_on_pipe_frames()
    assert sum(len(want[s][z][1]) for s in range(2) for z in range(PIPE_S)) > 0
    for s in range(2):
        for z in range(PIPE_S):
            _same_detections(res[s][z], want[s][z], 'step %d stream %d' % (s, z))
    assert late < 0 and b'before the first step' in msg            # the option is fixed once the pipeline has stepped


def test_pipeline_with_the_matrix_decode_in_a_child_process(tmp_path):
    """DD_YOLO_DEC=0: the heads write the [rows][85] matrix and yolov5_decode_letterbox reads it -- the same detections."""
    out = str(tmp_path / 'child.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, 'pipeline'], env=dict(os.environ, DD_YOLO_DEC='0'),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = _plugin_on_pipe_frames()
    with np.load(out) as z:
        for s in range(2):
            for q in range(PIPE_S):
                got = (z['b%d_%d' % (s, q)], [str(l) for l in z['l%d_%d' % (s, q)]], z['s%d_%d' % (s, q)])
                _same_detections(got, want[s][q], 'step %d stream %d' % (s, q))


def test_the_option_is_yolov5_s_alone():
    from deepdish_amd._lib import lib
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, make_detector
    with pytest.raises(ValueError):
        HotPath(model='synthetic-ssd_mobilenet_v1', detector_letterbox=True)
    with pytest.raises(ValueError):
        MultiStreamPipeline(1, 'synthetic-ssd_mobilenet_v1', detector_letterbox=114)
    with pytest.raises(ValueError):
        make_detector('synthetic-ssd_mobilenet_v1', letterbox=True)
    ssd = MultiStreamPipeline(1, 'synthetic-ssd_mobilenet_v1', input_size=(PIPE_W, PIPE_H))
    assert lib().dd_pipeline_detector_letterbox(ssd._h, 114) < 0
    assert b'YOLOv5' in lib().dd_last_error()


if __name__ == '__main__':
    saved = {}
    if sys.argv[2] == 'pixels':
        for i, case in enumerate(CHILD_CASES):
            path, got = _letterbox(case, 114)
            saved.update({'path%d' % i: np.int32(path), 'out%d' % i: got})
    else:
        res, _, _ = _run_pipeline()
        for s in range(2):
            for q in range(PIPE_S):
                b, l, sc = res[s][q]
                saved.update({'b%d_%d' % (s, q): b, 'l%d_%d' % (s, q): np.array(l, dtype=str), 's%d_%d' % (s, q): sc})
    np.savez(sys.argv[1], **saved)
