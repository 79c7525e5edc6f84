"""GPU: the top-down view from the kernels to the pipelines, held to tests/topdown_ref.py -- equality everywhere.

ground_points_k (csrc/ground.hip) against the host entry bit for bit; render_k's filled rectangle and even-width lines against the ref;
the pipelines' panel frame against the ref fed from dd_pipeline_overlay's arrays.  Outputs land in sentinel-guarded buffers."""
import functools
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_ref  # noqa: E402
import render_ref  # noqa: E402
import test_gpu_render as tgr  # noqa: E402  (its generators and guarded draw, imported, not edited)
import topdown_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
LEAD, TAIL = 16, 64                              # doubles around the output; LEAD keeps it 16-byte aligned
CAMERAS = [(3.6, (6.17, 4.55), (640, 480), 4.0, 60.0, 0.0), (3.6, (6.17, 4.55), (640, 480), 2.5, 30.0, 10.0), (2.8, (5.37, 4.04), (640, 480), 7.25, 85.0, -10.0),
           (8.0, (7.2, 5.4), (640, 480), 12.0, 0.0, 3.5), (4.2, (6.17, 4.55), (640, 480), 3.0, 45.0, -1.0), (3.6, (6.17, 4.55), (640, 480), 4.0, 89.0, 0.0),
           (6.0, (6.17, 4.55), (640, 480), 30.0, 10.0, 180.0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host(cams, pts, idx):
    from deepdish_amd._lib import lib
    out = np.empty_like(pts)
    rc = lib().dd_ground_from_image(None, cams.ctypes.data, len(cams), None if idx is None else idx.ctypes.data, pts.ctypes.data, len(pts), out.ctypes.data, 0, None)
    assert rc == 0
    return out


def _device(cams, pts, idx):
    """dd_ground_from_image on device arrays into a sentinel-filled, guarded buffer -> host [n, 2]."""
    import torch
    from deepdish_amd._lib import lib, check, P
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    n = len(pts)
    buf = torch.full((LEAD + 2 * n + TAIL,), SENTINEL, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()                                       # the fill ran on torch's stream, the launch runs on the context's
    out = buf[LEAD:LEAD + 2 * n]
    d_cams, d_pts = ctx.to_device(cams), ctx.to_device(pts)
    d_idx = None if idx is None else ctx.to_device(idx)
    check(lib().dd_ground_from_image(ctx.handle, P(d_cams.data_ptr()), len(cams), P(d_idx.data_ptr()) if d_idx is not None else P(None), P(d_pts.data_ptr()), n,
                                     P(out.data_ptr()), 1, None), 'dd_ground_from_image')
    host = ctx.to_host(buf)
    assert (host[:LEAD] == SENTINEL).all() and (host[LEAD + 2 * n:] == SENTINEL).all(), 'doubles outside the output were written'
    return host[LEAD:LEAD + 2 * n].reshape(n, 2)


def _points(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-100.0, 800.0, (n, 2))
    p[::7] = np.round(p[::7])
    if n >= 63:                                                       # non-finite inputs, each form
        p[5] = (np.nan, 100.0)
        p[17] = (300.0, np.inf)
        p[40] = (-np.inf, np.nan)
    return p


def _grid_cap_points():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


@pytest.mark.parametrize('n_cams', [1, 7])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4099, 'one grid pass + 3'])
def test_ground_points_kernel_equals_the_host_entry_bit_for_bit(n, n_cams):
    """A single lane, a wave less one, a wave, a wave and one, 17 waves less 61 lanes, and three points more than the capped grid covers
    in one pass (8 workgroups per CU).  Camera indices change inside every wave (runs of 5), so a wave takes several turns; NaN inputs and
    rows at and above the horizon are in the set (tilts of 85 and 89 degrees put the horizon across the image)."""
    if not isinstance(n, int):
        n = _grid_cap_points() + 3
    cams = np.stack([topdown_ref.camera(*c) for c in CAMERAS[:n_cams]])
    pts = _points(n, 1000 * n_cams + n % 9973)
    idx = None if n_cams == 1 else ((np.arange(n) // 5 + np.arange(n) // 64) % n_cams).astype(np.int32)
    want = _host(cams, pts, idx)
    got = _device(cams, pts, idx)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    if n <= 4099:
        np.testing.assert_array_equal(_bits(want), _bits(topdown_ref.space_from_image(cams, pts, idx)))
    if n >= 63:
        nan = np.isnan(want[:, 0])
        assert nan[[5, 17, 40]].all() and (n_cams == 1 or 0.02 < nan.mean() < 0.98)
    if n >= 64 and n_cams > 1:
        assert len(set(idx[:64].tolist())) > 3                       # the first wave alone serves several cameras


def test_an_index_outside_the_table_yields_nan_on_the_device_and_leaves_its_neighbours():
    cams = np.stack([topdown_ref.camera(*c) for c in CAMERAS])
    n = 200
    pts = np.random.default_rng(8).uniform(50.0, 600.0, (n, 2))
    pts[:, 1] = np.random.default_rng(9).uniform(300.0, 470.0, n)   # well below the horizon of cameras 0, 1 and 4
    idx = np.array([0, 1, 4], dtype=np.int32)[np.arange(n) % 3]
    good = _host(cams, pts, idx)
    assert np.isfinite(good).all()
    bad = idx.copy()
    where = [0, 63, 64, 100, 199]
    bad[where] = [7, -1, 2 ** 31 - 1, -2 ** 31, 8]
    got = _device(cams, pts, bad)
    assert np.isnan(got[where]).all() and (_bits(got[where]) == 0x7ff8000000000000).all()
    keep = np.setdiff1d(np.arange(n), where)
    np.testing.assert_array_equal(_bits(got[keep]), _bits(good[keep]))


def test_device_tensors_through_the_python_class():
    import torch
    from deepdish_amd.ground import GroundPlane
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    table = GroundPlane.stack([GroundPlane(c[0], sensor_mm=c[1], image=c[2], elevation_m=c[3], tilt_deg=c[4], roll_deg=c[5]) for c in CAMERAS[:3]])
    pts = _points(333, 4)
    idx = (np.arange(333) // 11 % 3).astype(np.int32)
    got = table.space_from_image(ctx.to_device(pts), ctx.to_device(idx))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    np.testing.assert_array_equal(_bits(ctx.to_host(got)), _bits(table.space_from_image(pts, idx)))
    got0 = table.space_from_image(ctx.to_device(pts))
    np.testing.assert_array_equal(_bits(ctx.to_host(got0)), _bits(table.space_from_image(pts)))
    assert tuple(table.space_from_image(ctx.to_device(np.zeros((0, 2)))).shape) == (0, 2)


# ------------------------------------------------------------------ render_k: kind 3 and even widths
CANVASES = [(64, 16), (65, 17), (130, 35)]                           # one tile; one pixel over in both directions; 390-byte rows (not dword-aligned)


@functools.lru_cache(maxsize=None)
def _renderer(H, W):
    """A renderer of record set 2 (fills and even widths) -> (Renderer, {atlas offset: mask}), with masks as test_gpu_render's has them."""
    from deepdish_amd.render import Renderer
    r = Renderer(H, W, records=2)
    rng = np.random.default_rng(H + W)
    masks = {}
    for w, h in ((5, 3), (13, 9), (1, 1), (7, 16), (66, 2), (4, 4), (3, 21)):
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m[rng.random((h, w)) < 0.2] = 0
        m[rng.random((h, w)) < 0.2] = 255
        masks[r.put_mask(m)] = m
    return r, masks


def _one_by_one(W, H, recs):
    r, atlas = _renderer(H, W)
    frames = tgr._frames(1, H, W)
    prims = [np.asarray(q, dtype=np.int32).reshape(1, 8) for q in recs]
    got = tgr._draw(r, frames, prims, streams=[0] * len(prims))
    return got, [topdown_ref.paint_records(frames[0], q, atlas) for q in prims], frames[0]


@pytest.mark.parametrize('canvas', CANVASES, ids=lambda c: '%dx%d' % c)
def test_fills_on_tiles_edges_and_outside(canvas):
    W, H = canvas
    ink = 0x30d0a0
    boxes = [(0, 0, 63, 15), (60, 12, 70, 20), (0, 0, W - 1, H - 1), (0, 3, 5, 9), (W - 3, 2, W - 1, 8), (4, 0, 9, 2), (4, H - 2, 9, H - 1), (-5, -5, W + 5, H + 5),
             (-8192, -8192, 8191, 8191), (7, 7, 7, 7), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (3, 5, 40, 5), (9, 1, 9, 14), (63, 15, 64, 16),
             (-20, -20, -1, -1), (W, 0, W + 10, 10), (0, H, 10, H + 10), (-30, 2, -1, 9), (5, -9, 20, -1), (-3, -3, 2, 2), (W - 2, H - 2, W + 9, H + 9)]
    got, want, frame = _one_by_one(W, H, [(3,) + b + (0, ink, 0) for b in boxes])
    for i, b in enumerate(boxes):
        np.testing.assert_array_equal(got[i], want[i], err_msg=str(b))
    for i in range(15, 20):
        np.testing.assert_array_equal(got[i], frame)                 # wholly outside
    bgr = (ink & 255, (ink >> 8) & 255, ink >> 16)
    assert (got[2] == bgr).all() and (got[7] == bgr).all() and (got[8] == bgr).all()
    assert int((got[9] != frame).any(axis=-1).sum()) == 1 and (got[9][7, 7] == bgr).all()
    assert int((got[0] == bgr).all(axis=-1).sum()) >= 64 * 16       # exactly one tile (a noise pixel may have the ink's colour)


@pytest.mark.parametrize('width', [2, 4, 6, 14])
def test_lines_of_even_width(width):
    W, H = 130, 35
    segs = [(10, 15, 120, 15), (63, 0, 63, 34), (64, 3, 64, 30), (0, 0, 129, 34), (129, 0, 0, 34), (70, 20, 70, 20), (0, 0, 0, 0), (129, 34, 129, 34),
            (-8192, -8192, 8191, 8191), (8191, 10, -8192, 11), (60, 12, 70, 20), (127, 15, 129, 17), (-5, -5, -1, -1), (300, 50, 210, 60), (62, 14, 66, 18)]
    got, want, frame = _one_by_one(W, H, [(1,) + s + (width, 0x00ff00, 0) for s in segs])
    for i, s in enumerate(segs):
        np.testing.assert_array_equal(got[i], want[i], err_msg=str(s))
    if width == 2:                                                    # a zero-length segment of width 2: the pixel and its four neighbours
        changed = (got[5] != frame).any(axis=-1)
        assert changed.sum() <= 5 and not changed[:19].any() and not changed[22:].any() and not changed[:, :69].any() and not changed[:, 72:].any()
    np.testing.assert_array_equal(got[13], frame)


def _prims_of_four_kinds(rng, H, W, masks, k):
    """test_gpu_render's generator, then half of the outlines turned into fills and half of the lines given an even width."""
    p = tgr._random_prims(rng, H, W, masks, k)
    for i in range(k):
        if p[i, 0] == 0 and rng.random() < 0.5:
            p[i, 0] = 3
        elif p[i, 0] == 1 and rng.random() < 0.5:
            p[i, 5] = 2 * int(rng.integers(1, 8))
    return p


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'out+1'])
@pytest.mark.parametrize('canvas', CANVASES, ids=lambda c: '%dx%d' % c)
def test_more_than_256_records_of_all_four_kinds_and_a_frame_without(canvas, shift):
    W, H = canvas
    r, masks = _renderer(H, W)
    frames = tgr._frames(2, H, W)
    rng = np.random.default_rng(W * 7 + H)
    prims = [_prims_of_four_kinds(rng, H, W, masks, 300), np.zeros((0, 8), np.int32)]
    kinds = prims[0][:, 0]
    assert all((kinds == k).sum() >= 20 for k in range(4)) and ((kinds == 1) & (prims[0][:, 5] % 2 == 0)).sum() >= 10
    assert len(set(kinds[250:262].tolist())) >= 3                    # several kinds around the end of the first LDS batch
    got = tgr._draw(r, frames, prims, shift=shift)
    want = topdown_ref.paint_records(frames[0], prims[0], masks)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], frames[1])                 # a frame without records is a copy
    assert (want != topdown_ref.paint_records(frames[0], prims[0][:tgr.CHUNK], masks)).any()      # the second batch paints
    assert (want != topdown_ref.paint_records(frames[0], prims[0][::-1], masks)).any()            # and the order matters in this scene


def test_kinds_0_to_2_and_odd_widths_still_equal_render_ref():
    """One mixed scene of tests/test_gpu_render.py's own generator (outlines, odd-width lines, masks) on several tiles: the frames equal
    tests/render_ref.py, the definition from before the fill and the even widths."""
    W, H, n = 200, 120, 2
    r, masks = tgr._renderer(H, W)
    frames = tgr._frames(n, H, W)
    rng = np.random.default_rng(W * 31 + H)
    prims = [tgr._random_prims(rng, H, W, masks, 60) for _ in range(n)]
    got = tgr._draw(r, frames, prims)
    for i in range(n):
        np.testing.assert_array_equal(got[i], render_ref.paint_records(frames[i], prims[i], masks), err_msg='frame %d' % i)
        np.testing.assert_array_equal(got[i], topdown_ref.paint_records(frames[i], prims[i], masks), err_msg='frame %d' % i)
    r2, masks2 = _renderer(H, W)                                     # and the same through a renderer of record set 2
    prims2 = [tgr._random_prims(np.random.default_rng(5 + i), H, W, masks2, 60) for i in range(n)]
    got2 = tgr._draw(r2, frames, prims2)
    for i in range(n):
        np.testing.assert_array_equal(got2[i], render_ref.paint_records(frames[i], prims2[i], masks2), err_msg='record set 2, frame %d' % i)


def test_bad_fills_and_widths_are_refused_before_the_launch():
    from deepdish_amd._lib import DeepDishHipError
    r, _ = _renderer(35, 130)
    dev = r.ctx.to_device(tgr._frames(1, 35, 130))
    for bad in ((3, 5, 5, 4, 9, 0, 0, 0), (3, 5, 5, 9, 4, 0, 0, 0), (3, 0, 0, 9000, 5, 0, 0, 0), (3, -8193, 0, 5, 5, 0, 0, 0), (4, 0, 0, 1, 1, 0, 0, 0),
                (1, 0, 0, 5, 5, 0, 0, 0), (1, 0, 0, 5, 5, 16, 0, 0), (1, 0, 0, 5, 5, -2, 0, 0)):
        with pytest.raises(DeepDishHipError, match='dd_render_draw'):
            r.draw(dev, [np.array([bad], dtype=np.int32)])
    plain, _ = tgr._renderer(35, 130)                                # a renderer of record set 1 refuses what set 2 adds, as it always has
    for bad, what in (((3, 0, 0, 1, 1, 0, 0, 0), 'kind 3'), ((1, 0, 0, 5, 5, 2, 0, 0), r'line width 2 \(odd')):
        with pytest.raises(DeepDishHipError, match=what):
            plain.draw(dev, [np.array([bad], dtype=np.int32)])
    r.draw(dev, [np.array([(3, 0, 0, 1, 1, 0, 0, 0), (1, 0, 0, 5, 5, 2, 0, 0)], dtype=np.int32)])
    from deepdish_amd.render import Renderer
    with pytest.raises(DeepDishHipError, match='dd_render_record_set'):
        Renderer(35, 130, records=3)


# ------------------------------------------------------------------ pipelines
S, W, H, STEPS = 4, tgr.PIPE_W, tgr.PIPE_H, 6
SIZE_M = (20, 10)
PIPE_CAMERAS = [dict(tilt_deg=45.0, elevation_m=3.0, roll_deg=0.0), dict(tilt_deg=30.0, elevation_m=5.0, roll_deg=5.0),
                dict(tilt_deg=80.0, elevation_m=2.0, roll_deg=-3.0),      # horizon near row 35: the upper object's path lies above it
                dict(tilt_deg=0.0, elevation_m=9.0, roll_deg=0.0)]


def _camera(z):
    from deepdish_amd.ground import GroundPlane
    return GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(W, H), **PIPE_CAMERAS[z])


@functools.lru_cache(maxsize=None)
def _run():
    """6 steps of 4 streams on 128 x 96 noise frames with injected detections, once with a camera per stream and once without; a
    single-stream pipeline beside stream 2.  -> what the checks need of the last step."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    font = tgr._font()
    cams = [_camera(z) for z in range(S)]
    mp = MultiStreamPipeline(S, input_size=(W, H), run_detector=False, ground=cams, topdownview_size_m=SIZE_M)
    plain = MultiStreamPipeline(S, input_size=(W, H), run_detector=False)
    hp = HotPath(input_size=(W, H), run_detector=False, ground=cams[2], topdownview_size_m=SIZE_M)
    for f in range(STEPS):
        frames = np.array(tgr._frames(S, H, W + f)[:, :, :W])
        dev = ctx.to_device(frames)
        per = [(tgr._scene_boxes(z, f), ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(S)]
        mp.step(dev, mp.pack_injected(per))
        plain.step(dev, plain.pack_injected(per))
        hp.step(dev[2], injected=per[2])
    sel = [0, 2]
    return dict(frames=frames, cams=cams, overlay=mp.overlay(sel), counts=mp.counts().copy(), sel=sel,
                mp=ctx.to_host(mp.render(dev, streams=sel, font=font)), mp_all=ctx.to_host(mp.render(dev, font=font)),
                plain=ctx.to_host(plain.render(dev, streams=sel, font=font)), hp=ctx.to_host(hp.render(dev[2], font=font))[0],
                paths=mp.ground_paths(sel), jpeg=mp.render_jpeg(dev, streams=sel, font=font))


def _want(rec, i, topdown):
    z, o = rec['sel'][i], rec['overlay'][i]
    at, tracks = 0, []
    for tid, lbl, box, n in zip(o['track_ids'], o['track_labels'], o['track_tlbr'], o['path_counts']):
        tracks.append((int(tid), lbl, box, o['points'][at:at + n]))
        at += n
    counters = [('person', int(rec['counts'][z][0, 1]), int(rec['counts'][z][0, 0]))]
    font = tgr._font()
    if not topdown:
        return render_ref.paint(rec['frames'][z], render_ref.overlay_elements(W, H, o['line'], tracks, o['crossings'], o['det_tlbr'], counters, 'label', font=font), font=font)
    ground = [topdown_ref.space_from_image(rec['cams'][z].table, t[3]) for t in tracks]
    scale = np.array([W / 4, H / 4]) / np.array(SIZE_M, dtype=np.float64)
    el = topdown_ref.overlay_elements(W, H, o['line'], tracks, o['crossings'], o['det_tlbr'], counters, 'label', font=font, ground_paths=ground, scale=scale)
    return topdown_ref.paint(rec['frames'][z], el, font=font)


def test_pipeline_render_with_the_panel_equals_the_ref():
    rec = _run()
    nan_points = drawn = 0
    for i, z in enumerate(rec['sel']):
        want = _want(rec, i, True)
        np.testing.assert_array_equal(rec['mp'][i], want, err_msg='stream %d' % z)
        np.testing.assert_array_equal(rec['mp_all'][z], want, err_msg='stream %d of all' % z)
        assert (want[:H // 4 + 1, :W // 4 + 1] == 0).all(axis=-1).sum() > 0.5 * (H // 4) * (W // 4)      # a black panel in the corner
        assert (want != _want(rec, i, False)).any()
        o = rec['overlay'][i]
        drawn += len(o['track_ids'])
        nan_points += int(np.isnan(topdown_ref.space_from_image(rec['cams'][z].table, o['points'])).any(axis=1).sum())
        assert (o['path_counts'] >= 2).any()                          # a polyline, not only markers
    assert drawn >= 4 and nan_points >= 1                            # stream 2's upper object walks above the horizon


def test_ground_paths_equal_the_host_entry_on_the_overlay_s_points():
    rec = _run()
    for i, z in enumerate(rec['sel']):
        o, g = rec['overlay'][i], rec['paths'][i]
        np.testing.assert_array_equal(g['track_ids'], o['track_ids'])
        np.testing.assert_array_equal(g['path_counts'], o['path_counts'])
        want = _host(rec['cams'][z].table, np.ascontiguousarray(o['points']), None) if len(o['points']) else np.zeros((0, 2))
        np.testing.assert_array_equal(_bits(g['points']), _bits(want))
        assert len(g['points']) == o['path_counts'].sum() > 0


def test_without_ground_the_frame_is_the_one_render_ref_expects():
    rec = _run()
    for i, z in enumerate(rec['sel']):
        np.testing.assert_array_equal(rec['plain'][i], _want(rec, i, False), err_msg='stream %d' % z)


def test_single_stream_pipeline_renders_the_same_panel_frame():
    rec = _run()
    np.testing.assert_array_equal(rec['hp'], _want(rec, rec['sel'].index(2), True))


def test_render_jpeg_of_the_panel_frame():
    from PIL import Image
    rec = _run()
    for i, z in enumerate(rec['sel']):
        want_file = jpeg_ref.encode(_want(rec, i, True), 95, 1)
        got = np.array(Image.open(io.BytesIO(rec['jpeg'][i])).convert('RGB'))
        np.testing.assert_array_equal(got, np.array(Image.open(io.BytesIO(want_file)).convert('RGB')), err_msg='stream %d' % z)
        assert got.shape == (H, W, 3) and rec['jpeg'][i] == want_file


def test_constructor_refusals():
    from deepdish_amd.ground import GroundPlane
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    other = GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=3.0, tilt_deg=45.0)
    with pytest.raises(ValueError, match='640 x 480'):
        MultiStreamPipeline(2, input_size=(W, H), run_detector=False, ground=[other, other])
    with pytest.raises(ValueError, match='640 x 480'):
        HotPath(input_size=(W, H), run_detector=False, ground=other)
    with pytest.raises(ValueError, match='3 cameras for 4 streams'):
        MultiStreamPipeline(4, input_size=(W, H), run_detector=False, ground=[_camera(0)] * 3)
    with pytest.raises(ValueError, match='without ground'):
        MultiStreamPipeline(2, input_size=(W, H), run_detector=False, topdownview_size_m=(20, 10))
    with pytest.raises(ValueError, match='without ground'):
        HotPath(input_size=(W, H), run_detector=False, topdownview_size_m=(20, 10))
    with pytest.raises(ValueError, match='ground_paths'):
        _run_plain_paths()


def _run_plain_paths():
    from deepdish_amd.multipipe import MultiStreamPipeline
    MultiStreamPipeline(1, input_size=(W, H), run_detector=False).ground_paths()
