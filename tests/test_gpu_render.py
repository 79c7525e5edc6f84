"""GPU: the overlay renderer (csrc/render.hip) from the kernel to the pipelines, held to tests/render_ref.py -- equality everywhere.

Frames are noise; outputs land in sentinel-guarded buffers.  The kernel's tile is 64 x 16 pixels, 256 records are staged in LDS at a time,
and rows move as dwords only when W is a multiple of 4 and both frame arrays are dword-aligned."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import render_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LEAD, TAIL = 64, 256
TILE_W, TILE_H, CHUNK = 64, 16, 256
STRINGS = ('person', '12', 'bicycle 7', '')
RED, GREEN, BLUE, WHITE = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)


@functools.lru_cache(maxsize=None)
def _frames(n, H, W):
    f = np.random.default_rng(H * 10007 + W * 13 + n).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _renderer(H, W):
    """-> (Renderer, {atlas offset: mask}) with a few random coverage masks in the atlas: widths that are no multiple of 4 among them."""
    from deepdish_amd.render import Renderer
    r = Renderer(H, W)
    rng = np.random.default_rng(H + W)
    masks = {}
    for w, h in ((5, 3), (13, 9), (1, 1), (7, 16), (66, 2), (4, 4), (3, 21)):
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m[rng.random((h, w)) < 0.2] = 0
        m[rng.random((h, w)) < 0.2] = 255
        masks[r.put_mask(m)] = m
    return r, masks


def _draw(r, frames, prims, streams=None, shift=0):
    """Renderer.draw into a guarded buffer (shift: bytes by which the output is moved off its 64-byte alignment) -> host [n, H, W, 3]."""
    import torch
    n = len(prims)
    nb = n * r.H * r.W * 3
    buf = torch.full((LEAD + shift + nb + TAIL,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()                                       # the fill ran on torch's stream, the launch runs on the context's
    out = buf[LEAD + shift:LEAD + shift + nb].view(n, r.H, r.W, 3)
    dev = frames if hasattr(frames, 'data_ptr') else r.ctx.to_device(frames)
    got = r.draw(dev, prims, streams=streams, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = r.ctx.to_host(buf)
    assert (host[:LEAD + shift] == 0xA5).all() and (host[LEAD + shift + nb:] == 0xA5).all(), 'bytes outside the output frames were written'
    return host[LEAD + shift:LEAD + shift + nb].reshape(n, r.H, r.W, 3)


def _random_prims(rng, H, W, masks, k):
    from deepdish_amd import render as rd
    offs = sorted(masks)
    out = np.zeros((k, 8), dtype=np.int32)
    for i in range(k):
        kind = int(rng.integers(0, 3))
        ink = int(rng.integers(0, 1 << 24))
        if kind == rd.KIND_RECT:
            x0, y0 = int(rng.integers(-10, W + 5)), int(rng.integers(-10, H + 5))
            out[i] = (kind, x0, y0, x0 + int(rng.integers(0, W)), y0 + int(rng.integers(0, H)), 0, ink, 0)
        elif kind == rd.KIND_LINE:
            out[i] = (kind, rng.integers(-10, W + 10), rng.integers(-10, H + 10), rng.integers(-10, W + 10), rng.integers(-10, H + 10),
                      2 * int(rng.integers(0, 8)) + 1, ink, 0)
        else:
            off = offs[int(rng.integers(0, len(offs)))]
            h, w = masks[off].shape
            out[i] = (kind, rng.integers(-w, W + 2), rng.integers(-h, H + 2), w, h, off, ink, 0)
    return out


# ------------------------------------------------------------------ kernel geometries
GEOMETRIES = [(TILE_W, TILE_H, 1), (TILE_W + 1, TILE_H + 1, 1), (70, 37, 3), (200, 120, 2)]


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'out+1'])
@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: '%dx%dx%d' % g)
def test_random_primitives_at_every_geometry(geom, shift):
    """One tile exactly, a tile plus one pixel each way, rows of 210 bytes (neither dword- nor 16-byte-aligned), several tiles each way;
    with the output moved one byte off its alignment the dword geometries take the byte-wise path too."""
    W, H, n = geom
    r, masks = _renderer(H, W)
    frames = _frames(n, H, W)
    rng = np.random.default_rng(W * 31 + H)
    prims = [_random_prims(rng, H, W, masks, 40) for _ in range(n)]
    got = _draw(r, frames, prims, shift=shift)
    for i in range(n):
        np.testing.assert_array_equal(got[i], render_ref.paint_records(frames[i], prims[i], masks), err_msg='frame %d' % i)
        assert (got[i] != frames[i]).any()


# ------------------------------------------------------------------ per kind
def _one_by_one(W, H, recs, masks=None):
    """Each record alone on its own frame, one launch -> (got, want) lists."""
    r, atlas = _renderer(H, W)
    frames = _frames(1, H, W)
    prims = [np.asarray(q, dtype=np.int32).reshape(1, 8) for q in recs]
    got = _draw(r, frames, prims, streams=[0] * len(prims))
    return got, [render_ref.paint_records(frames[0], q, masks or atlas) for q in prims]


def test_rectangles_on_every_edge_and_outside():
    W, H = 70, 37
    ink = 0x10c0f0
    boxes = [(-3, 5, 10, 20), (60, 5, 80, 20), (5, -4, 30, 9), (5, 30, 30, 50), (-5, -5, 75, 40), (-5, -5, 69, 36), (0, 0, 69, 36), (0, 0, 0, 0),
             (69, 36, 69, 36), (5, 5, 5, 5), (5, 5, 6, 5), (5, 36, 9, 36), (63, 15, 64, 16), (10, 15, 60, 15), (-8192, -8192, 8191, 8191),
             (-20, -20, -3, -3), (75, 5, 90, 20), (5, 40, 30, 60), (-30, 5, -1, 20), (10, -1, 20, -1)]
    got, want = _one_by_one(W, H, [(0,) + b + (0, ink, 0) for b in boxes])
    frame = _frames(1, H, W)[0]
    for i, b in enumerate(boxes):
        np.testing.assert_array_equal(got[i], want[i], err_msg=str(b))
    for i in range(15, 19):
        np.testing.assert_array_equal(got[i], frame)                 # fully outside
    assert (got[19] != frame).any()                                  # y1 == y0 == -1 colours row 0 at both ends, as Pillow does
    assert (got[14] == frame).all() and (got[4] == frame).all()     # the canvas lies inside the box


@pytest.mark.parametrize('width', [1, 3, 5, 7, 9, 11, 13, 15])
def test_lines_of_each_odd_width(width):
    """Horizontal, vertical, diagonal, zero-length, with an endpoint at the coordinate limits, and crossing tile borders (x = 64, 128;
    y = 16, 32, ...) of a 200 x 120 canvas."""
    W, H = 200, 120
    segs = [(10, 15, 190, 15), (63, 0, 63, 119), (64, 3, 64, 100), (0, 0, 199, 119), (199, 0, 0, 119), (100, 60, 100, 60), (0, 0, 0, 0),
            (199, 119, 199, 119), (-8192, -8192, 8191, 8191), (8191, 40, -8192, 41), (50, 8191, 60, -8192), (100, 50, 8191, 8191), (-8192, 16, 64, 16),
            (60, 12, 70, 20), (127, 31, 129, 33), (-5, -5, -1, -1), (300, 50, 210, 60)]
    got, want = _one_by_one(W, H, [(1,) + s + (width, 0x0000ff, 0) for s in segs])
    for i, s in enumerate(segs):
        np.testing.assert_array_equal(got[i], want[i], err_msg=str(s))
    frame = _frames(1, H, W)[0]
    assert int((got[5] != frame).any(axis=-1).sum()) >= {1: 0, 3: 4}.get(width, 8)      # a zero-length segment is a disc (a blue pixel may already be blue)


def test_masks_at_negative_offsets_and_clipped():
    W, H = 70, 37
    r, masks = _renderer(H, W)
    recs = []
    for off, m in masks.items():
        h, w = m.shape
        for x, y in ((10, 10), (-w + 1, 5), (5, -h + 1), (-2, -1), (W - 1, 3), (W - w + 2, H - h + 1), (3, H - 1), (62, 14), (W, 5), (5, H), (-w, 0), (0, -h)):
            recs.append((2, x, y, w, h, off, 0xf0b010, 0))
    assert any(m.shape[1] % 4 for m in masks.values())
    got, want = _one_by_one(W, H, recs)
    changed = 0
    for i, q in enumerate(recs):
        np.testing.assert_array_equal(got[i], want[i], err_msg=str(q))
        changed += int((got[i] != _frames(1, H, W)[0]).any())
    assert changed >= 2 * len(masks)


def test_bad_records_are_refused_before_the_launch():
    from deepdish_amd._lib import DeepDishHipError
    r, masks = _renderer(37, 70)
    dev = r.ctx.to_device(_frames(1, 37, 70))
    off = max(masks)
    for bad in ((0, 5, 5, 4, 9, 0, 0, 0), (1, 0, 0, 5, 5, 2, 0, 0), (1, 0, 0, 5, 5, 17, 0, 0), (1, 0, 0, 9000, 5, 3, 0, 0), (3, 0, 0, 1, 1, 0, 0, 0),
                (2, 0, 0, 4000, 4000, off, 0, 0), (2, 0, 0, 2, 2, -1, 0, 0), (2, 0, 0, 0, 2, 0, 0, 0)):
        with pytest.raises(DeepDishHipError, match='dd_render_draw'):
            r.draw(dev, [np.array([bad], dtype=np.int32)])
    with pytest.raises(DeepDishHipError, match='out of place'):
        r.draw(dev, [np.zeros((0, 8), np.int32)], out=dev)
    from deepdish_amd.render import Renderer
    with pytest.raises(DeepDishHipError, match='canvas'):
        Renderer(8193, 16)


# ------------------------------------------------------------------ order, mixed launch, stream selection
def test_painters_order():
    W, H = 70, 37
    a = (0, 5, 5, 40, 30, 0, 0x0000ff, 0)
    b = (1, 0, 0, 69, 36, 5, 0x00ff00, 0)
    r, masks = _renderer(H, W)
    frames = _frames(1, H, W)
    ab, ba = np.array([a, b], np.int32), np.array([b, a], np.int32)
    got = _draw(r, frames, [ab, ba], streams=[0, 0])
    np.testing.assert_array_equal(got[0], render_ref.paint_records(frames[0], ab, masks))
    np.testing.assert_array_equal(got[1], render_ref.paint_records(frames[0], ba, masks))
    assert (got[0] != got[1]).any()


def test_mixed_launch_300_one_and_no_primitives():
    W, H = 200, 120
    r, masks = _renderer(H, W)
    frames = _frames(3, H, W)
    rng = np.random.default_rng(300)
    prims = [_random_prims(rng, H, W, masks, 300), _random_prims(rng, H, W, masks, 1), np.zeros((0, 8), np.int32)]
    assert len(prims[0]) > CHUNK
    got = _draw(r, frames, prims)
    for i in range(2):
        np.testing.assert_array_equal(got[i], render_ref.paint_records(frames[i], prims[i], masks), err_msg='frame %d' % i)
    np.testing.assert_array_equal(got[2], frames[2])
    # records past the first LDS chunk are painted: the last 44 alone change the frame that the first 256 leave
    assert (got[0] != render_ref.paint_records(frames[0], prims[0][:CHUNK], masks)).any()


def test_stream_selection():
    W, H = 70, 37
    r, masks = _renderer(H, W)
    frames = _frames(3, H, W)
    box = np.array([(0, 3, 3, 30, 30, 0, 0xffffff, 0)], np.int32)
    got = _draw(r, frames, [np.zeros((0, 8), np.int32), box], streams=[2, 0])
    np.testing.assert_array_equal(got[0], frames[2])
    np.testing.assert_array_equal(got[1], render_ref.paint_records(frames[0], box, masks))


# ------------------------------------------------------------------ text
def test_text_equals_pillow_and_strings_are_rasterised_once():
    from PIL import Image, ImageDraw
    from deepdish_amd.render import Renderer
    W, H = 640, 48                                                   # the default font of a 640-wide canvas: size 24
    r = Renderer(H, W)
    frame = _frames(1, H, W)
    spots = ((10, 8), (-7, -5), (W - 20, 10), (30, H - 16), (W - 8, H - 14), (300.9, 4.9))
    for rep in range(2):
        misses = r.cache_misses
        prims = [r.text(x, y, s, (10, 250, 130)) for s in STRINGS for x, y in spots]
        assert r.cache_misses - misses == (len(STRINGS) if rep == 0 else 0) and r.cache_hits > 0
        got = _draw(r, frame, prims, streams=[0] * len(prims))
        for i, (s, (x, y)) in enumerate((s, p) for s in STRINGS for p in spots):
            im = Image.fromarray(np.ascontiguousarray(frame[0][..., ::-1]), 'RGB')
            ImageDraw.Draw(im).text((int(x), int(y)), s, fill=(10, 250, 130), font=r.font)
            np.testing.assert_array_equal(got[i][..., ::-1], np.array(im), err_msg=repr((s, x, y)))
            assert (s == '') == (got[i] == frame[0]).all()


# ------------------------------------------------------------------ pipelines
PIPE_S, PIPE_W, PIPE_H, PIPE_F = 3, 128, 96, 12
ANNOTATIONS = ('label', 'id', 'none')


def _scene_boxes(z, f):
    """Three objects a stream walking across the count line (x = 64): tlwh, one of them against the others' direction."""
    out = []
    for k in range(3):
        x = (22 + 6 * f + 3 * z) if k != 1 else (100 - 5 * f - 2 * z)
        out.append((float(x), float(8 + 28 * k), 14.0, 24.0))
    return out


def _font():
    from PIL import ImageFont
    return ImageFont.load_default(size=9)


@functools.lru_cache(maxsize=None)
def _run_scene(render):
    """12 steps of 3 streams on 128 x 96 noise frames with injected detections -> per step what the checks need."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    font = _font()
    mp = MultiStreamPipeline(PIPE_S, input_size=(PIPE_W, PIPE_H), run_detector=False)
    hps = [HotPath(input_size=(PIPE_W, PIPE_H), run_detector=False) for _ in range(PIPE_S)] if render else []
    steps = []
    for f in range(PIPE_F):
        frames = _frames(PIPE_S, PIPE_H, PIPE_W + f)[:, :, :PIPE_W].copy() if f else np.array(_frames(PIPE_S, PIPE_H, PIPE_W))
        dev = ctx.to_device(frames)
        per = [(_scene_boxes(z, f), ['person'] * 3, [0.9, 0.8, 0.7]) for z in range(PIPE_S)]
        mp.step(dev, mp.pack_injected(per))
        rec = dict(frames=frames, tables=[mp.tracker(z).table() for z in range(PIPE_S)], counts=mp.counts().copy())
        if render:
            rec['overlay'] = mp.overlay()
            for z, hp in enumerate(hps):
                hp.step(dev[z], injected=per[z])
            for a in ANNOTATIONS:
                rec['mp_' + a] = ctx.to_host(mp.render(dev, annotation=a, font=font))
                rec['hp_' + a] = [ctx.to_host(hp.render(dev[z], annotation=a, font=font))[0] for z, hp in enumerate(hps)]
            rec['mp_20'] = ctx.to_host(mp.render(dev, streams=[2, 0], font=font))
        steps.append(rec)
    return steps


def _tlbr(means):
    w = means[:, 2] * means[:, 3]
    x1, y1 = means[:, 0] - w / 2, means[:, 1] - means[:, 3] / 2
    return np.stack([x1, y1, x1 + w, y1 + means[:, 3]], axis=1)


def test_overlay_elements_equal_the_pipeline_s_public_state():
    """dd_pipeline_overlay against the tracker tables, the counters and the injected boxes; and the scene is the one the checks below
    need: a crossing segment, a path of >= 3 points and a non-zero counter in some step."""
    steps = _run_scene(True)
    crossings = longest = 0
    paths = {}
    for f, rec in enumerate(steps):
        for z, o in enumerate(rec['overlay']):
            ints, means = rec['tables'][z]
            drawn = (ints[:, 1] == 2) & (ints[:, 2] <= 1)
            np.testing.assert_array_equal(o['track_ids'], ints[drawn, 0])
            np.testing.assert_array_equal(o['track_tlbr'], _tlbr(means[drawn]))
            assert o['track_labels'] == ['person'] * int(drawn.sum())
            np.testing.assert_array_equal(o['counts'], rec['counts'][z])
            b = np.array(_scene_boxes(z, f))
            np.testing.assert_array_equal(o['det_tlbr'], np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], axis=1))
            at = 0
            for tid, box, n in zip(o['track_ids'], o['track_tlbr'], o['path_counts']):      # the path grows by this step's bottom centre
                pts = o['points'][at:at + n]
                at += n
                np.testing.assert_array_equal(pts[:-1], paths.get((z, tid), np.zeros((0, 2))))
                np.testing.assert_array_equal(pts[-1], [(box[0] + box[2]) / 2, box[3]])
                paths[(z, tid)] = pts
                longest = max(longest, n)
            assert at == len(o['points'])
            for c in o['crossings']:
                assert (c[0] - 64) * (c[2] - 64) <= 0                # the segment spans the line
            crossings += len(o['crossings'])
    assert crossings >= 3 and longest >= 3 and steps[-1]['counts'].sum() > 0
    assert steps[-1]['counts'][:, 0, 2].sum() == crossings           # intcount: every crossing segment was drawn in its step


@pytest.mark.parametrize('annotation', ANNOTATIONS)
def test_pipeline_render_equals_the_restatement_and_the_single_stream_path(annotation):
    steps = _run_scene(True)
    font = _font()
    texts = 0
    for f, rec in enumerate(steps):
        for z, o in enumerate(rec['overlay']):
            at, tracks = 0, []
            for tid, lbl, box, n in zip(o['track_ids'], o['track_labels'], o['track_tlbr'], o['path_counts']):
                tracks.append((int(tid), lbl, box, o['points'][at:at + n]))
                at += n
            counters = [('person', int(rec['counts'][z][0, 1]), int(rec['counts'][z][0, 0]))]
            el = render_ref.overlay_elements(PIPE_W, PIPE_H, o['line'], tracks, o['crossings'], o['det_tlbr'], counters, annotation, font=font)
            want = render_ref.paint(rec['frames'][z], el, font=font)
            np.testing.assert_array_equal(rec['mp_' + annotation][z], want, err_msg='step %d stream %d' % (f, z))
            np.testing.assert_array_equal(rec['hp_' + annotation][z], want, err_msg='single-stream path, step %d stream %d' % (f, z))
            texts += len(tracks)
    assert texts > 0
    last = steps[-1]
    assert (last['mp_label'] != last['mp_none']).any() and (last['mp_label'] != last['mp_id']).any()


def test_pipeline_render_of_selected_streams():
    for rec in _run_scene(True):
        np.testing.assert_array_equal(rec['mp_20'], rec['mp_label'][[2, 0]])


def test_a_pipeline_that_never_renders_is_untouched():
    with_render, without = _run_scene(True), _run_scene(False)
    for a, b in zip(with_render, without):
        for (ia, ma), (ib, mb) in zip(a['tables'], b['tables']):
            np.testing.assert_array_equal(ia, ib)
            np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(a['counts'], b['counts'])
    assert without[-1]['counts'].sum() > 0
