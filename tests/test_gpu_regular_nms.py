"""GPU: TFLite_Detection_PostProcess with use_regular_nms = true (csrc/post_regular.hip) against the test-side restatement
(tests/regular_nms_ref.py): the decoded entry and the uint8 front end bit for bit (rows, classes, scores, count, zero rows past the
count), the f32 front end by the (class, anchor) sequence, box bits and scores within 1e-6; then the plugins and the two pipelines on
model files that state the mode.  (Parity against TensorFlow Lite itself is unpinned: the library is absent.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_nms_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _ctx():
    from deepdish_amd.runtime import default_context
    return default_context()


def _outs(c, batch, max_det):
    # pre-filled: the kernel must write every row, the zero rows included
    return (torch.full((batch, max_det, 4), 7.0, dtype=torch.float32, device='cuda'), torch.full((batch, max_det), 7.0, dtype=torch.float32, device='cuda'),
            torch.full((batch, max_det), 7.0, dtype=torch.float32, device='cuda'), torch.full((batch,), -3, dtype=torch.int32, device='cuda'))


def _host(c, outs):
    c.sync()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def run_decoded(boxes, scores, col0, C, max_det, per_class, thr, iou):
    """boxes f32 [B, A, 4], scores f32 [B, A, ld] -> the op's four outputs on the host."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    c = _ctx()
    B, A, ld = scores.shape
    db, ds = c.to_device(boxes, np.float32), c.to_device(scores, np.float32)
    outs = _outs(c, B, max_det)
    check(lib().dd_ssd_regular_nms_decoded(c.handle, ptr(db), ptr(ds), ld, col0, A, C, max_det, per_class, thr, iou, *[ptr(o) for o in outs], B, None),
          'dd_ssd_regular_nms_decoded')
    return _host(c, outs)


def gpu_decode(raw, anchors):
    """dd_ssd_decode's boxes for raw f32 [B, A, 4 + n]: the bits every front end's rows must carry."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    c = _ctx()
    B, A, cols = raw.shape
    dr, da = c.to_device(raw, np.float32), c.to_device(anchors, np.float32)
    b, s, k = c.empty((B, A, 4), torch.float32), c.empty((B, A), torch.float32), c.empty((B, A), torch.float32)
    cl = c.empty((B, A), torch.int32)
    check(lib().dd_ssd_decode(c.handle, ptr(dr), ptr(da), A, cols - 4, 1e-8, ptr(b), ptr(s), ptr(cl), ptr(k), B, None), 'dd_ssd_decode')
    return c.to_host(b)


# ------------------------------------------------------------------------------------------- decoded entry
def _boxes(rng, A, clustered):
    if clustered:                                             # a dozen centres, small jitter: heavy overlap inside a cluster
        centres = rng.random((12, 2)).astype(np.float32) * np.float32(0.7)
        yx = centres[rng.integers(0, 12, A)] + rng.random((A, 2)).astype(np.float32) * np.float32(0.03)
        hw = np.float32(0.2) + rng.random((A, 2)).astype(np.float32) * np.float32(0.03)
    else:
        yx = rng.random((A, 2)).astype(np.float32) * np.float32(0.7)
        hw = rng.random((A, 2)).astype(np.float32) * np.float32(0.3) + np.float32(0.02)
    return np.concatenate([yx, yx + hw], axis=1).astype(np.float32)


def _case(name):
    """-> dict(boxes [B, A, 4], scores [B, A, ld], col0, C, max_det, per_class, thr, iou).  Scores in steps of 1 / 256: ties within and
    across classes are the normal case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = dict(
        one_class_b70=(65, 1, 70, 1, 1, 1e-8, 0.6, False, 0, 0),
        clustered_b70=(130, 3, 70, 10, 2, 1e-8, 0.6, True, 2, 1),          # a padded score matrix: two leading columns, one trailing
        ssd_shape=(1917, 90, 3, 10, 100, 1e-8, 0.6, True, 1, 0),            # the detector's own shape; one anchor planted under two classes
        big_64=(4096, 90, 1, 64, 100, 0.3, 0.5, True, 0, 0),
        class_cap=(4096, 3, 3, 64, 2, 1e-8, 0.6, False, 0, 0),              # ends by exhaustion: every class is full after two rows
        chain=(1917, 3, 3, 64, 100, 1e-8, 0.6, False, 0, 0),                # ends by exhaustion: one class is one long chain
        all_below=(130, 3, 1, 10, 100, 0.5, 0.6, False, 0, 0),
        few_candidates=(1917, 90, 1, 10, 100, 0.5, 0.6, False, 0, 0),
        iou_one=(1917, 1, 3, 64, 100, 1e-8, 1.0, True, 0, 0),               # IoU > 1 never holds: nothing is suppressed
        nan_and_flat=(130, 3, 3, 10, 100, 1e-8, 0.3, True, 0, 0),
    )[name]
    A, C, B, max_det, per_class, thr, iou, clustered, col0, trail = shape
    ld = col0 + C + trail
    boxes = np.stack([_boxes(rng, A, clustered) for _ in range(B)])
    scores = (rng.integers(0, 257, (B, A, ld)) / 256.0).astype(np.float32)
    if name == 'ssd_shape':
        for z in range(B):
            scores[z, 100 + z, col0 + 5] = scores[z, 100 + z, col0 + 17] = np.float32(1.5)
    if name == 'chain':
        # anchors 0..7: disjoint boxes scored in class 1 (anchor 0 in class 2 as well); every other anchor: one box, jittered, scored in class 0
        scores[:] = 0
        for z in range(B):
            for a in range(8):
                boxes[z, a] = [0.1 * a, 0.1 * a, 0.1 * a + 0.05, 0.1 * a + 0.05]
            boxes[z, 8:, :2] = np.float32(0.3) + rng.random((A - 8, 2)).astype(np.float32) * np.float32(0.002)
            boxes[z, 8:, 2:] = boxes[z, 8:, :2] + np.float32(0.4)
            scores[z, :8, 1] = (rng.integers(1, 257, 8) / 256.0).astype(np.float32)
            scores[z, 0, 2] = np.float32(0.5)
            scores[z, 8:, 0] = (rng.integers(1, 257, A - 8) / 256.0).astype(np.float32)
    if name == 'all_below':
        scores = np.minimum(scores, np.float32(127 / 256.0))
    if name == 'few_candidates':
        scores = np.minimum(scores, np.float32(100 / 256.0))
        for a, cc, s in ((7, 3, 0.75), (7, 80, 0.75), (1900, 0, 0.5), (64, 89, 0.875), (65, 89, 0.875)):
            scores[0, a, cc] = np.float32(s)
    if name == 'nan_and_flat':
        scores[rng.random(scores.shape) < 0.05] = np.nan
        flat = rng.random((B, A)) < 0.1
        boxes[..., 2] = np.where(flat, boxes[..., 0] - np.float32(0.01), boxes[..., 2])
        boxes[0, 5, 2] = boxes[0, 5, 0]                                      # zero area exactly
    return dict(boxes=boxes, scores=scores, col0=col0, C=C, max_det=max_det, per_class=per_class, thr=thr, iou=iou)


CASES = ['one_class_b70', 'clustered_b70', 'ssd_shape', 'big_64', 'class_cap', 'chain', 'all_below', 'few_candidates', 'iou_one', 'nan_and_flat']


@pytest.fixture(scope='module')
def decoded_results():
    """Every case once: (case, the kernel's outputs, the restatement's per image)."""
    out = {}
    for name in CASES:
        k = _case(name)
        got = run_decoded(k['boxes'], k['scores'], k['col0'], k['C'], k['max_det'], k['per_class'], k['thr'], k['iou'])
        want = [R.regular_nms(k['boxes'][z], k['scores'][z][:, k['col0']:k['col0'] + k['C']], k['max_det'], k['per_class'], k['thr'], k['iou'])
                for z in range(len(k['boxes']))]
        out[name] = (k, got, want)
    return out


def _assert_rows_equal(got, want, where):
    gb, gc, gs, gn = got
    for z, w in enumerate(want):
        assert int(gn[z]) == w[3], (where, z, int(gn[z]), w[3])
        np.testing.assert_array_equal(gc[z], w[1], err_msg='%s image %d classes' % (where, z))
        np.testing.assert_array_equal(gs[z].view(np.uint32), w[2].view(np.uint32), err_msg='%s image %d scores' % (where, z))
        np.testing.assert_array_equal(gb[z].view(np.uint32), w[0].view(np.uint32), err_msg='%s image %d boxes' % (where, z))


@pytest.mark.parametrize('name', CASES)
def test_decoded_entry_is_bit_exact(decoded_results, name):
    k, got, want = decoded_results[name]
    _assert_rows_equal(got, want, name)
    n = [w[3] for w in want]
    if name == 'all_below':
        assert n == [0] and not got[0].any() and not got[1].any() and not got[2].any()
    if name == 'few_candidates':
        assert n == [5] and want[0][4] == [(89, 64), (89, 65), (3, 7), (80, 7), (0, 1900)]
    if name == 'class_cap':
        assert n == [6, 6, 6]
    if name == 'chain':
        assert n == [10, 10, 10]                                               # the chain's head, eight disjoint boxes, anchor 0 again


def test_decoded_cases_cover_exhaustion_and_repeated_anchors(decoded_results):
    """The case list cannot silently stop covering: at least two cases end by exhaustion (count < max_detections although more than
    128 pairs were candidates), at least two put one anchor into two rows, images of a batch differ."""
    exhausted, repeated = set(), set()
    for name, (k, got, want) in decoded_results.items():
        for z, w in enumerate(want):
            sc = k['scores'][z][:, k['col0']:k['col0'] + k['C']]
            with np.errstate(invalid='ignore'):
                n_cand = int((sc >= np.float32(k['thr'])).sum())
            if w[3] < k['max_det'] and n_cand > 128:
                exhausted.add(name)
            anchors = [a for _, a in w[4]]
            if len(set(anchors)) < len(anchors):
                repeated.add(name)
        if len(want) > 1:
            assert any(want[0][4] != w[4] for w in want[1:]), name
    assert len(exhausted) >= 2 and {'class_cap', 'chain'} <= exhausted, exhausted
    assert len(repeated) >= 2 and {'ssd_shape', 'chain'} <= repeated, repeated


def test_shapes_outside_the_bounds_are_argument_errors():
    from deepdish_amd._lib import lib
    from deepdish_amd.runtime import ptr
    c = _ctx()
    b, s = c.empty((1, 130, 4), torch.float32), c.empty((1, 130, 300), torch.float32)
    outs = _outs(c, 1, 64)
    call = lambda A, C, md, per, batch: lib().dd_ssd_regular_nms_decoded(c.handle, ptr(b), ptr(s), 300, 0, A, C, md, per, 1e-8, 0.6, *[ptr(o) for o in outs], batch, None)
    for bad in ((64, 3, 10, 100, 1), (4097, 3, 10, 100, 1), (130, 3, 0, 100, 1), (130, 3, 65, 100, 1), (130, 3, 10, 0, 1), (130, 0, 10, 100, 1),
                (130, 257, 10, 100, 1), (130, 3, 10, 100, 0)):
        assert call(*bad) < 0, bad
        assert b'bad shape' in lib().dd_last_error()
    assert call(130, 256, 10, 100, 1) == 0                                     # the stated bounds themselves are taken
    c.sync()


# ------------------------------------------------------------------------------------------- uint8 front end
def _run_u8(box_q, cls_q, lut, quant, anchors, n_classes, max_det, per_class, thr, iou):
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    c = _ctx()
    B, A, stride = cls_q.shape
    dbq, dcq, dl, da = c.to_device(box_q, np.uint8), c.to_device(cls_q, np.uint8), c.to_device(lut, np.uint8), c.to_device(anchors, np.float32)
    q4 = np.asarray(quant, np.float32)
    outs = _outs(c, B, max_det)
    check(lib().dd_ssd_postprocess_regular_u8(c.handle, ptr(dbq), ptr(dcq), stride, ptr(dl), ptr(q4), ptr(da), A, n_classes, max_det, per_class,
                                              thr, iou, *[ptr(o) for o in outs], B, None), 'dd_ssd_postprocess_regular_u8')
    return _host(c, outs)


def _u8_quant(qm):
    from deepdish_amd import quantize
    Lb, Lc, Lo = qm['layers']['box0'], qm['layers']['cls0'], qm['logistic']
    lut = quantize.logistic_table(Lc['out_scale'], Lc['out_zp'], Lo['out_scale'], Lo['out_zp'])
    return lut, [Lb['out_scale'], Lb['out_zp'], Lo['out_scale'], Lo['out_zp']]


def _want_u8(qm, box_q, cls_q, n_classes, anchors, max_det, per_class, thr, iou):
    """The restatement per image, on the boxes dd_ssd_decode gives the dequantised encodings (numpy's exp and the device's expf differ in
    the last bits; the dequantisation itself -- one subtraction, one product -- has one result)."""
    Lb = qm['layers']['box0']
    enc = np.float32(Lb['out_scale']) * (box_q.astype(np.float32) - np.float32(Lb['out_zp']))
    raw = np.concatenate([enc, np.zeros(enc.shape[:2] + (2,), np.float32)], axis=2)
    boxes = gpu_decode(raw, anchors)
    return [R.regular_nms_u8(qm, box_q[z], cls_q[z][:, :n_classes], anchors, max_det, per_class, thr, iou, boxes=boxes[z]) for z in range(len(box_q))]


def test_uint8_front_end_on_seeded_head_bytes_is_bit_exact():
    from deepdish_amd import quantize, nets
    from oracle import nets_quant
    qm = quantize.synthetic_ssd_quant_model(1234)
    lut, quant = _u8_quant(qm)
    np.testing.assert_array_equal(lut, nets_quant.logistic_table(qm['layers']['cls0']['out_scale'], qm['layers']['cls0']['out_zp'],
                                                                   qm['logistic']['out_scale'], qm['logistic']['out_zp']))
    anchors = np.ascontiguousarray(nets.ssd_anchors(300)[0], dtype=np.float32)
    rng = np.random.default_rng(91)
    B, A = 3, len(anchors)
    zp = int(qm['layers']['box0']['out_zp'])
    box_q = np.clip(zp + rng.integers(-30, 31, (B, A, 4)), 0, 255).astype(np.uint8)     # moderate encodings: finite boxes
    cls_q = rng.integers(0, 256, (B, A, 96), dtype=np.uint8)                             # 91 columns in rows of 96 bytes
    for max_det, per_class, thr in ((10, 100, 1e-8), (64, 2, 0.5)):
        got = _run_u8(box_q, cls_q, lut, quant, anchors, 91, max_det, per_class, thr, 0.6)
        want = _want_u8(qm, box_q, cls_q, 91, anchors, max_det, per_class, thr, 0.6)
        _assert_rows_equal(got, want, 'seeded bytes %d/%d' % (max_det, per_class))
        assert all(w[3] > 0 for w in want)
    ties = sum(int(len(set(w[2][:w[3]].tolist())) < w[3]) for w in want)
    assert ties > 0                                                                       # 256 score levels: equal scores are what is seen


def _write(kind, path, post):
    from deepdish_amd import nets, quantize
    from deepdish_amd.tools import tflite_writer
    if kind == 'v1-uint8':
        tflite_writer.write_ssd_mobilenet(quantize.synthetic_ssd_quant_model(1234), path, post=post)
    elif kind == 'v2-uint8':
        tflite_writer.write_ssd_mobilenet_v2(quantize.synthetic_ssd_v2_quant_model(1234), path, post=post)
    else:
        folded = {}
        for name, k, w, b, stride, act in quantize.folded_ssd_layers(nets.synthetic_ssd_weights(1234)):
            folded[name + '/weights'] = w if k == 'conv' else w[:, :, :, None]
            folded[name + '/biases'] = b
        meta = None
        if kind == 'f32-metadata':
            from deepdish_amd.pipeline import DEFAULT_LABELS
            coco = list(filter(len, [l.strip() for l in open(DEFAULT_LABELS)][1:]))
            meta = dict(mean=[127.5], std=[127.5], labels=coco)
        tflite_writer.write_ssd_mobilenet(folded, path, post=post, metadata=meta)
    return path


REGULAR = dict(use_regular_nms=True, detections_per_class=100)


def _labels():
    from deepdish_amd.pipeline import DEFAULT_LABELS
    return {i: l.strip() for i, l in enumerate(open(DEFAULT_LABELS))}


def _wanted():
    return sorted({l for l in _labels().values() if l and l != '???'})


def _scene_frames(n=3):
    from deepdish_amd.synth import Scene
    a, b = Scene(seed=3, n_obj=8, n_frames=4), Scene(seed=11, n_obj=20, n_frames=4)
    return [a.frame(0), b.frame(1), a.frame(3), b.frame(2)][:n]


def _op_rows(ssdm, frame):
    """The post-process op's four outputs for one BGR frame through the plugin's own device stages."""
    out = ssdm.invoke_device(ssdm.prepare_image_device(torch.from_numpy(frame).cuda(), frame.shape[0], frame.shape[1], 3, swap_rb=True))
    return out[0], out[1], out[2], int(out[3])


@pytest.mark.parametrize('kind', ['v1-uint8', 'v2-uint8'])
def test_uint8_front_end_through_a_real_forward_is_bit_exact(tmp_path, kind):
    """Plugin on a written file that states the mode: the op's rows against the restatement on the head tensors the forward left."""
    from deepdish_amd.pipeline import DEFAULT_LABELS
    from deepdish_amd.tools.ssd_mobilenet import SSD_MOBILENET
    path = _write(kind, str(tmp_path / ('ssd_mobilenet_%s.tflite' % kind)), REGULAR)
    det = SSD_MOBILENET(wanted_labels=_wanted(), model_file=path, label_file=DEFAULT_LABELS)
    s = det.ssdm
    assert s.quantized and s.detections_per_class == 100
    meta = s.net.program.meta
    n_rows = 0
    for frame in _scene_frames(2):
        gb, gc, gs, gn = _op_rows(s, frame)
        box_q = s.net.read(1, tensor=meta['box_tensor']).reshape(1, len(s.anchors), 4)
        cls_q = s.net.read(1, tensor=meta['cls_tensor']).reshape(1, len(s.anchors), meta['cls_row'])
        want = _want_u8(s.weights, box_q, cls_q, s.n_classes, s.anchors, s.MAX_DET, 100, s.nms_score_threshold, s.nms_iou_threshold)
        _assert_rows_equal((gb[None], gc[None], gs[None], np.array([gn])), want, kind)
        n_rows += gn
    assert n_rows > 0


# ------------------------------------------------------------------------------------------- f32 front end
def test_f32_front_end_sequence_boxes_and_scores():
    """Logits on a grid of eighths in [-6, 6]: distinct logits give scores >= ~3e-4 apart (far above any expf rounding difference), equal
    logits equal bits -- the order is unambiguous.  Rows are identified by their box bits (dd_ssd_decode's box of the anchor; the
    anchors' boxes are distinct); scores within 1e-6 absolute (f32 sigmoid of |x| <= 6 with a few-ulp expf: <= ~2e-7)."""
    from deepdish_amd import nets
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    c = _ctx()
    anchors = np.ascontiguousarray(nets.ssd_anchors(300)[0], dtype=np.float32)
    rng = np.random.default_rng(6)
    B, A, NC = 3, len(anchors), 91
    raw = np.zeros((B, A, 4 + NC), np.float32)
    raw[..., :4] = (rng.random((B, A, 4)).astype(np.float32) - np.float32(0.5)) * np.float32(2.0)
    raw[..., 4:] = (rng.integers(-48, 49, (B, A, NC)) / 8.0).astype(np.float32)
    boxes = gpu_decode(raw, anchors)
    for max_det, per_class, thr, iou in ((10, 100, 1e-8, 0.6), (64, 3, 0.9, 0.4)):
        dr, da = c.to_device(raw, np.float32), c.to_device(anchors, np.float32)
        outs = _outs(c, B, max_det)
        check(lib().dd_ssd_postprocess_regular(c.handle, ptr(dr), ptr(da), A, NC, max_det, per_class, thr, iou, *[ptr(o) for o in outs], B, None),
              'dd_ssd_postprocess_regular')
        gb, gc, gs, gn = _host(c, outs)
        for z in range(B):
            index = {boxes[z, a].tobytes(): a for a in range(A)}
            assert len(index) == A                                             # distinct boxes: a row names its anchor
            want = R.regular_nms_raw(raw[z], anchors, max_det, per_class, thr, iou, boxes=boxes[z])
            n = int(gn[z])
            assert n == want[3] and n > 0
            seq = [(int(gc[z, j]), index[gb[z, j].tobytes()]) for j in range(n)]     # KeyError: a box that is no anchor's
            assert seq == want[4], (z, seq, want[4])
            np.testing.assert_allclose(gs[z, :n], want[2][:n], rtol=0, atol=1e-6)
            assert not gb[z, n:].any() and not gc[z, n:].any() and not gs[z, n:].any()


# ------------------------------------------------------------------------------------------- plugins and pipelines
def _same_detections(got, want, where):
    assert list(got[1]) == list(want[1]), (where, got[1], want[1])
    np.testing.assert_allclose(np.asarray(got[0], np.float64).reshape(-1, 4), np.asarray(want[0], np.float64).reshape(-1, 4), rtol=0, atol=1e-9, err_msg=where)
    np.testing.assert_array_equal(np.asarray(got[2], np.float64), np.asarray(want[2], np.float64), err_msg=where)


@pytest.mark.parametrize('kind', ['v1-uint8', 'v1-f32'])
def test_plugin_hotpath_and_batched_pipeline_run_the_mode_the_file_states(tmp_path, kind):
    """SSD_MOBILENET, HotPath and MultiStreamPipeline(3 streams) on one written file with use_regular_nms: every stream's adaptor output
    equals the single-frame plugin's on the same frame, track tables equal HotPath's per stream -- and on the same weights the op's rows
    differ from the fast mode's on at least one frame (the mode is routed, not ignored)."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, DEFAULT_LABELS
    from deepdish_amd.synth import Scene
    from deepdish_amd.tools.ssd_mobilenet import SSD_MOBILENET
    wanted = _wanted()
    path = _write(kind, str(tmp_path / ('ssd_mobilenet_%s_regular.tflite' % kind)), REGULAR)
    fast_path = _write(kind, str(tmp_path / ('ssd_mobilenet_%s_fast.tflite' % kind)), None)
    det = SSD_MOBILENET(wanted_labels=wanted, model_file=path, label_file=DEFAULT_LABELS)
    fast = SSD_MOBILENET(wanted_labels=wanted, model_file=fast_path, label_file=DEFAULT_LABELS)
    assert det.ssdm.detections_per_class == 100 and fast.ssdm.detections_per_class is None
    assert det.ssdm.quantized == (kind == 'v1-uint8')
    S, F = 3, 4
    scenes = [Scene(seed=20 + z, n_obj=6 + 4 * z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, model=path, wanted_labels=wanted)
    hps = [HotPath(model=path, wanted_labels=wanted) for _ in range(S)]
    assert hps[0].object_detector.ssdm.detections_per_class == 100
    differs = n_rows = seen = 0
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        dev = torch.from_numpy(frames).cuda()
        mp.step(dev)
        for z in range(S):
            one = det.detect_frame_device(dev[z], 480, 640)
            _same_detections(mp.detections(z), one, 'frame %d stream %d' % (f, z))
            hps[z].step(dev[z])
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hps[z].tracker.tracks], dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(mp.tracker(z).table()[0][:, :5], want, err_msg='frame %d stream %d' % (f, z))
            seen = max(seen, len(want))
            n_rows += len(one[0])
            a, b = _op_rows(det.ssdm, frames[z]), _op_rows(fast.ssdm, frames[z])
            differs += int(a[3] != b[3] or not all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])))
    got = mp.counts()
    for z in range(S):
        np.testing.assert_array_equal(got[z], hps[z].counts())
    for frame in _scene_frames(4):              # (random weights put most top rows into one class: further frames for the comparison of the modes)
        a, b = _op_rows(det.ssdm, frame), _op_rows(fast.ssdm, frame)
        differs += int(a[3] != b[3] or not all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])))
    assert differs > 0 and n_rows > 0 and seen > 0


def test_generic_tflite_adaptor_runs_the_mode_the_file_states(tmp_path):
    """tools/tflite.py's adaptor on an f32 file with metadata: the regular op's rows (dd_ssd_postprocess_regular on the same head
    matrix), and other rows than the fast-NMS copy of the file gives."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    from deepdish_amd.tools.tflite import TFLITE
    wanted = _wanted()
    det = TFLITE(wanted_labels=wanted, model_file=_write('f32-metadata', str(tmp_path / 'efficientdet_regular.tflite'), REGULAR))
    fast = TFLITE(wanted_labels=wanted, model_file=_write('f32-metadata', str(tmp_path / 'efficientdet_fast.tflite'), None))
    d = det.detector
    assert d._per_class == 100 and fast.detector._per_class is None
    differs = 0
    for frame in _scene_frames(3):
        rgb = np.ascontiguousarray(frame[..., ::-1])
        got = det.detect_image(rgb)
        rows = [t.cpu().numpy().copy() for t in (d._boxes, d._classes, d._scores, d._count)]
        outs = _outs(d.ctx, 1, d.MAX_DET)
        check(lib().dd_ssd_postprocess_regular(d.ctx.handle, d.net.output_ptr(), ptr(d._anchors_dev), len(d._anchors), d._n_classes, d.MAX_DET, 100,
                                               d._score_thr, d._iou_thr, *[ptr(o) for o in outs], 1, None), 'dd_ssd_postprocess_regular')
        again = _host(d.ctx, outs)
        for x, y in zip(rows, again):
            np.testing.assert_array_equal(x.reshape(-1), y.reshape(-1))
        assert len(got[0]) > 0
        fast.detect_image(rgb)
        f = fast.detector
        differs += int(not all(np.array_equal(x, t.cpu().numpy()) for x, t in zip(rows, (f._boxes, f._classes, f._scores, f._count))))
    assert differs > 0


def test_fast_nms_files_never_enter_the_new_code():
    """A fast-NMS model: no per-class mode anywhere, and a written fast-NMS file of the same weights gives the rows of
    model='synthetic-ssd_mobilenet_v1' bit for bit (the existing tests cover the fast path itself)."""
    import tempfile
    from deepdish_amd.pipeline import make_detector, DEFAULT_LABELS
    from deepdish_amd.tools.ssd_mobilenet import SSD_MOBILENET
    wanted = _wanted()
    named = make_detector('synthetic-ssd_mobilenet_v1', wanted_labels=wanted)
    assert named.ssdm.detections_per_class is None and named.ssdm._heads_u8 is None
    with tempfile.TemporaryDirectory() as tmp:
        written = SSD_MOBILENET(wanted_labels=wanted, model_file=_write('v1-f32', os.path.join(tmp, 'ssd_mobilenet_v1_fast.tflite'), None),
                                label_file=DEFAULT_LABELS)
    assert written.ssdm.detections_per_class is None
    for frame in _scene_frames(2):
        a, b = _op_rows(named.ssdm, frame), _op_rows(written.ssdm, frame)
        assert a[3] == b[3] and a[3] > 0
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
