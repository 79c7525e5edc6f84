"""GPU: the uint8 SSD-MobileNet-v2 program (csrc/netsq.hip: q_conv_k's natural bordered epilogue with the residual ADD, q_add_k) against
the test-side integer restatement of TFLite's reference kernels (tests/quant_v2_ref.py).  Integer work: the bar is bit-exact, tensor by
tensor, borders included.  (Parity against a real ssdmobilenetv2.tflite is unpinned: the blob is absent.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_v2_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL = 'synthetic-ssd_mobilenet_v2-uint8.tflite'


def _base_frames():
    """Three distinct inputs: a calibration frame, white noise (every clamp and both signs of every rounding), zeros."""
    from deepdish_amd import quantize
    fr = np.zeros((3, 300, 300, 3), np.uint8)
    fr[0] = quantize.calibration_frames(1, seed=11)[0]
    fr[1] = np.random.default_rng(11).integers(0, 256, (300, 300, 3), dtype=np.uint8)
    return fr


@pytest.fixture(scope='module', params=['asymmetric', 'symmetric'])
def v2(request):
    from deepdish_amd import quantize
    qm = quantize.synthetic_ssd_v2_quant_model(1234, symmetric_weights=request.param == 'symmetric')
    base = _base_frames()
    names = set(qm['layers']) | set(qm['add']) | set(quant_v2_ref.blocks(qm))
    box, cls, kept = quant_v2_ref.ssd_v2_forward(qm, base, keep=names)
    return qm, base, box, cls, kept


def _compile(qm, fuse=True):
    from deepdish_amd import netsq
    old = netsq.ADD_FUSE
    netsq.ADD_FUSE = fuse
    try:
        return netsq.compile_ssd_mobilenet_quant(qm)
    finally:
        netsq.ADD_FUSE = old


def _check_layers(prog, net, n, src_of, kept, where):
    """Every layer tensor of the last forward against the restatement of its slot's input (src_of[slot]), borders included."""
    from deepdish_amd import netsq
    for name, t in prog.meta['layer_tensors'].items():
        d = prog.tensors[t]
        raw = net.read(n, tensor=t)
        got = netsq.unpack_q16(raw, d['h'], d['w'], d['c'])
        want = kept[name][src_of]
        c = want.shape[3]
        bad = int((got[..., :c] != want).sum())
        assert bad == 0, '%s, %s: %d of %d bytes differ' % (where, name, bad, want.size)
        assert (got[..., c:] == d['zp']).all(), '%s, %s: phantom channels do not hold the zero point' % (where, name)
        assert (netsq.borders_q16(raw, d['h'], d['w'], d['c']) == d['zp']).all(), '%s, %s: border overwritten' % (where, name)


def _check_heads(prog, net, n, src_of, box, cls, where):
    got_box = net.read(n, tensor=prog.meta['box_tensor'])[:, :, 0, :]
    got_cls = net.read(n, tensor=prog.meta['cls_tensor'])[:, :, 0, :prog.meta['n_classes']]
    np.testing.assert_array_equal(got_box, box[src_of], err_msg=where)
    np.testing.assert_array_equal(got_cls, cls[src_of], err_msg=where)


def test_every_layer_is_bit_exact(v2):
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches
    qm, base, box, cls, kept = v2
    prog = _compile(qm)
    net = Net(prog, max_batch=91)
    for n in (1, 3, 23, 91):
        src_of = np.arange(n) % 3
        net.forward(base[src_of])
        _check_layers(prog, net, n, src_of, kept, '%d frames' % n)
        _check_heads(prog, net, n, src_of, box, cls, '%d frames' % n)
        codes = net_op_launches(net)
        assert sum(int(c) == 21 for c in codes) == 10, codes                 # ten projections ran with the ADD in their epilogue
    assert len(np.unique(cls)) > 100 and len(np.unique(box)) > 50          # not a degenerate comparison


def test_fused_and_unfused_add_give_the_same_bits(v2):
    from deepdish_amd import netsq
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches
    qm, base, box, cls, kept = v2
    fused, split = _compile(qm, True), _compile(qm, False)
    assert sum(int(o[0]) == netsq.OP_QADD for o in split.ops) == 10 and not any(int(o[0]) == netsq.OP_QADD for o in fused.ops)
    nf, ns = Net(fused, max_batch=5), Net(split, max_batch=5)
    src_of = np.array([0, 1, 2, 1, 0])
    nf.forward(base[src_of])
    ns.forward(base[src_of])
    codes = net_op_launches(ns)
    assert sum(int(c) == 22 for c in codes) == 10, codes                     # q_add_k ran for every block with a residual
    for b in qm['add']:
        tf, ts = fused.meta['layer_tensors'][b], split.meta['layer_tensors'][b]
        np.testing.assert_array_equal(nf.read(5, tensor=tf), ns.read(5, tensor=ts), err_msg=b)
    _check_layers(split, ns, 5, src_of, kept, 'unfused')
    _check_heads(split, ns, 5, src_of, box, cls, 'unfused')


def test_1536_frame_launch():
    """The bench's launch size: b1's 150 x 150 x 96 expansion is 3.4 GB (offsets past 2^31 from frame 969 on).  Picked slots on both sides
    of that limit and the last one against the restatement; every slot against slot (k mod 3) on the device."""
    from deepdish_amd import netsq, quantize
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches
    qm = quantize.synthetic_ssd_v2_quant_model(1234)
    base = _base_frames()
    box, cls, kept = quant_v2_ref.ssd_v2_forward(qm, base, keep=('b1_expand', 'b1_dw', 'b2', 'b13_expand', 'b15', 'conv_last'))
    prog = _compile(qm)
    N = 1536
    net = Net(prog, max_batch=N)
    src_of = np.arange(N) % 3
    x = torch.from_numpy(base).cuda()[torch.from_numpy(src_of).cuda()]
    torch.cuda.synchronize()                                             # (the gather runs on torch's stream, the forward on the engine's)
    net.forward(x)
    codes = net_op_launches(net)
    kinds = [int(o[0]) for o in prog.ops]
    assert all(int(c) == 17 for c, k in zip(codes, kinds) if k == netsq.OP_QDW), 'q_dwm_k runs every depthwise layer'
    assert sum(int(c) == 21 for c in codes) == 10
    picked = [0, 967, 968, 969, 970, 1535]
    for name in ('b1_expand', 'b1_dw', 'b2', 'b13_expand', 'b15', 'conv_last'):
        t = prog.meta['layer_tensors'][name]
        d = prog.tensors[t]
        dev = net.read(N, tensor=t, to_host=False)
        net.ctx.sync()                                                   # (the copy runs on the engine's stream, the comparison on torch's)
        # every slot equals the first slot with the same input, compared on the device
        for r in range(3):
            same = dev[r::3]
            assert bool((same == same[:1]).all()), '%s: slots with input %d differ' % (name, r)
        got = netsq.unpack_q16(dev[picked].cpu().numpy(), d['h'], d['w'], d['c'])
        want = kept[name][src_of[picked]]
        np.testing.assert_array_equal(got[..., :want.shape[3]], want, err_msg=name)
    got_box = net.read(N, tensor=prog.meta['box_tensor'])[:, :, 0, :]
    got_cls = net.read(N, tensor=prog.meta['cls_tensor'])[:, :, 0, :prog.meta['n_classes']]
    np.testing.assert_array_equal(got_box, box[src_of])
    np.testing.assert_array_equal(got_cls, cls[src_of])


def test_row_pipelines_never_take_a_v2_program(v2, monkeypatch):
    """netq_run_front / netq_run_mid match q_conv0_k followed by fused MobileNet-v1 blocks (OP_QDWPW); v2 has none, so its ops run one by
    one at any batch size."""
    from deepdish_amd import netsq
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches
    qm, base, box, cls, kept = v2
    prog = _compile(qm)
    assert not any(int(o[0]) == netsq.OP_QDWPW for o in prog.ops)
    monkeypatch.setenv('DD_Q_FRONT_MIN', '1')
    net = Net(prog, max_batch=3)
    net.forward(base)
    codes = [int(c) for c in net_op_launches(net)]
    assert 19 not in codes and 20 not in codes and 1 not in codes, codes
    _check_heads(prog, net, 3, np.arange(3), box, cls, 'front switch on')


# ------------------------------------------------------------------------------------------- the detector surface
def _labels():
    from deepdish_amd.pipeline import DEFAULT_LABELS
    return {i: l.strip() for i, l in enumerate(open(DEFAULT_LABELS))}


def _scene_frames():
    from deepdish_amd.synth import Scene
    a = Scene(seed=3, n_obj=8, n_frames=4)
    rng = np.random.default_rng(5)
    return [a.frame(0), a.frame(3), rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)]


def _oracle_detect(qm, frame_bgr, wanted, score_threshold=0.5, max_det=10, score_thr=1e-8, iou_thr=0.6):
    """Pillow Lanczos -> the v2 restatement -> the post-process op (oracle/nets_quant.py decode, oracle/nets_torch.py) -> predict()'s
    tail and detect_image()'s filter (oracle/detectors_np.py)."""
    from PIL import Image
    from oracle import nets_quant, nets_torch, detectors_np
    h, w = frame_bgr.shape[:2]
    rgba = np.dstack([frame_bgr[..., ::-1], np.full((h, w, 1), 255, np.uint8)])
    resized = np.asarray(Image.fromarray(rgba, 'RGBA').convert('RGB').resize((300, 300), Image.LANCZOS))
    box_q, cls_q, _ = quant_v2_ref.ssd_v2_forward(qm, resized[None])
    b, s, c, _ = nets_quant.ssd_quant_decode(qm, box_q[0], cls_q[0], nets_quant.ssd_anchors(300), score_thr)
    op = nets_torch.ssd_postprocess_decoded(b, s, c, max_det, score_thr, iou_thr)
    boxes, names, scores = detectors_np.ssd_predict_tail(list(op), _labels(), original_image_size=(w, h))
    return detectors_np.ssd_detect_filter(boxes, names, scores, wanted, score_threshold) + (op,)


def _same(got, want, where):
    assert [str(l) for l in got[1]] == [str(l) for l in want[1]], (where, got[1], want[1])
    assert [float(s) for s in got[2]] == [float(s) for s in want[2]], where
    if len(want[0]):
        np.testing.assert_allclose(np.asarray(got[0], np.float64), np.asarray(want[0], np.float64), rtol=0, atol=2e-6 * 640, err_msg=where)


def test_detect_image_equals_the_oracle_chain():
    from PIL import Image
    from deepdish_amd.pipeline import DEFAULT_LABELS
    from deepdish_amd.tools.ssd_mobilenet import SSD_MOBILENET
    wanted = [l for l in _labels().values() if l and l != '???']
    det = SSD_MOBILENET(wanted_labels=wanted, model_file=MODEL, label_file=DEFAULT_LABELS, score_threshold=0.0)
    assert det.ssdm.quantized and det.ssdm.weights['kind'] == 'ssd_mobilenet_v2_uint8'
    qm = det.ssdm.weights
    n_rows = 0
    for k, frame in enumerate(_scene_frames()):
        rgba = np.dstack([frame[..., ::-1], np.full(frame.shape[:2] + (1,), 255, np.uint8)])
        wb, wl, ws, op = _oracle_detect(qm, frame, wanted, score_threshold=0.0)
        out = det.ssdm.invoke_device(det.ssdm.prepare_image_device(torch.from_numpy(rgba).cuda(), 480, 640, 4))
        assert int(out[3]) == op[3], k
        np.testing.assert_array_equal(out[1][:op[3]], op[1][:op[3]])
        np.testing.assert_array_equal(out[2][:op[3]], op[2][:op[3]])
        np.testing.assert_allclose(out[0][:op[3]], op[0][:op[3]], rtol=0, atol=2e-6)
        got = det.detect_image(Image.fromarray(rgba, 'RGBA'))
        g = sorted(zip([str(l) for l in got[1]], [float(s) for s in got[2]]))
        w = sorted(zip([str(l) for l in wl], [float(s) for s in ws]))
        assert g == w, (k, g, w)
        n_rows += len(wl)
    assert n_rows > 0


def test_make_detector_on_a_written_v2_file_and_the_batched_pipeline(tmp_path):
    """A written ...ssdmobilenetv2.tflite goes through tools/tflite_reader.py to the same QModel; the batched pipeline runs its own v2 detector
    and leaves every stream with the track table of a single-stream pipeline on the same file."""
    from deepdish_amd import quantize
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, make_detector
    from deepdish_amd.synth import Scene
    from deepdish_amd.tools import tflite_writer
    qm = quantize.synthetic_ssd_v2_quant_model(77)
    path = str(tmp_path / 'ssdmobilenetv2.tflite')
    tflite_writer.write_ssd_mobilenet_v2(qm, path)
    wanted = sorted({l for l in _labels().values() if l and l != '???'})
    det = make_detector(path, wanted_labels=wanted)
    assert det.ssdm.weights['kind'] == 'ssd_mobilenet_v2_uint8'
    frame = _scene_frames()[0]
    got = det.detect_frame_device(torch.from_numpy(frame).cuda(), 480, 640)
    assert len(got) == 3
    S, F = 4, 4
    scenes = [Scene(seed=20 + z, n_obj=4 + 2 * z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, model=path, wanted_labels=wanted)
    assert mp.det_dtype == 'u8'
    hps = [HotPath(model=path, wanted_labels=wanted) for _ in range(S)]
    for f in range(F):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        mp.step(frames)
        for z in range(S):
            hps[z].step(frames[z])
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hps[z].tracker.tracks], dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg='frame %d stream %d' % (f, z))
