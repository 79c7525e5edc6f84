"""GPU: the assembled hot path (crop -> MARS -> tracker -> counts; SSD / YOLO detector plugins)
against the oracle's CPU path on the same seeded frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_graft_smoke():
    import __graft_entry__
    __graft_entry__.smoke()


def test_hot_path_counts_match_oracle():
    """60 frames, 12 objects: identical track ids / states / crossing counts; appearance features
    come from the HIP MARS (f16) on one side and the f32 oracle on the other."""
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    sc = Scene(seed=11, n_obj=12, n_frames=60)
    hp = HotPath(run_detector=False)
    wd = hp.encoder.image_encoder.weights
    otrk = ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60)
    ocnt = cl.CountLine(sc.countline())
    worst = 0.0
    for f in range(60):
        frame = sc.frame(f)
        boxes, scores, _, _ = sc.detections(f)
        inj = ([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores])
        hp.step(torch.from_numpy(frame).cuda(), injected=inj)
        keep = ds.non_max_suppression(boxes, 0.6, scores)
        patches = np.stack([image_np.extract_image_patch(frame, boxes[i], (64, 32)) for i in keep])
        feats = nets_torch.mars_forward(wd, patches)
        otrk.predict(); otrk.update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
        ocnt.step(otrk)
        got = [(t.track_id, t.state, t.time_since_update, t.hits, t.age) for t in hp.tracker.tracks]
        want = [(t.track_id, t.state, t.time_since_update, t.hits, t.age) for t in otrk.tracks]
        assert got == want, f
        if want:
            worst = max(worst, float(np.abs(np.array([t.mean for t in hp.tracker.tracks]) -
                                            np.array([t.mean for t in otrk.tracks])).max()))
    assert worst < 1e-6, worst
    np.testing.assert_array_equal(hp.counts(), ocnt.vector())
    assert hp.counts().sum() > 0
    assert set(hp.timings) >= {'objd', 'feat', 'trak', 'e2e'}


def test_ssd_plugin_vs_oracle():
    from PIL import Image
    from deepdish_amd.pipeline import make_detector, DEFAULT_LABELS
    from deepdish_amd import nets
    from deepdish_amd.synth import Scene
    from oracle import nets_torch, nets_quant, deepsort_np
    det = make_detector('synthetic-ssd_mobilenet_v1.tflite', wanted_labels=[l.strip() for l in open(DEFAULT_LABELS)][1:])
    assert (det.width, det.height) == (300, 300) and det.labels[1] == 'person' and det.use_edgetpu is False
    frame = Scene(seed=3, n_obj=8).frame(0)
    rgba = np.dstack([frame[..., ::-1], np.full(frame.shape[:2] + (1,), 255, np.uint8)])
    img = Image.fromarray(rgba, 'RGBA')                                  # deepdish.py:882
    boxes, labels, scores = det.detect_image(img)
    boxes2, labels2, scores2 = det.detect_frame_device(torch.from_numpy(frame).cuda(), 480, 640)
    assert labels == labels2 and np.allclose(scores, scores2) and np.allclose(boxes, boxes2)
    # oracle: Pillow resize -> f32 torch forward (same f16-rounded weights) -> post-process restatement
    wd = det.ssdm.weights
    resized = np.asarray(img.convert('RGB').resize((300, 300), Image.LANCZOS))
    raw = nets_torch.ssd_forward(wd, resized[None], w16=True)[0]
    ob, oc, osc, n = nets_torch.ssd_postprocess(raw, nets_quant.ssd_anchors())          # the oracle's own anchor generator, not the product's
    out = det.ssdm.invoke_device(det.ssdm.prepare_image_device(torch.from_numpy(rgba).cuda(), 480, 640, 4))
    assert int(out[3]) == n == 10
    # (1) the post-process op by itself: the oracle's restatement applied to the HIP head tensor must pick the SAME ten
    # anchors -- classes identical row by row, boxes and scores equal to f32 rounding (expf vs numpy's exp)
    raw_hip = det.ssdm.net.read()[0, :, 0, :]
    hb, hc, hs, hn = nets_torch.ssd_postprocess(raw_hip, nets_quant.ssd_anchors())
    assert hn == 10
    np.testing.assert_array_equal(out[1], hc)
    np.testing.assert_allclose(out[0], hb, rtol=0, atol=2e-6)
    np.testing.assert_allclose(out[2], hs, rtol=0, atol=2e-6)
    # (2) against the independent f32 forward (f16 activations vs f32): scores within 5e-3; candidates whose scores are
    # closer than that may swap places or fall off the end of the top ten, so rows are matched by (class, box)
    np.testing.assert_allclose(out[2], osc, atol=5e-3)
    matched = 0
    for b, c in zip(out[0], out[1]):
        d = np.abs(ob - b).max(axis=1)
        j = int(np.argmin(d))
        matched += int(d[j] < 5e-3 and oc[j] == c)
    gaps = np.abs(np.diff(np.sort(osc)))
    print('ssd plugin vs f32 oracle: %d of 10 rows matched; smallest score gap among the oracle top ten %.1e' % (matched, gaps.min()))
    assert matched >= 10 - int((gaps < 5e-3).sum()) - 1, matched       # every row not involved in a near-tie (one spare for the 10th / 11th boundary)
    assert len(boxes) > 0 and all(s >= 0.5 for s in scores)


def test_yolov5_plugin_vs_oracle():
    """a12 end to end on a synthetic frame: (1) the plugin's decode + label filter + tlwh conversion applied to the
    HIP head tensor equals the oracle's restatement of tools/yolov5.py:120-146 applied to the SAME tensor, bit for
    bit, over all 25200 rows; (2) against the independent f32 forward every detection whose confidence is clear of
    the threshold is found with the same class, box within 1e-2 (image-normalised) and confidence within 2e-2."""
    from deepdish_amd.pipeline import make_detector
    from deepdish_amd.synth import Scene
    from oracle import nets_torch, nets_quant, image_np, detectors_np
    det = make_detector('synthetic-yolov5s-fp16.tflite', wanted_labels=['person'])
    frame = Scene(seed=4, n_obj=8).frame(0)
    rgb = np.ascontiguousarray(frame[..., ::-1])
    every = [det.labels[i] for i in sorted(det.labels)]
    wanted = every
    for round_ in range(2):        # all labels wanted, then only two of the labels that occur (random weights: any class may)
        det.wanted_labels = wanted
        boxes, labels, scores = det.detect_image(rgb)
        raw_hip = det.net.read()[:, :, 0, :]                             # [1, 25200, 85] as the reference reads it (:109)
        ob, ol, osc = detectors_np.yolov5_detect_tail(raw_hip, det.labels, wanted, 0.25, (640, 480))
        assert len(scores) == len(osc) > (5 if round_ == 0 else 0)
        np.testing.assert_array_equal(np.asarray(boxes, np.float32), np.asarray(ob, np.float32))
        assert labels == ol
        np.testing.assert_array_equal(np.asarray(scores, np.float32), np.asarray(osc, np.float32))
        seen = sorted(set(labels))
        assert round_ == 1 or len(seen) > 2
        wanted = seen[:2]
    assert all(l in wanted for l in labels) and len(labels) < len(osc) + 1
    # (2) independent forward: Pillow-exact resize -> f32 torch forward (same f16-rounded weights) -> reference decode
    resized = image_np.lanczos_resize_u8(rgb, 640, 640)
    raw = nets_torch.yolov5s_forward(det.weights, resized[None], w16=True)[0]
    xyxy, conf, cls = nets_torch.yolov5_decode(raw, 0.25 - 2e-2, 640, 480)
    gb, gs, gc = det._run_device(torch.from_numpy(rgb).cuda(), 480, 640, 3, False)
    assert len(gs) > 20, len(gs)
    norm = np.array([640, 480, 640, 480], np.float32)
    sure = np.flatnonzero(conf > 0.25 + 2e-2)
    assert len(sure) > 15, len(sure)
    worst_b = worst_s = 0.0
    for r in sure:                                                       # every clear oracle detection exists on the HIP side
        same = np.flatnonzero(gc == cls[r])
        assert len(same), r
        d = np.abs((gb[same] - xyxy[r]) / norm).max(axis=1)
        j = same[int(np.argmin(d))]
        worst_b, worst_s = max(worst_b, float(d.min())), max(worst_s, abs(float(gs[j]) - float(conf[r])))
    for j in np.flatnonzero(gs > 0.25 + 2e-2):                           # and every clear HIP detection in the oracle's list
        same = np.flatnonzero(cls == gc[j])
        assert len(same), j
        d = np.abs((xyxy[same] - gb[j]) / norm).max(axis=1)
        worst_b = max(worst_b, float(d.min()))
    print('yolov5 plugin vs f32 oracle: worst box error %.2e (image-normalised), worst confidence error %.2e' % (worst_b, worst_s))
    assert worst_b <= 1e-2 and worst_s <= 2e-2, (worst_b, worst_s)


def test_multistream_pipeline_matches_oracle_per_stream():
    """3 streams batched in C++ == 3 independent oracle runs: track tables and crossing counts."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    S, F = 3, 45
    scenes = [Scene(seed=21 + z, n_obj=10 + 3 * z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=True)
    otrk = [ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for _ in range(S)]
    ocnt = [cl.CountLine(sc.countline()) for sc in scenes]
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        per = []
        for z, sc in enumerate(scenes):
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]))
            keep = ds.non_max_suppression(boxes, 0.6, scores)
            patches = np.stack([image_np.extract_image_patch(frames[z], boxes[i], (64, 32)) for i in keep])
            feats = nets_torch.mars_forward(mp.enc_weights, patches)
            otrk[z].predict()
            otrk[z].update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
            ocnt[z].step(otrk[z])
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per))
        for z in range(S):
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in otrk[z].tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in otrk[z].tracks]), rtol=1e-6, atol=1e-6)
    got = mp.counts()
    for z in range(S):
        np.testing.assert_array_equal(got[z], ocnt[z].vector())
    assert got.sum() > 0
    assert mp.stage_ms()['steps'] == F


def test_multistream_detector_output_matches_plugin():
    """Without injection the C++ pipeline consumes the detector's own output: same boxes as the
    Python plugin produces for the same frame -> same tracks after a few frames."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    from deepdish_amd.pipeline import DEFAULT_LABELS
    wanted = sorted({l.strip() for l in open(DEFAULT_LABELS)} - {'???'})
    sc = Scene(seed=3, n_obj=8, n_frames=6)
    seen = 0
    mp = MultiStreamPipeline(1, wanted_labels=wanted)
    hp = HotPath(wanted_labels=wanted)
    for f in range(6):
        fr = torch.from_numpy(sc.frame(f)).cuda()
        mp.step(fr[None])
        hp.step(fr)
        ints, means = mp.tracker(0).table()
        want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hp.tracker.tracks],
                        dtype=np.int64).reshape(-1, 5)
        np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f}')
        if len(want):
            np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-9, atol=1e-9)
        seen = max(seen, len(want))
    assert seen > 0


def test_multistream_yolov5_pipeline_matches_plugin():
    """BASELINE config 3 in the batched C++ pipeline (--model *yolov5*, deepdish.py:482-502): Lanczos to 640x640,
    YOLOv5s forward with the fused Detect decode, batched dd_yolov5_decode, label filter + tlwh (tools/yolov5.py:
    120-146), then box hygiene, deep_sort NMS over the (many) candidates, crops, MARS, tracker.  Two streams batched in
    C++ must equal two single-stream Python pipelines built from the reference-shaped YOLOV5 plugin, frame by frame."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, DEFAULT_YOLO_LABELS
    from deepdish_amd.synth import Scene
    wanted = sorted({l.strip() for l in open(DEFAULT_YOLO_LABELS)})
    scenes = [Scene(seed=3, n_obj=8, n_frames=4), Scene(seed=5, n_obj=5, n_frames=4)]
    mp = MultiStreamPipeline(2, model='synthetic-yolov5s-fp16.tflite', wanted_labels=wanted)
    hps = [HotPath(model='synthetic-yolov5s-fp16.tflite', wanted_labels=wanted) for _ in scenes]
    seen = 0
    for f in range(4):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        mp.step(frames)
        for z, hp in enumerate(hps):
            hp.step(frames[z])
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hp.tracker.tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-9, atol=1e-9)
            seen = max(seen, len(want))
    assert seen > 3, seen


def test_multistream_generic_tflite_pipeline_matches_plugin():
    """a13 in the batched C++ pipeline: a --model name with 'tflite' but neither 'yolo' nor 'mobilenet' selects the generic
    TFLite-Task adaptor (deepdish.py:493-495): cv2 bilinear stretch of the RGB frame, SSD forward, post-process op, then
    tflite_object_detector.py:234-295 + tools/tflite.py:26-41 (score >= 0.5, int() corners, stable sort by score, wanted
    labels).  Three streams batched in C++ == three single-stream Python pipelines built from the TFLITE plugin."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, DEFAULT_LABELS
    from deepdish_amd.synth import Scene
    wanted = sorted({l.strip() for l in open(DEFAULT_LABELS)} - {'???'})
    model = 'synthetic-efficientdet_lite0.tflite'
    scenes = [Scene(seed=3, n_obj=8, n_frames=5), Scene(seed=5, n_obj=5, n_frames=5), Scene(seed=9, n_obj=8, n_frames=5)]
    mp = MultiStreamPipeline(3, model=model, wanted_labels=wanted)
    assert mp.kind == 'tflite'
    hps = [HotPath(model=model, wanted_labels=wanted) for _ in scenes]
    assert type(hps[0].object_detector).__name__ == "TFLITE"
    seen = 0
    for f in range(5):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        mp.step(frames)
        for z, hp in enumerate(hps):
            hp.step(frames[z])
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hp.tracker.tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-9, atol=1e-9)
            seen = max(seen, len(want))
    assert seen > 0, seen


def test_detector_and_encoder_run_concurrently_on_two_contexts():
    """SURVEY 8(b) threading: the reference keeps ONE detector call and ONE encoder call in flight on different pool
    threads (deepdish.py:935,985,1008).  Two host threads, each with its own dd_ctx (own stream, own scratch), hammer
    the SSD forward + post-process and the MARS forward at the same time: every result equals the single-threaded one."""
    import threading
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    from deepdish_amd.runtime import Context
    from deepdish_amd.pipeline import make_detector, DEFAULT_LABELS
    from deepdish_amd.tools import generate_detections as gdet
    from deepdish_amd.synth import Scene
    names = [l.strip() for l in open(DEFAULT_LABELS)][1:]
    ctx_d, ctx_e = Context(0), Context(0)
    det = make_detector('synthetic-ssd_mobilenet_v1.tflite', wanted_labels=names, context=ctx_d)
    enc = gdet.create_box_encoder('synthetic-mars-64x32x3', batch_size=32, context=ctx_e)
    sc = Scene(seed=12, n_obj=10, n_frames=8)
    frames = [sc.frame(f) for f in range(8)]
    boxes = [sc.detections(f)[0] for f in range(8)]
    want_d = [det.detect_frame_device(torch.from_numpy(fr).cuda(), 480, 640) for fr in frames]
    want_e = [enc(fr, [b for b in bx]) for fr, bx in zip(frames, boxes)]
    got_d, got_e, errs = [], [], []

    def run_d():
        try:
            for _ in range(6):
                got_d.append([det.detect_frame_device(torch.from_numpy(fr).cuda(), 480, 640) for fr in frames])
        except Exception as e:                       # surfaces in the main thread below
            errs.append(e)

    def run_e():
        try:
            for _ in range(6):
                got_e.append([enc(fr, [b for b in bx]) for fr, bx in zip(frames, boxes)])
        except Exception as e:
            errs.append(e)

    th = [threading.Thread(target=run_d), threading.Thread(target=run_e)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for rep in got_d:
        for (b, l, s), (wb, wl, ws) in zip(rep, want_d):
            assert l == wl and np.array_equal(np.asarray(b), np.asarray(wb)) and np.array_equal(np.asarray(s), np.asarray(ws))
    for rep in got_e:
        for g, w in zip(rep, want_e):
            np.testing.assert_array_equal(g, w)


def test_tflite_plugin_vs_oracle():
    """a13: generic TFLite-Task adaptor = cv2 bilinear stretch + SSD forward + post-process + int() boxes."""
    from deepdish_amd.pipeline import make_detector, DEFAULT_LABELS
    from deepdish_amd.synth import Scene
    from oracle import nets_torch, nets_quant, image_np
    names = [l.strip() for l in open(DEFAULT_LABELS)]
    wanted = sorted(set(names) - {'???'})
    det = make_detector('synthetic-efficientdet_lite0.tflite', wanted_labels=wanted)
    assert type(det).__name__ == 'TFLITE' and det.labels[1] == 'person' and (det.width, det.height) == (300, 300)
    rgb = np.ascontiguousarray(Scene(seed=9, n_obj=8).frame(0)[..., ::-1])
    boxes, labels, scores = det.detect_image(rgb)
    resized = image_np.resize_linear_u8(rgb, 300, 300)
    raw = nets_torch.ssd_forward(det.detector.weights, resized[None], w16=True)[0]
    ob, oc, osc, n = nets_torch.ssd_postprocess(raw, nets_quant.ssd_anchors())
    want = []
    for i in range(n):
        if osc[i] >= 0.5:
            y0, x0, y1, x1 = ob[i]
            want.append(([int(x0 * 640), int(y0 * 480), int(x1 * 640) - int(x0 * 640), int(y1 * 480) - int(y0 * 480)],
                         names[int(oc[i]) + 1], float(osc[i])))
    want.sort(key=lambda t: -t[2])
    assert len(boxes) == len(want) > 0
    hits = 0
    for b, l, s in zip(boxes, labels, scores):
        for wb, wl, ws in want:
            if l == wl and abs(s - ws) < 5e-3 and max(abs(np.array(b) - np.array(wb))) <= 2:
                hits += 1
                break
    assert hits >= len(want) - 2, (hits, len(want))
    assert all(isinstance(v, int) for v in boxes[0])
    assert list(scores) == sorted(scores, reverse=True)


def test_tflite_plugin_takes_labels_and_normalisation_from_the_model_file(tmp_path):
    """TFLITE(model_file=...) as deepdish.py:497-499 constructs it, with NO label file: mean / std and the label list come from the model
    file's metadata (tools/tflite_object_detector.py:117-137, tools/tflite.py:16-23 upstream).  A file whose metadata states the defaults
    and the COCO names detects what the synthetic model + label file detect; other label names come out as the file states them; a
    file without metadata is refused unless a label file makes up for it."""
    from deepdish_amd import nets, quantize
    from deepdish_amd.pipeline import DEFAULT_LABELS
    from deepdish_amd.synth import Scene
    from deepdish_amd.tools import tflite_writer, tflite_reader
    from deepdish_amd.tools.tflite import TFLITE
    names = [l.strip() for l in open(DEFAULT_LABELS)]
    coco = list(filter(len, names[1:]))
    wanted = sorted(set(coco) - {'???'})
    wd = nets.synthetic_ssd_weights(1234)
    folded = {}
    for name, kind, w, b, stride, act in quantize.folded_ssd_layers(wd):
        folded[name + '/weights'] = w if kind == 'conv' else w[:, :, :, None]
        folded[name + '/biases'] = b
    rgb = np.ascontiguousarray(Scene(seed=9, n_obj=8).frame(0)[..., ::-1])
    ref = TFLITE(wanted_labels=wanted, model_file='synthetic-efficientdet_lite0.tflite', label_file=DEFAULT_LABELS)
    want = ref.detect_image(rgb)
    assert len(want[0]) > 0
    p1 = str(tmp_path / 'efficientdet_lite0.tflite')
    tflite_writer.write_ssd_mobilenet(folded, p1, metadata=dict(mean=[127.5], std=[127.5], labels=coco))
    det = TFLITE(wanted_labels=wanted, model_file=p1)                                  # no label_file: the reference passes none either
    assert det.label_list == coco and det.labels[1] == coco[0] and (det.detector._mean, det.detector._std) == (127.5, 127.5)
    got = det.detect_image(rgb)
    assert got[1] == want[1] and got[0] == want[0]
    np.testing.assert_allclose(np.asarray(got[2], np.float64), np.asarray(want[2], np.float64), rtol=0, atol=2e-3)      # (folded weights through f32 on disk)
    # the label list is the file's: other names, same rows
    other = ['label-%d' % i for i in range(len(coco))]
    p2 = str(tmp_path / 'other-names.tflite')
    tflite_writer.write_ssd_mobilenet(folded, p2, metadata=dict(mean=[127.5], std=[127.5], labels=other))
    det2 = TFLITE(wanted_labels=other, model_file=p2, label_file=DEFAULT_LABELS)       # (a label file is ignored when the model carries metadata)
    got2 = det2.detect_image(rgb)
    assert got2[0] == want[0] and got2[1] == [other[coco.index(l)] for l in want[1]]
    # another normalisation changes what the network sees
    p3 = str(tmp_path / 'other-norm.tflite')
    tflite_writer.write_ssd_mobilenet(folded, p3, metadata=dict(mean=[100.0], std=[160.0], labels=coco))
    det3 = TFLITE(wanted_labels=wanted, model_file=p3)
    assert (det3.detector._mean, det3.detector._std) == (100.0, 160.0)
    got3 = det3.detect_image(rgb)
    assert got3[0] != want[0] or got3[1] != want[1] or list(got3[2]) != list(want[2])
    # no metadata: refused without a label file, taken with one
    p4 = str(tmp_path / 'plain.tflite')
    tflite_writer.write_ssd_mobilenet(folded, p4)
    with pytest.raises(tflite_reader.UnsupportedModel):
        TFLITE(wanted_labels=wanted, model_file=p4)
    got4 = TFLITE(wanted_labels=wanted, model_file=p4, label_file=DEFAULT_LABELS).detect_image(rgb)
    assert got4[0] == want[0] and got4[1] == want[1]


def test_fake_encoders_vs_reference_statements():
    """DummyImageEncoder / ConstantImageEncoder (generate_detections.py:86-116), restated inline."""
    from deepdish_amd.tools.generate_detections import create_box_encoder
    from oracle import image_np
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    frame[100:200, 100:150] = 128                                   # a zero-norm patch after the -128 shift
    boxes = [np.array(b) for b in ([30, 40, 25, 60], [300, 200, 40, 90], [110, 110, 20, 40])]
    enc = create_box_encoder('dummy-encoder')
    assert (enc.width, enc.height) == (8, 16)
    got = enc(frame, boxes)
    patches = np.stack([image_np.extract_image_patch(frame, b, (16, 8)) for b in boxes])
    mat = np.average(np.array(patches, dtype=np.float32), axis=3).reshape((-1, 128)) - 128
    want = np.zeros_like(mat)
    for i in range(len(mat)):
        l = np.sqrt(np.sum(mat[i] ** 2, axis=0))
        if l == 0:
            want[i] = mat[i]; want[i, 0] = 1
        else:
            want[i] = mat[i] / l
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    assert got[2, 0] == 1.0 and not got[2, 1:].any()
    const = create_box_encoder('constant-encoder')(frame, boxes)
    assert const.shape == (3, 128) and np.all(const[:, 0] == 1) and not const[:, 1:].any()
    assert create_box_encoder('dummy')(frame, []).shape == (0,)


def test_yolo_candidates_through_nms_and_tracker():
    """Config 3 shape: YOLOv5 rows (no NMS in the adaptor) -> deep_sort NMS over a few hundred
    candidates (general NMS path) == oracle NMS on the same boxes -> encoder -> tracker step."""
    from deepdish_amd.pipeline import HotPath, clean_boxes, DEFAULT_YOLO_LABELS
    from deepdish_amd.deep_sort import preprocessing
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds
    wanted = [l.strip() for l in open(DEFAULT_YOLO_LABELS)]
    hp = HotPath(model='synthetic-yolov5s-fp16.tflite', wanted_labels=wanted)
    sc = Scene(seed=4, n_obj=8)
    frame = torch.from_numpy(sc.frame(0)).cuda()
    b0, l0, s0 = hp.object_detector.detect_frame_device(frame, 480, 640)
    assert len(b0) > 64                                              # exercises the rank + lazy NMS kernels
    boxes, labels, scores = clean_boxes(b0, l0, s0, 640, 480)
    keep = preprocessing.non_max_suppression(np.array(boxes), 0.6, np.array(scores))
    assert keep == ds.non_max_suppression(np.array(boxes), 0.6, np.array(scores))
    assert 0 < len(keep) < len(boxes)
    for f in range(3):
        hp.step(torch.from_numpy(sc.frame(f)).cuda())
    assert len(hp.tracker.tracks) > 0


def test_multistream_720p_streams():
    """Config 5 shape: 1280x720 streams, one tracker each, counts vector per stream."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    S, F = 2, 12
    scenes = [Scene(seed=40 + z, n_obj=12, width=1280, height=720, n_frames=F, vmax=6.0) for z in range(S)]
    mp = MultiStreamPipeline(S, input_size=(1280, 720))
    otrk = [ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for _ in range(S)]
    ocnt = [cl.CountLine(sc.countline()) for sc in scenes]
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        per = []
        for z, sc in enumerate(scenes):
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]))
            keep = ds.non_max_suppression(boxes, 0.6, scores)
            patches = np.stack([image_np.extract_image_patch(frames[z], boxes[i], (64, 32)) for i in keep])
            feats = nets_torch.mars_forward(mp.enc_weights, patches)
            otrk[z].predict()
            otrk[z].update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
            ocnt[z].step(otrk[z])
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per))
    for z in range(S):
        ints, _ = mp.tracker(z).table()
        want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in otrk[z].tracks], dtype=np.int64)
        np.testing.assert_array_equal(ints[:, :5], want.reshape(-1, 5))
        np.testing.assert_array_equal(mp.counts()[z], ocnt[z].vector())


def test_multistream_ragged_and_empty_inputs():
    """Streams with no detections, one detection, and detections that vanish mid-run; a frame with no
    detections anywhere; NaN boxes (the whole frame's boxes are dropped, deepdish.py:947)."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    S, F = 3, 14
    sc = Scene(seed=77, n_obj=6, n_frames=F, p_miss=0.0, churn=False)
    mp = MultiStreamPipeline(S, run_detector=False)
    otrk = [ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for _ in range(S)]
    for f in range(F):
        frame = sc.frame(f)
        boxes, scores, _, _ = sc.detections(f)
        full = ([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores])
        per = [full if f not in (5, 6) else ([], [], []),              # stream 0: nothing on frames 5-6
               ([], [], []),                                            # stream 1: never anything
               (full[0][:1], full[1][:1], full[2][:1]) if f < 9 else ([], [], [])]   # stream 2: one box, then gone
        if f == 3:                                                      # NaN anywhere -> every box of that stream dropped
            per[0] = ([(float('nan'), 1.0, 2.0, 3.0)] + full[0], ['person'] + full[1], [0.9] + full[2])
        frames = np.stack([frame] * S)
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per))
        for z in range(S):
            b, l, s = per[z]
            if f == 3 and z == 0:
                b, l, s = [], [], []
            bb = np.array(b, dtype=np.int64).reshape(-1, 4)
            keep = ds.non_max_suppression(bb, 0.6, np.array(s)) if len(b) else []
            dets = []
            if keep:
                patches = np.stack([image_np.extract_image_patch(frame, bb[i], (64, 32)) for i in keep])
                feats = nets_torch.mars_forward(mp.enc_weights, patches)
                dets = [ds.Det(bb[i], 'person', s[i], feats[j]) for j, i in enumerate(keep)]
            otrk[z].predict(); otrk[z].update(dets)
            ints, _ = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in otrk[z].tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
    assert len(otrk[1].tracks) == 0 and len(otrk[0].tracks) > 0


def test_clean_boxes_and_hygiene_in_cpp_match():
    """Oversized / out-of-frame / fractional boxes go through the same int(clip()) path in the Python
    harness and in the C++ pipeline: both feed the tracker identical integer boxes."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    frame = Scene(seed=8, n_obj=5).frame(0)
    weird = ([(-10.5, 20.7, 60.2, 130.9), (600.0, 400.0, 100.0, 200.0), (0.0, 0.0, 639.0, 479.0), (100.2, 100.9, 40.5, 90.5)],
             ['person'] * 4, [0.9, 0.8, 0.7, 0.6])
    mp = MultiStreamPipeline(1, run_detector=False)
    hp = HotPath(run_detector=False)
    fr = torch.from_numpy(frame).cuda()
    for _ in range(4):
        mp.step(fr[None], mp.pack_injected([weird]))
        hp.step(fr, injected=weird)
    ints, means = mp.tracker(0).table()
    want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hp.tracker.tracks], dtype=np.int64)
    np.testing.assert_array_equal(ints[:, :5], want)
    np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-12, atol=1e-12)
    assert len(want) == 3                                               # the 639x479 box exceeds 90 % of the frame


def test_detector_lookahead_gives_the_same_results():
    """step(frames, frames_next=...) queues the next detector run on the detector stream; detections, tracks and
    counts must not depend on it (no injection here: the tracker is fed by the detector's own output)."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 3, 8
    scenes = [Scene(seed=120 + z, n_obj=10, n_frames=F) for z in range(S)]
    labels = [l.strip() for l in open(__import__('deepdish_amd.pipeline', fromlist=['DEFAULT_LABELS']).DEFAULT_LABELS)][1:]
    frames = [torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda() for f in range(F)]
    res = []
    for ahead in (False, True):
        mp = MultiStreamPipeline(S, wanted_labels=labels)
        for f in range(F):
            mp.step(frames[f], None, frames[f + 1] if ahead and f + 1 < F else None)
        res.append(([mp.tracker(z).table() for z in range(S)], mp.counts()))
    seen = 0
    for z in range(S):
        np.testing.assert_array_equal(res[0][0][z][0], res[1][0][z][0])
        np.testing.assert_array_equal(res[0][0][z][1], res[1][0][z][1])
        seen += len(res[0][0][z][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert seen > 0


def test_host_path_reports_crossings_and_resumes_from_its_log(tmp_path):
    """deepdish.py:1116-1123,1147-1166,545-561: one MQTT message + one log line per crossing, carrying the counters
    after the update; --restore-from-log brings counters and frame count back."""
    import json
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    sc = Scene(seed=11, n_obj=12, n_frames=60)
    path = str(tmp_path / 'dd.log')
    sent = []
    hp = HotPath(run_detector=False, log=path, mqtt_publish=lambda topic, msg: sent.append(json.loads(msg)), mqtt_acp_id='dd-test')
    for f in range(60):
        boxes, scores, _, _ = sc.detections(f)
        inj = ([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores])
        hp.step(torch.from_numpy(sc.frame(f)).cuda(), injected=inj, t_frame=1000.0 + f / 25)
    pos, neg, tot, dele = hp.counts()[0]
    assert tot > 0 and len(sent) == tot
    assert [m['acp_event_value'] for m in sent].count('pos') == pos and [m['acp_event_value'] for m in sent].count('neg') == neg
    assert [m['intcount_person'] for m in sent] == sorted(m['intcount_person'] for m in sent)      # counters only grow
    assert (sent[-1]['poscount_person'], sent[-1]['negcount_person'], sent[-1]['diff_person']) == (pos, neg, pos - neg)
    lines = [json.loads(l) for l in open(path)]
    assert len(lines) == tot and lines[-1]['intcount_person'] == tot and 1 <= lines[-1]['frame_count'] <= 60
    hp.sink.heartbeat(now=2000.0)
    hp2 = HotPath(run_detector=False, log=path, restore_from_log=True)
    np.testing.assert_array_equal(hp2.counts(), hp.counts())
    assert hp2.frame_count == 60


def _bench_two_ranks(extra_env):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR')}
    env.update(extra_env)
    args = ['--streams', '8', '--groups', '2', '--steps', '6', '--warmup', '2', '--no-cpu-baseline']
    two = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2'] + args, capture_output=True, text=True, env=env, timeout=900)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, two.stdout
    out2 = json.loads(lines[0])
    assert out2['n_gpus'] == 2 and out2['config']['frames_per_step'] == 16 and out2['value'] > 0
    singles = []
    for rank in (0, 1):              # the same streams (seeds 1000 * rank + s) run as two single-GPU jobs
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py')] + args, capture_output=True, text=True,
                           env=dict(env, DD_BENCH_SEED_RANK=str(rank)), timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        singles.append(json.loads(r.stdout.strip().splitlines()[-1])['counts_pos_neg_int_del'])
    assert out2['counts_pos_neg_int_del'] == [a + b for a, b in zip(*singles)]
    assert sum(out2['counts_pos_neg_int_del']) >= 0


def test_bench_two_ranks_rehearsed_on_one_gpu():
    """The N > 1 path of bench.py with real GPU compute on a one-GPU box: `--gpus 2` spawns two ranks (both mapped to
    device 0, count reduction over gloo because RCCL refuses two ranks on one device), each with two worker threads;
    one JSON line, n_gpus == 2, and the reduced crossing counts equal the sum of the two ranks run as single-GPU jobs."""
    _bench_two_ranks({'DD_BENCH_ONE_DEVICE': '1', 'DD_BENCH_BACKEND': 'gloo'})


def test_bench_two_ranks_on_two_gpus():
    """the same over RCCL with one GPU per rank -- per-rank device selection, worker threads on LOCAL_RANK 1.
    Needs two GPUs (the round's GPU box has one: skipped there; the driver's scaling run exercises it)."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    _bench_two_ranks({})


@pytest.mark.parametrize('S', [1536, 3072])
def test_multistream_pipeline_at_bench_scale_matches_oracle_per_stream(S):
    """The batched pipeline at the bench's shapes: S = 1 536 streams (one worker group of the headline; encoder engine 32 x S = 49 152
    crops) and 3 072 (--groups 1; 98 304), bench.N_OBJ objects a scene, injected detections, 5 frames.  The step's frame buffer is
    921 600 bytes a stream, so the crops of streams from 2 331 on read above byte 2^31 (stream 2 330 straddles it); the encoder's
    launch holds ~20 x S crops, and NMS runs over S problems at once.  Streams 0, 1, S/2, 2 330, 2 331, S-1: track tables and counts
    of test_multistream_pipeline_matches_oracle_per_stream's oracle chain."""
    import bench
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    F = 5
    scenes = [Scene(seed=z, n_obj=bench.N_OBJ, n_frames=F) for z in range(S)]
    picks = sorted({z for z in (0, 1, S // 2, 2330, 2331, S - 1) if z < S})
    mp = MultiStreamPipeline(S, run_detector=False)
    assert mp.enc.max_batch == 32 * S
    otrk = {z: ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for z in picks}
    ocnt = {z: cl.CountLine(scenes[z].countline()) for z in picks}
    n_crops = seen = 0
    for f in range(F):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        per = []
        for z, sc in enumerate(scenes):
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]))
            n_crops += len(boxes)
            if z in otrk:
                frame = frames[z].cpu().numpy()
                keep = ds.non_max_suppression(boxes, 0.6, scores)
                patches = np.stack([image_np.extract_image_patch(frame, boxes[i], (64, 32)) for i in keep])
                feats = nets_torch.mars_forward(mp.enc_weights, patches)
                otrk[z].predict()
                otrk[z].update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
                ocnt[z].step(otrk[z])
        mp.step(frames, mp.pack_injected(per))
        del frames
        for z in picks:
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in otrk[z].tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                seen += 1
                np.testing.assert_allclose(means, np.array([t.mean for t in otrk[z].tracks]), rtol=1e-6, atol=1e-6)
    got = mp.counts()
    for z in picks:
        np.testing.assert_array_equal(got[z], ocnt[z].vector())
    assert mp.stage_ms()['steps'] == F
    assert n_crops > 15 * S * F and seen >= 3 * len(picks)             # ~bench.N_OBJ crops a stream and frame went through one launch
