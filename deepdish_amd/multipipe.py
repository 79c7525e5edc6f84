"""Multi-stream hot path on one GPU (csrc/pipeline.hip): S independent DeepDish streams advanced one
frame each per step, device work batched across streams.  Mirrors `pipeline.HotPath` (one stream,
reference-shaped Python objects) but keeps the per-frame orchestration in C++."""
import ctypes
import os
import numpy as np

from ._lib import lib, check, P
from .runtime import default_context, ptr
from . import nets, netsq
from .engine import Net
from .pipeline import DEFAULT_LABELS, DEFAULT_YOLO_LABELS
from .deep_sort.nn_matching import metric_kind as _metric_kind
from .deep_sort.tracker import association_kind as _association_kind, _association_stats
from .tools.weights_io import load_named_weights, load_ssd_model, load_mars_weights, load_yolov5_weights, ssd_post_options


class _TrackerView:
    """Read-only view of one stream's C++ tracker (for parity tests)."""

    def __init__(self, handle):
        self._h = handle

    def table(self):
        n = ctypes.c_int()
        check(lib().dd_tracker_count(self._h, 0, ctypes.byref(n)))
        ints = np.zeros((n.value, 6), dtype=np.int64)
        means = np.zeros((n.value, 8), dtype=np.float64)
        if n.value:
            check(lib().dd_tracker_read(self._h, 0, ptr(ints), ptr(means), None))
        return ints, means

    def gallery(self, track_id):
        """Test aid: (rows f32 [n, 128] of one live track's gallery in storage order, samples appended so far)."""
        n, total = ctypes.c_int(), ctypes.c_int()
        check(lib().dd_tracker_gallery_read(self._h, int(track_id), None, 0, ctypes.byref(n), ctypes.byref(total)), 'dd_tracker_gallery_read')
        rows = np.zeros((n.value, 128), dtype=np.float32)
        if n.value:
            check(lib().dd_tracker_gallery_read(self._h, int(track_id), ptr(rows), n.value, ctypes.byref(n), ctypes.byref(total)), 'dd_tracker_gallery_read')
        return rows, total.value

    @property
    def next_id(self):
        v = ctypes.c_int64()
        check(lib().dd_tracker_next_id(self._h, ctypes.byref(v)))
        return v.value


def _skip_streams(skip_frames, skip_phase, S):
    """object_detector_skip_frames / object_detector_skip_phase -> (N int32 [S], phase int32 [S] or None) for the per-stream form,
    (None, None) for the int form or no option; ValueError for what neither form takes."""
    def per_stream(v, what):
        a = np.asarray(v)
        if a.ndim == 0:
            a = np.full(S, a)
        if a.ndim != 1 or a.shape[0] != S:
            raise ValueError('%s: one value per stream, %d of them, got shape %r' % (what, S, a.shape))
        if a.dtype.kind not in 'iu':
            raise ValueError('%s: integers, got %s' % (what, a.dtype))
        return np.ascontiguousarray(a, dtype=np.int32)
    seq = skip_frames is not None and np.ndim(skip_frames) > 0
    if not seq and skip_phase is None:
        return None, None
    if skip_frames is None:
        raise ValueError('object_detector_skip_phase without object_detector_skip_frames: a phase shortens the first cycle of a stream\'s N')
    if not seq:
        raise ValueError('object_detector_skip_phase with object_detector_skip_frames=%r: an int is the pipeline-wide counter, which has no '
                         'phase; pass object_detector_skip_frames=[%r] * %d for one counter per stream' % (skip_frames, skip_frames, S))
    n = per_stream(skip_frames, 'object_detector_skip_frames')
    if (n < 0).any():
        raise ValueError('object_detector_skip_frames: N >= 0 for every stream, got %r' % (n.tolist(),))
    phase = None
    if skip_phase is not None:
        phase = per_stream(skip_phase, 'object_detector_skip_phase')
        if ((phase < 0) | (phase > n)).any():
            raise ValueError('object_detector_skip_phase: 0 .. N[z] for every stream, got %r for N = %r' % (phase.tolist(), n.tolist()))
    return n, phase


def _stream_values(v, what, S, integer=False):
    """A parameter the reference takes per process (max_age, n_init, max_cosine_distance, max_iou_distance, nms_max_overlap): a Python or
    NumPy scalar, for all streams, or a sequence of exactly S values -> contiguous [S], int32 (integer=True) or float64.  ValueError
    naming the parameter for a str, another rank or length, a non-integer in an integer parameter, a non-finite value."""
    if isinstance(v, (str, bytes)) or v is None:
        raise ValueError('%s: a number, or one per stream (%d of them), got %r' % (what, S, v))
    a = np.asarray(v)
    if a.dtype.kind not in 'iuf':
        raise ValueError('%s: a number, or one per stream (%d of them), got %r' % (what, S, v))
    if a.ndim == 0:
        a = np.full(S, int(a) if integer else float(a))           # (an integer parameter given as one float is truncated, as int(max_age) always did)
    elif a.ndim != 1 or a.shape[0] != S:
        raise ValueError('%s: one value, or one per stream with shape (%d,), got shape %r' % (what, S, a.shape))
    elif integer and a.dtype.kind not in 'iu':
        raise ValueError('%s: integers, got %s' % (what, a.dtype))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s: finite values, got %r' % (what, a.tolist()))
    if (a < 0).any():
        raise ValueError('%s: >= 0 for every stream, got %r' % (what, a.tolist()))
    return np.ascontiguousarray(a, dtype=np.int32 if integer else np.float64)


def _stream_lines(line, S, W, H):
    """line= -> float64 [S, 4] (x1, y1, x2, y2 per stream).  None: the reference's default [[W/2, 0], [W/2, H]] (deepdish.py:739-741) for
    every stream; a value of size 4: the pipeline's line, as always; shape (S, 4) or (S, 2, 2): one line per stream.  ValueError naming
    `line` for anything else and for a coordinate that is not finite."""
    if line is None:
        line = np.array([[W / 2, 0], [W / 2, H]], dtype=int)        # deepdish.py:739-741
    try:
        a = np.asarray(line, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('line: 4 numbers, or an array of shape (%d, 4) or (%d, 2, 2), got %r' % (S, S, line)) from None
    if a.size == 4:
        a = np.tile(a.reshape(1, 4), (S, 1))
    elif a.shape in ((S, 4), (S, 2, 2)):
        a = a.reshape(S, 4)
    else:
        raise ValueError('line: 4 numbers, or one line per stream with shape (%d, 4) or (%d, 2, 2), got shape %r' % (S, S, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError('line: finite coordinates, got %r' % (a.tolist(),))
    return np.ascontiguousarray(a)


def _stream_wanted(wanted_labels, S):
    """wanted_labels= -> (wanted, per_stream).  A sequence of str: the list of every stream -> (that list, None).  A sequence of S
    sequences of str: one list per stream (an empty one is legal) -> (their union in order of first appearance, scanning streams
    0 .. S - 1, the S lists).  ValueError naming `wanted_labels` for a bare str, a mix of both forms, another number of lists, or a list
    entry that is not a str."""
    if isinstance(wanted_labels, (str, bytes)) or wanted_labels is None:
        raise ValueError('wanted_labels: a sequence of label names (or one such sequence per stream), got %r' % (wanted_labels,))
    top = list(wanted_labels)
    if all(isinstance(l, str) for l in top):
        return top, None
    if any(isinstance(l, (str, bytes)) for l in top):
        raise ValueError('wanted_labels: label names, or one list of label names per stream, not a mix of both: %r' % (top,))
    if len(top) != S:
        raise ValueError('wanted_labels: one list per stream, %d of them, got %d' % (S, len(top)))
    per = []
    for z, lst in enumerate(top):
        try:
            lst = list(lst)
        except TypeError:
            raise ValueError('wanted_labels[%d]: a list of label names, got %r' % (z, lst)) from None
        if not all(isinstance(l, str) for l in lst):
            raise ValueError('wanted_labels[%d]: label names must be str, got %r' % (z, lst))
        per.append(lst)
    union = []
    for lst in per:
        union += [l for l in lst if l not in union]
    return union, per


def _stream_ratio(ratio, S):
    """background_subtraction_ratio= -> None (subtraction off: None or one negative value, --disable-background-subtraction) or float64
    [S].  One value holds for all streams; a sequence gives S values, each in [0, 1] -- subtraction cannot be off for some streams only,
    so a None or negative entry inside a sequence is a ValueError, as are another length, rank or type."""
    if ratio is None:
        return None
    if isinstance(ratio, (str, bytes)):
        raise ValueError('background_subtraction_ratio: a number, None, or one number per stream, got %r' % (ratio,))
    if np.ndim(ratio) == 0:
        return None if float(ratio) < 0 else np.full(S, float(ratio))
    seq = list(ratio) if np.ndim(ratio) == 1 else None
    if seq is None or len(seq) != S:
        raise ValueError('background_subtraction_ratio: one value, or one per stream with shape (%d,), got shape %r' % (S, np.shape(ratio)))
    if any(r is None for r in seq):
        raise ValueError('background_subtraction_ratio: None inside a sequence -- subtraction is on or off for the whole pipeline, got %r' % (seq,))
    a = np.asarray(seq)
    if a.dtype.kind not in 'iuf' or not np.all((a >= 0) & (a <= 1)):
        raise ValueError('background_subtraction_ratio: every stream\'s value in [0, 1] (subtraction cannot be off for some streams only), '
                         'got %r' % (seq,))
    return np.ascontiguousarray(a, dtype=np.float64)


def _stream_gate(motion_gate, S, ratio, skip_frames):
    """motion_gate= -> None (no gate) or int32 [S] thresholds, each >= 0: an int holds for all streams, a sequence gives S ints.
    `ratio`: _stream_ratio's result, `skip_frames`: object_detector_skip_frames as given.  ValueError naming the parameter for a
    wrong type, rank, length or sign, and for what the gate does not go with: subtraction off, a stream's ratio equal to 0, either
    form of object_detector_skip_frames with some N > 0."""
    if motion_gate is None:
        return None
    if isinstance(motion_gate, (str, bytes, bool)):
        raise ValueError('motion_gate: None, an int, or one int per stream (%d of them), got %r' % (S, motion_gate))
    a = np.asarray(motion_gate)
    if a.dtype.kind not in 'iu':
        raise ValueError('motion_gate: integers (foreground pixels), got %r' % (motion_gate,))
    if a.ndim == 0:
        a = np.full(S, int(a))
    elif a.ndim != 1 or a.shape[0] != S:
        raise ValueError('motion_gate: one value, or one per stream with shape (%d,), got shape %r' % (S, a.shape))
    if (a < 0).any() or (a > np.iinfo(np.int32).max).any():
        raise ValueError('motion_gate: 0 <= threshold < 2**31 for every stream, got %r' % (a.tolist(),))
    if ratio is None:
        raise ValueError('motion_gate with background_subtraction_ratio off: the gate reads the foreground mask')
    if (ratio == 0).any():
        raise ValueError('motion_gate with background_subtraction_ratio = 0 (%r): every box passes count >= 0, so an empty mask '
                         'decides nothing' % (ratio.tolist(),))
    if skip_frames is not None and (np.asarray(skip_frames) > 0).any():
        raise ValueError('motion_gate with object_detector_skip_frames=%r: not built -- a gated step leaves no detector output for the '
                         'skip steps after it to reuse (the reference would test the retained boxes against the next frame\'s mask)'
                         % (skip_frames,))
    return np.ascontiguousarray(a, dtype=np.int32)


def _reset_streams(streams, S):
    """reset(streams) -> contiguous int32 list; ValueError for an index outside 0 .. S - 1 or listed twice."""
    a = np.asarray(list(streams))
    if a.size == 0:
        return np.zeros(0, np.int32)
    if a.ndim != 1 or a.dtype.kind not in 'iu':
        raise ValueError('streams: a list of stream indices, got %r' % (streams,))
    if ((a < 0) | (a >= S)).any():
        raise ValueError('streams: indices 0 .. %d, got %r' % (S - 1, a.tolist()))
    if len(set(a.tolist())) != a.size:
        raise ValueError('streams: a stream is listed twice in %r' % (a.tolist(),))
    return np.ascontiguousarray(a, dtype=np.int32)


class MultiStreamPipeline:
    def __init__(self, n_streams, model='synthetic-ssd_mobilenet_v1', encoder_model='synthetic-mars-64x32x3',
                 labels=None, wanted_labels=('person',), input_size=(640, 480), line=None, max_cosine_distance=0.2,
                 nms_max_overlap=0.6, max_iou_distance=0.7, max_age=60, n_init=3, context=None, run_detector=True,
                 encoder_max_batch=None, track_capacity=512, gallery_capacity=256, background_subtraction_ratio=None,
                 background_masking=False, graph=None, object_detector_skip_frames=None, metric='cosine',
                 association='host', detector_letterbox=False, ground=None, topdownview_size_m=None, object_detector_skip_phase=None,
                 motion_gate=None):
        from .tools.yolov5 import letterbox_pad
        from .ground import for_pipeline
        # the reference's --3d mode (deepdish.py:592-611): a GroundPlane, or a list with one per stream; None: no top-down view
        self.ground, self.topdown_scale = for_pipeline(ground, topdownview_size_m, input_size, int(n_streams))      # ValueError before anything is built
        self.detector_letterbox = letterbox_pad(detector_letterbox)      # None, or the pad value of the YOLOv5 detector's letterboxed input
        if self.detector_letterbox is not None and 'yolov5' not in model:      # before anything is built
            raise ValueError('%s: detector_letterbox is the YOLOv5 detector\'s option; the other detectors are trained on stretched input' % model)
        # an int: one counter per pipeline (lock-step); S ints, or any phase: one counter per stream -- ValueError before anything is built
        skip_n, skip_phase = _skip_streams(object_detector_skip_frames, object_detector_skip_phase, int(n_streams))
        # what the reference takes per process -- one value for all streams, or one per stream (ValueError before anything is built)
        S = int(n_streams)
        lines = _stream_lines(line, S, input_size[0], input_size[1])
        wanted, wanted_per = _stream_wanted(wanted_labels, S)
        v_age, v_init = _stream_values(max_age, 'max_age', S, integer=True), _stream_values(n_init, 'n_init', S, integer=True)
        v_cos, v_iou = _stream_values(max_cosine_distance, 'max_cosine_distance', S), _stream_values(max_iou_distance, 'max_iou_distance', S)
        v_nms = _stream_values(nms_max_overlap, 'nms_max_overlap', S)
        # the motion gate: None, one threshold (foreground pixels) for all streams or one per stream -- and what it does not go with
        gate = _stream_gate(motion_gate, S, _stream_ratio(background_subtraction_ratio, S), object_detector_skip_frames)
        self.metric = metric
        metric_kind = _metric_kind(metric)   # 'cosine' or 'euclidean' (nn_matching.py:126-132), else ValueError -- before anything is built
        self.association = association
        association_where = _association_kind(association)       # 'host' or 'device', else ValueError -- likewise
        self.ctx = context or default_context()
        self.S = int(n_streams)
        self.W, self.H = input_size
        self.wanted = wanted                  # all streams' labels: the layout of counts(); wanted_of(z) is stream z's own list
        self._wanted_per = wanted_per
        self.model_name = str(model)
        # the reference picks the detector plugin by a substring of --model (deepdish.py:482-502)
        self.kind = ('yolov5' if 'yolov5' in model else None if ('yolo' in model or 'saved_model' in model) else
                     'ssd_mobilenet' if 'mobilenet' in model else 'tflite' if 'tflite' in model else None)
        if self.kind is None:
            raise ValueError('the multi-stream pipeline batches the SSD-MobileNet, YOLOv5 and generic TFLite detectors (got %s)' % model)
        with open(labels or (DEFAULT_YOLO_LABELS if self.kind == 'yolov5' else DEFAULT_LABELS)) as f:
            self.label_lines = [l.strip() for l in f.readlines()]
        meta = None
        if self.kind == 'tflite' and str(model).endswith('.tflite') and os.path.exists(str(model)):
            # the generic adaptor takes its label list and input normalisation from the model file's metadata (tools/tflite_object_detector.py:117-137
            # upstream); a file without metadata keeps the label file and the 127.5 / 127.5 defaults (see tools/tflite.py here)
            from .tools import tflite_reader
            try:
                meta = tflite_reader.read_metadata(str(model))
                self.label_lines = ['???'] + list(meta['labels'])      # (line 0 = the background entry the adaptor's label map skips)
            except tflite_reader.UnsupportedModel:
                if labels is None:
                    raise
        self.det = None
        anchors, n_anchors, n_classes = None, 0, 0
        if run_detector and self.kind == 'yolov5':
            wd = load_yolov5_weights(model)                        # a yolov5s .tflite file on disk goes through tools/tflite_reader.load_yolov5s
            prog = nets.compile_yolov5s(wd, int(wd.get('__in_size__', 640)))
            self.det = Net(prog, max_batch=self.S, context=self.ctx)
            n_anchors, n_classes = prog.meta['rows'], prog.meta['n_classes']
        elif run_detector:
            kind, wd = load_ssd_model(model)                        # ('uint8', QModel): the reference's own arithmetic (csrc/netsq.hip)
            prog = (netsq.compile_ssd_mobilenet_quant(wd) if kind == 'uint8' else
                    nets.compile_ssd_mobilenet(wd, mean=meta['mean'], std=meta['std']) if meta else nets.compile_ssd_mobilenet(wd))
            self.det_dtype = 'u8' if kind == 'uint8' else 'f16'
            self.det = Net(prog, max_batch=self.S, context=self.ctx)
            anchors = np.ascontiguousarray(prog.meta['anchors'], dtype=np.float32)
            n_anchors, n_classes = len(anchors), prog.meta['n_classes']
            ssd_post = ssd_post_options(wd)                         # the post-process op's options as the model file states them
        wd = load_mars_weights(encoder_model)                       # a mars .tflite file on disk goes through tools/tflite_reader.load_mars
        self.enc_weights = wd
        self.enc_hw = tuple(int(v) for v in wd.get('__in_hw__', (64, 32)))      # the crop size the weights state (deepdish.py:505-510: ImageEncoder reads it off the graph)
        if self.enc_hw not in nets.MARS_SIZES:
            raise ValueError('%s takes %d x %d crops: the batched pipeline runs the 64 x 32, 128 x 64 and 256 x 128 encoders '
                             '(mars-64x32x3, mars-128x64x3, mars-256x128x3)' % (encoder_model, self.enc_hw[0], self.enc_hw[1]))
        # crops per encoder forward: the activation arena per crop grows 4.8 x / 19 x with the crop (nets.MARS_ARENA_BYTES_PER_CROP), so the default
        # shrinks by that much -- the arena stays within what 64 x 32 takes at the same stream count (never below 16 crops).
        # The pipeline forwards in chunks of this many and the forward is crop-independent: the same bits however the crops fall into chunks.
        # (The number itself is the engine's max_batch, which fixes the K split of its convolutions: another value, other last bits.)
        if not encoder_max_batch:
            per_crop = nets.MARS_ARENA_BYTES_PER_CROP
            encoder_max_batch = max(16, max(64, 32 * self.S) * per_crop[(64, 32)] // per_crop[self.enc_hw])
        # the pipeline never reads an intermediate encoder tensor: its activation buffers share memory by lifetime (6.2 -> ~2 GB at 12 288 crops)
        self.enc = Net(nets.compile_mars(wd, *self.enc_hw), max_batch=encoder_max_batch, context=self.ctx,
                       shared=os.environ.get('DD_NET_SHARED', '1') != '0')
        # latency mode: with a handful of streams a forward is a train of 20-75 kernels of a few microseconds each;
        # replaying it as one hipGraph takes the per-launch host cost out of the frame latency (DD_GRAPH=0/1 overrides)
        if graph is None:
            graph = self.S <= 4 if os.environ.get('DD_GRAPH') is None else os.environ['DD_GRAPH'] == '1'
        self.graph = bool(graph)
        if self.graph:
            self.enc.use_graph(True)
            if self.det is not None:
                self.det.use_graph(True)
        self.lines = lines                    # [S, 4]; self.line: the pipeline's line (stream 0's, when every stream has its own)
        self.line = np.ascontiguousarray(lines[0])
        h = P()
        check(lib().dd_pipeline_create(self.ctx.handle, self.S, self.H, self.W, self.det._h if self.det else None,
                                       ptr(anchors), n_anchors, n_classes, self.enc._h,
                                       '\n'.join(self.label_lines).encode(), '\n'.join(self.wanted).encode(),
                                       float(v_cos[0]), float(v_nms[0]), float(v_iou[0]),
                                       int(v_age[0]), int(v_init[0]), ptr(self.line), int(track_capacity),
                                       int(gallery_capacity), ctypes.byref(h)), 'dd_pipeline_create')
        self._h = h
        # only values that really differ between streams reach the per-stream setters: S equal values are the scalar pipeline exactly
        if (lines != lines[0]).any():
            check(lib().dd_pipeline_stream_lines(self._h, ptr(lines)), 'dd_pipeline_stream_lines')
        if wanted_per is not None and any(set(l) != set(wanted) for l in wanted_per):
            mask = np.ascontiguousarray([[int(l in own) for l in wanted] for own in wanted_per], dtype=np.uint8).reshape(self.S, len(wanted))
            check(lib().dd_pipeline_stream_wanted(self._h, ptr(mask)), 'dd_pipeline_stream_wanted')
        differ = [a if (a != a[0]).any() else None for a in (v_cos, v_iou, v_age, v_init)]
        if any(a is not None for a in differ):
            check(lib().dd_pipeline_stream_tracker_params(self._h, *[ptr(a) for a in differ]), 'dd_pipeline_stream_tracker_params')
        if (v_nms != v_nms[0]).any():
            check(lib().dd_pipeline_stream_nms_overlap(self._h, ptr(v_nms)), 'dd_pipeline_stream_nms_overlap')
        if metric_kind:         # NearestNeighborDistanceMetric("euclidean", max_cosine_distance, None) for every stream's tracker
            check(lib().dd_pipeline_metric(self._h, metric_kind), 'dd_pipeline_metric')
        if association_where:   # every stream's matching cascade and assignments on the device, one wave per stream (csrc/assoc.hip)
            check(lib().dd_pipeline_association(self._h, association_where), 'dd_pipeline_association')
        if self.det is not None and self.kind != 'yolov5':
            check(lib().dd_pipeline_ssd_options(self._h, int(ssd_post['max_detections']), float(ssd_post['nms_score_threshold']),
                                                float(ssd_post['nms_iou_threshold'])), 'dd_pipeline_ssd_options')
            if ssd_post.get('use_regular_nms'):                     # the file asks for the op's per-class NMS (csrc/post_regular.hip)
                check(lib().dd_pipeline_ssd_regular_nms(self._h, int(ssd_post['detections_per_class'])), 'dd_pipeline_ssd_regular_nms')
        if self.detector_letterbox is not None and self.det is not None:      # the step's stretch becomes the letterbox launch (csrc/letterbox.hip)
            check(lib().dd_pipeline_detector_letterbox(self._h, self.detector_letterbox), 'dd_pipeline_detector_letterbox')
        if self.kind == 'tflite' and self.det is not None:          # tools/tflite.py's adaptor instead of tools/ssd_mobilenet.py's
            check(lib().dd_pipeline_detector_adaptor(self._h, 2), 'dd_pipeline_detector_adaptor')
        off = 0 if self.kind == 'yolov5' else 1                     # yolov5.py:134 labels[idx]; ssd_mobilenet.py:142-147 labels[idx + 1]
        self._class_id = {name: i - off for i, name in enumerate(self.label_lines) if i >= off}
        if background_subtraction_ratio is not None:
            self.background_subtraction(background_subtraction_ratio, background_masking)
        # --object-detector-skip-frames (deepdish.py:892-893,929-938,1003-1014): detector + encoder on one step in N + 1 (None: every step)
        # An int is the pipeline-wide counter: all streams detect on the same steps.  A sequence of S ints (and / or
        # object_detector_skip_phase) gives every stream its own counter, the reference's rule per camera; that form takes presence masks.
        self.object_detector_skip_frames = object_detector_skip_frames
        self.object_detector_skip_phase = object_detector_skip_phase
        self.skip_per_stream = skip_n is not None
        if self.skip_per_stream:
            check(lib().dd_pipeline_detector_skip_streams(self._h, ptr(skip_n), ptr(skip_phase)), 'dd_pipeline_detector_skip_streams')
        elif object_detector_skip_frames is not None:
            check(lib().dd_pipeline_detector_skip_frames(self._h, int(object_detector_skip_frames)), 'dd_pipeline_detector_skip_frames')
        # the motion gate (dd_pipeline_motion_gate): a stream whose foreground mask holds at most motion_gate[z] pixels runs no detector
        # and no encoder in that step and hands its tracker zero detections; None: every stream runs both, as always
        self.motion_gate = None if gate is None else gate.copy()
        if gate is not None:
            check(lib().dd_pipeline_motion_gate(self._h, ptr(gate)), 'dd_pipeline_motion_gate')

    def background_subtraction(self, ratio, masking=False):
        """deepdish.py:512,889,957: ratio = --background-subtraction-ratio (reference default 0.25); None or a negative
        value = --disable-background-subtraction (how a pipeline starts, and how the reference's benchmarks run).  ratio may also be a
        sequence of S values, each in [0, 1]: every stream's motion test then compares against its own.  Turning subtraction off for
        some streams only is not offered: a None or negative entry inside a sequence is a ValueError.  masking is one bool."""
        r = _stream_ratio(ratio, self.S)
        check(lib().dd_pipeline_background_subtraction(self._h, -1.0 if r is None else float(r[0]), int(bool(masking))),
              'dd_pipeline_background_subtraction')
        if r is not None and (r != r[0]).any():
            check(lib().dd_pipeline_stream_motion_ratio(self._h, ptr(r)), 'dd_pipeline_stream_motion_ratio')

    def motion_mask(self, read=True):
        """-> (fgMask of the last step as ndarray u8 [S, H, W], boxes rejected by the motion test so far)."""
        n = ctypes.c_longlong()
        out = np.zeros((self.S, self.H, self.W), dtype=np.uint8) if read else None
        check(lib().dd_pipeline_motion_mask(self._h, ptr(out), 0, ctypes.byref(n)), 'dd_pipeline_motion_mask')
        return out, n.value

    def __del__(self):
        try:
            if self._h:
                lib().dd_pipeline_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def pack_injected(self, per_stream):
        """per_stream: list of (boxes tlwh, labels, scores) per stream -> arrays for step()."""
        off = np.zeros(self.S + 1, dtype=np.int32)
        b, sc, cl = [], [], []
        for z, (boxes, labels, scores) in enumerate(per_stream):
            b += [tuple(float(v) for v in bb) for bb in boxes]
            sc += [float(v) for v in scores]
            cl += [self._class_id[l] for l in labels]
            off[z + 1] = len(sc)
        return (np.ascontiguousarray(np.array(b, dtype=np.float64).reshape(-1, 4)), np.array(sc, dtype=np.float64),
                np.array(cl, dtype=np.int32), off)

    def _mask(self, present, what):
        """present= of step(): None, or S values of 0 / 1 -> contiguous uint8 [S] (ValueError otherwise)."""
        if present is None:
            return None
        a = np.asarray(present)
        if a.ndim != 1 or a.shape[0] != self.S:
            raise ValueError('%s: one value per stream, shape (%d,), got %r' % (what, self.S, a.shape))
        if a.dtype != np.bool_ and not (a.dtype.kind in 'iuf' and np.all((a == 0) | (a == 1))):
            raise ValueError('%s: values must be 0 or 1 (bool, uint8 or a list of them)' % what)
        return np.ascontiguousarray(a != 0, dtype=np.uint8)

    def step(self, frames_dev, injected=None, frames_next=None, present=None, present_next=None):
        """frames_dev: u8 [S, H, W, 3] BGR torch tensor in HBM; injected: pack_injected(...) or None.
        frames_next: the frames of the following step (same shape): their detector run is queued on the
        detector stream and overlaps this step's NMS / encoder / tracker; the next step() must receive them.
        With object_detector_skip_frames, a skip step ignores `injected` (it stands for the detector's output, and the
        detector does not run), and frames_next is queued only when the next step is a detector step.
        present: None (every stream), or S values of 0 / 1: the streams that have a frame in this step.  For the others the step does
        not exist -- their slot of frames_dev and their rows of `injected` may hold anything, nothing of their state moves, and the
        detector runs on the present frames only.  present_next belongs to frames_next; a next step that arrives with another mask than
        announced runs its detector itself, with the same result.  An all-zero mask is a legal step.  Not with the int form of
        object_detector_skip_frames (one counter per pipeline: all streams in lock-step); the per-stream form (a sequence of S ints)
        takes masks: a stream's counter moves only on the steps it is present in.
        With motion_gate set no frames_next run is queued ahead (the next step's detector list is not known before its mask is): the
        argument stays legal, the next step runs its detector itself, and `injected` rows of a gated stream are ignored."""
        assert tuple(frames_dev.shape) == (self.S, self.H, self.W, 3)
        assert frames_next is None or tuple(frames_next.shape) == (self.S, self.H, self.W, 3)
        present, present_next = self._mask(present, 'present'), self._mask(present_next, 'present_next')
        if present_next is not None and frames_next is None:
            raise ValueError('present_next belongs to frames_next, which is missing')
        if (present is not None or present_next is not None) and not self.skip_per_stream and self.object_detector_skip_frames is not None \
                and int(self.object_detector_skip_frames) > 0:
            raise ValueError('object_detector_skip_frames=%d with a presence mask: an int is one counter per pipeline (all streams in '
                             'lock-step); pass a sequence, object_detector_skip_frames=[%d] * %d, for one counter per stream'
                             % (int(self.object_detector_skip_frames), int(self.object_detector_skip_frames), self.S))
        b, sc, cl, off = injected if injected is not None else (None, None, None, None)
        check(lib().dd_pipeline_step3(self._h, ptr(frames_dev), ptr(present), ptr(frames_next), ptr(present_next), ptr(b), ptr(sc), ptr(cl),
                                      ptr(off)), 'dd_pipeline_step')

    def wanted_of(self, stream):
        """Stream z's own wanted labels in its own order (self.wanted is the union over the streams, the layout of counts())."""
        if not 0 <= int(stream) < self.S:
            raise ValueError('stream %r of %d' % (stream, self.S))
        return list(self.wanted if self._wanted_per is None else self._wanted_per[int(stream)])

    def reset(self, streams):
        """The listed streams start over -- what restarting the camera's process is to the reference; for a camera that was swapped or
        reconnects after a long gap.  Between steps, at any time.  Afterwards every listed stream is in the state of a stream of a freshly
        built pipeline with the same parameters: no tracks and ids from 1 again, its gallery back in the pool, empty paths and votes,
        counts zero, no detections, frames_seen() 0, an overlay that reports "never stepped", the MOG2 model, its frame count and the
        motion-mask plane as at creation, the per-stream skip counter and phase as at construction with the retained detector output
        and encoder rows dropped.  Every other stream is untouched.  A queued look-ahead detector run is discarded: the next step runs
        the detector itself.  An empty list does nothing; an index out of range or listed twice is a ValueError.  Not with the int form
        of object_detector_skip_frames (one counter for all streams cannot give one stream a fresh first detector step): pass a
        sequence."""
        a = _reset_streams(streams, self.S)
        if not self.skip_per_stream and self.object_detector_skip_frames is not None and int(self.object_detector_skip_frames) > 0:
            raise ValueError('object_detector_skip_frames=%d with reset(): an int is one counter per pipeline (all streams in lock-step); '
                             'pass a sequence, object_detector_skip_frames=[%d] * %d, for one counter per stream'
                             % (int(self.object_detector_skip_frames), int(self.object_detector_skip_frames), self.S))
        check(lib().dd_pipeline_reset_streams(self._h, ptr(a) if a.size else None, int(a.size)), 'dd_pipeline_reset_streams')

    def snapshot(self, streams=None, background=True):
        """The state of `streams` (default: all) as a StreamSnapshot (host bytes: deepdish_amd/snapshot.py), between steps.  A pure read:
        it waits for the main stream and changes nothing, a queued look-ahead detector run stays queued, and the pipeline steps on
        exactly as one that was never asked.  Per stream it carries the tracker (tracks and deleted list, ids, means, covariances, every
        gallery in storage order), paths, votes, counts by label name, frames_seen, the last step's detections, the per-stream skip
        counter with the retained detector output and encoder rows, and -- background=True and subtraction on -- the MOG2 model with its
        frame count and the motion-mask plane (about 31 MB per 640 x 480 stream).  Parameters are recorded to be checked by restore(),
        not carried; stage timers, the *_stats() counters, the tracker's last cost matrices and matches, the Python-side `ground`
        cameras and fonts are not stream state.  Not with the int form of object_detector_skip_frames (N > 0)."""
        from .snapshot import StreamSnapshot
        a = np.arange(self.S, dtype=np.int32) if streams is None else _reset_streams(streams, self.S)
        n = ctypes.c_int64()
        check(lib().dd_pipeline_snapshot_bytes(self._h, ptr(a) if a.size else None, int(a.size), int(bool(background)), ctypes.byref(n)),
              'dd_pipeline_snapshot_bytes')
        blob = np.empty(n.value, dtype=np.uint8)
        check(lib().dd_pipeline_snapshot(self._h, ptr(a) if a.size else None, int(a.size), int(bool(background)), ptr(blob), n.value, ctypes.byref(n)),
              'dd_pipeline_snapshot')
        return StreamSnapshot(blob)

    def restore(self, snapshot, streams=None):
        """Entry i of `snapshot` becomes stream streams[i] (default: streams 0 .. len(snapshot) - 1): reset([z]) followed by loading the
        state, every other stream untouched, a queued look-ahead run discarded.  From its next step on the stream is bit for bit the
        stream the snapshot was taken from -- in this pipeline, in another process, in a pipeline with another number of streams, on
        another GPU (with the same encoder_max_batch: the engine's max_batch fixes the last bits of the features).  Everything is checked
        before anything changes, and a restore that raises leaves the pipeline exactly as it was.  ValueError: a stream out of range or
        listed twice, len(streams) != len(snapshot), a parameter of the source stream that differs from the destination's (named),
        a snapshot with background into a pipeline with subtraction off, a blob the validator refuses.  DeepDishHipError: more tracks
        than track_capacity (DD_E_CAPACITY), the int form of object_detector_skip_frames with N > 0 (DD_E_STATE: pass a sequence, as
        for reset())."""
        from ._lib import DeepDishHipError
        a = np.arange(len(snapshot), dtype=np.int32) if streams is None else _reset_streams(streams, self.S)
        if a.size != len(snapshot):
            raise ValueError('streams: %d streams for a snapshot of %d entries' % (a.size, len(snapshot)))
        blob = snapshot._blob
        rc = lib().dd_pipeline_restore(self._h, ptr(blob), int(blob.size), ptr(a) if a.size else None, int(a.size))
        if rc == -1:                               # DD_E_ARG
            raise ValueError(lib().dd_last_error().decode())
        check(rc, 'dd_pipeline_restore')

    def stream_param_stats(self):
        """Which kernels per-stream parameters selected: launches of the per-problem NMS variant and of the per-stream association
        variant (both 0 while all streams share their values), reset() calls that reset a stream and the streams they reset."""
        out = np.zeros(4, dtype=np.int64)
        check(lib().dd_pipeline_stream_param_stats(self._h, ptr(out)), 'dd_pipeline_stream_param_stats')
        return dict(nms_stream_launches=int(out[0]), association_stream_launches=int(out[1]), resets=int(out[2]), streams_reset=int(out[3]))

    def mog2_state(self, stream):
        """Test aid: the background model of one stream (dd_mog2_state) -> (weight [5, P], variance [5, P], mean [5, 3, P], nmodes [P])."""
        h = P()
        check(lib().dd_pipeline_mog2(self._h, ctypes.byref(h)), 'dd_pipeline_mog2')
        if not h.value:
            raise ValueError('mog2_state: background subtraction is off')
        n = self.H * self.W
        wt, var, mu = np.zeros((5, n), np.float32), np.zeros((5, n), np.float32), np.zeros((5, 3, n), np.float32)
        nm = np.zeros(n, np.uint8)
        check(lib().dd_mog2_state(h, int(stream), ptr(wt), ptr(var), ptr(mu), ptr(nm)), 'dd_mog2_state')
        return wt, var, mu, nm

    def frames_seen(self):
        """int64 [S]: the number of steps each stream was present in -- every stream has its own frame number."""
        out = np.zeros(self.S, dtype=np.int64)
        check(lib().dd_pipeline_frames_seen(self._h, ptr(out)), 'dd_pipeline_frames_seen')
        return out

    def present_stats(self):
        """Which path the steps took: steps that carried a mask, frames_gather_k launches, streams advanced summed over the steps."""
        out = np.zeros(3, dtype=np.int64)
        check(lib().dd_pipeline_present_stats(self._h, ptr(out)), 'dd_pipeline_present_stats')
        return dict(masked_steps=int(out[0]), gather_launches=int(out[1]), streams_stepped=int(out[2]))

    def skip_stats(self):
        """Detector stream-steps and skip stream-steps summed over the steps; with per-stream counters also the launches of the retained-rows
        kernel (csrc/featrows.hip), the feature rows retained now and the bytes allocated for their store (all 0 otherwise); `skipped`:
        bool [S], whether each stream's last step was a skip step."""
        out, sk = np.zeros(5, dtype=np.int64), np.zeros(self.S, dtype=np.uint8)
        check(lib().dd_pipeline_skip_stats(self._h, ptr(out), ptr(sk)), 'dd_pipeline_skip_stats')
        return dict(detector_stream_steps=int(out[0]), skip_stream_steps=int(out[1]), carry_launches=int(out[2]), rows_retained=int(out[3]),
                    store_bytes=int(out[4]), skipped=sk.astype(bool))

    def gate_stats(self):
        """The motion gate's counters: `steps` on which it ran (some stream was on a detector step), `gated_stream_steps` summed over
        the steps, and per stream `count` int32 [S] -- the foreground pixels measured on its last detector-eligible step, -1 before its
        first and after its reset -- and `gated` bool [S], whether that step was gated.  A step without the stream keeps its entry."""
        out, cnt, g = np.zeros(2, dtype=np.int64), np.zeros(self.S, dtype=np.int32), np.zeros(self.S, dtype=np.uint8)
        check(lib().dd_pipeline_gate_stats(self._h, ptr(out), ptr(cnt), ptr(g)), 'dd_pipeline_gate_stats')
        return dict(steps=int(out[0]), gated_stream_steps=int(out[1]), count=cnt, gated=g.astype(bool))

    def detector_stream(self):
        """The stream the look-ahead detector run is queued on (None without a detector): the consumer to name when acquiring the NEXT
        step's frames from an ingest ring (`ring.frames(slot, stream=pipe.detector_stream())`), so that their upload is waited for by
        their own detector run and not by this step's kernels.  A skip step (object_detector_skip_frames) has no detector run: its
        main stream waits at step entry for what this stream holds, so frames acquired for it are uploaded before MOG2 reads them."""
        h = P()
        check(lib().dd_pipeline_detector_stream(self._h, ctypes.byref(h)), 'dd_pipeline_detector_stream')
        return h if h.value else None

    def counts(self):
        out = np.zeros((self.S, len(self.wanted), 4), dtype=np.int64)
        check(lib().dd_pipeline_counts(self._h, ptr(out)), 'dd_pipeline_counts')
        return out

    def tracker(self, stream):
        h = P()
        check(lib().dd_pipeline_tracker(self._h, stream, ctypes.byref(h)), 'dd_pipeline_tracker')
        return _TrackerView(h)

    def association_stats(self):
        """Tracker.association_stats() for the pipeline's tracker group: group updates decided on the device / on the host, and streams
        that fell back to the host code."""
        return _association_stats(self.tracker(0)._h)

    def stage_ms(self):
        """Per step: the stages' GPU milliseconds under the reference's timer names (deepdish.py:975-981 objd, :1018-1021 feat, :1031-1032
        trak; nms = the deep_sort NMS of :995), measured with HIP events on the streams the kernels run on, `host` = the step's wall time
        outside its waits for the GPU, `wall` = the step.  objd runs on the detector stream, one frame ahead beside the other stages, so
        the stages do not add up to `wall`.  `host_wall` = the old host-side stopwatch per program section (NOT per-stage GPU time: its
        `trak` contains the wait for the encoder kernels)."""
        g = np.zeros(6, dtype=np.float64)
        n = ctypes.c_longlong()
        check(lib().dd_pipeline_stage_gpu_ms(self._h, ptr(g), ctypes.byref(n)), 'dd_pipeline_stage_gpu_ms')
        t = np.zeros(4, dtype=np.float64)
        check(lib().dd_pipeline_stage_seconds(self._h, ptr(t), ctypes.byref(n)), 'dd_pipeline_stage_seconds')
        k = max(1, n.value)
        return dict(objd=g[0] / k, nms=g[1] / k, feat=g[2] / k, trak=g[3] / k, host=g[4] / k, wall=g[5] / k, steps=n.value,
                    host_wall=dict(objd=1e3 * t[0] / k, nms=1e3 * t[1] / k, feat=1e3 * t[2] / k, trak=1e3 * t[3] / k))

    def overlay(self, streams=None):
        """The overlay elements of the last step (dd_pipeline_overlay) for `streams` (default: all): a list with one dict per stream --
        line f64 [4], the stream's own count line; track_ids int64 [t], track_labels (voted label names), track_tlbr f64 [t, 4] and path_counts int64 [t] for the
        confirmed tracks with time_since_update <= 1 in track order; points f64 [sum(path_counts), 2], their bottom-centre paths behind
        one another; crossings f64 [c, 4], the segments that crossed the line in this step; det_tlbr f64 [d, 4], the detections that
        went into the tracker; counts int64 [n_wanted, 4] = pos, neg, int, del."""
        streams = np.arange(self.S, dtype=np.int32) if streams is None else np.ascontiguousarray(list(streams), dtype=np.int32)
        n = len(streams)
        sizes = np.zeros((n, 4), dtype=np.int32)
        none = P(None)
        check(lib().dd_pipeline_overlay(self._h, ptr(streams), n, ptr(sizes), none, none, none, none, none, none, none, none), 'dd_pipeline_overlay')
        caps = np.ascontiguousarray(sizes.sum(axis=0), dtype=np.int32)
        ti, tb = np.zeros((caps[0], 3), np.int64), np.zeros((caps[0], 4), np.float64)
        pts, cr, dt = np.zeros((caps[1], 2), np.float64), np.zeros((caps[2], 4), np.float64), np.zeros((caps[3], 4), np.float64)
        counts, line = np.zeros((n, len(self.wanted), 4), np.int64), np.zeros(4, np.float64)
        check(lib().dd_pipeline_overlay(self._h, ptr(streams), n, ptr(sizes), ptr(caps), ptr(ti), ptr(tb), ptr(pts), ptr(cr), ptr(dt), ptr(counts),
                                        ptr(line)), 'dd_pipeline_overlay')
        lines = np.zeros((n, 4), np.float64)
        check(lib().dd_pipeline_lines(self._h, ptr(streams), n, ptr(lines)), 'dd_pipeline_lines')
        end = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(sizes, axis=0)])
        out = []
        for i in range(n):
            (t0, p0, c0, d0), (t1, p1, c1, d1) = end[i], end[i + 1]
            out.append(dict(line=lines[i], track_ids=ti[t0:t1, 0], track_labels=[self.label_lines[k] if k >= 0 else '' for k in ti[t0:t1, 1]],
                            track_tlbr=tb[t0:t1], path_counts=ti[t0:t1, 2], points=pts[p0:p1], crossings=cr[c0:c1], det_tlbr=dt[d0:d1],
                            counts=counts[i]))
        return out

    def render(self, frames_dev, streams=None, annotation='label', out=None, font=None):
        """The reference's annotated output frame (deepdish.py:295-408, 1187-1207) of `streams` (default: all) after the last step, painted
        over frames_dev (the frames that step received) in one launch (csrc/render.hip) -> u8 [n, H, W, 3] BGR on the device, in the order
        of `streams`.  annotation = --object-annotation: 'label', 'id' or 'none'.  font: a PIL font (default: Pillow's default face at
        int(24 / 640 * W)).  With `ground` set the frame carries the top-down panel (deepdish.py:410-440).  Nothing of this runs unless it
        is called."""
        from . import render as rd
        rd.annotation_kind(annotation)
        assert tuple(frames_dev.shape) == (self.S, self.H, self.W, 3)
        streams = list(range(self.S)) if streams is None else [int(z) for z in streams]
        if not hasattr(self, '_renderers'):
            self._renderers = {}
        key = id(font) if font is not None else None
        if key not in self._renderers:
            self._renderers[key] = (rd.Renderer(self.H, self.W, font=font, context=self.ctx, records=2 if self.ground is not None else 1), font)      # (the font is kept alive with its id)
        r = self._renderers[key][0]
        overlays = self.overlay(streams)
        topdown = [None] * len(streams)
        if self.ground is not None:
            topdown = [(self.W / 4, self.H / 4, g, self.topdown_scale) for g in self._ground_of(streams, overlays)]
        prims = [rd.overlay_primitives(r, o['line'], o['track_ids'], o['track_labels'], o['track_tlbr'], o['points'], o['path_counts'], o['crossings'],
                                       o['det_tlbr'], self._counters(z, o['counts']), annotation, topdown=t)
                 for z, o, t in zip(streams, overlays, topdown)]
        return r.draw(frames_dev, prims, streams=streams, out=out)

    def _counters(self, stream, counts):
        """(label, negcount, poscount) of the counters the reference process of this stream's camera draws (deepdish.py:1142): its own
        wanted labels, in its own order."""
        if self._wanted_per is None:
            return [(l, int(c[1]), int(c[0])) for l, c in zip(self.wanted, counts)]
        return [(l, int(counts[self.wanted.index(l)][1]), int(counts[self.wanted.index(l)][0])) for l in self._wanted_per[stream]]

    def _ground_of(self, streams, overlays):
        """The path points of every overlay, unprojected with their stream's camera in one call -> f64 [points, 2] per overlay."""
        counts = [len(o['points']) for o in overlays]
        pts = np.concatenate([o['points'] for o in overlays], axis=0) if overlays else np.zeros((0, 2))
        cam = np.repeat(np.asarray(streams, dtype=np.int32), counts) if len(self.ground) > 1 else None
        g = self.ground.space_from_image(pts, cam)
        return np.split(g, np.cumsum(counts)[:-1]) if overlays else []

    def ground_paths(self, streams=None):
        """Where the drawn tracks of the last step are, in metres on the ground: per stream of `streams` (default: all) a dict with
        track_ids int64 [t], path_counts int64 [t] and points f64 [sum(path_counts), 2] -- overlay()'s bottom-centre paths behind one
        another, each through its stream's camera (GroundPlane.space_from_image; NaN at or above the horizon)."""
        if self.ground is None:
            raise ValueError('ground_paths: the pipeline was built without ground=')
        streams = list(range(self.S)) if streams is None else [int(z) for z in streams]
        overlays = self.overlay(streams)
        return [dict(track_ids=o['track_ids'], path_counts=o['path_counts'], points=g) for o, g in zip(overlays, self._ground_of(streams, overlays))]

    def render_jpeg(self, frames_dev, streams=None, annotation='label', quality=95, font=None):
        """render(...) and then csrc/jpeg.hip: the annotated output frames of `streams` as JPEG files, a list of bytes in the order of
        `streams` -- what the reference makes of its output frame with cv2.imencode(".jpg", frame) (deepdish.py:168) for the web stream,
        --output-cvat-dir and --stream-path, but for the restart markers (jpeg.py).  The raw frames never leave the device."""
        from .jpeg import JpegEncoder
        frames = self.render(frames_dev, streams=streams, annotation=annotation, font=font)
        if not hasattr(self, '_jpeg_encoders'):
            self._jpeg_encoders = {}
        key = (self.H, self.W, int(quality))
        if key not in self._jpeg_encoders:
            self._jpeg_encoders[key] = JpegEncoder(self.H, self.W, quality=quality, context=self.ctx)
        return self._jpeg_encoders[key].encode_to_host(frames)

    def detections(self, stream):
        """The detector adaptor's output for one stream in the last step: what the reference's detect_image(...) returns
        (tools/ssd_mobilenet.py:198-213) -- (boxes tlwh f64 [n, 4], label names, scores f64 [n]); on a skip step, the last
        detector step's."""
        n = ctypes.c_int()
        check(lib().dd_pipeline_detections(self._h, int(stream), None, None, None, 0, ctypes.byref(n)), 'dd_pipeline_detections')
        b, sc, cl = np.zeros((n.value, 4), np.float64), np.zeros(n.value, np.float64), np.zeros(n.value, np.int32)
        if n.value:
            check(lib().dd_pipeline_detections(self._h, int(stream), ptr(b), ptr(sc), ptr(cl), n.value, ctypes.byref(n)), 'dd_pipeline_detections')
        off = 0 if self.kind == 'yolov5' else 1
        return b, [self.label_lines[int(c) + off] for c in cl], sc
