"""GPU: every launch of the detector post-process (csrc/post.hip) and of the suppression kernels (csrc/nms.hip) alone, through the C ABI,
against tests/post_ref.py on the cases of tests/post_cases.py -- the smallest shapes at which each kernel's loop bounds, tails, dispatch
edges and tie rules can go wrong.  tests/test_post_ref.py holds the references to the oracle and the cases to their conditions on the CPU.

Everything is compared bit for bit, every element of every output, the rows behind the count included (zero where the contract says zero,
an untouched sentinel elsewhere) -- except dd_ssd_decode's boxes and scores, which are held to the bound post_ref.ssd_decode derives."""
import numpy as np
import pytest
import torch

import net_op_ref
import post_cases as pc
import post_ref

pytestmark = pytest.mark.gpu

TAIL = 16                                  # sentinel rows behind every output


def _env():
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context, ptr
    return default_context(), lib(), check, ptr


def _full(ctx, shape, dtype, value):
    return torch.full(shape, value, dtype=dtype, device=f'cuda:{ctx.device}')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


# ------------------------------------------------------------------------------------------------ YOLO
def _yolo_out(ctx, batch, cap):
    """per-image [batch][cap] outputs as one flat buffer each with TAIL sentinel rows behind them (so cap = 0 still has an address)"""
    n = batch * cap + TAIL
    return (_full(ctx, (n, 4), torch.float32, float(pc.SENTINEL_F)), _full(ctx, (n,), torch.float32, float(pc.SENTINEL_F)),
            _full(ctx, (n,), torch.int32, int(pc.SENTINEL_I)), _full(ctx, (batch + TAIL,), torch.int32, int(pc.SENTINEL_I)))


def _check_yolo(ctx, outs, want_rows, batch, cap, what):
    """want_rows[z] = the image's passing rows in row order.  out_n = the full count; the first min(n, cap) rows; sentinels everywhere else."""
    ob, os_, oc, on = (ctx.to_host(t) for t in outs)
    wb = np.full_like(ob, pc.SENTINEL_F); ws = np.full_like(os_, pc.SENTINEL_F); wc = np.full_like(oc, pc.SENTINEL_I)
    wn = np.full_like(on, pc.SENTINEL_I)
    for z in range(batch):
        n, (b, s, c) = post_ref.capped(want_rows[z], cap)
        wn[z] = n
        m = len(s)
        assert m == min(n, cap)
        wb[z * cap:z * cap + m], ws[z * cap:z * cap + m], wc[z * cap:z * cap + m] = b, s, c
    _same(on, wn, (what, 'out_n'))
    _same(ob, wb, (what, 'boxes')); _same(os_, ws, (what, 'scores')); _same(oc, wc, (what, 'classes'))
    return wn[:batch]


def _decode_batch(raw, geom, cap):
    ctx, lib, check, ptr = _env()
    batch, n_rows, cols = raw.shape
    W, H, lb = geom
    d_raw = ctx.to_device(raw, np.float32)
    outs = _yolo_out(ctx, batch, cap)
    nw, nh = lb if lb else (0, 0)
    check(lib.dd_yolov5_decode_batch(ctx.handle, ptr(d_raw), n_rows, cols - 5, float(pc.YOLO_THR), float(W), float(H), nw, nh,
                                     *[ptr(t) for t in outs[:3]], cap, ptr(outs[3]), batch, None), 'dd_yolov5_decode_batch')
    with np.errstate(invalid='ignore'):
        want = [post_ref.yolo_rows(raw[z], pc.YOLO_THR, W, H, lb) for z in range(batch)]
    return _check_yolo(ctx, outs, want, batch, cap, (raw.shape, geom, cap))


@pytest.mark.parametrize('n_cls', pc.YOLO_CLASSES)
def test_yolo_conf_and_compact(n_cls):
    """yolo_conf_k + yolo_compact_k (dd_yolov5_decode_batch), stretch and letterboxed: every row count and batch size of one class count."""
    for n_rows, batch in pc.yolo_launches(n_cls):
        raw = pc.yolo_raw(n_rows, n_cls, batch)
        for geom in [pc.YOLO_STRETCH, pc.YOLO_LETTERBOX[(n_rows + batch) % 2]]:
            n = _decode_batch(raw, geom, n_rows)
            assert 0 < n.sum() < batch * n_rows                                # passing and failing rows
            assert batch == 1 or n[1] == 0                                     # the empty image


@pytest.mark.parametrize('n_rows,n_cls,batch', [(1025, 80, 3), (2049, 92, 1), (7, 1, 3)])
def test_yolo_compact_overflow_counts_every_row_and_writes_the_first_cap(n_rows, n_cls, batch):
    raw = pc.yolo_raw(n_rows, n_cls, batch)
    full = _decode_batch(raw, pc.YOLO_STRETCH, n_rows)
    for cap in (int(full.max()) // 2, 1, 0):
        n = _decode_batch(raw, pc.YOLO_STRETCH, cap)
        np.testing.assert_array_equal(n, full)
        assert n.max() > cap                                                   # the capacity IS exceeded
    # n_rows == 0: out_n zeroed, nothing launched
    ctx, lib, check, ptr = _env()
    outs = _yolo_out(ctx, batch, 4)
    check(lib.dd_yolov5_decode_batch(ctx.handle, ptr(outs[0]), 0, n_cls, 0.25, 640.0, 480.0, 0, 0, *[ptr(t) for t in outs[:3]], 4, ptr(outs[3]), batch, None),
          'dd_yolov5_decode_batch')
    on = ctx.to_host(outs[3])
    assert (on[:batch] == 0).all() and (on[batch:] == pc.SENTINEL_I).all()
    assert lib.dd_yolov5_decode_batch(ctx.handle, ptr(outs[0]), 4, n_cls, 0.25, 640.5, 480.0, 640, 640, *[ptr(t) for t in outs[:3]], 4, ptr(outs[3]), batch, None) < 0
    assert lib.dd_yolov5_decode_batch(ctx.handle, ptr(outs[0]), 4, n_cls, 0.25, 640.0, 480.0, 0, 0, *[ptr(t) for t in outs[:3]], -1, ptr(outs[3]), batch, None) < 0


def test_yolo_conf_grid_stride():
    """300 images x 256 rows x 1 class in ONE launch: 76 800 rows, more than the 8 192 blocks x 8 rows of yolo_conf_k's grid."""
    imgs, rows, n_cls = pc.YOLO_GRID_STRIDE
    raw = pc.yolo_raw(rows, n_cls, imgs)
    n = _decode_batch(raw, pc.YOLO_STRETCH, rows)
    assert (n[1::3] == 0).all() and n[0::3].min() > 0 and n[(8192 * 8) // rows:].sum() > 0


@pytest.mark.parametrize('n_rows', pc.YOLO_ROWS)
def test_yolo_compact_alone(n_rows):
    """yolo_compact_k on crafted (box, confidence, class) rows (dd_yolov5_select_batch): stretch, two letterbox geometries, and the square canvas,
    which gives the stretch bits."""
    ctx, lib, check, ptr = _env()
    for batch in pc.YOLO_BATCHES:
        if n_rows == 1 and batch == 1:
            continue
        boxes, conf, cls = pc.select_inputs(n_rows, batch)
        d = [ctx.to_device(boxes, np.float32), ctx.to_device(conf, np.float32), ctx.to_device(cls, np.int32)]
        got = {}
        for W, H, lb in [pc.YOLO_STRETCH, (640.0, 640.0, None), pc.YOLO_SQUARE] + pc.YOLO_LETTERBOX:
            outs = _yolo_out(ctx, batch, n_rows)
            nw, nh = lb if lb else (0, 0)
            check(lib.dd_yolov5_select_batch(ctx.handle, *[ptr(t) for t in d], n_rows, float(pc.YOLO_THR), float(W), float(H), nw, nh,
                                             *[ptr(t) for t in outs[:3]], n_rows, ptr(outs[3]), batch, None), 'dd_yolov5_select_batch')
            want = [post_ref.select_rows(boxes[z], conf[z], cls[z], pc.YOLO_THR, W, H, lb) for z in range(batch)]
            n = _check_yolo(ctx, outs, want, batch, n_rows, (n_rows, batch, W, H, lb))
            assert 0 < n.sum() < batch * n_rows
            got[(W, H, lb)] = ctx.to_host(outs[0])
        _same(got[pc.YOLO_SQUARE], got[(640.0, 640.0, None)], 'square canvas == stretch')
        assert (got[pc.YOLO_LETTERBOX[0]] != got[pc.YOLO_STRETCH]).any()


@pytest.mark.parametrize('batch', pc.PACK_BATCHES)
def test_yolo_pack(batch):
    ctx, lib, check, ptr = _env()
    boxes, scores, cls, counts = pc.pack_inputs(batch)
    cap = pc.PACK_CAP
    want = post_ref.pack(boxes, scores, cls, counts, cap)
    total = int(np.minimum(counts, cap).sum())
    assert len(want) == total and (counts > cap).any() == (batch > 1)
    packed = _full(ctx, (total + TAIL, 6), torch.float32, float(pc.SENTINEL_F))
    d = [ctx.to_device(boxes, np.float32), ctx.to_device(scores, np.float32), ctx.to_device(cls, np.int32), ctx.to_device(counts, np.int32)]
    check(lib.dd_yolov5_pack(ctx.handle, *[ptr(t) for t in d], cap, batch, ptr(packed), None), 'dd_yolov5_pack')
    got = ctx.to_host(packed)
    _same(got[:total], want, ('packed', batch))
    assert (got[total:] == pc.SENTINEL_F).all()                               # nothing behind the total
    _same(got[:total, 5].view(np.int32), np.concatenate([cls[z, :min(n, cap)] for z, n in enumerate(counts)]), 'class bits')


# ------------------------------------------------------------------------------------------------ SSD
@pytest.mark.parametrize('n_classes', pc.SSD_CLASSES)
def test_ssd_decode(n_classes):
    """ssd_decode_k against csrc/ssd_dev.h restated in float64: class exact (in range for every input), boxes and scores within the derived
    bound, the key what the score and the threshold make it."""
    ctx, lib, check, ptr = _env()
    thr = np.float32(pc.SSD_THR)
    for A in pc.SSD_ANCHORS:
        for batch in pc.SSD_BATCHES:
            raw, anchors = pc.ssd_decode_inputs(A, n_classes, batch)
            want = post_ref.ssd_decode(raw, anchors, pc.SSD_THR)
            n = batch * A
            ob, os_ = _full(ctx, (n + TAIL, 4), torch.float32, -7777.0), _full(ctx, (n + TAIL,), torch.float32, -7777.0)
            oc, ok = _full(ctx, (n + TAIL,), torch.int32, -77), _full(ctx, (n + TAIL,), torch.float32, -7777.0)
            d_raw, d_anchors = ctx.to_device(raw, np.float32), ctx.to_device(anchors, np.float32)
            check(lib.dd_ssd_decode(ctx.handle, ptr(d_raw), ptr(d_anchors), A, n_classes, float(thr),
                                    ptr(ob), ptr(os_), ptr(oc), ptr(ok), batch, None), 'dd_ssd_decode')
            ob, os_, oc, ok = (ctx.to_host(t) for t in (ob, os_, oc, ok))
            what = 'classes %d anchors %d batch %d' % (n_classes, A, batch)
            assert (ob[n:] == pc.SENTINEL_F).all() and (os_[n:] == pc.SENTINEL_F).all() and (oc[n:] == pc.SENTINEL_I).all() and (ok[n:] == pc.SENTINEL_F).all()
            cls = oc[:n].reshape(batch, A)
            assert cls.min() >= 0 and cls.max() <= n_classes - 2, what
            np.testing.assert_array_equal(cls, want['cls'], err_msg=what)
            score = os_[:n].reshape(batch, A)
            net_op_ref.assert_within(what + ' score', score, want['score'], want['score_bound'])
            net_op_ref.assert_within(what + ' boxes', ob[:n].reshape(batch, A, 4), want['boxes'], want['boxes_bound'])
            np.testing.assert_array_equal(score >= thr, want['passes'], err_msg=what)
            _same(ok[:n].reshape(batch, A), np.where(score >= thr, score, np.float32(-1)).astype(np.float32), what + ' keys')
            if A >= 16:
                assert score[0, 3] == 0 and score[0, 4] == 0 and cls[0, 3] == 0 and cls[0, 4] == 0        # no class wins: class 0, score 0
            if A * batch >= 16:
                assert set((cls[np.isfinite(want['best'])] // 128).tolist()) == set(range(pc.ssd_sweeps(n_classes)))


@pytest.mark.parametrize('A,max_det', pc.SSD_POST)
def test_ssd_second_stage(A, max_det):
    """nms_greedy_f32_k + ssd_gather_k (dd_ssd_postprocess_decoded) against oracle/nets_torch.ssd_postprocess_decoded: tied scores, NaN scores
    and boxes -- the f32 path's order is total (bit keys; a NaN score is no candidate)."""
    from oracle import nets_torch
    ctx, lib, check, ptr = _env()
    cs = [pc.ssd_post_case(A, max_det), pc.ssd_post_case(A, max_det, thr=0.4, iou=0.9)]
    cs[1]['score'] = cs[0]['score'][::-1].copy(); cs[1]['keys'] = cs[0]['keys'][::-1].copy()
    n = len(cs)
    d = [ctx.to_device(np.stack([c[k] for c in cs]), t) for k, t in (('boxes', np.float32), ('score', np.float32), ('cls', np.int32), ('keys', np.float32))]
    ob, oc = _full(ctx, (n, max_det, 4), torch.float32, -7777.0), _full(ctx, (n, max_det), torch.float32, -7777.0)
    os_, on = _full(ctx, (n, max_det), torch.float32, -7777.0), _full(ctx, (n,), torch.int32, -77)
    for c in cs[1:]:
        assert (c['thr'], c['A']) == (cs[0]['thr'], cs[0]['A'])
    # one launch per IoU threshold (the call takes one for the batch)
    for z, c in enumerate(cs):
        check(lib.dd_ssd_postprocess_decoded(ctx.handle, *[ptr(t[z]) for t in d], A, max_det, float(c['thr']), float(c['iou']), ptr(ob[z]), ptr(oc[z]),
                                             ptr(os_[z]), ptr(on[z:]), 1, None), 'dd_ssd_postprocess_decoded')
    gb, gc, gs, gn = (ctx.to_host(t) for t in (ob, oc, os_, on))
    for z, c in enumerate(cs):
        wb, wc, ws, wn = nets_torch.ssd_postprocess_decoded(c['boxes'], c['score'], c['cls'], max_det, c['thr'], c['iou'])
        assert gn[z] == wn and 0 < wn <= max_det, (gn[z], wn)
        _same(gb[z], wb, 'boxes'); _same(gc[z], wc.astype(np.float32), 'classes'); _same(gs[z], ws, 'scores')      # rows behind the count are zero
        assert (c['score'] >= np.float32(c['thr'])).sum() > 10 * wn or max_det == 64


@pytest.mark.parametrize('max_det', pc.FINISH_MAX_DET)
def test_ssd_finish(max_det):
    """ssd_finish_k (dd_ssd_detections) against oracle/detectors_np.ssd_predict_tail, class by class in pick order."""
    ctx, lib, check, ptr = _env()
    N = max_det
    W, H = pc.FINISH_SIZE
    for batch in pc.FINISH_BATCHES:
        boxes, cls, scores, kinds = pc.finish_batch(N, batch)
        d = [ctx.to_device(boxes, np.float32), ctx.to_device(cls, np.float32), ctx.to_device(scores, np.float32)]
        ob, oc = _full(ctx, (batch * N + TAIL, 4), torch.float64, -7777.0), _full(ctx, (batch * N + TAIL,), torch.int32, -77)
        osc, on = _full(ctx, (batch * N + TAIL,), torch.float64, -7777.0), _full(ctx, (batch + TAIL,), torch.int32, -77)
        check(lib.dd_ssd_detections(ctx.handle, *[ptr(t) for t in d], batch, N, pc.FINISH_CONF, pc.FINISH_IOU, W, H, ptr(ob), ptr(oc), ptr(osc), ptr(on), None),
              'dd_ssd_detections')
        ob, oc, osc, on = (ctx.to_host(t) for t in (ob, oc, osc, on))
        assert (on[batch:] == -77).all()
        for z in range(batch):
            want = post_ref.ssd_finish(boxes[z], cls[z], scores[z], pc.FINISH_CONF, pc.FINISH_IOU, W, H)
            n = int(on[z])
            assert n == sum(len(v) for v in want.values()), (max_det, kinds[z], n)
            rows = slice(z * N, z * N + n)
            got = {}
            for b, c, s in zip(ob[rows], oc[rows], osc[rows]):
                got.setdefault(int(c), []).append((tuple(float(v) for v in b), float(s)))
            assert got == want, (max_det, kinds[z])
            assert list(oc[rows]) == sorted(oc[rows])
            rest = slice(z * N + n, (z + 1) * N)                              # rows behind the count: untouched
            assert (ob[rest] == -7777.0).all() and (oc[rest] == -77).all() and (osc[rest] == -7777.0).all()
        assert (ob[batch * N:] == -7777.0).all() and (oc[batch * N:] == -77).all() and (osc[batch * N:] == -7777.0).all()


# ------------------------------------------------------------------------------------------------ suppression, f64
def _nms(mode, boxes, keys, thr):
    """-> (rc, out_n, out_idx [k + TAIL]) of dd_nms (mode 0) / dd_nms_ssd (mode 1); outputs pre-filled with -1"""
    ctx, lib, check, ptr = _env()
    k = len(keys)
    out, cnt = _full(ctx, (k + TAIL,), torch.int32, -1), _full(ctx, (1 + TAIL,), torch.int32, -1)
    fn = lib.dd_nms if mode == 0 else lib.dd_nms_ssd
    d_boxes, d_keys = ctx.to_device(boxes, np.float64), ctx.to_device(keys, np.float64)
    rc = fn(ctx.handle, ptr(d_boxes), ptr(d_keys), k, float(thr), ptr(out), ptr(cnt), None)
    return rc, ctx.to_host(cnt), ctx.to_host(out)


def _check_nms(mode, boxes, keys, thr, what):
    k = len(keys)
    rc, cnt, out = _nms(mode, boxes, keys, thr)
    assert rc == 0, what
    n = int(cnt[0])
    assert 0 <= n <= k and (cnt[1:] == -1).all(), (what, n)
    keep = out[:n]
    assert ((keep >= 0) & (keep < k)).all(), (what, keep.min(), keep.max())   # every index names a box
    assert len(set(keep.tolist())) == n, what                                 # none twice
    assert (out[n:] == -1).all(), what                                        # nothing behind the survivors
    want = post_ref.NMS_REF[mode](boxes, thr, keys)
    assert keep.tolist() == want, (what, n, len(want))
    return want


@pytest.mark.parametrize('k', pc.NMS_SIZES)
@pytest.mark.parametrize('mode', [0, 1])
def test_nms_f64(mode, k):
    """dd_nms / dd_nms_ssd at one size: every kind of case at every threshold against the tie-defined reference; the tie-free case against
    the oracle function itself too (mode 1 up to 129 boxes: its Python loops -- tests/test_post_ref.py holds the larger sizes to it)."""
    for thr in pc.NMS_THRS:
        for kind in pc.NMS_KINDS:
            boxes, keys = pc.nms_case(k, kind, thr, mode)
            want = _check_nms(mode, boxes, keys, thr, (mode, k, kind, thr))
            if kind == 'tie_free' and (mode == 0 or k <= 129):
                with np.errstate(divide='ignore', invalid='ignore'):
                    assert want == [int(i) for i in post_ref.NMS_ORACLE[mode](boxes, thr, keys)]
            if k >= 64 and not pc.nms_exempt(kind, thr):
                assert 0.1 * k <= len(want) <= 0.9 * k, (k, kind, thr, len(want))


@pytest.mark.parametrize('k', pc.NMS_NAN_SIZES)
@pytest.mark.parametrize('mode', [0, 1])
def test_nms_f64_nan_keys_rank_first(mode, k):
    """A NaN key is the largest key, among NaN keys the higher index first: the survivors are the reference's, every index names a box."""
    for thr in pc.NMS_THRS[:2]:
        boxes, keys = pc.nms_case(k, 'tie_free', thr, mode, nan=True)
        want = _check_nms(mode, boxes, keys, thr, (mode, k, 'nan', thr))
        assert np.isnan(keys[want[0]])
    keys = np.full(k, np.nan)                                                 # nothing but NaN keys
    boxes, _ = pc.nms_case(k, 'tie_free', 0.3, mode)
    assert _check_nms(mode, boxes, keys, 0.3, (mode, k, 'all nan'))[0] == k - 1


@pytest.mark.parametrize('mode', [0, 1])
def test_nms_f64_refuses_more_than_its_capacity(mode):
    k = pc.NMS_CAPACITY + 1
    boxes, keys = pc.nms_case(k, 'tie_free', 0.3, mode)
    rc, cnt, out = _nms(mode, boxes, keys, 0.3)
    assert rc < 0
    from deepdish_amd._lib import lib
    assert b'capacity' in lib().dd_last_error()
    assert (out == -1).all() and (cnt == -1).all()                            # refused before anything ran


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize('n', pc.COUNT_SIZES)
def test_counts_accumulate(n):
    ctx, lib, check, ptr = _env()
    a, b, c = pc.counts_inputs(n)
    acc = ctx.to_device(np.concatenate([a, np.full(TAIL, -77, np.int64)]), np.int64)
    check(lib.dd_counts_accumulate(ctx.handle, ptr(acc), ptr(b), n, None), 'dd_counts_accumulate')
    np.testing.assert_array_equal(ctx.to_host(acc)[:n], a + b)
    check(lib.dd_counts_accumulate(ctx.handle, ptr(acc), ptr(c), n, None), 'dd_counts_accumulate')
    got = ctx.to_host(acc)
    np.testing.assert_array_equal(got[:n], a + b + c)
    assert (got[n:] == -77).all() and (np.abs(got[:n]) > 2 ** 32).any() and (got[:n] < 0).any()
