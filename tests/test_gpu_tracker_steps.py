"""GPU: every launch of a tracker step (csrc/tracker.hip) held to tests/tracker_step_ref.py -- kf_predict over the slot list, the whole
matrices of tracker_assoc_k (appearance values, every gate decision, every IoU entry) and what tracker_apply_k wrote, each judged on ONE
step from the device's own previous state; the ragged group launch against groups of one, bit for bit; and the stand-alone cosine, gate
and IoU kernels at the shapes around their tiles and blocks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tracker_step_ref as ref
from oracle import deepsort_np as ds

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ----------------------------------------------------------------------------- one step at a time
@pytest.mark.parametrize('case, association', [('big', 'host'), ('big', 'device'), ('big-euclid', 'host'), ('ring', 'host')])
def test_every_launch_of_a_step_matches_the_reference(case, association):
    """The device tracker and the oracle tracker in lockstep over a case of tracker_step_ref.CASES (track_capacity 256, gallery_capacity
    32: the chunk table is re-built at 33 and 65 samples).  Per frame StepChecker gets the device's state before the frame, its predicted
    covariances, its two cost matrices, its matches and its state after -- see StepChecker.step for what is asserted.  Reached: n_det of
    1, 15 / 16 / 17 and 63 / 64 / 65 (blockIdx.y 0 -> 1); galleries around the 16-row tile and the 32-row chunk, and in a wrapped ring;
    tentative rows, rows at time_since_update 1, 2 and beyond; 1 .. 80 and more track rows."""
    from deepdish_amd.deep_sort import nn_matching
    from deepdish_amd.deep_sort.tracker import Tracker
    from deepdish_amd.deep_sort.detection import Detection
    c = ref.CASES[case]
    trk = Tracker(nn_matching.NearestNeighborDistanceMetric(c['metric'], c['threshold'], c['budget']), max_iou_distance=0.7,
                  max_age=c['max_age'], track_capacity=256, gallery_capacity=32, association=association)
    otrk = ref.oracle_tracker(case)
    chk = ref.StepChecker(c['metric'])
    frames = ref.lockstep_inputs(case)
    for f, frame in enumerate(frames):
        boxes, scores, feats = frame
        dets = [Detection(boxes[i], 'person', scores[i], feats[i]) for i in range(len(boxes))]
        M = np.array([t.mean for t in trk.tracks]).reshape(-1, 8)               # the state after the previous update
        C = np.array([t.covariance for t in trk.tracks]).reshape(-1, 8, 8)
        trk.predict(); otrk.predict()
        trk._fill_covariances()                                                 # the device's predicted covariances (t.mean stays as it was)
        C_pred = np.array([t._covariance for t in trk.tracks]).reshape(-1, 8, 8)
        state = [t.state for t in trk.tracks]
        tsu = [t.time_since_update for t in trk.tracks]
        ids = [t.track_id for t in trk.tracks]
        gallery = {t.track_id: list(otrk.metric.samples[t.track_id]) for t in otrk.tracks if t.state == ds.CONFIRMED}
        trk.update(dets); otrk.update(ref.oracle_dets(frame))
        # the same tracks on both sides: what makes the oracle's gallery the device's
        np.testing.assert_array_equal(ref.table(trk.tracks), ref.table(otrk.tracks), err_msg=f'frame {f}')
        app, iou = trk.last_cost()
        index = {id(d): i for i, d in enumerate(dets)}
        founded = [(t.track_id, index[id(t.detections[-1])]) for t in trk.tracks if t.track_id not in ids]
        chk.step(M, C, C_pred, state, tsu, ids, boxes, feats, gallery, app, iou, trk.last_matches(), founded,
                 [t.track_id for t in trk.tracks], np.array([t.mean for t in trk.tracks]).reshape(-1, 8),
                 np.array([t.covariance for t in trk.tracks]).reshape(-1, 8, 8))
    chk.report('%s, %s association' % (case, association))
    chk.assert_coverage(case)                                                   # the floors, the set conditions, and no gate entry left out
    assert chk.counters['updates'] > 1000 and chk.counters['initiates'] >= 24
    want = dict(device_updates=len(frames), host_updates=0, fallback_streams=0) if association == 'device' else \
        dict(device_updates=0, host_updates=len(frames), fallback_streams=0)
    assert trk.association_stats() == want


# ----------------------------------------------------------------------------- the ragged group launch
def _last_cost(handle):
    """dd_tracker_last_cost through a handle (as tests/test_gpu_euclidean.py::_raw_run calls it) -> appearance, IoU [rows, cols]."""
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    r, c = ctypes.c_int(), ctypes.c_int()
    check(lib().dd_tracker_last_cost(handle, None, None, 0, ctypes.byref(r), ctypes.byref(c)), 'dd_tracker_last_cost')
    app, iou = np.zeros((r.value, c.value)), np.zeros((r.value, c.value))
    if app.size:
        check(lib().dd_tracker_last_cost(handle, ptr(app), ptr(iou), app.size, ctypes.byref(r), ctypes.byref(c)), 'dd_tracker_last_cost')
    return app, iou


GROUP = dict(S=4, F=16, n_obj=90, encoder_max_batch=128)       # 137 crops a step in the group: two encoder launches, one in a group of one


def _group_detections(scenes, f):
    """Per stream what is injected at frame f: stream 0 everything (90 small boxes, more than 80 survive the pipeline's NMS), stream 1 15 /
    16 / 17 boxes, stream 2 one box, stream 3 thirty boxes or, every fourth frame, none.  The counted ones are taken from the boxes that
    survive NMS, so the tracker sees exactly that many."""
    want = [None, (15, 16, 17)[f % 3], 1, 0 if f % 4 == 3 else 30]
    per = []
    for sc, k in zip(scenes, want):
        boxes, scores, _, _ = sc.detections(f)
        take = range(len(boxes)) if k is None else sorted(ds.non_max_suppression(boxes, 0.6, scores))[:k]
        per.append(([tuple(int(v) for v in boxes[i]) for i in take], ['person'] * len(take), [float(scores[i]) for i in take]))
    return per, want


def test_group_of_streams_gives_each_stream_the_bits_of_a_group_of_one():
    """One MultiStreamPipeline of four streams against four pipelines of one stream on the same frames and injected detections.  In the
    group all streams' rows go through ONE tracker_assoc_k grid with per-row det_off / n_det / cost_off / iou_delta; in a group of one
    every offset is zero.  Track table, means, the whole IoU matrix and the confirmed rows of the appearance matrix of every stream and
    frame must agree bit for bit.  The appearance rows also rest on the encoder giving a crop the same bits whatever shares its launch,
    which tests/test_gpu_properties.py holds it to -- for ONE engine: the split of a convolution's K axis, and with it the order of
    every sum, follows the engine's max_batch (csrc/nets.hip: launch_conv), and a pipeline sizes its encoder by its stream count.  So all
    five pipelines get the same encoder_max_batch here; with the defaults (128 crops for four streams, 64 for one) the features, and
    these rows, differ by up to 5e-5 while everything else still agrees.  At least one step has, across the streams, 0, 1, 15..17 and
    >= 65 detections."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = GROUP['S'], GROUP['F']
    scenes = [Scene(seed=300 + z, n_obj=GROUP['n_obj'], n_frames=F, p_miss=0.0, churn=False, n_dup=0.0, wrange=(14, 30), hrange=(30, 60))
              for z in range(S)]
    group = MultiStreamPipeline(S, run_detector=False, encoder_max_batch=GROUP['encoder_max_batch'])
    solos = [MultiStreamPipeline(1, run_detector=False, encoder_max_batch=GROUP['encoder_max_batch']) for _ in range(S)]
    prev = [np.zeros((0, 6), np.int64) for _ in range(S)]
    shapes_seen, iou_entries, app_entries = [], 0, 0
    for f in range(F):
        per, want = _group_detections(scenes, f)
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        group.step(frames, group.pack_injected(per))
        cols = []
        for z in range(S):
            solos[z].step(frames[z:z + 1], solos[z].pack_injected(per[z:z + 1]))
            gv, sv = group.tracker(z), solos[z].tracker(0)
            (gi, gm), (si, sm) = gv.table(), sv.table()
            what = f'frame {f} stream {z}'
            assert gi.shape == si.shape and gi.tobytes() == si.tobytes(), what
            assert gm.tobytes() == sm.tobytes(), what
            (ga, gu), (sa, su) = _last_cost(gv._h), _last_cost(sv._h)
            assert ga.shape == gu.shape == sa.shape == su.shape, what
            assert gu.tobytes() == su.tobytes(), what + ': IoU matrix'
            if ga.size:
                assert ga.shape[0] == len(prev[z]), what                       # the rows are the tracks the previous update left
                confirmed = prev[z][:, 1] == ds.CONFIRMED
                assert ga[confirmed].tobytes() == sa[confirmed].tobytes(), what + ': appearance rows'
                assert np.all((gu == ds.INFTY_COST) | ((gu >= 0) & (gu <= 1))), what
                iou_entries += gu.size
                app_entries += int(confirmed.sum()) * ga.shape[1]
            cols.append(ga.shape[1])                                           # (0 also while the stream has no track yet)
            prev[z] = gi
        shapes_seen.append((want[3], cols))
    # a step with 0, 1, 15..17 and >= 65 detections in its four streams, each of the last three with tracks to associate them with
    ragged = [c for empty, c in shapes_seen if empty == 0 and c[3] == 0 and c[2] == 1 and 15 <= c[1] <= 17 and c[0] >= 65]
    assert ragged, shapes_seen
    assert {c[1] for _, c in shapes_seen} >= {15, 16, 17}
    assert iou_entries > 50000 and app_entries > 30000, (iou_entries, app_entries)
    assert all((group.tracker(z).table()[0][:, 1] == ds.CONFIRMED).any() for z in range(S))


# ----------------------------------------------------------------------------- the stand-alone kernels at their edge shapes
@pytest.fixture(scope='module')
def cosine_case():
    """tests/golden/euclidean.npz's layout -- 12 targets with galleries of 1 .. 65 un-normalised rows, 65 queries -- and the f64 cosine
    reference of every (target, query), computed once."""
    g = np.load(os.path.join(G, 'euclidean.npz'))
    off = np.concatenate([[0], np.cumsum(g['gallery_sizes'])])
    want = np.array([ref.cosine_nn_f64(g['gallery'][off[t]:off[t + 1]], g['query'][:65]) for t in range(12)])
    d = dict(gallery=g['gallery'], sizes=g['gallery_sizes'], query=g['query'][:65], want=want)
    for v in d.values():
        v.setflags(write=False)
    return d


@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65])
def test_standalone_cosine_cost_matches_the_f64_reference(cosine_case, n):
    """dd_cosine_nn_cost through NearestNeighborDistanceMetric('cosine') on rows of norm 0.05 .. 2 (it normalises them itself): n queries
    around the wave's 16 and the block's 64, galleries around the 16-row tile; 2e-6, the cosine tolerance of tests/test_gpu_deepsort.py."""
    from deepdish_amd.deep_sort.nn_matching import NearestNeighborDistanceMetric
    c = cosine_case
    assert set(c['sizes'].tolist()) >= {1, 15, 16, 17, 31, 32, 33, 64, 65}
    targets = list(range(1, 13))
    m = NearestNeighborDistanceMetric('cosine', 0.2, None)
    m.partial_fit(c['gallery'], np.repeat(np.arange(1, 13), c['sizes']), targets)
    got = m.distance(c['query'][:n].copy(), targets)
    assert got.dtype == np.float64 and got.shape == (12, n)
    err = np.abs(got - c['want'][:, :n])
    print('dd_cosine_nn_cost n=%d: worst error %.3g of 2e-6' % (n, err.max()))
    assert np.all(err <= ref.COSINE_TOL), float(err.max())


def _gate_case():
    """Five states and 300 measurements scattered around them (a third near a state, the rest anywhere), with the longdouble d2."""
    m, P, _ = ref.random_states(5, 11)
    rng = np.random.default_rng(12)
    zs = np.stack([rng.uniform(0, 1600, 300), rng.uniform(0, 1200, 300), rng.uniform(0.3, 0.8, 300), rng.uniform(40, 150, 300)], axis=1)
    k = np.arange(0, 300, 3)
    zs[k] = m[k % 5, :4] + rng.standard_normal((len(k), 4)) * np.array([4.0, 4.0, 0.05, 4.0])
    d = dict(m=m, P=P, zs=zs, d2=ref.gating_d2(m, P, zs), d2_pos=ref.gating_d2(m, P, zs, only_position=True))
    for v in d.values():
        v.setflags(write=False)
    for want in (d['d2'], d['d2_pos']):                                               # both sides of the gate
        assert (want < 9.4877).sum() >= 20 and (want > 9.4877).sum() >= 1000
    return d


@pytest.fixture(scope='module')
def gate_case():
    return _gate_case()


@pytest.mark.parametrize('only_position', [False, True])
@pytest.mark.parametrize('n_det', [1, 127, 128, 129, 300])
def test_standalone_gate_matches_the_longdouble_reference(gate_case, n_det, only_position):
    """dd_kf_gate: 5 tracks x n_det measurements around the block's 128-thread stride, at test_kalman_golden's rtol = 1e-11."""
    from deepdish_amd.deep_sort.kalman_filter import KalmanFilter
    c = gate_case
    got = KalmanFilter().gating_distance(c['m'].copy(), c['P'].copy(), c['zs'][:n_det].copy(), only_position=only_position)
    want = (c['d2_pos'] if only_position else c['d2'])[:, :n_det]
    assert got.shape == (5, n_det)
    rel = np.abs(got.astype(np.longdouble) - want) / want
    print('dd_kf_gate n_det=%d only_position=%d: worst relative error %.3g of 1e-11' % (n_det, only_position, float(rel.max())))
    assert np.all(rel <= 1e-11), float(rel.max())


IOU_SHAPES = [(1, 1), (15, 17), (16, 16), (17, 15), (3, 171)]


def _iou_case():
    """17 track boxes and 171 candidate boxes with fractional coordinates; candidates 0 .. 16 repeat or nudge a track box, so the IoU
    is 1, close to 1, partial and 0."""
    rng = np.random.default_rng(13)
    box = lambda k: np.stack([rng.uniform(0, 300, k), rng.uniform(0, 300, k), rng.uniform(10, 80, k), rng.uniform(20, 120, k)], axis=1)
    a, b = box(17), box(171)
    b[:17] = a
    b[1:17, :2] += rng.uniform(-6, 6, (16, 2))
    d = dict(a=a, b=b, iou=np.array([ds.iou(x, b) for x in a]))
    for v in d.values():
        v.setflags(write=False)
    for n_t, n_d in IOU_SHAPES[1:]:
        u = d['iou'][:n_t, :n_d]
        assert u.max() > 1 - 1e-12 and (u == 0).any() and ((u > 0.05) & (u < 0.95)).any(), (n_t, n_d)
    return d


@pytest.fixture(scope='module')
def iou_case():
    return _iou_case()


@pytest.mark.parametrize('with_tsu', [False, True])
@pytest.mark.parametrize('n_t, n_d', IOU_SHAPES)
def test_standalone_iou_cost_matches_the_oracle(iou_case, n_t, n_d, with_tsu):
    """dd_iou_cost at 1, 255, 256, 255 and 513 elements (the last partial 256-thread block), with and without time_since_update, at
    test_iou_golden's tolerance."""
    from deepdish_amd.deep_sort import iou_matching
    c = iou_case
    tsu = np.array([1 + (k % 3 == 1) * (1 + k) for k in range(n_t)], dtype=np.int32) if with_tsu else None     # 1, 3, 1, 1, 6, 1, ...
    cost = iou_matching._iou_cost_arrays(c['a'][:n_t].copy(), tsu, c['b'][:n_d].copy())
    assert cost.shape == (n_t, n_d)
    barred = (tsu > 1) if with_tsu else np.zeros(n_t, bool)
    assert np.all(cost[barred] == ds.INFTY_COST)
    np.testing.assert_allclose(1.0 - cost[~barred], c['iou'][:n_t, :n_d][~barred], rtol=1e-15, atol=1e-16)
