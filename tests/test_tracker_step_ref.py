"""CPU: tests/tracker_step_ref.py itself.  Its longdouble Kalman filter against oracle.deepsort_np on random states; the oracle tracker
run alone through StepChecker over every case (it must pass with tolerance to spare, and reach the coverage the cases were built for);
and nine deliberately wrong stand-ins for the device, each of which the checker must catch in the item that owns the fault."""
import functools

import numpy as np
import pytest

import tracker_step_ref as ref
from oracle import deepsort_np as ds


# ----------------------------------------------------------------------------- the helper agrees with the oracle
def test_longdouble_filter_agrees_with_the_oracle():
    """predict / project / update / gating_d2 rounded to f64 against oracle.deepsort_np.kf_*, at the tolerances the checker uses for the
    same functions (tests/test_gpu_deepsort.py::test_kalman_golden's); initiate: the mean exactly, the covariance at item 5's 1e-15 (the
    oracle squares 2 * (1 / 20) * h in f64: three roundings away from the longdouble value)."""
    m, P, z = ref.random_states(200, 7)
    pm, pc = ref.predict(m, P)                                     # the batch form ...
    assert pm.dtype == np.longdouble and pc.shape == (200, 8, 8)
    for i in range(200):
        om, oc = ds.kf_predict(m[i], P[i])
        np.testing.assert_array_equal(pm[i].astype(np.float64), om)
        np.testing.assert_allclose(pc[i].astype(np.float64), oc, rtol=1e-13, atol=1e-18)
        sm, sc = ref.predict(m[i], P[i])                           # ... and one state at a time
        assert np.array_equal(sm, pm[i]) and np.array_equal(sc, pc[i])
        jm, jc = ref.project(m[i], P[i])
        om, oc = ds.kf_project(m[i], P[i])
        np.testing.assert_array_equal(jm.astype(np.float64), om)
        np.testing.assert_allclose(jc.astype(np.float64), oc, rtol=1e-13, atol=1e-18)
        um, uc = ref.update(m[i], P[i], z[i])
        om, oc = ds.kf_update(m[i], P[i], z[i])
        np.testing.assert_allclose(um.astype(np.float64), om, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(uc.astype(np.float64), oc, rtol=1e-10, atol=1e-13)
        zs = z[(i + np.arange(5)) % 200]
        for pos in (False, True):
            np.testing.assert_allclose(ref.gating_d2(m[i], P[i], zs, pos).astype(np.float64),
                                       ds.kf_gating_distance(m[i], P[i], zs, pos), rtol=1e-11)
        im, ic = ref.initiate(z[i])
        om, oc = ds.kf_initiate(z[i])
        np.testing.assert_array_equal(im.astype(np.float64), om)
        np.testing.assert_allclose(ic.astype(np.float64), oc, rtol=1e-15, atol=0)
    um, uc = ref.update(m, P, z)                                   # batch forms of the rest
    assert np.array_equal(um[3], ref.update(m[3], P[3], z[3])[0]) and np.array_equal(uc[3], ref.update(m[3], P[3], z[3])[1])
    assert np.array_equal(ref.gating_d2(m[:4], P[:4], z[:9])[2], ref.gating_d2(m[2], P[2], z[:9]))


def test_appearance_references():
    rng = np.random.default_rng(3)
    g = (rng.standard_normal((17, 128)) * rng.uniform(0.5, 2, (17, 1))).astype(np.float32)
    q = (rng.standard_normal((5, 128)) * rng.uniform(0.5, 2, (5, 1))).astype(np.float32)
    q[2] = 3 * g[11]
    got = ref.cosine_nn_f64(g, q)
    assert got.dtype == np.float64 and abs(got[2]) < 1e-15
    assert np.abs(got - ds.nn_cosine_distance(g, q)).max() <= 2e-6          # the f32 oracle sits inside the stated tolerance


# ----------------------------------------------------------------------------- the oracle through the checker
@functools.lru_cache(maxsize=None)
def _oracle_run(case):
    """oracle.deepsort_np.Tracker alone over a case, standing in for the device: per frame its f64 state before and after, and the
    matrices and decisions of its own _gated_metric / iou_cost / _match."""
    trk = ref.oracle_tracker(case)
    seen = {}
    match, distance = trk._match, trk.metric.distance

    def _match(dets):
        seen['match'] = match(dets)
        return seen['match']

    def _distance(feats, targets):
        seen['raw'] = distance(feats, targets)
        return seen['raw'].copy()
    trk._match, trk.metric.distance = _match, _distance
    recs = []
    for boxes, scores, feats in ref.lockstep_inputs(case):
        dets = ref.oracle_dets((boxes, scores, feats))
        M = np.array([t.mean for t in trk.tracks]).reshape(-1, 8)
        C = np.array([t.covariance for t in trk.tracks]).reshape(-1, 8, 8)
        trk.predict()
        T, n = len(trk.tracks), len(dets)
        state = np.array([t.state for t in trk.tracks], dtype=np.int64)
        conf = [i for i in range(T) if state[i] == ds.CONFIRMED]
        app, iou, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((0, n))
        zs = np.array([d.to_xyah() for d in dets]).reshape(-1, 4)
        if T and n:
            iou = ds.iou_cost(trk.tracks, dets, list(range(T)), list(range(n)))
        if conf and n:
            app[conf] = trk._gated_metric(trk.tracks, dets, conf, list(range(n)))
            raw = seen['raw']
        r = dict(M=M, C=C, C_pred=np.array([t.covariance for t in trk.tracks]).reshape(-1, 8, 8),
                 M_pred=np.array([t.mean for t in trk.tracks]).reshape(-1, 8), state=state,
                 tsu=np.array([t.time_since_update for t in trk.tracks], dtype=np.int64),
                 track_id=np.array([t.track_id for t in trk.tracks], dtype=np.int64), tlwh=boxes.astype(np.float64), feats=feats, zs=zs,
                 gallery={trk.tracks[i].track_id: list(trk.metric.samples[trk.tracks[i].track_id]) for i in conf},
                 conf=conf, app=app, iou=iou, raw=raw,
                 d2=np.array([ds.kf_gating_distance(trk.tracks[i].mean, trk.tracks[i].covariance, zs) for i in conf]) if conf and n else None)
        first_new = trk._next_id
        trk.update(dets)
        matches, _, un_d = seen['match']
        r.update(matches=matches, founded=[(first_new + k, d) for k, d in enumerate(un_d)],
                 ids_new=np.array([t.track_id for t in trk.tracks], dtype=np.int64),
                 M_new=np.array([t.mean for t in trk.tracks]).reshape(-1, 8),
                 C_new=np.array([t.covariance for t in trk.tracks]).reshape(-1, 8, 8))
        recs.append(r)
    return recs


def _check(case, mutate=None):
    chk = ref.StepChecker(ref.CASES[case]['metric'])
    for r in _oracle_run(case):
        if mutate is not None:
            r = mutate(dict(r))
        chk.step(r['M'], r['C'], r['C_pred'], r['state'], r['tsu'], r['track_id'], r['tlwh'], r['feats'], r['gallery'], r['app'], r['iou'],
                 r['matches'], r['founded'], r['ids_new'], r['M_new'], r['C_new'], d2=r['d2'])
    return chk


@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_oracle_passes_the_checker_with_tolerance_to_spare(case):
    chk = _check(case)
    chk.report('oracle, ' + case)
    chk.assert_coverage(case)
    cn = chk.counters
    assert cn['updates'] > 1000 and cn['initiates'] >= 24
    for name, (measured, floor) in ref.COVERAGE[case]['floors'].items():
        assert cn[name] == measured and 0.75 * measured <= floor <= 0.82 * measured, (name, cn[name], measured, floor)   # the table states what this run gives
    # items 1, 3 and 5: the f64 oracle uses at most 1 % of each tolerance on these states, so none of them is tight for a correct f64
    # implementation -- even for covariances that were predicted 31 times without an update.  (The covariance of a new track is held to
    # 1e-15, a few roundings: there is no room to spare there, and none is claimed.)
    for name in ('predict_cov', 'd2', 'update_mean', 'update_cov'):
        assert chk.worst[name] < 0.01, (name, chk.worst[name])
    assert chk.worst['initiate_cov'] <= 1.0 and chk.worst['gate_margin'] > 1e-5


# ----------------------------------------------------------------------------- the checker bites
def _d2_f64(m, P, zs, w_pos=1.0 / 20):
    sd = np.array([w_pos * m[3], w_pos * m[3], 1e-1, w_pos * m[3]])
    L = np.linalg.cholesky(P[:4, :4] + np.diag(sd * sd))
    y = np.linalg.solve(L, (zs - m[:4]).T)
    return (y * y).sum(axis=0)


def _regate(r, means, **kw):
    if r['conf'] and len(r['zs']):
        r['app'] = r['app'].copy()
        for k, i in enumerate(r['conf']):
            r['app'][i] = np.where(_d2_f64(means[i], r['C_pred'][i], r['zs'], **kw) > ds.CHI2INV95_4, ds.INFTY_COST, r['raw'][k])
    return r


def _gate_w_pos(r):
    return _regate(r, r['M_pred'], w_pos=1.0 / 19)


def _gate_from_old_mean(r):
    return _regate(r, r['M'])


def _iou_plus_one(r):
    def iou1(box, cands):
        tl = np.maximum(box[:2], cands[:, :2])
        br = np.minimum(box[:2] + box[2:], cands[:, :2] + cands[:, 2:])
        wh = np.maximum(0.0, br - tl + 1)
        inter = wh[:, 0] * wh[:, 1]
        return inter / ((box[2] + 1) * (box[3] + 1) + (cands[:, 2] + 1) * (cands[:, 3] + 1) - inter)
    if r['iou'].size:
        r['iou'] = np.array([np.full(len(r['tlwh']), ds.INFTY_COST) if r['tsu'][i] > 1 else
                             1.0 - iou1(ds.mean_to_tlwh(r['M_pred'][i]), r['tlwh']) for i in range(len(r['M']))])
    return r


def _iou_rows_not_barred(r):
    if r['iou'].size:
        r['iou'] = np.array([1.0 - ds.iou(ds.mean_to_tlwh(m), r['tlwh']) for m in r['M_pred']])
    return r


def _reappear(r, rows_of, feats):
    if r['conf'] and len(r['zs']):
        r['app'] = r['app'].copy()
        for i in r['conf']:
            cost = ds.nn_cosine_distance(rows_of(r['gallery'][int(r['track_id'][i])]), feats)
            r['app'][i] = np.where(r['app'][i] == ds.INFTY_COST, ds.INFTY_COST, cost)
    return r


def _last_gallery_row_ignored(r):
    return _reappear(r, lambda rows: rows[:-1] if len(rows) > 1 else rows, r['feats'])


def _features_shifted(r):
    return _reappear(r, lambda rows: rows, np.roll(r['feats'], 1, axis=0))


def _predict_w_vel(r):
    r['C_pred'] = r['C_pred'].copy()
    for i, m in enumerate(r['M']):
        for k in (4, 5, 7):
            r['C_pred'][i, k, k] += (m[3] / 150) ** 2 - (m[3] / 160) ** 2
    return r


def _update_cov_without_noise(r):
    r['C_new'] = r['C_new'].copy()
    where = {int(t): k for k, t in enumerate(r['ids_new'])}
    for i, _ in r['matches']:
        m, P = r['M_pred'][i], r['C_pred'][i]
        _, S = ds.kf_project(m, P)
        K = np.linalg.solve(S, P[:4, :]).T
        r['C_new'][where[int(r['track_id'][i])]] = P - K @ P[:4, :4] @ K.T          # H P H^T where S belongs
    return r


def _initiate_w_pos(r):
    r['C_new'] = r['C_new'].copy()
    where = {int(t): k for k, t in enumerate(r['ids_new'])}
    for t, d in r['founded']:
        for k in (0, 1, 3):
            r['C_new'][where[t], k, k] = (r['zs'][d][3] / 20) ** 2
    return r


@pytest.mark.parametrize('mutate, item', [
    (_gate_w_pos, 3), (_gate_from_old_mean, 3), (_iou_plus_one, 2), (_iou_rows_not_barred, 2), (_last_gallery_row_ignored, 4),
    (_features_shifted, 4), (_predict_w_vel, 1), (_update_cov_without_noise, 5), (_initiate_w_pos, 5)],
    ids=lambda v: v.__name__.strip('_') if callable(v) else str(v))
def test_the_checker_catches(mutate, item):
    """One fault at a time in the stand-in for the device, everything else the oracle's: the `big` run must fail, in the item named."""
    with pytest.raises(ref.StepMismatch) as e:
        _check('big', mutate)
    print(e.value)
    assert e.value.item == item, str(e.value)
