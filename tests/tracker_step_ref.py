"""TEST INFRASTRUCTURE ONLY -- a one-step reference for every launch of the HBM-resident tracker (csrc/tracker.hip): the Kalman filter
restated in extended precision, float64 appearance references, the scenes the step tests run, and StepChecker, which holds what ONE
frame's predict / association / apply produced to those references, starting from the state the implementation under test itself
had before the frame.  A filter recursion contracts errors; a single step does not.  No GPU import: tests/test_tracker_step_ref.py
runs the checker on the CPU against oracle.deepsort_np (and against nine deliberately wrong stand-ins), tests/test_gpu_tracker_steps.py
runs it against the device tracker.
"""
import numpy as np

import euclidean_ref as er
from oracle import deepsort_np as ds

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, 'numpy.longdouble is no wider than float64 here: the extended-precision reference needs the x87 80-bit format'

GATE = LD(ds.CHI2INV95_4)          # the threshold as the device holds it: 9.4877 rounded to float64
INFTY = ds.INFTY_COST
GATE_BAND = 1e-11                  # relative; the project's tolerance of dd_kf_gate (tests/test_gpu_deepsort.py::test_kalman_golden)
COSINE_TOL = 2e-6                  # tests/test_gpu_tracker.py / tests/test_gpu_deepsort.py::test_cosine_golden


# --------------------------------------------------------------------------- Kalman filter, longdouble (kalman_filter.py:23-229 upstream)
# Every function takes one state (m [8], P [8, 8]) or a batch of them (leading dimensions).  Products are written out; the 4 x 4 Cholesky
# factor and the two triangular solves are plain loops -- no LAPACK, which has no longdouble anyway.
def _ld(x):
    return np.array(x, dtype=LD)


def _std_project(h):
    """kalman_filter.py:140-145: (h/20, h/20, 1/10, h/20)."""
    one = np.ones_like(h)
    return np.stack([h / LD(20), h / LD(20), one * (LD(1) / LD(10)), h / LD(20)], axis=-1)


def _std_predict(h):
    """kalman_filter.py:107-117: positions h/20 (aspect 1/100), velocities h/160 (aspect 1/100000)."""
    one = np.ones_like(h)
    return np.stack([h / LD(20), h / LD(20), one * (LD(1) / LD(100)), h / LD(20),
                     h / LD(160), h / LD(160), one * (LD(1) / LD(100000)), h / LD(160)], axis=-1)


def _std_initiate(h):
    """kalman_filter.py:75-84: 2 h/20 and 10 h/160."""
    one = np.ones_like(h)
    return np.stack([2 * (h / LD(20)), 2 * (h / LD(20)), one * (LD(1) / LD(100)), 2 * (h / LD(20)),
                     10 * (h / LD(160)), 10 * (h / LD(160)), one * (LD(1) / LD(100000)), 10 * (h / LD(160))], axis=-1)


def _chol(S):
    """Lower Cholesky factor of S [..., n, n]."""
    n = S.shape[-1]
    L = np.zeros_like(S)
    for i in range(n):
        for j in range(i + 1):
            s = S[..., i, j].copy()
            for k in range(j):
                s = s - L[..., i, k] * L[..., j, k]
            L[..., i, j] = np.sqrt(s) if i == j else s / L[..., j, j]
    return L


def _solve_lower(L, B):
    """Y with L Y = B; L [..., n, n] lower, B [..., n, m]."""
    n = L.shape[-1]
    Y = np.zeros_like(B)
    for i in range(n):
        s = B[..., i, :].copy()
        for k in range(i):
            s = s - L[..., i, k, None] * Y[..., k, :]
        Y[..., i, :] = s / L[..., i, i, None]
    return Y


def _solve_upper_t(L, Y):
    """X with L^T X = Y."""
    n = L.shape[-1]
    X = np.zeros_like(Y)
    for i in reversed(range(n)):
        s = Y[..., i, :].copy()
        for k in range(i + 1, n):
            s = s - L[..., k, i, None] * X[..., k, :]
        X[..., i, :] = s / L[..., i, i, None]
    return X


def initiate(z):
    """kalman_filter.py:55-86.  z = (cx, cy, a, h) -> mean [..., 8], covariance [..., 8, 8]."""
    z = _ld(z)
    m = np.concatenate([z, np.zeros_like(z)], axis=-1)
    sd = _std_initiate(z[..., 3])
    P = np.zeros(z.shape[:-1] + (8, 8), dtype=LD)
    for i in range(8):
        P[..., i, i] = sd[..., i] * sd[..., i]
    return m, P


def predict(m, P):
    """kalman_filter.py:88-123: F m, F P F^T + Q with F = [[I, I], [0, I]] and Q from the height BEFORE the step."""
    m, P = _ld(m), _ld(P)
    sd = _std_predict(m[..., 3])
    out = m.copy()
    out[..., :4] += m[..., 4:]
    B = P.copy()
    B[..., :, :4] += P[..., :, 4:]                       # P F^T
    R = B.copy()
    R[..., :4, :] += B[..., 4:, :]                       # F (P F^T)
    for i in range(8):
        R[..., i, i] += sd[..., i] * sd[..., i]
    return out, R


def project(m, P):
    """kalman_filter.py:125-152: H m, H P H^T + R with H = [I, 0]."""
    m, P = _ld(m), _ld(P)
    sd = _std_project(m[..., 3])
    S = P[..., :4, :4].copy()
    for i in range(4):
        S[..., i, i] += sd[..., i] * sd[..., i]
    return m[..., :4].copy(), S


def update(m, P, z):
    """kalman_filter.py:154-186: K = P H^T S^-1 by the Cholesky factor of S, m + K (z - H m), P - K S K^T."""
    m, P, z = _ld(m), _ld(P), _ld(z)
    pm, S = project(m, P)
    L = _chol(S)
    Kt = _solve_upper_t(L, _solve_lower(L, P[..., :4, :].copy()))        # S^-1 (H P) = K^T, [..., 4, 8]
    innov = z - pm
    out = m.copy()
    for k in range(4):
        out = out + innov[..., k, None] * Kt[..., k, :]
    SKt = np.zeros_like(Kt)                                              # S K^T
    for a in range(4):
        for b in range(4):
            SKt[..., a, :] += S[..., a, b, None] * Kt[..., b, :]
    KSKt = np.zeros_like(P)
    for a in range(4):
        KSKt += Kt[..., a, :, None] * SKt[..., a, None, :]
    return out, P - KSKt


def gating_d2(m, P, zs, only_position=False):
    """kalman_filter.py:188-229: squared Mahalanobis distance of every measurement zs [N, 4] to the projected state(s): [..., N]."""
    pm, S = project(m, P)
    zs = _ld(zs)
    k = 2 if only_position else 4
    L = _chol(S[..., :k, :k])
    d = zs[..., :k] - pm[..., None, :k]                                  # [..., N, k]
    y = _solve_lower(L, np.swapaxes(d, -1, -2))
    return (y * y).sum(axis=-2)


def random_states(n, seed):
    """Well-conditioned filter states: boxes of 40 .. 150 px height on the big scene's canvas, covariance D (I + 0.3 B B^T / 8) D with
    D the standard deviations a new track starts with -- symmetric positive definite, correlated, scaled like the tracker's."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(40, 150, n)
    m = np.stack([rng.uniform(0, 1600, n), rng.uniform(0, 1200, n), rng.uniform(0.3, 0.8, n), h,
                  rng.uniform(-3, 3, n), rng.uniform(-1, 1, n), rng.uniform(-1e-3, 1e-3, n), rng.uniform(-1, 1, n)], axis=1)
    P = np.zeros((n, 8, 8))
    for i in range(n):
        d = np.sqrt(np.diag(ds.kf_initiate(m[i, :4])[1]))
        b = rng.standard_normal((8, 8))
        P[i] = d[:, None] * (np.eye(8) + 0.3 * (b @ b.T) / 8) * d[None, :]
    z = m[:, :4] + rng.standard_normal((n, 4)) * np.stack([h / 20, h / 20, np.full(n, 0.05), h / 20], axis=1)
    return m, P, z


# --------------------------------------------------------------------------- appearance, float64 from the f32 rows as stored
def cosine_nn_f64(gallery, queries):
    """1 - max over the gallery rows of the cosine with every query row (nn_matching.py:31-54, 78-96), rows normalised in f64."""
    g = np.asarray(gallery, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    g = g / np.sqrt((g * g).sum(axis=1, keepdims=True))
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    return 1.0 - (g @ q.T).max(axis=0)


# --------------------------------------------------------------------------- the scenes
# frame % 20 -> detections kept (None: all that survive NMS): n_det of 1 (every lane clamps to detection 0), around the wave's 16 and
# around the block's 64 (blockIdx.y 0 -> 1)
SCHEDULE = {3: 1, 6: 15, 9: 16, 11: 17, 14: 63, 16: 64, 18: 65}

_BIG = dict(seed=41, n_obj=80, width=1600, height=1200, n_frames=84, p_miss=0.05, churn=True, n_dup=0.0)
CASES = {
    'big': dict(scene=_BIG, schedule=True, scale=None, metric='cosine', threshold=0.2, max_age=30, budget=None),
    'big-euclid': dict(scene=_BIG, schedule=True, scale=(0.6, 1.6), metric='euclidean', threshold=0.4, max_age=30, budget=None),
    'ring': dict(scene=dict(seed=43, n_obj=24, n_frames=70, p_miss=0.1, n_dup=0.0), schedule=False, scale=None, metric='cosine',
                 threshold=0.2, max_age=8, budget=40),
}

# What a run of a case must have reached.  sets: values that must occur; floors: about 80 % of what oracle.deepsort_np alone reaches (measured
# on the CPU, the first number of each pair; tests/test_tracker_step_ref.py holds the table to that run) -- the slack allows for last-bit differences between device and oracle state, it is a floor
# on coverage and no tolerance.
_BIG_SETS = dict(ndet={1, 15, 16, 17, 63, 64, 65}, gallery={3, 15, 16, 17, 31, 32, 33, 63, 64, 65})
COVERAGE = {
    'big': dict(sets=_BIG_SETS, min_max_tsu=31,
                floors=dict(live=(4583, 3500), gated=(308541, 250000), near_lo=(351, 280), near_hi=(925, 700), iou_mid=(4941, 3800),
                            inf_rows=(1558, 1200), tentative_rows=(266, 200))),
    'big-euclid': dict(sets=_BIG_SETS, min_max_tsu=31,
                       floors=dict(live=(4579, 3663), gated=(307823, 246258), near_lo=(350, 280), near_hi=(931, 744), iou_mid=(4943, 3954),
                                   inf_rows=(1552, 1241), tentative_rows=(274, 219))),
    'ring': dict(sets=dict(ndet=set(), gallery={40}), min_max_tsu=9, max_gallery=40,
                 floors=dict(live=(1246, 996), gated=(25617, 20493), near_lo=(43, 34), near_hi=(196, 156), iou_mid=(2375, 1900),
                             inf_rows=(236, 188), tentative_rows=(62, 49))),
}


def lockstep_inputs(case):
    """-> per frame (tlwh int64 [n, 4], scores f64 [n], features f32 [n, 128]): what goes into the tracker, after NMS and the schedule."""
    from deepdish_amd.synth import Scene
    c = CASES[case]
    scene = Scene(**c['scene'])
    rng = np.random.default_rng(42)                                # one generator for the whole run
    out = []
    for f in range(scene.n_frames):
        boxes, scores, _, feats = scene.detections(f)
        if c['scale']:
            feats = er.scale_features(feats, f, *c['scale'])
        keep = ds.non_max_suppression(boxes, 0.6, scores)
        k = SCHEDULE.get(f % 20) if c['schedule'] else None
        if k is not None and len(keep) > k:
            keep = sorted(rng.choice(keep, k, replace=False).tolist())
        out.append((boxes[keep].reshape(-1, 4), scores[keep], np.ascontiguousarray(feats[keep], dtype=np.float32).reshape(-1, 128)))
    return out


def oracle_tracker(case):
    c = CASES[case]
    metric = (er.Metric if c['metric'] == 'euclidean' else ds.Metric)(c['threshold'], c['budget'])
    return ds.Tracker(metric, max_iou_distance=0.7, max_age=c['max_age'])


def oracle_dets(frame):
    boxes, scores, feats = frame
    return [ds.Det(boxes[i], 'person', scores[i], feats[i]) for i in range(len(boxes))]


def table(tracks):
    return np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in tracks], dtype=np.int64).reshape(-1, 5)


# --------------------------------------------------------------------------- the checker
class StepMismatch(AssertionError):
    """One item of StepChecker.step failed: .item is its number (1 predict, 2 IoU, 3 gate, 4 appearance, 5 apply)."""

    def __init__(self, item, frame, text):
        super().__init__('frame %d, item %d: %s' % (frame, item, text))
        self.item, self.frame = item, frame


class StepChecker:
    """One object per run; step() once per frame.  Every tolerance is one the project already states for the same device function.
    .counters: what the run covered; .band: gate entries left out because they sat on the threshold; .worst: per comparison the largest
    error seen as a fraction of its tolerance."""

    def __init__(self, metric='cosine'):
        assert metric in ('cosine', 'euclidean')
        self.metric = metric
        self.frame = -1
        self.band = 0
        self.counters = dict(ndet=set(), gallery=set(), live=0, gated=0, near_lo=0, near_hi=0, iou_mid=0, inf_rows=0, tentative_rows=0,
                             updates=0, initiates=0, max_tsu=0)
        self.worst = dict(predict_cov=0.0, iou=0.0, gate_margin=np.inf, appearance=0.0, update_mean=0.0, update_cov=0.0, initiate_cov=0.0)

    def _close(self, item, name, got, want, rtol, atol, what):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            raise StepMismatch(item, self.frame, '%s: shape %r, expected %r' % (what, got.shape, want.shape))
        if got.size == 0:
            return
        err = np.abs(got.astype(LD) - want)
        with np.errstate(divide='ignore', invalid='ignore'):        # (no error is no error, also where the tolerance is 0)
            frac = np.where(err == 0, LD(0), err / (atol + rtol * np.abs(want)))
        w = float(frac.max())
        if not w <= 1.0:                                            # (a NaN fails here too)
            k = np.unravel_index(int(np.argmax(np.where(np.isnan(frac), np.inf, frac))), frac.shape)
            raise StepMismatch(item, self.frame, '%s: %.3g tolerances at %r (got %r, reference %r; rtol %g, atol %g)'
                               % (what, w, k, float(got[k]), float(want[k]), rtol, atol))
        self.worst[name] = max(self.worst[name], w)

    def step(self, M, C, C_pred, state, tsu, track_id, tlwh, feats, gallery, app, iou, matches, founded, ids_new, M_new, C_new, d2=None):
        """M [T, 8], C [T, 8, 8]: the state after the previous update.  C_pred [T, 8, 8]: the covariances after predict.  state, tsu,
        track_id [T]: per row, after predict.  tlwh [n, 4], feats f32 [n, 128]: the detections.  gallery: track id -> stored rows, for
        every confirmed id.  app, iou [T, n]: the cost matrices of the update (unconfirmed rows of app are not read).  matches: (row,
        detection) pairs.  founded: (track id, detection) of the tracks this update started.  ids_new [T'], M_new [T', 8], C_new
        [T', 8, 8]: the live tracks after the update.  d2 (optional, [confirmed rows, n]): the implementation's own gating distances;
        only their error is recorded (.worst['d2'], as a fraction of 1e-11 relative)."""
        self.frame += 1
        cn = self.counters
        M = np.asarray(M, dtype=np.float64).reshape(-1, 8)
        T, n = len(M), len(tlwh)
        C = np.asarray(C, dtype=np.float64).reshape(T, 8, 8)
        C_pred = np.asarray(C_pred, dtype=np.float64).reshape(T, 8, 8)
        state, tsu, track_id = (np.asarray(v, dtype=np.int64).reshape(T) for v in (state, tsu, track_id))
        tlwh = np.asarray(tlwh, dtype=np.float64).reshape(n, 4)
        # the predicted means: one IEEE add per element, the add predict_wave does
        M_pred = M.copy()
        M_pred[:, :4] = M[:, :4] + M[:, 4:]
        if T:
            cn['max_tsu'] = max(cn['max_tsu'], int(tsu.max()))
        conf = np.nonzero(state == ds.CONFIRMED)[0]

        # ---- 1. predict
        if T:
            self._close(1, 'predict_cov', C_pred, predict(M, C)[1], 1e-13, 1e-18, 'predicted covariance')

        if T and n:
            app, iou = np.asarray(app, dtype=np.float64), np.asarray(iou, dtype=np.float64)
            for name, a in (('appearance', app), ('IoU', iou)):
                if a.shape != (T, n):
                    raise StepMismatch(2, self.frame, '%s cost matrix is %r, expected %r' % (name, a.shape, (T, n)))
            # ---- 2. IoU, every row
            far = tsu > 1
            if not np.all(iou[far] == INFTY):
                raise StepMismatch(2, self.frame, 'IoU rows of tracks with time_since_update > 1 are not all 1e5')
            near = np.nonzero(~far)[0]
            want = np.array([ds.iou(ds.mean_to_tlwh(M_pred[r]), tlwh) for r in near]).reshape(len(near), n)
            self._close(2, 'iou', 1.0 - iou[near], want, 1e-15, 1e-16, 'IoU')
            cn['iou_mid'] += int(((iou[near] > 0) & (iou[near] < 1)).sum())
            cn['inf_rows'] += int(far.sum())
            cn['tentative_rows'] += int((state[near] == ds.TENTATIVE).sum())

        if len(conf) and n:
            cn['ndet'].add(n)
            zs = np.array([ds.tlwh_to_xyah(b) for b in tlwh])
            # ---- 3. gate, confirmed rows, every entry
            d2_ref = gating_d2(M_pred[conf], C_pred[conf], zs)
            rel = np.abs(d2_ref - GATE) / GATE
            band = rel <= GATE_BAND
            self.band += int(band.sum())
            gated_ref = d2_ref > GATE
            gated_got = app[conf] == INFTY
            bad = (gated_ref != gated_got) & ~band
            if bad.any():
                r, d = np.argwhere(bad)[0]
                raise StepMismatch(3, self.frame, '%d gate decisions differ; track %d x detection %d: d2 = %.17g, cost %r'
                                   % (bad.sum(), track_id[conf[r]], d, float(d2_ref[r, d]), app[conf[r], d]))
            self.worst['gate_margin'] = min(self.worst['gate_margin'], float(rel.min()))
            if d2 is not None:
                e = float((np.abs(np.asarray(d2).astype(LD) - d2_ref) / d2_ref).max()) / GATE_BAND
                self.worst['d2'] = max(self.worst.get('d2', 0.0), e)
            use = ~band
            cn['live'] += int((~gated_ref & use).sum())
            cn['gated'] += int((gated_ref & use).sum())
            cn['near_lo'] += int(((d2_ref >= 4) & (d2_ref < GATE) & use).sum())
            cn['near_hi'] += int(((d2_ref > GATE) & (d2_ref < 20) & use).sum())
            # ---- 4. appearance, confirmed rows, ungated entries
            for k, r in enumerate(conf):
                rows = np.asarray(gallery[int(track_id[r])], dtype=np.float32).reshape(-1, 128)
                cn['gallery'].add(len(rows))
                cols = np.nonzero(~gated_ref[k] & use[k])[0]
                if not len(cols):
                    continue
                got = app[r, cols]
                what = 'appearance cost of track %d (%d rows)' % (track_id[r], len(rows))
                if self.metric == 'cosine':
                    self._close(4, 'appearance', got, cosine_nn_f64(rows, feats[cols]), 0.0, COSINE_TOL, what)
                else:
                    if not np.all(got >= 0.0):
                        raise StepMismatch(4, self.frame, what + ': negative')
                    want = er.nn_euclidean_distance_f64(rows, feats[cols])
                    tol = er.tolerance(rows, feats[cols])
                    self._close(4, 'appearance', got / tol, want / tol, 0.0, 1.0, what)

        # ---- 5. apply
        ids_new = np.asarray(ids_new, dtype=np.int64).reshape(-1)
        M_new = np.asarray(M_new, dtype=np.float64).reshape(len(ids_new), 8)
        C_new = np.asarray(C_new, dtype=np.float64).reshape(len(ids_new), 8, 8)
        where = {int(t): k for k, t in enumerate(ids_new)}
        matches = [(int(r), int(d)) for r, d in matches]
        if matches:
            rows = np.array([r for r, _ in matches])
            if not all(int(track_id[r]) in where for r in rows):
                raise StepMismatch(5, self.frame, 'a matched track is not in the table after the update')
            at = np.array([where[int(track_id[r])] for r in rows])
            z = np.array([ds.tlwh_to_xyah(tlwh[d]) for _, d in matches])
            want_m, want_c = update(M_pred[rows], C_pred[rows], z)
            self._close(5, 'update_mean', M_new[at], want_m, 1e-11, 1e-11, 'updated mean')
            self._close(5, 'update_cov', C_new[at], want_c, 1e-10, 1e-13, 'updated covariance')
            cn['updates'] += len(matches)
        if founded:
            at = np.array([where[int(t)] for t, _ in founded])
            want_m, want_c = initiate(np.array([ds.tlwh_to_xyah(tlwh[d]) for _, d in founded]))
            if not np.array_equal(M_new[at], want_m.astype(np.float64)):
                raise StepMismatch(5, self.frame, 'mean of a track founded in this update')
            self._close(5, 'initiate_cov', C_new[at], want_c, 1e-15, 0.0, 'covariance of a track founded in this update')
            cn['initiates'] += len(founded)
        matched = {r for r, _ in matches}
        for r in range(T):
            k = where.get(int(track_id[r]))
            if r in matched or k is None:
                continue
            if M_new[k].tobytes() != M_pred[r].tobytes() or C_new[k].tobytes() != C_pred[r].tobytes():
                raise StepMismatch(5, self.frame, 'track %d was not matched, yet its state is not the predicted one' % track_id[r])

    # ------------------------------------------------------------------- after the run
    def assert_coverage(self, case):
        cov, cn = COVERAGE[case], self.counters
        assert self.band == 0, '%d gate entries sat within 1e-11 of the threshold and were left out' % self.band
        for name, need in cov['sets'].items():
            assert need <= cn[name], (case, name, sorted(need - cn[name]), sorted(cn[name]))
        assert cn['max_tsu'] >= cov['min_max_tsu'], (case, cn['max_tsu'])
        if 'max_gallery' in cov:
            assert max(cn['gallery']) == cov['max_gallery'], (case, max(cn['gallery']))
        for name, (_, floor) in cov['floors'].items():
            assert cn[name] >= floor, (case, name, cn[name], floor)

    def report(self, title):
        cn = dict(self.counters)
        cn['ndet'], cn['gallery'] = sorted(cn['ndet']), sorted(cn['gallery'])
        print('%s: worst error as a fraction of its tolerance: %s' % (title, ', '.join('%s %.3g' % kv for kv in sorted(self.worst.items()))))
        print('%s: counters %s, gate entries left out %d' % (title, cn, self.band))
