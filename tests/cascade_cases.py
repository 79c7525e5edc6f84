"""Inputs of the association-decision fixture (tests/golden/cascade_cases.npz): the generator scripts/make_golden_cascade.py fed to the
reference's matching_cascade / min_cost_matching, and the tests feed to dd_match_cascade.  A case is (seed, T, n, kind, max_age): the
matrices are regenerated from it here and checked against the fixture's digest, so the fixture stores no matrix.

kind 0  tie-free: every cost below its threshold, no two equal
kind 1  integer-valued costs 0 / 1 / 2 under thresholds of 1.5: exact ties everywhere, the 2s clamped
kind 2  mostly clamped: 70 % of the appearance costs gated (1e5), 60 % of the IoU costs 1.0; appearance rows of unconfirmed tracks are NaN
        (nobody may read them)
kind 3  all clamped
"""
import hashlib
import numpy as np

TENTATIVE, CONFIRMED = 1, 2
LEVELS = (1, 2, 4, 7)                      # time_since_update of confirmed tracks: cascade levels 0, 1, 3, 6 -- 2, 4, 5 and 7.. hold no track


def thresholds(kind):
    return (1.5, 1.5) if kind == 1 else (0.2, 0.7)          # (max_cosine_distance, max_iou_distance)


def make_case(seed, T, n, kind, max_age):
    """-> app [T, n], iou [T, n] f64, state [T], tsu [T] int32."""
    rng = np.random.default_rng(int(seed))
    state = np.where(rng.random(T) < 0.7, CONFIRMED, TENTATIVE).astype(np.int32)
    tsu = np.asarray(LEVELS, dtype=np.int32)[rng.integers(0, len(LEVELS), T)]
    tsu[rng.random(T) < 0.45] = 1                           # most tracks were seen last frame
    tsu[rng.random(T) < 0.05] = max_age                     # the last level
    tsu[state == TENTATIVE] = 1                             # a tentative track that missed a frame is gone (track.py:190-196)
    if kind == 0:
        app, iou = rng.random((T, n)) * 0.19, rng.random((T, n)) * 0.69
    elif kind == 1:
        app, iou = rng.integers(0, 3, (T, n)).astype(np.float64), rng.integers(0, 3, (T, n)).astype(np.float64)
    elif kind == 2:
        app, iou = rng.random((T, n)) * 0.25, rng.random((T, n))
        app[rng.random((T, n)) < 0.7] = 1e5
        iou[rng.random((T, n)) < 0.6] = 1.0
        app[state != CONFIRMED] = np.nan
    else:
        app, iou = np.full((T, n), 1e5), np.full((T, n), 1.0)
    if kind != 1:
        iou[tsu > 1] = 1e5                                  # iou_matching.py:74-76
    return np.ascontiguousarray(app), np.ascontiguousarray(iou), state, tsu


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint64)[0]


def load_cases(path):
    """-> list of dicts: the regenerated inputs (digest checked) and the three expected lists."""
    g = np.load(path)
    out = []
    rp, mp, up, dp = g['row_ptr'], g['match_ptr'], g['un_rows_ptr'], g['un_dets_ptr']
    for i, (seed, T, n, kind, max_age) in enumerate(g['cases'].tolist()):
        app, iou, state, tsu = make_case(seed, T, n, kind, max_age)
        assert digest(app, iou, state, tsu) == g['input_digest'][i], f'case {i}: the generator no longer reproduces the fixture inputs'
        np.testing.assert_array_equal(state, g['state'][rp[i]:rp[i + 1]])
        np.testing.assert_array_equal(tsu, g['tsu'][rp[i]:rp[i + 1]])
        max_cos, max_iou = thresholds(kind)
        out.append(dict(i=i, T=T, n=n, kind=kind, max_age=max_age, app=app, iou=iou, state=state, tsu=tsu, max_cos=max_cos, max_iou=max_iou,
                        matches=g['matches'][mp[i]:mp[i + 1]].reshape(-1, 2).tolist(), un_rows=g['un_rows'][up[i]:up[i + 1]].tolist(),
                        un_dets=g['un_dets'][dp[i]:dp[i + 1]].tolist()))
    return out


def match_cascade(case, where, ctx=None):
    """dd_match_cascade on one case -> (matches [[row, det]], un_rows, un_dets).  where=1 uploads the matrices through `ctx`."""
    import ctypes
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    T, n = case['T'], case['n']
    app, iou = case['app'], case['iou']
    if where:
        app, iou = ctx.to_device(app), ctx.to_device(iou)
    m, ur, ud = np.zeros((min(T, n), 2), np.int32), np.zeros(T, np.int32), np.zeros(n, np.int32)
    nm, nur, nud = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().dd_match_cascade(ctx.handle if ctx else None, where, ptr(app), ptr(iou), T, n, ptr(case['state']), ptr(case['tsu']),
                                 case['max_cos'], case['max_iou'], case['max_age'], ptr(m), ctypes.byref(nm), ptr(ur), ctypes.byref(nur),
                                 ptr(ud), ctypes.byref(nud)), 'dd_match_cascade')
    return m[:nm.value].tolist(), ur[:nur.value].tolist(), ud[:nud.value].tolist()
