"""GPU: every op of the uint8 engine (csrc/netsq.hip) against the int64 reference (tests/q_op_ref.py), one op at a time, at the smallest
shapes that reach each branch of the dispatcher -- the whole-model tests only ever show a kernel the two synthetic 300 x 300 models'
geometry, channel counts and requantisation parameters.

A case (tests/q_op_cases.py) is a small program: first layer -> feeder -> the op under test.  The feeder's bytes are read back and the
op's reference is computed from THEM, so the feeder's correctness is no part of the op's comparison; first layer and feeder are held to the
chain reference separately and fail under their own names.  Integer work: every byte equal, phantom channels and borders included; rows
outputs also outside the written ranges (the tensors have slack before, behind and, in some cases, between the pixels' rows).  The launch code and the kernel variant that ran each op (dd_net_op_launches,
dd_net_op_variants) equal the case's literals, so a case meant for one branch cannot quietly take another.  The one tolerance is the
decoded boxes' atol = 2e-6 (device expf against numpy), as in test_gpu_quant.py::test_decoded_arrays."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_op_ref as R  # noqa: E402
import q_op_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c['id'] for c in Q.CASES]


def _bordered(net, P, tensor, n, want, what, errors):
    """Every byte of a bordered tensor against want [n,h,w,C stored], and its borders against the zero point."""
    from deepdish_amd import netsq
    d = P.T(tensor)
    raw = net.read(n, tensor=tensor)
    got = netsq.unpack_q16(raw, d['h'], d['w'], d['c'])
    if got.shape != want.shape:
        errors.append('%s: shape %s, the reference has %s' % (what, got.shape, want.shape))
        return raw, got
    bad = got != want
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        pix = np.argwhere(bad.any(axis=3))
        errors.append('%s: %d of %d bytes differ in %d pixels, (frame, y, x) %s; first at (frame, y, x, channel) %s: %d, the reference has %d' %
                      (what, int(bad.sum()), bad.size, len(pix), [tuple(int(v) for v in p) for p in pix[:6]], k, got[k], want[k]))
    if not (netsq.borders_q16(raw, d['h'], d['w'], d['c']) == d['zp']).all():
        errors.append('%s: a border byte no longer holds the zero point' % what)
    return raw, got


def _rows(net, tensor, n, want, what, errors, mask=None):
    got = net.read(n, tensor=tensor).reshape(n, -1)
    if got.shape != want.shape:
        errors.append('%s: %d bytes per frame, the reference has %d' % (what, got.shape[1], want.shape[1]))
        return got
    bad = got != want
    if mask is not None and (bad & ~mask).any():
        errors.append('%s: %d bytes outside the written ranges lost their initial fill' % (what, int((bad & ~mask).sum())))
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        errors.append('%s: %d of %d bytes differ, first at (frame, byte) %s: %d, the reference has %d' % (what, int(bad.sum()), bad.size, k, got[k], want[k]))
    return got


@pytest.mark.parametrize('cid', IDS)
def test_op(cid):
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches, q_op_variants
    c = Q.BY_ID[cid]
    layers = Q.layers_of(c)
    P, t = Q.build_program(c, layers)
    n = c['frames']
    net = Net(P, max_batch=n)
    chain = Q.chain_reference(c, layers)
    if c['kind'] == 'decode':
        net.ssd_decode(Q.anchors_of(c), Q.TUNED[cid]['thr'])
    net.forward(chain['frames'])
    errors = []
    # which kernels ran: the literals of the case, op by op
    got_ops = [(int(code), None if v is None else tuple(v)) for code, v in zip(net_op_launches(net), q_op_variants(net))]
    want_ops = [(code, tuple(v)) for code, v in Q.TUNED[cid]['ops']]
    print('%s: %s' % (cid, got_ops))
    if got_ops != want_ops:
        errors.append('kernels: ran %s, the case expects %s' % (got_ops, want_ops))
    if any(code in (19, 20) for code, _ in got_ops):
        errors.append('a row pipeline took the program')
    _bordered(net, P, t['conv0'], n, chain['conv0'], 'first layer', errors)
    if c['kind'] != 'conv0':
        _, x = _bordered(net, P, t['feed'], n, chain['feed'], 'feeder', errors)
        ref = Q.op_reference(c, layers, x)                   # the op under test on the DEVICE's feeder bytes
        kind = c['kind']
        if kind in ('conv', 'dw', 'dwpw'):
            _bordered(net, P, t['out'], n, ref['out'], 'op', errors)
            if 'mid' in t:
                _bordered(net, P, t['mid'], n, ref['mid'], 'op (depthwise half of the two-op form)', errors)
        elif kind == 'conv_add':
            raw_f, _ = _bordered(net, P, t['out'], n, ref['out'], 'op (ADD in the projection\'s epilogue)', errors)
            _bordered(net, P, t['proj'], n, ref['proj'], 'projection alone', errors)
            raw_u, _ = _bordered(net, P, t['out_unfused'], n, ref['out'], 'q_add_k behind the projection', errors)
            if not np.array_equal(raw_f, raw_u):
                errors.append('the fused and the unfused ADD differ')
        elif kind == 'rows':
            if 'down' in t:
                _bordered(net, P, t['down'], n, ref['down'], 'second map', errors)
            _rows(net, t['rows'], n, ref['rows'], 'op', errors, ref['rows_mask'])
        else:
            box = _rows(net, t['box'], n, ref['box'], 'op (box rows)', errors, ref['box_mask'])
            cls = _rows(net, t['cls'], n, ref['cls'], 'op (class rows)', errors, ref['cls_mask'])
            if kind == 'decode':
                n_cols = c['op']['n_cols']
                boxes, score, best, keys = net.ssd_decoded()
                split = 0
                for z in range(n):
                    wb, ws, wc, wk = R.decode(box[z].reshape(-1, 4), cls[z].reshape(-1, ref['row_cols'])[:, :n_cols], layers['box'], layers['cls'], Q.LOGISTIC,
                                              Q.anchors_of(c), Q.TUNED[cid]['thr'])
                    for name, g, w in (('scores', score[z], ws), ('classes', best[z], wc), ('keys', keys[z], wk)):
                        if not np.array_equal(g, w):
                            errors.append('decode, frame %d: %d %s differ' % (z, int((g != w).sum()), name))
                    if not np.allclose(boxes[z], wb, rtol=0, atol=2e-6):
                        errors.append('decode, frame %d: boxes off by up to %g' % (z, float(np.abs(boxes[z] - wb).max())))
                    split += int((wk >= 0).sum())
                    if c['op'].get('tie'):
                        lut = R.nq.logistic_table(layers['cls']['out_scale'], layers['cls']['out_zp'], Q.LOGISTIC['out_scale'], Q.LOGISTIC['out_zp'])
                        sq = lut[cls[z].reshape(-1, ref['row_cols'])[:, 1:n_cols]]
                        lo_c, hi_c = c['op']['tie'][0] - 1, c['op']['tie'][1] - 1
                        tied = (sq[:, lo_c] == sq.max(axis=1)) & (sq[:, :lo_c].astype(np.int64).max(axis=1, initial=-1) < sq[:, lo_c])
                        assert tied.any() and (sq[:, lo_c] == sq[:, hi_c]).all()          # the two classes tie, and win somewhere
                        if not (best[z][tied] == lo_c).all():
                            errors.append('decode, frame %d: a tie did not go to the lowest class' % z)
                assert 0 < split < n * len(Q.anchors_of(c))                          # the threshold splits the anchors
    assert not errors, '%s:\n  ' % cid + '\n  '.join(errors)


def test_first_layer_refuses_a_batch_that_is_not_4_byte_aligned():
    """33 x 33 frames are 3 267 bytes: three of them are no whole number of dwords, and the first layer's loads are dwords -- DD_E_ARG, not a run."""
    from deepdish_amd._lib import DeepDishHipError
    from deepdish_amd.engine import Net
    c = Q.BY_ID['conv0_33x33x4']
    P, t = Q.build_program(c)
    net = Net(P, max_batch=4)
    fr = Q.frames_of(c)
    with pytest.raises(DeepDishHipError) as e:
        net.forward(fr[:3])
    assert 'first layer' in str(e.value) and '4-byte aligned' in str(e.value)
    net.forward(fr)                                          # the same engine still runs the aligned batch
    errors = []
    _bordered(net, P, t['conv0'], 4, Q.chain_reference(c)['conv0'], 'first layer', errors)
    assert not errors, errors
