"""GPU: every op of the f16 engine (csrc/nets.hip) on its own, against the float64 references of tests/net_op_ref.py.

Each case is a one-op program: an input op, a 1x1 feeder layer (3 -> Cin, no activation) whose tensor is read back -- those bits are the
reference's input, so the feeder's own error is not part of the comparison -- and the op under test.  The bound per element is derived in
net_op_ref's docstring from the arithmetic alone; every element of every output is compared, pad channels included.  Every conv case also asserts
which kernel ran it (dd_net_op_launches) and with which tile, fill mode and K split (dd_net_op_variants), as literals in tests/net_op_cases.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import net_op_ref as R  # noqa: E402
import net_op_cases as C  # noqa: E402
from net_op_rig import Rig  # noqa: E402

pytestmark = pytest.mark.gpu


def _post_aff(p, cout, aff2):
    """EPI_F32 with a post-activation affine, set on the last op the way Program.fc sets it."""
    a = np.zeros((2, R.rup(cout, 8)), dtype=np.float32)
    a[0, :cout], a[1, :cout] = aff2
    p.ops[-1][18] = p.add_blob(a)
    p.ops[-1][19] = 1


def _assert_kernel(rig, op, name, opk, variant):
    from deepdish_amd.profile import OPK_NAMES, CONV_MODES
    code, var = rig.kernel_of(op)
    what = OPK_NAMES.get(code, 'the generic launcher') + ('' if var is None else ' %s<%d,%d,%d,%d,%d> splitk %d' % ((CONV_MODES[var[5]],) + var[:5] + (var[6],)))
    print('%s: ran on %s (code %d, variant %s)' % (name, what, code, var))
    assert code == opk, '%s: launch code %d (%s), expected %d' % (name, code, what, opk)
    assert var == variant, '%s: variant %s (%s), expected %s' % (name, var, what, variant)


def _run_conv(c):
    nets = C_nets()
    rig = Rig(c.H, c.W, c.n)
    p = rig.p
    feed = rig.feeder(c.cin, 1)
    res = rig.feeder(c.cout, 2) if c.res else -1
    w, b, aff2 = C.conv_weights(c)
    kw = {}
    dst2 = -1
    if c.dst2:
        dst2 = p.tensor(c.ho, c.wo, c.cout)
        kw = dict(dst2=dst2, aff2=aff2)
    dst = p.conv(feed, w, b, stride=c.stride, pad=c.pad, act=c.act, res=res, epi=nets.EPI_F16 if c.epi == 'f16' else nets.EPI_F32,
                 pool=c.pool, **kw)
    if c.epi == 'f32aff':
        _post_aff(p, c.cout, aff2)
    op = len(p.ops) - 1
    assert (p.ops[op][28], p.ops[op][13]) == (c.bk, c.kpad)
    rig.run(dst, c.max_batch)
    _assert_kernel(rig, op, c.name, c.opk, c.variant)
    ref, _ = C.conv_reference(c, rig.read(feed), rig.read(res) if c.res else None)
    got = rig.read(dst)
    assert got.shape[-1] == c.cout_pad                      # all channels up to cs
    used = R.assert_within(c.name + ' out', got, ref['out'][0], ref['out'][1])
    if c.dst2:
        used = max(used, R.assert_within(c.name + ' out2', rig.read(dst2), ref['out2'][0], ref['out2'][1]))
    return used


def C_nets():
    from deepdish_amd import nets
    return nets


@pytest.mark.parametrize('c', C.CONV_CASES, ids=[c.name for c in C.CONV_CASES])
def test_conv_dispatch_branches(c):
    _run_conv(c)


@pytest.mark.parametrize('c', C.EPILOGUE_CASES, ids=[c.name for c in C.EPILOGUE_CASES])
def test_conv_epilogue_flavours(c):
    assert c.cout % 8 == 5
    _run_conv(c)


# ---------------------------------------------------------------------------------------------- channel views
def _view_program(kind, with_op):
    """The op reads view(t, 8, Cin) of a tensor 16 channels wider and writes view(cat, 8, cout) of a concat 24 channels wider whose slices on both
    sides (8 in front, 16 behind) other ops filled first."""
    nets = C_nets()
    up = kind.startswith('upsample')
    H, W = (6, 10) if up else (7, 5)
    rig = Rig(H, W, 3)
    p = rig.p
    cin = {'bk32': 8, 'glds': 128, 'splitk': 64, 'rw': 32, 'dw': 40, 'maxpool': 16, 'upsample8': 8, 'upsample40': 40}[kind]
    cout = {'bk32': 24, 'glds': 32, 'splitk': 24, 'rw': 32}.get(kind, cin)
    neg = kind == 'maxpool'
    wide = rig.feeder(cin + 16, 1, stride=2 if up else 1, gain=0.15 if neg else 1.0, bias=-2.0 if neg else 0.0)
    src = p.view(wide, 8, cin)
    cat = p.tensor(H, W, cout + 24)
    rig.feeder(8, 3, dst=p.view(cat, 0, 8))
    rig.feeder(16, 4, dst=p.view(cat, 8 + cout, 16))
    mid = p.view(cat, 8, cout)
    case = None
    if with_op:
        if kind in ('bk32', 'glds', 'splitk', 'rw'):
            case = {'bk32': C.Conv('view_bk32', (H, W), 3, 3, 8, 24, C.M32, act=R.ACT_RELU6),
                    'glds': C.Conv('view_glds', (H, W), 3, 1, 128, 32, C.G(C.T32, 1), act=R.ACT_SILU),
                    'splitk': C.Conv('view_splitk', (H, W), 3, 3, 64, 24, C.G(C.T32, 2, 2), act=R.ACT_ELU),
                    'rw': C.Conv('view_rw', (H, W), 3, 3, 32, 32, None, act=R.ACT_ELU)}[kind]
            w, b, _ = C.conv_weights(case)
            p.conv(src, w, b, act=case.act, dst=mid)
        elif kind == 'dw':
            # (Program.dwconv allocates its own output: the op record is pointed at the slice)
            w, b = C.dw_weights(cin, R.ACT_SILU)
            p.dwconv(src, w, b, 1, nets.ACT_SILU)
            p.ops[-1][2] = mid
        elif kind == 'maxpool':
            p.maxpool(src, 5, 1, 2, dst=mid)
        else:
            p.upsample2(src, mid)
    rig.run(cat)
    return rig, wide, cat, cin, cout, case


@pytest.mark.parametrize('kind', ['bk32', 'glds', 'splitk', 'rw', 'dw', 'maxpool', 'upsample8', 'upsample40'])
def test_channel_views(kind):
    before, _, cat0, _, cout, _ = _view_program(kind, False)
    rig, wide, cat, cin, cout, case = _view_program(kind, True)
    a, b = before.raw(cat0), rig.raw(cat)
    assert np.abs(a[..., :8].astype(np.float32)).max() > 0.1 and np.abs(a[..., 8 + cout:].astype(np.float32)).max() > 0.1
    np.testing.assert_array_equal(a[..., :8].view(np.uint16), b[..., :8].view(np.uint16))                      # the neighbouring slices: bit-identical
    np.testing.assert_array_equal(a[..., 8 + cout:].view(np.uint16), b[..., 8 + cout:].view(np.uint16))
    assert not a[..., 8:8 + cout].any()
    x = rig.read(wide)[..., 8:8 + cin]
    got = rig.read(cat)[..., 8:8 + cout]
    if case is not None:
        _assert_kernel(rig, len(rig.p.ops) - 1, case.name, case.opk, case.variant)
        ref, _ = C.conv_reference(case, x)
        R.assert_within(case.name, got, ref['out'][0], ref['out'][1])
    elif kind == 'dw':
        w, b_ = C.dw_weights(cin, R.ACT_SILU)
        s, S = R.dwconv3(x, R.f16(w), b_, 1, 1, 1, 7, 5)
        want = R.act(s, R.ACT_SILU)
        R.assert_within('view_dw', got, want, R.bound(want, S, 9, 1, R.ACT_SILU))
    elif kind == 'maxpool':
        assert (x < 0).all()
        np.testing.assert_array_equal(got, R.maxpool(x, 5, 1, 2))
    else:
        np.testing.assert_array_equal(got, R.upsample2(x))


# ---------------------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize('d', C.DW_CASES, ids=[d.name for d in C.DW_CASES])
def test_dwconv(d):
    rig = Rig(d.H, d.W, d.n, seed=12)
    feed = rig.feeder(d.c, 1)
    w, b = C.dw_weights(d.c, d.act)
    dst = rig.p.dwconv(feed, w, b, d.stride, d.act)
    rig.run(dst)
    s, S = R.dwconv3(rig.read(feed), R.f16(w), b, d.stride, d.pad_t, d.pad_l, d.ho, d.wo)
    want = R.act(s, d.act)
    R.assert_within(d.name, rig.read(dst), want, R.bound(want, S, 9, 1, d.act))


@pytest.mark.parametrize('c,cout,stride', C.DWPW_SHAPES)
@pytest.mark.parametrize('acts', [(R.ACT_RELU6, R.ACT_RELU6), (R.ACT_SILU, R.ACT_NONE)], ids=['relu6', 'silu_none'])
def test_dwpw(c, cout, stride, acts):
    """dwpw_k keeps the depthwise result as f16 in LDS (o[i] = (_Float16)apply_act(acc) before the MFMA reads it), so the reference rounds its
    depthwise values to f16 too; an element within the depthwise f32 error of a rounding boundary may come out as the neighbouring f16, which
    the bound carries through the pointwise weights (net_op_ref.dwpw)."""
    nets = C_nets()
    H, W = C.DWPW_MAPS[stride]
    rig = Rig(H, W, 2, seed=13)
    feed = rig.feeder(c, 1)
    dw_w, dw_b = C.dw_weights(c, acts[0])
    rng = np.random.default_rng([14, c, cout])
    g = C.pre_gain(acts[1]) / np.sqrt(c) / (3.0 if acts[0] == R.ACT_RELU6 else 1.0)
    pw = R.f16(g * rng.standard_normal((c, cout))).astype(np.float32)
    pw_b = (0.5 * C.pre_gain(acts[1]) * rng.standard_normal(cout)).astype(np.float32)
    dst = rig.p.dwpw(feed, dw_w, dw_b, stride, acts[0], pw.reshape(1, 1, c, cout), pw_b, acts[1])
    assert rig.p.ops[-1][0] == nets.OP_DWPW
    rig.run(dst)
    assert rig.kernel_of(len(rig.p.ops) - 1) == (0, None)
    ho, wo, pt, pl = R.geometry(H, W, 3, 3, stride, None)
    want, bnd = R.dwpw(rig.read(feed), R.f16(dw_w), dw_b, stride, pt, pl, ho, wo, acts[0], R.f16(pw), pw_b, acts[1])
    R.assert_within('dwpw_%d_%d_s%d' % (c, cout, stride), rig.read(dst), want, bnd)


# ---------------------------------------------------------------------------------------------- pooling, upsampling
@pytest.mark.parametrize('hw,k,stride,pad', C.POOL_CASES)
@pytest.mark.parametrize('c', [8, 40])
def test_maxpool(hw, k, stride, pad, c):
    rig = Rig(hw[0], hw[1], 3, seed=15)
    feed = rig.feeder(c, 1, gain=0.15, bias=-2.0)            # all negative: a kernel that padded with zeros would let the padding win
    dst = rig.p.maxpool(feed, k, stride, pad)
    rig.run(dst)
    x = rig.read(feed)
    assert (x[..., :c] < 0).all()
    np.testing.assert_array_equal(rig.read(dst), R.maxpool(x, k, stride, pad))


@pytest.mark.parametrize('hw,c', C.CASCADE_CASES)
def test_pool_cascade(hw, c):
    rig = Rig(hw[0], hw[1], 3, seed=16)
    cat = rig.p.tensor(hw[0], hw[1], 4 * c)                 # [x | 5 | 9 | 13], as YOLOv5's SPP lays it out
    src = rig.p.view(cat, 0, c)
    rig.feeder(c, 1, gain=0.15, bias=-2.0, dst=src)
    rig.p.pool_cascade(src, 5, 3, rig.p.view(cat, c, c))
    rig.run(cat)
    got = rig.read(cat)
    assert (got[..., :c] < 0).all()
    np.testing.assert_array_equal(got[..., c:], R.pool_cascade(got[..., :c], 5, 3))


# ---------------------------------------------------------------------------------------------- input ops, first layer
@pytest.mark.parametrize('kw', C.INPUT_CASES, ids=lambda k: 'swap%d_m%g_sc%.4f_s2d%d_c%d' % (k['swap_rb'], k['mean'], k['scale'], k['s2d'], k['c_pad']))
def test_input_op(kw):
    rig = Rig(*C.INPUT_MAP, 3, seed=17, program_input=False)
    assert rig.img.min() == 0 and rig.img.max() == 255
    t = rig.p.input(**kw)
    rig.run(t)
    want, bnd = R.input_op(rig.img, **kw)
    R.assert_within('input', rig.read(t), want, bnd)


@pytest.mark.parametrize('kw', C.STEM_CASES, ids=lambda k: '%dx%d_s%d_c%d' % (k['hw'] + (k['stride'], k['cout'])))
def test_stem(kw):
    rig = Rig(*kw['hw'], 3, seed=18, program_input=False)
    rng = np.random.default_rng([19, kw['cout']])
    g = C.pre_gain(kw['act']) / 3.0                         # 27 taps of variance 1/3 (pixels in [-1, 1], or in [0, 2) before the bias centres them)
    w = R.f16(g * rng.standard_normal((3, 3, 3, kw['cout']))).astype(np.float32)
    b = (0.5 * C.pre_gain(kw['act']) * rng.standard_normal(kw['cout'])).astype(np.float32)
    if kw['mean'] == 0:
        b -= w.sum(axis=(0, 1, 2)) * 127.5 * kw['scale']           # un-centred pixels: centre the sums so that both signs occur
    dst = rig.p.stem(w, b, kw['stride'], kw['act'], kw['swap_rb'], mean=kw['mean'], scale=kw['scale'])
    rig.run(dst)
    s, S, nt = R.stem(rig.img, w, b, kw['stride'], kw['swap_rb'], kw['mean'], kw['scale'])
    assert 0.05 <= (s > 0).mean() <= 0.95
    ref = R.epilogue(s, S, nt, 32, kw['act'])
    got = rig.read(dst)
    assert got.shape[-1] == 32
    R.assert_within('stem', got, ref['out'][0], ref['out'][1])


# ---------------------------------------------------------------------------------------------- fc, l2norm
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('cout,variant', [(128, C.G(C.T64, 1)), (20, C.G(C.T32, 1)), (24, C.G(C.T32, 1))])
@pytest.mark.parametrize('aff', [False, True])
def test_fc_l2norm(n, cout, variant, aff):
    """K = 4 * 2 * 16 -> cout as the engine runs it (a pointwise convolution over a [1, 1, K] view, f32 output); behind the 128- and the
    24-channel layers an l2norm (eps as MARS), checked against the f32 rows it read."""
    rig = Rig(4, 2, n, seed=20)
    feed = rig.feeder(16, 1)
    rng = np.random.default_rng([21, cout])
    w = R.f16(2.0 / np.sqrt(128) * rng.standard_normal((128, cout))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    aff2 = (rng.uniform(0.5, 1.5, cout).astype(np.float32), (0.3 * rng.standard_normal(cout)).astype(np.float32)) if aff else None
    f = rig.p.fc(feed, w, b, rig.nets.ACT_ELU, aff2=aff2)
    op = len(rig.p.ops) - 1
    out = rig.p.l2norm(f, 1e-8) if cout % 8 == 0 else f
    rig.run(out)
    _assert_kernel(rig, op, 'fc_%d' % cout, 0, variant)
    x = rig.read(feed).reshape(n, 128)
    ref = R.fc(x, R.f16(w), b, R.ACT_ELU, 1, aff2)['out']
    got = rig.read(f)
    R.assert_within('fc_%d' % cout, got, ref[0], ref[1])
    if cout % 8 == 0:
        want, bnd = R.l2norm(got[:, 0, 0, :], 1e-8)
        R.assert_within('l2norm_%d' % cout, rig.read(out)[:, 0, 0, :], want, bnd)


# ---------------------------------------------------------------------------------------------- head epilogues, matrix form
@pytest.mark.parametrize('cin,variant', [(16, C.M32), (128, C.G(C.T32, 1))])
def test_ssd_head_matrix(cin, variant):
    """EPI_SSD_HEAD on a 3x5 map with 2 anchors, p words as compile_ssd_mobilenet sets them; a second head op fills the other map's rows first, and
    every row of the matrix is compared."""
    nets = C_nets()
    A, ncls, n = 2, 5, 2
    ld, rows = 4 + ncls, 2 * 15 * A
    rig = Rig(3, 5, n, seed=22)
    f1, f2 = rig.feeder(cin, 1), rig.feeder(cin, 5)
    out = rig.p.tensor(rows, 1, ld, cs=ld, dtype=nets.DT_F32)
    refs, ops = [], []
    for base, ft, seed in ((15 * A, f2, 2), (0, f1, 1)):                   # the op under test runs last, on rows 0 .. 29
        rng = np.random.default_rng([23, seed])
        w = R.f16(2.0 / np.sqrt(cin) * rng.standard_normal((1, 1, cin, A * ld))).astype(np.float32)
        b = rng.standard_normal(A * ld).astype(np.float32)
        rig.p.conv(ft, w, b, dst=out, epi=nets.EPI_SSD_HEAD, p=[ncls, rows, base, ld, 4 * A, A])
        refs.append((base, ft, w, b))
        ops.append(len(rig.p.ops) - 1)
    rig.run(out)
    _assert_kernel(rig, ops[-1], 'ssd_head_c%d' % cin, 0, variant)
    want, bnd = np.zeros((n, rows, ld)), np.zeros((n, rows, ld))
    for base, ft, w, b in refs:
        s, S = R.conv(rig.read(ft), R.f16(w), b, 1, 0, 0, 3, 5)
        idx, vals = R.ssd_head_rows(s, ncls, base, rows, ld)
        want[:, idx] = vals
        bnd[:, idx] = R.ssd_head_rows(R.error_f32(s, S, cin), ncls, base, rows, ld)[1]
    R.assert_within('ssd_head_c%d' % cin, rig.read(out)[:, :, 0, :], want, bnd)


@pytest.mark.parametrize('cin,variant', [(16, C.M32), (128, C.G(C.T32, 1))])
def test_yolo_head_matrix(cin, variant):
    """EPI_YOLO on a 3x5 map with 2 anchors (5 + 2 columns per row), p / f words as compile_yolov5s sets them."""
    nets = C_nets()
    A, no, n = 2, 7, 2
    rows = 2 * 15 * A
    anchors, stride, img_w, img_h = [10.0, 13.0, 16.0, 30.0], 8.0, 40, 24
    rig = Rig(3, 5, n, seed=24)
    f1, f2 = rig.feeder(cin, 1), rig.feeder(cin, 5)
    out = rig.p.tensor(rows, 1, no, cs=no, dtype=nets.DT_F32)
    refs, ops = [], []
    for base, ft, seed in ((15 * A, f2, 2), (0, f1, 1)):
        rng = np.random.default_rng([25, seed])
        w = R.f16(3.0 / np.sqrt(cin) * rng.standard_normal((1, 1, cin, A * no))).astype(np.float32)
        b = rng.standard_normal(A * no).astype(np.float32)
        rig.p.conv(ft, w, b, dst=out, epi=nets.EPI_YOLO, p=[no, rows, base, 0, img_h, 0], f=anchors + [0.0, 0.0, stride, float(img_w)])
        refs.append((base, ft, w, b))
        ops.append(len(rig.p.ops) - 1)
    rig.run(out)
    _assert_kernel(rig, ops[-1], 'yolo_head_c%d' % cin, 0, variant)
    want, bnd = np.zeros((n, rows, no)), np.zeros((n, rows, no))
    for base, ft, w, b in refs:
        s, S = R.conv(rig.read(ft), R.f16(w), b, 1, 0, 0, 3, 5)
        idx, vals, bb = R.yolo_rows(s, S, cin, no, base, stride, (img_w, img_h), anchors)
        want[:, idx], bnd[:, idx] = vals, bb
    R.assert_within('yolo_head_c%d' % cin, rig.read(out)[:, :, 0, :], want, bnd)
