"""CPU: the float64 references of tests/net_op_ref.py are right (they equal torch.nn.functional in float64 at every case geometry), the bound
they come with would catch a subtly wrong kernel (mutants of the reference exceed it tenfold in every conv and depthwise case) without
rejecting a correct one (f32 accumulation in two summation orders stays inside it), and the seeded inputs reach both sides of every kink."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import net_op_ref as R  # noqa: E402
import net_op_cases as C  # noqa: E402

CONV_IDS = [c.name for c in C.ALL_CONV_CASES]


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _geoms():
    seen, out = set(), []
    for c in C.ALL_CONV_CASES:
        key = (c.H, c.W, c.kh, c.kw, c.stride, c.pad, c.cin, c.cout)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize('c', _geoms(), ids=lambda c: c.name)
def test_conv_equals_torch(c):
    rng = np.random.default_rng(1)
    n = min(c.n, 2)
    x, w, b = rng.standard_normal((n, c.H, c.W, c.cin)), rng.standard_normal((c.kh, c.kw, c.cin, c.cout)), rng.standard_normal(c.cout)
    s, S = R.conv(x, w, b, c.stride, c.pad_t, c.pad_l, c.ho, c.wo)
    pb, pr = (c.ho - 1) * c.stride + c.kh - c.pad_t - c.H, (c.wo - 1) * c.stride + c.kw - c.pad_l - c.W
    for xx, ww, bb, got in ((x, w, b, s), (np.abs(x), np.abs(w), np.abs(b), S)):
        xp = F.pad(_nchw(xx), (c.pad_l, max(pr, 0), c.pad_t, max(pb, 0)))
        want = _nhwc(F.conv2d(xp, torch.from_numpy(np.ascontiguousarray(np.transpose(ww, (3, 2, 0, 1)))), torch.from_numpy(bb), stride=c.stride))
        assert want.shape == got.shape
        assert np.abs(want - got).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('d', C.DW_CASES[::3], ids=lambda d: d.name)
def test_dwconv_equals_torch(d):
    rng = np.random.default_rng(2)
    x, w, b = rng.standard_normal((2, d.H, d.W, d.c)), rng.standard_normal((3, 3, d.c)), rng.standard_normal(d.c)
    s, _ = R.dwconv3(x, w, b, d.stride, d.pad_t, d.pad_l, d.ho, d.wo)
    pb, pr = (d.ho - 1) * d.stride + 3 - d.pad_t - d.H, (d.wo - 1) * d.stride + 3 - d.pad_l - d.W
    xp = F.pad(_nchw(x), (d.pad_l, max(pr, 0), d.pad_t, max(pb, 0)))
    want = _nhwc(F.conv2d(xp, torch.from_numpy(np.ascontiguousarray(np.transpose(w, (2, 0, 1))[:, None])), torch.from_numpy(b), stride=d.stride, groups=d.c))
    assert np.abs(want - s).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('hw,k,stride,pad', C.POOL_CASES)
def test_maxpool_equals_torch(hw, k, stride, pad):
    x = -np.abs(np.random.default_rng(3).standard_normal((2,) + hw + (8,))) - 0.1          # all negative: a zero pad would win
    want = _nhwc(F.max_pool2d(F.pad(_nchw(x), (pad,) * 4, value=float('-inf')), k, stride))
    got = R.maxpool(x, k, stride, pad)
    np.testing.assert_array_equal(got, want)
    assert (got < 0).all()


@pytest.mark.parametrize('hw,c', C.CASCADE_CASES[::2])
def test_pool_cascade_equals_torch(hw, c):
    x = np.random.default_rng(4).standard_normal((2,) + hw + (8,))
    t, outs = _nchw(x), []
    for k in (5, 9, 13):                 # a cascade of 5x5 pools is the 5, 9, 13 pools of the input (YOLOv5's SPP)
        outs.append(_nhwc(F.max_pool2d(F.pad(t, (k // 2,) * 4, value=float('-inf')), k, 1)))
    np.testing.assert_array_equal(R.pool_cascade(x, 5, 3), np.concatenate(outs, axis=3))


def test_upsample_equals_torch():
    x = np.random.default_rng(5).standard_normal((2, 3, 5, 8))
    np.testing.assert_array_equal(R.upsample2(x), _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode='nearest')))


@pytest.mark.parametrize('kw', C.INPUT_CASES, ids=lambda k: 'swap%d_m%g_s2d%d_c%d' % (k['swap_rb'], k['mean'], k['s2d'], k['c_pad']))
def test_input_op_equals_torch(kw):
    img = C.images(2, *C.INPUT_MAP, seed=6)
    want, bnd = R.input_op(img, **kw)
    x = img.astype(np.float64)
    if kw['swap_rb']:
        x = x[..., ::-1].copy()
    v = (_nchw(x) - float(np.float32(kw['mean']))) * float(np.float32(kw['scale']))
    if kw['s2d']:
        u = _nhwc(F.pixel_unshuffle(v, 2))                     # torch: channel c * 4 + dy * 2 + dx; the engine: (2 dx + dy) * 3 + c
        perm = [c * 4 + dy * 2 + dx for dx in (0, 1) for dy in (0, 1) for c in range(3)]
        v = u[..., perm]
    else:
        v = _nhwc(v)
    c = v.shape[-1]
    assert np.abs(want[..., :c] - v).max() <= 1e-12 and (want[..., c:] == 0).all()
    assert want.shape[-1] == (kw['c_pad'] or (16 if kw['s2d'] else 8))
    assert (bnd[..., c:] == 2.0 ** -25).all()                  # pad channels: only an exact zero passes
    assert (bnd[..., :c] <= 0.5 * np.spacing(np.abs(want[..., :c]).astype(np.float16)).astype(np.float64) * 1.01 + 2.0 ** -24).all()


def test_act_equals_torch():
    v = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    fs = {R.ACT_NONE: lambda t: t, R.ACT_RELU6: F.relu6, R.ACT_ELU: F.elu, R.ACT_SILU: F.silu, R.ACT_RELU: F.relu, R.ACT_SIGMOID: torch.sigmoid}
    for kind, f in fs.items():
        assert np.abs(R.act(v.numpy(), kind) - f(v).numpy()).max() <= 1e-12
    g = np.abs(np.diff(R.act(v.numpy(), R.ACT_SILU)) / np.diff(v.numpy())).max()
    assert g <= R.LIPSCHITZ[R.ACT_SILU] and np.abs(np.diff(R.act(v.numpy(), R.ACT_SIGMOID)) / np.diff(v.numpy())).max() <= 0.25


def test_stem_equals_torch():
    for kw in C.STEM_CASES:
        img = C.images(2, *kw['hw'], seed=7)
        rng = np.random.default_rng(8)
        w, b = R.f16(rng.standard_normal((3, 3, 3, kw['cout']))), rng.standard_normal(kw['cout']).astype(np.float32)
        s, _, _ = R.stem(img, w, b, kw['stride'], kw['swap_rb'], kw['mean'], kw['scale'])
        x = ((img.astype(np.float32) - np.float32(kw['mean'])) * np.float32(kw['scale'])).astype(np.float16).astype(np.float64)
        x = x[..., ::-1].copy() if kw['swap_rb'] else x
        ho, wo, pt, pl = R.geometry(*kw['hw'], 3, 3, kw['stride'], None)
        pb, pr = (ho - 1) * kw['stride'] + 3 - pt - kw['hw'][0], (wo - 1) * kw['stride'] + 3 - pl - kw['hw'][1]
        want = _nhwc(F.conv2d(F.pad(_nchw(x), (pl, max(pr, 0), pt, max(pb, 0))), torch.from_numpy(np.ascontiguousarray(np.transpose(w, (3, 2, 0, 1)))),
                              torch.from_numpy(b.astype(np.float64)), stride=kw['stride']))
        assert np.abs(want - s).max() <= 1e-12 * np.abs(want).max()


def test_l2norm_and_fc_equal_torch():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 24))
    want, _ = R.l2norm(x, 1e-8)
    t = torch.from_numpy(x)
    assert np.abs(want - (t / torch.sqrt(float(np.float32(1e-8)) + (t * t).sum(1, keepdim=True))).numpy()).max() <= 1e-12
    xf, w, b = rng.standard_normal((5, 128)), rng.standard_normal((128, 20)), rng.standard_normal(20)
    sc, sh = rng.standard_normal(20), rng.standard_normal(20)
    r = R.fc(xf, w, b, R.ACT_ELU, aff2=(sc, sh))['out'][0]
    ref = F.elu(F.linear(torch.from_numpy(xf), torch.from_numpy(w.T.copy()), torch.from_numpy(b))).numpy() * sc + sh
    assert r.shape == (5, 1, 1, 24) and np.abs(r[:, 0, 0, :20] - ref).max() <= 1e-12 and (r[..., 20:] == 0).all()


# ---------------------------------------------------------------------------------------------- the bound discriminates
def _mconv(x, w, b, c, pad_t=None, pad_l=None, shift_tap=None, edge=False):
    """The reference convolution restated with room for mutations: other padding side, one tap read a pixel to the right, clamped borders."""
    pt, pl = c.pad_t if pad_t is None else pad_t, c.pad_l if pad_l is None else pad_l
    m = 2
    hp, wp = (c.ho - 1) * c.stride + c.kh + 1, (c.wo - 1) * c.stride + c.kw + 1
    xp = np.pad(x, ((0, 0), (pt + m, max(hp - pt - x.shape[1], 0) + m), (pl + m, max(wp - pl - x.shape[2], 0) + m), (0, 0)),
                mode='edge' if edge else 'constant')
    s = np.zeros((x.shape[0], c.ho, c.wo, w.shape[3])) + b
    for dy in range(c.kh):
        for dx in range(c.kw):
            ox = dx + m + (1 if shift_tap == (dy, dx) else 0)
            v = xp[:, dy + m:dy + m + (c.ho - 1) * c.stride + 1:c.stride, ox:ox + (c.wo - 1) * c.stride + 1:c.stride]
            s += v @ w[dy, dx]
    return s


def _drop_k(c, w, k_from):
    """Weights with every K position >= k_from zeroed; K = (tap, padded channel), taps row-major, as the engine packs it."""
    wp = np.zeros((c.kh * c.kw, c.cin_pad, c.cout))
    wp[:, :c.cin] = w.reshape(c.kh * c.kw, c.cin, c.cout)
    flat = wp.reshape(-1, c.cout)
    flat[k_from:] = 0
    return flat.reshape(c.kh * c.kw, c.cin_pad, c.cout)[:, :c.cin].reshape(w.shape)


def _case_inputs(c, n):
    img = C.images(n, c.H, c.W, seed=11)
    x = C.emulate_feeder(img, *C.feeder_weights(c.cin, 1))
    res = C.emulate_feeder(img, *C.feeder_weights(c.cout, 2)) if c.res else None
    return x, res


def _exceeds(r, m):
    """Largest |mutant - want| / bound over all outputs."""
    return max(float((np.abs(m[k][0] - r[k][0]) / np.maximum(r[k][1], 1e-300)).max()) for k in r)


@pytest.mark.parametrize('c', C.ALL_CONV_CASES, ids=CONV_IDS)
def test_conv_bound_discriminates(c):
    x, res = _case_inputs(c, c.cpu_n)
    w, b, aff2 = C.conv_weights(c)
    w64, b64 = R.f16(w), b.astype(np.float64)
    (r, s), S = C.conv_reference(c, x, res), None
    s2, S = R.conv(x, w64, b, c.stride, c.pad_t, c.pad_l, c.ho, c.wo)
    assert np.abs(_mconv(x, w64, b64, c) - s).max() <= 1e-12 * np.abs(s).max()        # the restatement is the reference

    # the kinks: >= 5 % of the pre-activation values on each side of 0 (and of 6 for ReLU6)
    assert 0.05 <= (s > 0).mean() <= 0.95, (s > 0).mean()
    if c.act == R.ACT_RELU6:
        assert 0.05 <= (s > 6).mean() <= 0.95, (s > 6).mean()

    fin = lambda sm, resm=res: C.finish_reference(c, sm, S, resm, aff2)     # noqa: E731
    mutants = {}
    last = (c.kh - 1, c.kw - 1)
    mutants['tap shifted'] = fin(_mconv(x, w64, b64, c, shift_tap=last))
    mutants['neighbour bias'] = fin(s - b64 + np.roll(b64, 1))
    mutants['last K chunk dropped'] = fin(_mconv(x, _drop_k(c, w64, c.kpad - c.bk), b64, c))
    if c.splitk > 1:
        per = -(-(c.kpad // c.bk) // c.splitk)
        mutants['last split dropped'] = fin(_mconv(x, _drop_k(c, w64, (c.splitk - 1) * per * c.bk), b64, c))
    if c.stride == 2 and c.pad is None:
        alt = [max((o - 1) * 2 + k - size, 0) - p for o, k, size, p in ((c.ho, c.kh, c.H, c.pad_t), (c.wo, c.kw, c.W, c.pad_l))]
        if (alt[0], alt[1]) != (c.pad_t, c.pad_l):
            mutants['padding from the other side'] = fin(_mconv(x, w64, b64, c, pad_t=alt[0], pad_l=alt[1]))
    reads_last = not c.pool or ((c.ho - 3) % 2 == 0 or (c.wo - 3) % 2 == 0)      # a VALID 3x3/2 pool of an even-sized map never reads its last row / column
    if reads_last and ((c.ho - 1) * c.stride + c.kh - c.pad_t > c.H or (c.wo - 1) * c.stride + c.kw - c.pad_l > c.W):
        se, sm = _mconv(x, w64, b64, c, edge=True), s.copy()
        sm[:, -1], sm[:, :, -1] = se[:, -1], se[:, :, -1]
        mutants['clamped last row / column'] = fin(sm)
    if c.res and c.act != R.ACT_NONE:
        m = {k: (v[0].copy(), v[1]) for k, v in r.items()}
        pre = R.act(s + res[..., :c.cout], c.act)
        m['out'][0][..., :c.cout] = pre if c.epi != 'f32aff' else aff2[0] * pre + aff2[1]
        mutants['residual before the activation'] = m
    if c.cout < c.cout_pad:
        m = {k: (v[0].copy(), v[1]) for k, v in r.items()}
        for k in m:
            m[k][0][..., c.cout] = m[k][0][..., c.cout - 1]
        mutants['pad channel written'] = m
    for name, m in mutants.items():
        assert _exceeds(r, m) >= 10.0, '%s: mutant "%s" stays within %.2f x the bound' % (c.name, name, _exceeds(r, m))

    # ... and a correct f32 evaluation stays inside: taps and channels forwards with the bias first, backwards with the bias last
    x32, w32, b32 = x.astype(np.float32), w64.astype(np.float32), b.astype(np.float32)

    def f32_sum(rev):
        xp = np.pad(x32, ((0, 0), (c.pad_t, c.kh + c.stride), (c.pad_l, c.kw + c.stride), (0, 0)))
        acc = np.zeros((x.shape[0], c.ho, c.wo, c.cout), np.float32) + (0 if rev else b32)
        taps = [(dy, dx) for dy in range(c.kh) for dx in range(c.kw)]
        for dy, dx in (taps[::-1] if rev else taps):
            v = xp[:, dy:dy + (c.ho - 1) * c.stride + 1:c.stride, dx:dx + (c.wo - 1) * c.stride + 1:c.stride]
            for c0 in (range(c.cin - 1, -1, -1) if rev else range(c.cin)):
                acc += v[..., c0:c0 + 1] * w32[dy, dx, c0]
        return (acc + b32 if rev else acc).astype(np.float64)
    if c.n_terms <= 1200:                  # (channel-by-channel accumulation: the widest layers are left to the blocked sum below)
        sums = [f32_sum(False), f32_sum(True)]
    else:
        sums = [(x32.reshape(-1, c.cin) @ w32[0, 0] + b32).reshape(s.shape).astype(np.float64),
                (b32 + x32.reshape(-1, c.cin)[:, ::-1] @ w32[0, 0, ::-1]).reshape(s.shape).astype(np.float64)]
    for s32 in sums:
        got = C.finish_reference(c, s32, S, res, aff2)
        for k in r:
            g = got[k][0] if c.epi != 'f16' else R.f16(got[k][0])
            g = g.astype(np.float32).astype(np.float64)
            assert (np.abs(g - r[k][0]) <= r[k][1]).all(), (c.name, k, float((np.abs(g - r[k][0]) / np.maximum(r[k][1], 1e-300)).max()))


@pytest.mark.parametrize('d', C.DW_CASES, ids=lambda d: d.name)
def test_dwconv_bound_discriminates(d):
    img = C.images(d.n, d.H, d.W, seed=12)
    x = C.emulate_feeder(img, *C.feeder_weights(d.c, 1))
    w, b = C.dw_weights(d.c, d.act)
    w64, b64 = R.f16(w), b.astype(np.float64)
    s, S = R.dwconv3(x, w64, b, d.stride, d.pad_t, d.pad_l, d.ho, d.wo)
    assert 0.05 <= (s > 0).mean() <= 0.95
    if d.act == R.ACT_RELU6:
        assert 0.05 <= (s > 6).mean() <= 0.95, (s > 6).mean()
    want = R.act(s, d.act)
    bnd = R.bound(want, S, 9, 1, d.act)

    def dw(pad_t=d.pad_t, pad_l=d.pad_l, shift=None, edge=False, bias=b64):
        m = 2
        xp = np.pad(x, ((0, 0), (pad_t + m, 3 + d.stride + m), (pad_l + m, 3 + d.stride + m), (0, 0)), mode='edge' if edge else 'constant')
        out = np.zeros_like(s) + bias
        for dy in range(3):
            for dx in range(3):
                ox = dx + m + (1 if shift == (dy, dx) else 0)
                out += xp[:, dy + m:dy + m + (d.ho - 1) * d.stride + 1:d.stride, ox:ox + (d.wo - 1) * d.stride + 1:d.stride] * w64[dy, dx]
        return out
    assert np.abs(dw() - s).max() <= 1e-12 * np.abs(s).max()
    mutants = {'tap shifted': dw(shift=(2, 2)), 'neighbour bias': dw(bias=np.roll(b64, 1))}
    se, sm = dw(edge=True), s.copy()
    sm[:, -1], sm[:, :, -1] = se[:, -1], se[:, :, -1]
    mutants['clamped last row / column'] = sm
    if d.stride == 2:
        alt = (max((d.ho - 1) * 2 + 3 - d.H, 0) - d.pad_t, max((d.wo - 1) * 2 + 3 - d.W, 0) - d.pad_l)
        if alt != (d.pad_t, d.pad_l):
            mutants['padding from the other side'] = dw(pad_t=alt[0], pad_l=alt[1])
    for name, sm in mutants.items():
        worst = float((np.abs(R.act(sm, d.act) - want) / bnd).max())
        assert worst >= 10.0, '%s: mutant "%s" stays within %.2f x the bound' % (d.name, name, worst)
    x32, w32 = x.astype(np.float32), w64.astype(np.float32)
    xp = np.pad(x32, ((0, 0), (d.pad_t, 5), (d.pad_l, 5), (0, 0)))
    taps = [(dy, dx) for dy in range(3) for dx in range(3)]
    for rev in (False, True):
        acc = np.zeros(s.shape, np.float32) + (0 if rev else b)
        for dy, dx in (taps[::-1] if rev else taps):
            acc += xp[:, dy:dy + (d.ho - 1) * d.stride + 1:d.stride, dx:dx + (d.wo - 1) * d.stride + 1:d.stride] * w32[dy, dx]
        got = R.f16(R.act((acc + b if rev else acc).astype(np.float64), d.act))
        assert (np.abs(got - want) <= bnd).all()


def test_assert_within_excludes_nothing(capsys):
    want = np.array([1.0, -2.0, 0.0])
    assert R.assert_within('x', want + [1e-4, 0, 0], want, np.array([2e-4, 1e-9, 0.0])) == pytest.approx(0.5)
    assert '0 % excluded' in capsys.readouterr().out
    with pytest.raises(AssertionError):
        R.assert_within('x', want + [0, 0, 1e-30], want, np.array([2e-4, 1e-9, 0.0]))      # a zero bound admits only the exact value
    with pytest.raises(AssertionError):
        R.assert_within('x', want + [0, 2e-9, 0], want, np.array([2e-4, 1e-9, 0.0]))


def test_stem_tensor_holds_the_32_channels_the_kernel_stores():
    """stem_conv3_k stores all 32 packed channels of a pixel whatever cout is: a first layer with fewer filters needs a 32-channel stride, or a
    pixel's zero channels land on the next pixel (and the last pixel's behind the buffer)."""
    from deepdish_amd import nets
    p = nets.Program(7, 5)
    t = p.stem(np.zeros((3, 3, 3, 24), np.float32), np.zeros(24, np.float32), 1, nets.ACT_ELU, swap_rb=False)
    assert (p.T(t)['c'], p.T(t)['cs'], int(p.ops[-1][12])) == (24, 32, 32)
