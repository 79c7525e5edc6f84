"""float64 references of the f16 engine's ops (csrc/nets.hip), one op at a time, and the error bound each output is held to.

numpy only.  Activations are NHWC arrays [n, H, W, C]; a reference takes the EXACT f16 activations and f16 weights the kernel
read, widened to float64, and the f32 bias -- so the only thing compared is the arithmetic of the op itself.

The bound (`bound`, `bound_out2`, `bound_post_aff`): where every term comes from
-------------------------------------------------------------------------------
u = 2^-24 is the unit roundoff of f32 (half an ulp of a number in [1, 2)); "f32 ulp" below means u relative.

1. Products.  An f16 has 11 significant bits, so the product of two f16 values has at most 22: it is exact in f32 (and in
   the MFMA / v_fma_mix datapaths, which multiply f16 operands into an f32 accumulator).
2. Pre-activation sum.  s = b + sum of n_terms exact products, accumulated in f32 in SOME order (MFMA k-slices, K steps,
   split-K partial sums added by conv_splitk_finish_k, the bias first or last).  Every f32 addition rounds once, a value
   takes part in at most n_terms + splitk + 1 of them (n_terms products, one bias, splitk partial sums), and the standard
   forward bound for a sum, whatever the order, is
       |s_f32 - s| <= (n_terms + splitk + 1) * u * S,     S = |b| + sum |x * w|.
3. Activation.  The error passes through the activation's Lipschitz constant: 1 for none / ReLU / ReLU6 / ELU (ELU's slope is
   exp(v) <= 1 below 0), <= 1.1 for SiLU (its slope peaks at 1.0998), 0.25 for the sigmoid.
4. Transcendentals.  ELU, SiLU and the sigmoid use v_exp_f32 / v_rcp_f32, 1 ulp each by the ISA, plus the roundings of the
   few f32 operations around them (a product with log2 e, an add, a product or a subtraction exp(v) - 1 whose absolute error is
   an ulp of 1, not of the small result): 16 f32 ulps of max(1, |act|) covers them; about 2^-9 of the f16 rounding of term 6.
5. Residual.  out = act + res with res an f16 read exactly: one more f32 rounding, u * (|out| + error so far).
   Call the sum of 2..5 `e`.
6. Storage.  An f16 output rounds the f32 value y (|y - want| <= e) to nearest: half an f16 ulp AT |y| <= |want| + e, taken
   from np.spacing on float16 so that subnormal results (spacing 2^-24) are right.  bound = e + ulp_f16(|want| + e) / 2.
   An f32 output (EPI_F32) has no term 6.
7. Second output.  out2 = ELU(scale * out + shift) is formed from the UNROUNDED f32 `out` (conv_epilogue): |scale| * e, two f32
   roundings (product, sum; one if fused), ELU's Lipschitz 1 and term 4, then term 6.
   EPI_F32 with post_aff: scale * out + shift likewise, without ELU and without term 6.
8. Pad channels cout .. cout_pad are written as exact zeros: want 0, S 0, so the bound is half the smallest f16 subnormal,
   which only 0 meets (f32 outputs: bound 0).
9. maxpool / pool_cascade / upsample2 move f16 values and compare them: exact, assert_array_equal.
10. input_op: (x - mean) * scale in f32 is two roundings (2 f32 ulps of the result, the subtraction's ulp scaled by |scale|),
   then the f16 rounding.  l2norm: the sum of c squares (c + 1 roundings relative to the sum, halved by the square root), the
   square root and the quotient, each 1 rounding: (c + 4) * u relative covers it.
11. dwpw (depthwise + pointwise in one launch) keeps the depthwise result as f16 (dwpw_k stores act(f32 sum) to LDS as halves).
   The reference rounds its float64 depthwise result the same way; where that value lies within the depthwise f32 error of an
   f16 rounding boundary the kernel may legitimately pick the neighbouring f16, one f16 spacing away: `dwpw` returns that
   possible difference per element and the pointwise bound adds sum |w| * difference.

No constant here was read off a GPU run.
"""
import numpy as np

ACT_NONE, ACT_RELU6, ACT_ELU, ACT_SILU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3, 4, 5
ACTS = (ACT_NONE, ACT_RELU6, ACT_ELU, ACT_SILU, ACT_RELU, ACT_SIGMOID)
U = 2.0 ** -24
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU6: 1.0, ACT_ELU: 1.0, ACT_SILU: 1.1, ACT_RELU: 1.0, ACT_SIGMOID: 0.25}
TRANSCENDENTAL = (ACT_ELU, ACT_SILU, ACT_SIGMOID)


def rup(x, m):
    return (x + m - 1) // m * m


def f16(x):
    """Round to f16 (nearest even) and widen again."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def same_pad(size, k, stride):
    """TensorFlow SAME: (output size, pad before) -- the excess goes behind."""
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def geometry(h, w, kh, kw, stride, pad):
    """(ho, wo, pad_t, pad_l); pad None = TF SAME, else symmetric PyTorch-style padding."""
    if pad is None:
        ho, pt = same_pad(h, kh, stride)
        wo, pl = same_pad(w, kw, stride)
    else:
        pt = pl = pad
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    return ho, wo, pt, pl


def _padded(x, kh, kw, stride, pad_t, pad_l, ho, wo, value=0.0):
    n, h, w, c = x.shape
    hp, wp = (ho - 1) * stride + kh, (wo - 1) * stride + kw
    out = np.full((n, max(hp, pad_t + h), max(wp, pad_l + w), c), value, dtype=x.dtype)
    out[:, pad_t:pad_t + h, pad_l:pad_l + w] = x
    return out


def _window(xp, dy, dx, stride, ho, wo):
    return xp[:, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride]


def conv(x, w_hwio, b, stride, pad_t, pad_l, ho, wo):
    """Pre-activation sum s [n, ho, wo, cout] and S = |b| + sum |x * w| of a convolution with explicit top / left padding (what lies
    beyond the bottom / right edge is zero as well); any kh, kw."""
    x = np.asarray(x, np.float64); w = np.asarray(w_hwio, np.float64); b = np.asarray(b, np.float64)
    kh, kw, cin, cout = w.shape
    assert x.shape[3] == cin
    xp = _padded(x, kh, kw, stride, pad_t, pad_l, ho, wo)
    s = np.zeros((x.shape[0], ho, wo, cout)) + b
    S = np.zeros_like(s) + np.abs(b)
    for dy in range(kh):
        for dx in range(kw):
            v = _window(xp, dy, dx, stride, ho, wo)
            s += v @ w[dy, dx]
            S += np.abs(v) @ np.abs(w[dy, dx])
    return s, S


def dwconv3(x, w_hwc, b, stride, pad_t, pad_l, ho, wo):
    """Depthwise 3x3: (s, S) as `conv`."""
    x = np.asarray(x, np.float64); w = np.asarray(w_hwc, np.float64); b = np.asarray(b, np.float64)
    xp = _padded(x, 3, 3, stride, pad_t, pad_l, ho, wo)
    s = np.zeros((x.shape[0], ho, wo, x.shape[3])) + b
    S = np.zeros_like(s) + np.abs(b)
    for dy in range(3):
        for dx in range(3):
            v = _window(xp, dy, dx, stride, ho, wo)
            s += v * w[dy, dx]
            S += np.abs(v * w[dy, dx])
    return s, S


def maxpool(x, k, stride, pad):
    """k x k max pool, symmetric padding that never wins (taps outside the map are skipped)."""
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = _padded(x, k, k, stride, pad, pad, ho, wo, value=-np.inf)
    out = np.full((n, ho, wo, c), -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, _window(xp, dy, dx, stride, ho, wo))
    return out


def pool_cascade(x, k, n_casc):
    """n_casc stride-1 k x k pools of each other: [n, H, W, n_casc * c], result i in channels i*c .. (i+1)*c."""
    outs, cur = [], np.asarray(x, np.float64)
    for _ in range(n_casc):
        cur = maxpool(cur, k, 1, k // 2)
        outs.append(cur)
    return np.concatenate(outs, axis=3)


def upsample2(x):
    return np.repeat(np.repeat(np.asarray(x, np.float64), 2, axis=1), 2, axis=2)


def input_op(img, swap_rb, mean, scale, s2d=False, c_pad=0):
    """u8 [n, H, W, 3] -> (want, bound) of the input op's tensor with all its cs channels: channel swap, (x - mean) * scale with the f32
    mean / scale the op record holds, zeros behind the real channels; s2d: space-to-depth 2 in input_k's stated channel order
    (y0x0, y1x0, y0x1, y1x1) x rgb, i.e. channel (2 * dx + dy) * 3 + colour."""
    x = np.asarray(img).astype(np.float64)
    if swap_rb:
        x = x[..., ::-1]
    m, sc = float(np.float32(mean)), float(np.float32(scale))
    d = x - m
    v = d * sc
    e = U * np.abs(d) * abs(sc) + U * np.abs(v)          # the subtraction's rounding scaled, the product's rounding: 2 f32 ulps
    if s2d:
        v = np.concatenate([v[:, dy::2, dx::2] for dx in (0, 1) for dy in (0, 1)], axis=3)
        e = np.concatenate([e[:, dy::2, dx::2] for dx in (0, 1) for dy in (0, 1)], axis=3)
    cs = c_pad if c_pad else 16 if s2d else 8
    n, h, w, c = v.shape
    want, err = np.zeros((n, h, w, cs)), np.zeros((n, h, w, cs))
    want[..., :c], err[..., :c] = v, e
    return want, err + 0.5 * np.spacing((np.abs(want) + err).astype(np.float16)).astype(np.float64)


def stem_input(img, swap_rb, mean, scale):
    """What stem_conv3_k convolves: the f16 it makes of (x - mean) * scale in f32 (two f32 operations numpy repeats bit for bit), channels
    swapped when the swap is folded into the weights' order."""
    x = np.asarray(img).astype(np.float32)
    v = ((x - np.float32(mean)) * np.float32(scale)).astype(np.float16).astype(np.float64)
    return v[..., ::-1] if swap_rb else v


def stem(img, w_hwio, b, stride, swap_rb, mean, scale):
    """3x3 TF-SAME convolution on the u8 image (zero padding after normalisation): (s, S, n_terms).  w_hwio is indexed by the channel order
    the network sees (after the swap), as Program.stem takes it."""
    x = stem_input(img, swap_rb, mean, scale)
    ho, wo, pt, pl = geometry(x.shape[1], x.shape[2], 3, 3, stride, None)
    s, S = conv(x, f16(w_hwio), np.asarray(b, np.float32), stride, pt, pl, ho, wo)
    return s, S, 27


def act(v, kind):
    v = np.asarray(v, np.float64)
    if kind == ACT_NONE:
        return v
    if kind == ACT_RELU6:
        return np.clip(v, 0.0, 6.0)
    if kind == ACT_ELU:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    if kind == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if kind == ACT_RELU:
        return np.maximum(v, 0.0)
    if kind == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    raise ValueError(kind)


def _half_ulp_f16(mag):
    return 0.5 * np.spacing(np.asarray(mag, np.float64).astype(np.float16)).astype(np.float64)


def error_f32(want, S, n_terms, splitk=1, act=ACT_NONE, a=None, res=False, extra=0.0):
    """`e` of the module docstring: the error of the f32 value before it is stored.  a: the activation's value (default `want`: no
    residual); extra: further pre-activation error (dwpw: the depthwise f16 may be the neighbouring one)."""
    want = np.asarray(want, np.float64)
    a = want if a is None else np.asarray(a, np.float64)
    e = LIPSCHITZ[act] * ((n_terms + splitk + 1) * U * np.asarray(S, np.float64) + extra)
    if act in TRANSCENDENTAL:
        e = e + 16 * U * np.maximum(1.0, np.abs(a))
    if res:
        e = e + U * (np.abs(want) + e)
    return e


def bound(want, S, n_terms, splitk=1, act=ACT_NONE, a=None, res=False, f32=False, extra=0.0):
    """Per-element bound on |got - want| of an op's first output (f16, or f32 with f32=True)."""
    e = error_f32(want, S, n_terms, splitk, act, a, res, extra)
    return e if f32 else e + _half_ulp_f16(np.abs(want) + e)


def bound_out2(want2, pre2, e, scale):
    """out2 = ELU(scale * out + shift) from the unrounded out: pre2 = scale * out + shift (float64), e = error_f32 of out."""
    e2 = np.abs(scale) * e + U * (np.abs(pre2) + np.abs(scale) * e) * 2 + 16 * U * np.maximum(1.0, np.abs(want2))
    return e2 + _half_ulp_f16(np.abs(want2) + e2)


def bound_post_aff(want, e, scale):
    """EPI_F32 with post_aff: want = scale * out + shift, f32."""
    return np.abs(scale) * e + 2 * U * (np.abs(want) + np.abs(scale) * e)


def epilogue(s, S, n_terms, cout_pad, act_kind=ACT_NONE, splitk=1, res=None, aff2=None, f32=False, post_aff=None, extra=0.0):
    """conv_epilogue as it states itself: out = act(s) + res, pad channels cout .. cout_pad exactly 0; out2 = ELU(scale * out + shift)
    from the unrounded out (aff2 = (scale, shift), f16 outputs); EPI_F32 (f32=True) with or without post_aff = (scale, shift).
    Returns dict(out=(want, bound)[, out2=(want, bound)]) with cout_pad channels each."""
    s = np.asarray(s, np.float64)
    cout = s.shape[-1]
    a = act(s, act_kind)
    want = a if res is None else a + np.asarray(res, np.float64)
    e = error_f32(want, S, n_terms, splitk, act_kind, a, res is not None, extra)

    def padded(v, fill=0.0):
        out = np.full(v.shape[:-1] + (cout_pad,), fill)
        out[..., :cout] = v
        return out
    r = {}
    if f32:
        if post_aff is not None:
            sc, sh = (np.asarray(v, np.float64) for v in post_aff)
            w2 = sc * want + sh
            r['out'] = (padded(w2), padded(bound_post_aff(w2, e, sc)))
        else:
            r['out'] = (padded(want), padded(e))
        return r
    r['out'] = (padded(want), padded(e + _half_ulp_f16(np.abs(want) + e), 2.0 ** -25))
    if aff2 is not None:
        sc, sh = (np.asarray(v, np.float64) for v in aff2)
        pre2 = sc * want + sh
        w2 = act(pre2, ACT_ELU)
        r['out2'] = (padded(w2), padded(bound_out2(w2, pre2, e, sc), 2.0 ** -25))
    return r


def fc(x_flat, w_io, b, act_kind, splitk=1, aff2=None):
    """Fully connected layer on the NHWC-flattened f16 source [n, K] (the engine runs it as a 1x1 convolution over a [1, 1, K] view, EPI_F32,
    aff2 = the post-activation affine): dict(out=(want, bound)) with f32 rows [n, 1, 1, rup(cout, 8)].  splitk: the K slices the launcher used."""
    x = np.asarray(x_flat, np.float64)
    w = np.asarray(w_io, np.float64)
    s, S = conv(x[:, None, None, :], w[None, None], b, 1, 0, 0, 1, 1)
    return epilogue(s, S, w.shape[0], rup(w.shape[1], 8), act_kind, splitk, f32=True, post_aff=aff2)


def l2norm(x, eps):
    """(want, bound): x / sqrt(eps + sum x^2) over the last axis of the f32 rows the kernel read."""
    x = np.asarray(x, np.float64)
    c = x.shape[-1]
    want = x / np.sqrt(float(np.float32(eps)) + np.sum(x * x, axis=-1, keepdims=True))
    return want, (c + 4) * U * np.abs(want)


def dwpw(x, dw_hwc, dw_b, stride, pad_t, pad_l, ho, wo, dw_act, pw_io, pw_b, pw_act):
    """Depthwise 3x3 + pointwise 1x1 as dwpw_k runs them: the depthwise result act(sum) is kept as f16.  Returns (want, bound) of the f16
    output; the bound includes the pointwise image of every depthwise element that may round to the neighbouring f16 (docstring, 11)."""
    sd, Sd = dwconv3(x, dw_hwc, dw_b, stride, pad_t, pad_l, ho, wo)
    ad = act(sd, dw_act)
    ed = error_f32(ad, Sd, 9, 1, dw_act)
    d16 = f16(ad)
    # rounding is monotonic: the kernel's f16 is the rounding of some value within ed of ad, so it lies between these two
    flip = np.maximum(np.abs(f16(ad - ed) - d16), np.abs(f16(ad + ed) - d16))
    pw = np.asarray(pw_io, np.float64)
    s, S = conv(d16, pw[None, None], pw_b, 1, 0, 0, ho, wo)
    extra = flip @ np.abs(pw)
    want = act(s, pw_act)
    return want, bound(want, S, pw.shape[0], 1, pw_act, extra=extra)


def ssd_head_rows(s, p, base_rows, n_rows, ld):
    """EPI_SSD_HEAD: the conv's f32 sums [n, h, w, A * ld] -> (row index [h * w * A], values [n, h * w * A, ld]): pixel p's A rows of the head
    matrix start at base + p * A (channels already in [anchor][4 + C] order)."""
    n, h, w, c = s.shape
    A = c // ld
    rows = base_rows + np.arange(h * w * A)
    return rows, s.reshape(n, h * w * A, ld)


def yolo_rows(s, S, n_terms, no, base_rows, stride, img_wh, anchors):
    """EPI_YOLO: decoded Detect rows.  s, S [n, h, w, A * no]; img_wh = (width, height) the columns are normalised by.  Returns (rows [A * h * w],
    want [n, A * h * w, no], bound): row = base + a * h * w + p; a sigmoid everywhere, columns 0 / 1 = (2 s - 0.5 + grid x / y) * stride / (width /
    height), columns 2 / 3 = (2 s)^2 * anchor (w / h) / (width / height); f32 results, four (three) un-fused f32 operations behind the sigmoid."""
    n, h, w, c = s.shape
    A = c // no
    sg = act(s, ACT_SIGMOID).reshape(n, h, w, A, no)
    e = error_f32(sg, S.reshape(n, h, w, A, no), n_terms, 1, ACT_SIGMOID)
    want, bnd = sg.copy(), e.copy()
    gx, gy = np.arange(w)[None, None, :, None], np.arange(h)[None, :, None, None]
    an = np.asarray(anchors, np.float64)[:2 * A].reshape(A, 2)
    for col, grid in ((0, gx), (1, gy)):
        k = stride / img_wh[col]
        want[..., col] = (sg[..., col] * 2 - 0.5 + grid) * k
        bnd[..., col] = 2 * e[..., col] * k + 4 * U * (np.abs(sg[..., col] * 2 - 0.5) + grid + 2 * e[..., col]) * k
    for col in (2, 3):
        k = an[:, col - 2][None, None, None, :] / img_wh[col - 2]
        want[..., col] = (sg[..., col] * 2) ** 2 * k
        de = (8 * sg[..., col] * e[..., col] + 4 * e[..., col] ** 2) * k
        bnd[..., col] = de + 3 * U * (np.abs(want[..., col]) + de)
    want = want.transpose(0, 3, 1, 2, 4).reshape(n, A * h * w, no)
    bnd = bnd.transpose(0, 3, 1, 2, 4).reshape(n, A * h * w, no)
    return base_rows + np.arange(A * h * w), want, bnd


def assert_within(name, got, want, bnd):
    """Every element: |got - want| <= bound (none excluded); prints the share of its bound the worst element uses."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bnd = np.broadcast_to(np.asarray(bnd, np.float64), want.shape)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all(), name
    err = np.abs(got - want)
    share = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = int(np.argmax(share))
    used = float(share.reshape(-1)[worst])
    print('%s: worst of %d elements uses %.1f %% of its bound (|err| %.3e of %.3e at |want| %.3e; max |err| %.3e; 0 %% excluded)'
          % (name, want.size, 100 * used, float(err.reshape(-1)[worst]), float(bnd.reshape(-1)[worst]),
             float(np.abs(want).reshape(-1)[worst]), float(err.max())))
    assert used <= 1.0, '%s: element %s off by %.3e, bound %.3e (%.1f x)' % (
        name, np.unravel_index(worst, want.shape), float(err.reshape(-1)[worst]), float(bnd.reshape(-1)[worst]), used)
    return used
