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
12. Fused launches (res_unit_rows_k, res_pair_rows_k, mars_pair64_k, conv3x3_pool_rows_k<STEM>, stem_conv_pool_wide_k, ssd_front_k,
   conv_ws_dw_k) keep every tensor between two layers as f16 -- in an LDS ring or tile, rounded by the same (_Float16) conversion the
   layer-by-layer path applies before its store -- so the compositions below round at the same points (`flip_f16`) and carry term 11
   from layer to layer (`spread`: sum |w| * difference over the next layer's window; a skip tensor's difference adds to the sum as
   it is).  mars_ws128_k adds the partial sums of its two K halves and then the bias: a conv with splitk = 2 in term 2.
   A max pool of f16 results moves by no more than the largest bound in its window.
   What this costs: behind a layer of 288 or 576 terms the f32 error bound of term 2 is of the order of an f16 spacing, so nearly every
   element in between may be the neighbouring f16 and the composition's bound comes to some 20 half-ulps of the result (through the four
   layers of res_pair_rows_k: to the size of the result).  It is a bound and the GPU tests assert it, but the check that discriminates is
   EXACT_MID below: the same compositions fed with the tensors in between as the layer-by-layer run of the same engine wrote them (the fused
   launch's outputs must equal that run's bit for bit), each layer then held to its own one-op bound.

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


def error_out2(want2, pre2, e, scale):
    """The f32 error of out2 = ELU(scale * out + shift) before it is stored (docstring, 7)."""
    return np.abs(scale) * e + U * (np.abs(pre2) + np.abs(scale) * e) * 2 + 16 * U * np.maximum(1.0, np.abs(want2))


def bound_out2(want2, pre2, e, scale):
    """out2 = ELU(scale * out + shift) from the unrounded out: pre2 = scale * out + shift (float64), e = error_f32 of out."""
    e2 = error_out2(want2, pre2, e, scale)
    return e2 + _half_ulp_f16(np.abs(want2) + e2)


def bound_post_aff(want, e, scale):
    """EPI_F32 with post_aff: want = scale * out + shift, f32."""
    return np.abs(scale) * e + 2 * U * (np.abs(want) + np.abs(scale) * e)


def epilogue(s, S, n_terms, cout_pad, act_kind=ACT_NONE, splitk=1, res=None, aff2=None, f32=False, post_aff=None, extra=0.0, with_e=False):
    """conv_epilogue as it states itself: out = act(s) + res, pad channels cout .. cout_pad exactly 0; out2 = ELU(scale * out + shift)
    from the unrounded out (aff2 = (scale, shift), f16 outputs); EPI_F32 (f32=True) with or without post_aff = (scale, shift).
    Returns dict(out=(want, bound)[, out2=(want, bound)]) with cout_pad channels each; with_e: also e_out[, e_out2], the f32 errors before
    storage (what a fused launch's next layer needs to know which neighbouring f16 the kernel may have kept)."""
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
    if with_e:
        r['e_out'] = padded(e + np.zeros_like(want))
    if aff2 is not None:
        sc, sh = (np.asarray(v, np.float64) for v in aff2)
        pre2 = sc * want + sh
        w2 = act(pre2, ACT_ELU)
        r['out2'] = (padded(w2), padded(bound_out2(w2, pre2, e, sc), 2.0 ** -25))
        if with_e:
            r['e_out2'] = padded(error_out2(w2, pre2, e, sc))
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


HOOK = None      # tests/test_fused_op_ref.py: a callable (stage, value, ctx) -> value that turns a composition below into a mutant of itself
# True: the f16 tensors between the layers are KNOWN (a HOOK puts in at 'mid.h16' what the layer-by-layer run of the same engine wrote, whose
# final tensors the fused launch must equal bit for bit), so no neighbouring f16 has to be allowed for and each layer gets its own one-op bound.
# With a first layer of 288 or 576 terms the f32 error bound of term 2 is of the order of an f16 spacing, so the composition's own bound has
# to allow a neighbouring f16 for most elements of the tensor in between and comes to some 20 half-ulps of the result; this form does not.
EXACT_MID = False


def hook(stage, v, **ctx):
    """Stages of the fused compositions: 'mid.s' / 'last.s' the pre-activation sum of an inner / the last layer (ctx: x, w, b, geom = (stride,
    pad_t, pad_l, ho, wo), dw = depthwise), 'mid.h16' the f16 tensor between two layers (ctx: a = its unrounded value; 'mid.d16': the
    depthwise rows of a dw + pw pair, which no path of the engine writes to memory), 'res' the skip tensor, 'pool' the pooled result."""
    return v if HOOK is None or v is None else HOOK(stage, v, ctx)


def flip_f16(want, e, written=True):
    """(f16(want), flip): the f16 a kernel keeps of a value it computed within e of `want`, and how far that f16 may lie from f16(want).
    Rounding is monotonic: the kernel's f16 is the rounding of some value in [want - e, want + e], so it lies between the roundings of the
    two ends -- 0 almost everywhere, one f16 spacing where `want` is within e of a rounding boundary.  written=False: a tensor no path of the
    engine writes to memory (the depthwise rows of a dw + pw launch), which EXACT_MID therefore cannot know."""
    want = np.asarray(want, np.float64)
    d16 = f16(want)
    if EXACT_MID and written:
        return d16, np.zeros_like(d16)
    return d16, np.maximum(np.abs(f16(want - e) - d16), np.abs(f16(want + e) - d16))


def spread(flip, w_hwio, stride, pad_t, pad_l, ho, wo):
    """sum |w| * flip over a convolution's window: how far a layer's pre-activation sum moves when each input moves by its `flip`."""
    if flip is None or not np.any(flip):
        return 0.0
    w = np.abs(np.asarray(w_hwio, np.float64))
    kh, kw = w.shape[:2]
    xp = _padded(np.asarray(flip, np.float64), kh, kw, stride, pad_t, pad_l, ho, wo)
    return sum(_window(xp, dy, dx, stride, ho, wo) @ w[dy, dx] for dy in range(kh) for dx in range(kw))


def _kept_f16(s, S, n_terms, act_kind, extra=0.0, splitk=1, written=True):
    """(h16, flip) of a layer's result that the launch keeps as f16: act(s) rounded, as flip_f16."""
    a = act(s, act_kind)
    h16, flip = flip_f16(a, error_f32(a, S, n_terms, splitk, act_kind, extra=extra), written)
    return hook('mid.h16' if written else 'mid.d16', h16, a=a), flip


def layer_f16(x, w_hwio, b, stride, pad_t, pad_l, ho, wo, act_kind, x_flip=None, splitk=1):
    """A dense layer whose f16 result stays on the chip (an LDS ring or tile between the two layers of a fused launch): (h16, flip) as
    flip_f16; x_flip: the same for its own input (docstring, 12)."""
    w = np.asarray(w_hwio, np.float64)
    s, S = conv(x, w, b, stride, pad_t, pad_l, ho, wo)
    s = hook('mid.s', s, x=x, w=w, b=b, geom=(stride, pad_t, pad_l, ho, wo), dw=False)
    return _kept_f16(s, S, w.shape[0] * w.shape[1] * w.shape[2], act_kind, spread(x_flip, w, stride, pad_t, pad_l, ho, wo), splitk)


def res_unit(x, res, A, B, aff2, x_flip=None, res_flip=None, with_e=False, splitk=1):
    """Residual unit as res_unit_rows_k / res_pair_rows_k / mars_pair64_k run it: h1 = f16(ELU(conv_A(x) + b_A)) stays on the chip, then
    out = f16(conv_B(h1) + b_B + res) and out2 = f16(ELU(scale * out + shift)) from the unrounded out.  A = (w, b, stride, pad_t, pad_l, ho, wo),
    B = (w, b) (3x3, stride 1, pad 1).  Returns epilogue()'s dict; x_flip / res_flip: how far the f16 inputs themselves may be off."""
    wa, ba, stride, pt, pl, ho, wo = A
    h16, hflip = layer_f16(x, wa, ba, stride, pt, pl, ho, wo, ACT_ELU, x_flip, splitk)
    wb = np.asarray(B[0], np.float64)
    s, S = conv(h16, wb, B[1], 1, 1, 1, ho, wo)
    s = hook('last.s', s, x=h16, w=wb, b=B[1], geom=(1, 1, 1, ho, wo), dw=False)
    extra = spread(hflip, wb, 1, 1, 1, ho, wo) + (0.0 if res_flip is None else res_flip)
    return epilogue(s, S, 9 * wb.shape[2], wb.shape[3], ACT_NONE, splitk, res=hook('res', res), aff2=aff2, extra=extra, with_e=with_e)


def res_pair(x, A1, B1, aff1, A2, B2, aff2):
    """Two residual units as res_pair_rows_k runs them: the first unit's out and out2 cross to the second as f16 rows (its skip and its
    input); the first unit's skip is its own input."""
    r1 = res_unit(x, x, A1, B1, aff1, with_e=True)
    o16, oflip = flip_f16(r1['out'][0], r1['e_out'])
    p16, pflip = flip_f16(r1['out2'][0], r1['e_out2'])
    o16, p16 = hook('mid.h16', o16, a=r1['out'][0]), hook('mid.h16', p16, a=r1['out2'][0])
    return res_unit(p16, o16, A2, B2, aff2, x_flip=pflip, res_flip=oflip)


def proj_block(x, x2, A, Pj, B, aff2):
    """A widening block as mars_pair64_k<FIRST> runs it: the 1x1 stride-2 projection of x2 (Pj = (w, b), no activation) is kept as an f16
    tile (sk = (_Float16)(acc + bias) in the kernel) and is the skip of the unit A, B."""
    wp = np.asarray(Pj[0], np.float64)
    ho, wo = A[5], A[6]
    s, S = conv(x2, wp, Pj[1], 2, 0, 0, ho, wo)
    sk16, skflip = flip_f16(s, error_f32(s, S, wp.shape[2]))
    return res_unit(x, hook('mid.h16', sk16, a=s), A, B, aff2, res_flip=skflip)


def _stem_f16(img, w0, b0, stride, swap_rb, mean, scale, act_kind):
    s, S, nt = stem(img, w0, b0, stride, swap_rb, mean, scale)
    ho, wo, pt, pl = geometry(img.shape[1], img.shape[2], 3, 3, stride, None)
    s = hook('mid.s', s, x=stem_input(img, swap_rb, mean, scale), w=f16(w0), b=np.asarray(b0, np.float32), geom=(stride, pt, pl, ho, wo), dw=False)
    return _kept_f16(s, S, nt, act_kind)


def stem_conv_pool(img, w0, b0, swap_rb, mean, scale, w1, b1):
    """First layer + 3x3 32 -> 32 layer + VALID 3x3 / 2 max pool as conv3x3_pool_rows_k<STEM> / stem_conv_pool_wide_k run them (both ELU): the
    first layer's result is kept as f16 rows.  Returns {'out': (want, bound)} of the pooled tensor (a maximum moves by no more than its
    operands do; the kernels pool the f32 sums and then apply ELU and round, which is the same value: both are monotonic)."""
    h16, hflip = _stem_f16(img, w0, b0, 1, swap_rb, mean, scale, ACT_ELU)
    w = np.asarray(w1, np.float64)
    ho, wo = h16.shape[1], h16.shape[2]
    s1, S1 = conv(h16, w, b1, 1, 1, 1, ho, wo)
    s1 = hook('last.s', s1, x=h16, w=w, b=b1, geom=(1, 1, 1, ho, wo), dw=False)
    r = epilogue(s1, S1, 9 * w.shape[2], w.shape[3], ACT_ELU, extra=spread(hflip, w, 1, 1, 1, ho, wo))
    return {'out': (hook('pool', maxpool(r['out'][0], 3, 2, 0)), maxpool(r['out'][1], 3, 2, 0))}


def ssd_front(img, w0, b0, mean, scale, dw_hwc, dw_b, pw_io, pw_b):
    """First layer (stride 2, ReLU6) + the first MobileNet block (depthwise 3x3 + pointwise, ReLU6 both) as ssd_front_k runs them: the first
    layer's rows and the depthwise rows are f16.  (want, bound) of the block's output."""
    h16, hflip = _stem_f16(img, w0, b0, 2, False, mean, scale, ACT_RELU6)
    ho, wo = h16.shape[1], h16.shape[2]
    c = np.asarray(dw_hwc).shape[2]
    return dwpw(h16[..., :c], dw_hwc, dw_b, 1, 1, 1, ho, wo, ACT_RELU6, pw_io, pw_b, ACT_RELU6, x_flip=hflip[..., :c])


def pw_dw(x, pw_io, pw_b, dw_hwc, dw_b, splitk=1):
    """Pointwise layer (ReLU6) + the next block's depthwise 3x3 (stride 1, pad 1, ReLU6) as conv_ws_dw_k runs them: the pointwise result is
    kept as f16 (yv = (_Float16)act(acc + bias) in the kernel).  (want, bound) of the depthwise output."""
    pw = np.asarray(pw_io, np.float64)
    ho, wo = np.asarray(x).shape[1:3]
    y16, yflip = layer_f16(x, pw[None, None], pw_b, 1, 0, 0, ho, wo, ACT_RELU6, splitk=splitk)
    dw = np.asarray(dw_hwc, np.float64)
    s, S = dwconv3(y16, dw, dw_b, 1, 1, 1, ho, wo)
    s = hook('last.s', s, x=y16, w=dw, b=dw_b, geom=(1, 1, 1, ho, wo), dw=True)
    extra = dwconv3(yflip, np.abs(dw), np.zeros(dw.shape[2]), 1, 1, 1, ho, wo)[0]
    want = act(s, ACT_RELU6)
    return want, bound(want, S, 9, 1, ACT_RELU6, extra=extra)


def dwpw(x, dw_hwc, dw_b, stride, pad_t, pad_l, ho, wo, dw_act, pw_io, pw_b, pw_act, x_flip=None):
    """Depthwise 3x3 + pointwise 1x1 as dwpw_k runs them: the depthwise result act(sum) is kept as f16.  Returns (want, bound) of the f16
    output; the bound includes the pointwise image of every depthwise element that may round to the neighbouring f16 (docstring, 11).
    x_flip: how far the f16 input itself may be off (a first layer in the same launch)."""
    sd, Sd = dwconv3(x, dw_hwc, dw_b, stride, pad_t, pad_l, ho, wo)
    sd = hook('mid.s', sd, x=x, w=np.asarray(dw_hwc, np.float64), b=dw_b, geom=(stride, pad_t, pad_l, ho, wo), dw=True)
    dwa = np.abs(np.asarray(dw_hwc, np.float64))
    extra_d = 0.0 if x_flip is None else dwconv3(x_flip, dwa, np.zeros(dwa.shape[2]), stride, pad_t, pad_l, ho, wo)[0]
    # rounding is monotonic: the kernel's f16 is the rounding of some value within the depthwise error of act(sd), so it lies between the
    # roundings of the two ends (flip_f16)
    d16, flip = _kept_f16(sd, Sd, 9, dw_act, extra_d, written=False)
    pw = np.asarray(pw_io, np.float64)
    s, S = conv(d16, pw[None, None], pw_b, 1, 0, 0, ho, wo)
    s = hook('last.s', s, x=d16, w=pw[None, None], b=pw_b, geom=(1, 0, 0, ho, wo), dw=False)
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
