"""The definition of deepdish_amd.jpeg.JpegDecoder(..., scale=s) for s = 2, 4, 8: libjpeg's scaled decode (scale_num / scale_denom = 1 / s,
what Pillow's Image.draft selects) restated in numpy on top of tests/jpeg_dec_ref.py.  The entropy decoder is that file's; what changes is
jdmaster.c's block size per component, jidctred.c's reduced transforms, and which up-sampler jdsample.c picks.
tests/test_jpeg_scaled_ref.py holds it to Pillow byte for byte; tests/test_jpeg_scaled_host.py and tests/test_gpu_jpeg_scaled.py hold the
header's transforms and the kernels to it.

    decode(file_bytes, s) -> u8 [ceil(H / s), ceil(W / s), 3] BGR          s = 1 is jpeg_dec_ref.decode
    draft_scale((sw, sh), (dw, dh)) -> 1 | 2 | 4 | 8                        Pillow's JpegImageFile.draft rule
    block_size(hs, vs, hmax, vmax, s), plane_size(...)                      jdmaster.c
    idct_reduced(blocks, q, n) -> u8 [blocks, n, n]                         jidctred.c (n = 8: jidctint.c)"""
import functools

import numpy as np

from jpeg_dec_ref import RANGE_LIMIT, _fix, _up_h, coefficients, idct, parse
import jpeg_dec_ref

SCALES = (1, 2, 4, 8)

# jidctred.c: FIX(x) at CONST_BITS 13
F_0_211, F_0_509, F_0_601, F_0_720, F_0_765, F_0_850, F_0_899 = 1730, 4176, 4926, 5906, 6270, 6967, 7373
F_1_061, F_1_272, F_1_451, F_1_847, F_2_172, F_2_562, F_3_624 = 8697, 10426, 11893, 15137, 17799, 20995, 29692


def draft_scale(src_wh, want_wh):
    """The largest of 8, 4, 2, 1 that is <= min(sw // dw, sh // dh); 1 when that is 0."""
    (sw, sh), (dw, dh) = src_wh, want_wh
    k = min(sw // dw, sh // dh)
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def block_size(hs, vs, hmax, vmax, s):
    """Samples a side that a component's 8 x 8 block becomes (jdmaster.c, DCT_scaled_size)."""
    if s not in SCALES:
        raise ValueError('scale %r is none of 1, 2, 4, 8' % (s,))
    m = 8 // s
    n = m
    while n < 8 and (hmax * m) % (hs * n * 2) == 0 and (vmax * m) % (vs * n * 2) == 0:
        n *= 2
    return n


def plane_size(H, W, hs, vs, hmax, vmax, s):
    """-> (n, rows, columns) of a component before cropping to the output."""
    n = block_size(hs, vs, hmax, vmax, s)
    return n, -(-H * vs * n // (vmax * 8)), -(-W * hs * n // (hmax * 8))


def _pass4(c, shift):
    """jpeg_idct_4x4, one pass over the last axis (int64 [..., 8]; term 4 is not read) -> [..., 4]."""
    t0 = c[..., 0] << 14
    t2 = c[..., 2] * F_1_847 - c[..., 6] * F_0_765
    t10, t12 = t0 + t2, t0 - t2
    z1, z2, z3, z4 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    o0 = -z1 * F_0_211 + z2 * F_1_451 - z3 * F_2_172 + z4 * F_1_061
    o2 = -z1 * F_0_509 - z2 * F_0_601 + z3 * F_0_899 + z4 * F_2_562
    r = 1 << (shift - 1)
    return np.stack([(t10 + o2 + r) >> shift, (t12 + o0 + r) >> shift, (t12 - o0 + r) >> shift, (t10 - o2 + r) >> shift], axis=-1)


def _pass2(c, shift):
    """jpeg_idct_2x2, one pass over the last axis (terms 0, 1, 3, 5, 7) -> [..., 2]."""
    t10 = c[..., 0] << 15
    t0 = -c[..., 7] * F_0_720 + c[..., 5] * F_0_850 - c[..., 3] * F_1_272 + c[..., 1] * F_3_624
    r = 1 << (shift - 1)
    return np.stack([(t10 + t0 + r) >> shift, (t10 - t0 + r) >> shift], axis=-1)


def idct_reduced(blocks, q, n):
    """i16 [k, 64] quantised, natural order; q [64] natural -> u8 [k, n, n]."""
    if n == 8:
        return idct(blocks, q)
    c = (blocks.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    if n == 1:
        return RANGE_LIMIT[((c[:, 0, 0] + 4) >> 3) & 1023].reshape(-1, 1, 1)
    one, shifts = (_pass4, (12, 19)) if n == 4 else (_pass2, (13, 20))
    ws = one(c.transpose(0, 2, 1), shifts[0]).transpose(0, 2, 1)          # columns: [k, n, 8]
    return RANGE_LIMIT[one(ws, shifts[1]) & 1023]                           # rows: [k, n, n]


@functools.lru_cache(maxsize=1024)
def _parsed(data):
    """A file's header and coefficients, decoded once for all its scales."""
    c = coefficients(data)
    c.setflags(write=False)
    return parse(data), c


def planes(data, s):
    """Each component's samples over its own scaled size."""
    h, coef = _parsed(bytes(data))
    H, W, mx, my, bpm = h['height'], h['width'], h['mcus_x'], h['mcus_y'], h['blocks_per_mcu']
    coef = coef.reshape(my, mx, bpm, 64)
    out, k0 = [], 0
    for (_, hs, vs, tq) in h['comps']:
        n, rows, cols = plane_size(H, W, hs, vs, h['hmax'], h['vmax'], s)
        p = idct_reduced(coef[:, :, k0:k0 + hs * vs].reshape(-1, 64), h['quant'][tq], n).reshape(my, mx, vs, hs, n, n)
        out.append(p.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * n, mx * hs * n)[:rows, :cols])
        k0 += hs * vs
    return h, out


def _up_h2v1(p, fancy):
    p = p.astype(np.int64)
    even, odd = _up_h(p, fancy)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (even + 1) >> 2, (odd + 2) >> 2
    return out


def decode(data, s=1):
    if s not in SCALES:
        raise ValueError('scale %r is none of 1, 2, 4, 8' % (s,))
    if s == 1:
        return jpeg_dec_ref.decode(data)
    h, pl = planes(data, s)
    oh, ow = -(-h['height'] // s), -(-h['width'] // s)
    y = pl[0].astype(np.int64)
    assert y.shape == (oh, ow)
    if h['ncomp'] == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    ch = []
    for p in pl[1:]:
        if p.shape == (oh, ow):                                   # 4:4:4, and 4:2:0, whose chroma blocks stay twice the luma's
            ch.append(p.astype(np.int64) - 128)
        else:                                                       # 4:2:2: h2v1; fancy unless s = 8 (min_DCT_scaled_size 1) or a width <= 2
            assert p.shape[0] == oh and 2 * p.shape[1] >= ow
            ch.append(_up_h2v1(p, s < 8 and p.shape[1] > 2)[:, :ow] - 128)
    cb, cr = ch
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)

