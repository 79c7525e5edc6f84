"""Test-side int64 statement of every op of the uint8 engine (csrc/netsq.hip), from a layer dict alone -- what tests/test_gpu_q_ops.py holds
each kernel to, one op at a time, and what tests/test_q_op_ref.py checks on the CPU (against the whole-model restatements, for liveliness
and against mutants).

The arithmetic is oracle/nets_quant.py's (conv_u8, dwconv_u8, the fixed-point functions, ssd_quant_decode) and tests/quant_v2_ref.py's
add_u8.  Added here is only what a one-op program needs beyond them:
  * phantom channels: a bordered tensor stores a multiple of 16 channels, the ones beyond the layer's hold the output zero point;
  * rows outputs (the SSD heads): pixel p of a map writes `cout_store` bytes at `base_off + p * row_bytes` of a plain per-frame byte
    array; class rows are padded per anchor to a multiple of 16 columns, and the phantom columns are the bytes of a channel whose stored
    filter row is zero (weight byte 128) and whose folded bias is zero: bias = -K (za - 128)(zw - 128);
  * the residual ADD behind a projection;
  * the raw bordered layout [n][h + 2][c / 16][w + 2][16] (stored byte = a ^ 0x80), to state borders and stray writes.
A second, slower statement of the convolution and the depthwise layer (acc_conv: explicit loops over taps, int64) returns the accumulators -- the
quantiles the cases' biases and scales were chosen from -- and takes the mutants of test_q_op_ref.py.  It is checked equal to conv_u8.

Nothing here imports the packing or the requantisation words of deepdish_amd/netsq.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import nets_quant as nq  # noqa: E402
import quant_v2_ref  # noqa: E402

add_u8 = quant_v2_ref.add_u8
geometry = nq._same_geometry                                  # (size, k, stride) -> (output size, pad before)


# ------------------------------------------------------------------------------------------- ops
def phantom(y, c_store, zp):
    """[n,h,w,c] -> [n,h,w,c_store]: the channels a bordered tensor stores beyond the layer's hold the zero point."""
    if y.shape[3] == c_store:
        return y
    out = np.full(y.shape[:3] + (c_store,), zp, np.uint8)
    out[..., :y.shape[3]] = y
    return out


def conv(x, L, c_store=None):
    """Bordered output of a convolution: [n,ho,wo,c_store] (c_store: the next multiple of 16)."""
    y = nq.conv_u8(x[..., :L['w'].shape[2]], L)
    return phantom(y, c_store or (y.shape[3] + 15) // 16 * 16, L['out_zp'])


def dw(x, L):
    return nq.dwconv_u8(x, L)


def conv_add(x, L, res, add):
    """A projection with the residual ADD behind it (MobileNet-v2): ADD(conv(x), res) over every stored channel -- phantom channels of
    both operands hold their zero points, the sum's hold ADD(z1, z2)."""
    y = conv(x, L, res.shape[3])
    return add_u8(y, res, add)


def rows_layer(L, a, n_cols):
    """The layer a rows predictor computes column by column: a anchors x n_cols channels laid out as a rows of row_cols = n_cols padded to
    16; a phantom column is a channel with weight bytes 128 and bias -K (za - 128)(zw - 128) (zero filter row, zero folded bias)."""
    row_cols = (n_cols + 15) // 16 * 16
    kh, kw, cin, cout = L['w'].shape
    assert cout == a * n_cols
    w = np.full((kh, kw, cin, a * row_cols), 128, L['w'].dtype)
    b = np.full(a * row_cols, -(kh * kw * cin) * (int(L['in_zp']) - 128) * (int(L['w_zp']) - 128), np.int64)
    for an in range(a):
        w[..., an * row_cols:an * row_cols + n_cols] = L['w'][..., an * n_cols:(an + 1) * n_cols]
        b[an * row_cols:an * row_cols + n_cols] = L['bias'][an * n_cols:(an + 1) * n_cols]
    return dict(L, w=w, bias=b), row_cols


def rows_write(buf, y, base_off, row_bytes, cout_store):
    """buf u8 [n, frame bytes]; y u8 [n,ho,wo,C]: pixel p writes y[p, :cout_store] at base_off + p * row_bytes."""
    n, ho, wo, _ = y.shape
    yy = y.reshape(n, ho * wo, -1)
    for p in range(ho * wo):
        buf[:, base_off + p * row_bytes:base_off + p * row_bytes + cout_store] = yy[:, p, :cout_store]
    return buf


def rows_mask(shape, npix, base_off, row_bytes, cout_store):
    m = np.zeros(shape, bool)
    for p in range(npix):
        m[:, base_off + p * row_bytes:base_off + p * row_bytes + cout_store] = True
    return m


def decode(box_u8, cls_u8, Lb, Lc, logistic, anchors, thr):
    """One frame's per-anchor arrays (oracle/nets_quant.ssd_quant_decode on a two-layer model description)."""
    return nq.ssd_quant_decode(dict(layers=dict(box0=Lb, cls0=Lc), logistic=logistic), box_u8, cls_u8, anchors, thr)


# ------------------------------------------------------------------------------------------- raw layout
def to_raw(y, zp):
    """u8 [n,h,w,c] (c % 16 == 0) -> the bytes dd_net_read returns: [n][h + 2][c / 16][w + 2][16], stored a ^ 0x80, borders = zp."""
    n, h, w, c = y.shape
    raw = np.full((n, h + 2, c // 16, w + 2, 16), zp, np.uint8)
    raw[:, 1:-1, :, 1:-1, :] = np.transpose(y.reshape(n, h, w, c // 16, 16), (0, 1, 3, 2, 4))
    return raw ^ 0x80


# ------------------------------------------------------------------------------------------- explicit accumulators, mutants
def _requant(acc, L, mut=()):
    m, shift, lo, hi = nq.layer_fixed_point(L)
    if 'byte_clamp' in mut:
        lo, hi = 0, 255
    if 'floor_round' in mut:                                   # the second rounding as a plain arithmetic shift
        y = nq.srdhm(acc, m) >> (-shift)
    else:
        y = nq.multiply_by_quantized_multiplier(acc, m, shift)
    return np.clip(y + L['out_zp'], lo, hi).astype(np.uint8)


def acc_conv(x, L, mut=()):
    """int64 accumulators (bias included) of a convolution or (L['kind'] == 'dw') a depthwise layer, taps outside the frame skipped.
    mut: names of deliberate faults (tests/test_q_op_ref.py)."""
    depthwise = L.get('kind') == 'dw'
    w = L['w'].astype(np.int64) - int(L['w_zp'])
    k, stride = w.shape[0], L['stride']
    n, h, wd, cin = x.shape
    oh, pt = geometry(h, k, stride)
    ow, pl = geometry(wd, k, stride)
    if 'pad_side' in mut:                                      # the padding's odd pixel on the wrong side
        pt = max((oh - 1) * stride + k - h, 0) - pt
        pl = max((ow - 1) * stride + k - wd, 0) - pl
    xi = x.astype(np.int64) - int(L['in_zp'])
    if 'drop_plane' in mut and not depthwise:                  # the last 16-channel plane of the last 64-channel k slice
        xi = xi.copy()
        xi[..., (cin - 1) // 16 * 16:] = 0
    cout = w.shape[2] if depthwise else w.shape[3]
    acc = np.zeros((n, oh, ow, cout), np.int64)
    rowsum = np.zeros((n, oh, ow, cout if depthwise else 1), np.int64)
    for dy in range(k):
        for dx in range(k):
            sx = dx + 1 if ('shift_tap' in mut and (dy, dx) == (0, 0)) else dx
            for oy in range(oh):
                iy = oy * stride + dy - pt
                if not 0 <= iy < h:
                    continue
                ix = np.arange(ow) * stride + sx - pl
                ok = (ix >= 0) & (ix < wd)
                v = xi[:, iy, ix[ok], :]
                if depthwise:
                    acc[:, oy, ok, :] += v * w[dy, dx]
                    rowsum[:, oy, ok, :] += x[:, iy, ix[ok], :].astype(np.int64) - 128
                else:
                    acc[:, oy, ok, :] += (v.astype(np.float64) @ w[dy, dx].astype(np.float64)).astype(np.int64)      # exact: every sum < 2^53
                    rowsum[:, oy, ok, :] += (x[:, iy, ix[ok], :].astype(np.int64) - 128).sum(axis=-1, keepdims=True)
    if 'drop_rowsum' in mut:
        # the device sums stored bytes a' = a - 128 over the WHOLE window (border bytes hold za'), so the missing term is zwc * sum a' with
        # the padded taps at za': rowsum above + (taps outside) * channels * za'
        za, zw = int(L['in_zp']) - 128, int(L['w_zp']) - 128
        taps_in = np.zeros((oh, ow), np.int64)
        for dy in range(k):
            for dx in range(k):
                iy = np.arange(oh) * stride + dy - pt
                ix = np.arange(ow) * stride + dx - pl
                taps_in += ((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < wd))[None, :]
        per_tap = 1 if depthwise else cin
        full = rowsum + ((k * k - taps_in) * per_tap * za)[None, :, :, None]
        acc = acc + zw * full
    bias = L['bias'].astype(np.int64)
    if 'next_bias' in mut:
        bias = np.roll(bias, 1)
    return acc + bias


def conv_slow(x, L, mut=()):
    return _requant(acc_conv(x[..., :L['w'].shape[2]] if L.get('kind') != 'dw' else x, L, mut), L, mut)
