"""numpy restatement of the packed 4:2:2 (YUY2 / UYVY) -> BGR decoder (csrc/yuv.hip): the definition the kernels are held to, bit for bit.

It restates OpenCV's COLOR_YUV2BGR_YUY2 / COLOR_YUV2BGR_UYVY.  Per pixel the arithmetic is yuv_ref.yuv_to_bgr, unchanged: OpenCV's published
BT.601 fixed-point constants, 20 fractional bits, max(0, Y - 16), arithmetic shifts, saturation, output order B, G, R.  OpenCV itself is
absent, so parity with it is unpinned, as for NV12 / I420.  Decoder only -- the forward transform that makes synthetic inputs lives in
deepdish_amd.synth.to_yuv422 and pins nothing.

A row of W pixels (W even) is 2 W bytes, made of 4-byte macropixels:
    'yuy2'  Y0 U Y1 V:  pixel x has Y at byte 2x,     U at 4 (x >> 1) + 1, V at 4 (x >> 1) + 3
    'uyvy'  U Y0 V Y1:  pixel x has Y at byte 2x + 1, U at 4 (x >> 1),     V at 4 (x >> 1) + 2
The two pixels of a macropixel share its chroma: no chroma interpolation, and no vertical sub-sampling (H may be odd)."""
import numpy as np

from yuv_ref import yuv_to_bgr

ORDERS = ('yuy2', 'uyvy')


def samples(buf, height, width, order, pitch=0):
    """One frame's bytes (flat u8, or [H, W, 2] when dense) -> (Y [H, W], U [H, W / 2], V [H, W / 2]) views."""
    assert width > 0 and width % 2 == 0 and height > 0
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    p = pitch or 2 * width
    assert p >= 2 * width and buf.size >= p * (height - 1) + 2 * width
    if order == 'yuy2':
        y0, u0, v0 = 0, 1, 3
    elif order == 'uyvy':
        y0, u0, v0 = 1, 0, 2
    else:
        raise ValueError(order)
    strided = np.lib.stride_tricks.as_strided
    return (strided(buf[y0:], (height, width), (p, 2)), strided(buf[u0:], (height, width // 2), (p, 4)),
            strided(buf[v0:], (height, width // 2), (p, 4)))


def yuv422_to_bgr(buf, height, width, order, pitch=0):
    """One YUY2 / UYVY frame (flat or [H, W, 2] u8; pitch: bytes per row, 0 = 2 W) -> BGR u8 [H, W, 3]."""
    y, u, v = samples(buf, height, width, order, pitch)
    return yuv_to_bgr(y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1))
