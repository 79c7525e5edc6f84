"""numpy restatement of the NV12 / I420 -> BGR decoder (csrc/yuv.hip): the definition the kernels are held to, bit for bit.

It restates OpenCV's COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420.  The constants are OpenCV's published BT.601 fixed-point ones (20
fractional bits), taken from outside this project and quoted from general knowledge; OpenCV itself is absent, so parity with it is
unpinned.  Decoder only -- the forward transform that makes synthetic inputs lives in deepdish_amd.synth.to_yuv420 and pins nothing.

    c = max(0, Y - 16) * 1220542;  u = U - 128;  v = V - 128           (int32, arithmetic right shifts)
    R = sat8((c + 524288 + 1673527 v) >> 20)
    G = sat8((c + 524288 -  852492 v - 409993 u) >> 20)
    B = sat8((c + 524288 + 2116026 u) >> 20)                              output byte order B, G, R
The chroma sample of pixel (x, y) is that of block (x >> 1, y >> 1): no chroma interpolation."""
import numpy as np

CY, CVR, CVG, CUG, CUB, SHIFT = 1220542, 1673527, -852492, -409993, 2116026, 20
ROUND = 1 << (SHIFT - 1)


def yuv_to_bgr(Y, U, V):
    """Per-pixel arrays (any equal shape, integer) -> u8 [..., 3] in B, G, R order."""
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    c = np.maximum(Y - 16, 0) * np.int32(CY) + np.int32(ROUND)
    u, v = U - 128, V - 128
    r = (c + CVR * v) >> SHIFT
    g = (c + CVG * v + CUG * u) >> SHIFT
    b = (c + CUB * u) >> SHIFT
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def planes(buf, height, width, layout, pitch=0, chroma_offset=0):
    """One frame's bytes (flat u8) -> (Y [H, W], U [H/2, W/2], V [H/2, W/2]) views."""
    assert height % 2 == 0 and width % 2 == 0
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    p = pitch or width
    co = chroma_offset or p * height
    h2, w2 = height // 2, width // 2
    y = np.lib.stride_tricks.as_strided(buf, (height, width), (p, 1))
    if layout == 'nv12':
        u = np.lib.stride_tricks.as_strided(buf[co:], (h2, w2), (p, 2))
        v = np.lib.stride_tricks.as_strided(buf[co + 1:], (h2, w2), (p, 2))
    elif layout == 'i420':
        u = np.lib.stride_tricks.as_strided(buf[co:], (h2, w2), (p // 2, 1))
        v = np.lib.stride_tricks.as_strided(buf[co + (p // 2) * h2:], (h2, w2), (p // 2, 1))
    else:
        raise ValueError(layout)
    return y, u, v


def yuv420_to_bgr(buf, height, width, layout, pitch=0, chroma_offset=0):
    """One NV12 / I420 frame (flat or [H * 3 // 2, W] u8) -> BGR u8 [H, W, 3]."""
    y, u, v = planes(buf, height, width, layout, pitch, chroma_offset)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    return yuv_to_bgr(y, up(u), up(v))
