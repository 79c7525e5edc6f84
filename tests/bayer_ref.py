"""numpy restatement of the 8-bit Bayer mosaic / monochrome -> BGR converter (csrc/bayer.hip): the definition the kernels are held to, bit for bit.

Names give the sensor's top-left 2 x 2 block read row by row.  OpenCV names the block at (1, 1) instead, so each corresponds to:

    'bayer_rggb'  cv2.COLOR_BayerBG2BGR      'bayer_grbg'  cv2.COLOR_BayerGB2BGR
    'bayer_bggr'  cv2.COLOR_BayerRG2BGR      'bayer_gbrg'  cv2.COLOR_BayerGR2BGR

(newer versions carry the COLOR_BayerRGGB2BGR ... aliases).  The rule is OpenCV's published bilinear demosaic, restated; OpenCV itself is
absent, so parity with cv2.cvtColor is unpinned, as for the YUV formats.  The output is BGR.

    out(x, y) = D(clamp(x, 1, W - 2), clamp(y, 1, H - 2))

i.e. the outer ring of pixels repeats its inner neighbour, corners included.  For an interior site D is
    at an R or B site:  its own colour is the sample, G = (N + S + W + E + 2) >> 2, the opposite colour = (NW + NE + SW + SE + 2) >> 2
    at a G site:        G is the sample, the colour of its horizontal neighbours = (W + E + 1) >> 1, of its vertical ones = (N + S + 1) >> 1
W >= 3 and H >= 3 are required, either may be odd.  A tap never leaves the frame: only the evaluation point is clamped.

'gray' means B = G = R = the sample, for any W, H >= 1 (cv2.COLOR_GRAY2BGR).

No white balance, gamma or colour matrix: a camera that sends 8-bit Bayer has applied its own before the mosaic leaves it.  The forward
transforms that make synthetic inputs live in deepdish_amd.synth (to_bayer, to_gray) and pin nothing."""
import numpy as np

PATTERNS = ('bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr')
LAYOUTS = PATTERNS + ('gray',)


def plane(buf, height, width, pitch=0):
    """One frame's bytes (flat u8, or [H, W] when dense) -> its [H, W] view."""
    assert width >= 1 and height >= 1
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    p = pitch or width
    assert p >= width and buf.size >= p * (height - 1) + width
    return np.lib.stride_tricks.as_strided(buf, (height, width), (p, 1))


def site_colours(pattern, height, width):
    """[H, W] of 'r', 'g', 'b': the colour each site of the mosaic samples."""
    assert pattern in PATTERNS, pattern
    block = np.array(list(pattern[6:])).reshape(2, 2)
    return block[np.arange(height)[:, None] & 1, np.arange(width)[None, :] & 1]


def bayer_to_bgr(buf, height, width, pattern, pitch=0):
    """One Bayer frame (flat or [H, W] u8; pitch: bytes per row, 0 = W) -> BGR u8 [H, W, 3]."""
    assert width >= 3 and height >= 3, (width, height)
    m = plane(buf, height, width, pitch).astype(np.int32)
    c = m[1:-1, 1:-1]
    n, s, w, e = m[:-2, 1:-1], m[2:, 1:-1], m[1:-1, :-2], m[1:-1, 2:]
    cross = (n + s + w + e + 2) >> 2
    diag = (m[:-2, :-2] + m[:-2, 2:] + m[2:, :-2] + m[2:, 2:] + 2) >> 2
    hor, ver = (w + e + 1) >> 1, (n + s + 1) >> 1
    col = site_colours(pattern, height, width)
    here = col[1:-1, 1:-1]
    beside = col[1:-1, :-2]                                      # the colour of a site's horizontal neighbours
    chan = {}
    for k in 'rb':
        other = 'b' if k == 'r' else 'r'
        chan[k] = np.where(here == k, c, np.where(here == other, diag, np.where(beside == k, hor, ver)))
    chan['g'] = np.where(here == 'g', c, cross)
    inner = np.stack([chan['b'], chan['g'], chan['r']], axis=-1).astype(np.uint8)
    return np.pad(inner, ((1, 1), (1, 1), (0, 0)), mode='edge')


def gray_to_bgr(buf, height, width, pitch=0):
    """One monochrome frame -> BGR u8 [H, W, 3]."""
    return np.repeat(plane(buf, height, width, pitch)[..., None], 3, axis=2)


def raw8_to_bgr(buf, height, width, layout, pitch=0):
    if layout == 'gray':
        return gray_to_bgr(buf, height, width, pitch)
    return bayer_to_bgr(buf, height, width, layout, pitch)
