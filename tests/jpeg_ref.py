"""The definition of deepdish_amd.jpeg: a numpy restatement of libjpeg's baseline 4:2:0 encoder (integer colour conversion, h2v2
down-sampling, the accurate-integer forward DCT, quality-scaled ITU-T T.81 Annex K.1 / K.2 tables, Annex K.3 Huffman tables, restart
markers) that writes whole files.  tests/test_jpeg_ref.py holds it to Pillow byte for byte; tests/test_gpu_jpeg.py holds the kernel to it.

    encode(bgr, quality=95, restart_rows=1) -> bytes            bgr: u8 [H, W, 3]
    encode_info(...) -> (bytes, {'zrl': ZRL symbols written, 'scan': the entropy-coded bytes between the SOS segment and EOI})
    header(H, W, quality, restart_rows) -> bytes                SOI .. the SOS segment
"""
import numpy as np

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
# Annex K.1 / K.2, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)
# Annex K.3: number of codes of each length 1 .. 16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
            36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
            73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
            132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
            178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
            217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
              214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])

FIX = {k: int(round(v * 8192)) for k, v in dict(
    c0_298=0.298631336, c0_390=0.390180644, c0_541=0.541196100, c0_765=0.765366865, c0_899=0.899976223, c1_175=1.175875602,
    c1_501=1.501321110, c1_847=1.847759065, c1_961=1.961570560, c2_053=2.053119869, c2_562=2.562915447, c3_072=3.072711026).items()}


def quant_tables(quality):
    """(luma, chroma) in natural order: libjpeg's jpeg_set_quality with force_baseline."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError('quality %d: 1 .. 100' % quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def huffman_codes(table):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def geometry(H, W, restart_rows):
    H, W, restart_rows = int(H), int(W), int(restart_rows)
    if not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise ValueError('a %d x %d frame: 1 .. 8192 either way' % (W, H))
    mw, mh = (W + 15) // 16, (H + 15) // 16
    if restart_rows < 1 or restart_rows * mw > 65535:
        raise ValueError('restart_rows %d: >= 1, and at most 65535 MCUs in an interval' % restart_rows)
    return mw, mh


def header(H, W, quality=95, restart_rows=1):
    mw, _ = geometry(H, W, restart_rows)
    ql, qc = quant_tables(quality)
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    out += _segment(0xDB, bytes([0]) + bytes(int(v) for v in ql[ZIGZAG])) + _segment(0xDB, bytes([1]) + bytes(int(v) for v in qc[ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, (restart_rows * mw).to_bytes(2, 'big'))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint.c over the last axis of d (int64 [..., 8])."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * FIX['c0_541']
    out[2] = _descale(z1 + t13 * FIX['c0_765'], n)
    out[6] = _descale(z1 - t12 * FIX['c1_847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * FIX['c1_175']
    t4, t5, t6, t7 = t4 * FIX['c0_298'], t5 * FIX['c2_053'], t6 * FIX['c3_072'], t7 * FIX['c1_501']
    z1, z2, z3, z4 = -z1 * FIX['c0_899'], -z2 * FIX['c2_562'], -z3 * FIX['c1_961'] + z5, -z4 * FIX['c0_390'] + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _blocks(plane, q):
    """u8 [8a, 8b] -> quantised coefficients int64 [a, b, 64] in zigzag order."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int64).reshape(a, 8, b, 8).transpose(0, 2, 1, 3) - 128           # [a, b, row, col]
    d = _fdct_pass(d, True)                                                             # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)                # columns
    c = d.reshape(a, b, 64)
    div = 8 * q.astype(np.int64)
    return (np.sign(c) * ((np.abs(c) + (div >> 1)) // div))[..., ZIGZAG]


def planes(bgr):
    """The padded Y, Cb, Cr sample planes the DCT sees (Y: whole MCUs; Cb, Cr: half that either way)."""
    bgr = np.asarray(bgr)
    assert bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.dtype == np.uint8
    H, W = bgr.shape[:2]
    mw, mh = (W + 15) // 16, (H + 15) // 16
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    cols = np.minimum(np.arange(16 * mw), W - 1)
    y = y[np.minimum(np.arange(16 * mh), H - 1)][:, cols]
    out = [y]
    bias = np.tile([1, 2], 8 * mw // 2 + 1)[:8 * mw]
    for c in (cb, cr):
        c = c[np.minimum(np.arange(H + (H & 1)), H - 1)][:, cols]            # columns to whole MCUs, one more row when H is odd
        c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(c[np.minimum(np.arange(8 * mh), c.shape[0] - 1)])         # its own last row down to whole MCUs
    return [p.astype(np.uint8) for p in out]


def coefficients(bgr, quality=95):
    """Per MCU the six blocks' quantised coefficients, zigzag order, dummy blocks filled in: int64 [mh, mw, 6, 64]."""
    H, W = bgr.shape[:2]
    ql, qc = quant_tables(quality)
    y, cb, cr = planes(bgr)
    mw, mh = (W + 15) // 16, (H + 15) // 16
    cy = _blocks(y, ql).reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64)
    bw, bh = (W + 7) // 8, (H + 7) // 8
    for k in range(1, 4):                       # a dummy block: no AC, the DC of the block before it in the MCU
        by = 2 * np.arange(mh)[:, None] + (k >> 1)
        bx = 2 * np.arange(mw)[None, :] + (k & 1)
        dummy = (by >= bh) | (bx >= bw)
        cy[:, :, k, 1:][dummy] = 0
        cy[:, :, k, 0][dummy] = cy[:, :, k - 1, 0][dummy]
    return np.concatenate([cy, _blocks(cb, qc)[:, :, None], _blocks(cr, qc)[:, :, None]], axis=2)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        if self.n >= 512:
            keep = self.n & 7
            self.out += (self.acc >> keep).to_bytes((self.n - keep) // 8, 'big')
            self.acc &= (1 << keep) - 1
            self.n = keep

    def finish(self):
        pad = -self.n & 7
        self.put((1 << pad) - 1, pad)
        if self.n:
            self.out += self.acc.to_bytes(self.n // 8, 'big')
        return bytes(self.out).replace(b'\xff', b'\xff\x00')


def encode_info(bgr, quality=95, restart_rows=1):
    bgr = np.ascontiguousarray(bgr)
    H, W = bgr.shape[:2]
    mw, mh = geometry(H, W, restart_rows)
    coef = coefficients(bgr, quality).tolist()
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    scan, zrl = bytearray(), 0
    n_int = (mh + restart_rows - 1) // restart_rows
    for iv in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        for my in range(iv * restart_rows, min(mh, (iv + 1) * restart_rows)):
            for mx in range(mw):
                for k, c in enumerate(coef[my][mx]):
                    comp = max(0, k - 3)
                    tab = 1 if comp else 0
                    diff, pred[comp] = c[0] - pred[comp], c[0]
                    size = abs(diff).bit_length()
                    bits.put(*dc[tab][size])
                    if size:
                        bits.put((diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size)
                    run = 0
                    for v in c[1:]:
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            bits.put(*ac[tab][0xF0])
                            zrl += 1
                            run -= 16
                        size = abs(v).bit_length()
                        bits.put(*ac[tab][run * 16 + size])
                        bits.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)
                        run = 0
                    if run:
                        bits.put(*ac[tab][0x00])
        scan += bits.finish()
        if iv + 1 < n_int:
            scan += bytes([0xFF, 0xD0 + (iv & 7)])
    return header(H, W, quality, restart_rows) + bytes(scan) + b'\xff\xd9', {'zrl': zrl, 'scan': bytes(scan)}


def encode(bgr, quality=95, restart_rows=1):
    return encode_info(bgr, quality, restart_rows)[0]
