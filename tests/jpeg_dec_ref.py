"""The definition of deepdish_amd.jpeg.JpegDecoder: a numpy restatement of libjpeg's baseline decoder (Annex F Huffman decoding with
the file's own tables, restart intervals, jidctint.c's accurate-integer IDCT, fancy up-sampling, jdcolor.c's YCbCr -> RGB).
tests/test_jpeg_dec_ref.py holds it to Pillow byte for byte; tests/test_gpu_jpeg_decode.py holds the kernels to it.

    parse(file_bytes) -> dict                    the header, SOI .. the first SOS; ValueError names what is refused
    coefficients(file_bytes) -> i16 [blocks, 64] quantised coefficients, natural order, blocks in MCU order (the scan's own order)
    decode(file_bytes) -> u8 [H, W, 3] BGR       cv2.imread's channel order; a one-component file gives B = G = R = Y

Damaged entropy data raises ValueError('corrupt ...'); what libjpeg paints for such a file is not restated."""
import numpy as np

from jpeg_ref import FIX, ZIGZAG

MAX_SIDE = 8192


def _u16(d, i):
    return (d[i] << 8) | d[i + 1]


def parse(data):
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError('no SOI marker')
    out = {'quant': {}, 'huff': {}, 'restart_interval': 0, 'adobe_transform': None}
    sof = None
    i = 2
    while True:
        if i + 4 > n:
            raise ValueError('truncated: the file ends before an SOS segment')
        if d[i] != 0xFF:
            raise ValueError('no marker at offset %d' % i)
        m = d[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m == 0xD9:
            raise ValueError('truncated: EOI before an SOS segment')
        L = _u16(d, i + 2)
        if L < 2 or i + 2 + L > n:
            raise ValueError('truncated: a segment length runs past the file')
        p, e = i + 4, i + 2 + L
        if m == 0xC2 or m == 0xC6:
            raise ValueError('progressive files are refused')
        if m in (0xC3, 0xC7, 0xCB, 0xCF):
            raise ValueError('lossless files are refused')
        if m in (0xC9, 0xCA, 0xCD, 0xCE, 0xCC):
            raise ValueError('arithmetic coding is refused')
        if m == 0xC5:
            raise ValueError('hierarchical (differential) files are refused')
        if m in (0xC0, 0xC1):
            if sof is not None:
                raise ValueError('a second SOF segment')
            if L < 8:
                raise ValueError('truncated SOF segment')
            if d[p] != 8:
                raise ValueError('%d-bit precision is refused (8 only)' % d[p])
            H, W, nc = _u16(d, p + 1), _u16(d, p + 3), d[p + 5]
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise ValueError('size %d x %d: 1 .. %d either way' % (W, H, MAX_SIDE))
            if nc not in (1, 3):
                raise ValueError('%d components are refused (1 or 3)' % nc)
            if L != 8 + 3 * nc:
                raise ValueError('truncated SOF segment')
            comps = [(d[p + 6 + 3 * c], d[p + 7 + 3 * c] >> 4, d[p + 7 + 3 * c] & 15, d[p + 8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]          # a lone component's factors only scale the MCU: libjpeg ignores them
            else:
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    raise ValueError('sampling %s is refused (4:4:4, 4:2:2, 4:2:0)' % ', '.join('%dx%d' % (c[1], c[2]) for c in comps))
            if any(c[3] > 3 for c in comps):
                raise ValueError('quant table index above 3')
            sof = m
            out.update(height=H, width=W, ncomp=nc, comps=comps, sof=m)
        elif m == 0xDB:
            while p < e:
                pq, tq = d[p] >> 4, d[p] & 15
                if pq != 0:
                    raise ValueError('16-bit quant tables are refused')
                if tq > 3 or p + 65 > e:
                    raise ValueError('bad DQT segment')
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(d[p + 1:p + 65], np.uint8)
                out['quant'][tq] = t
                p += 65
        elif m == 0xC4:
            while p < e:
                if p + 17 > e:
                    raise ValueError('bad DHT segment')
                tc, th = d[p] >> 4, d[p] & 15
                if tc > 1 or th > 1:
                    raise ValueError('DHT class %d id %d: baseline holds two tables per class' % (tc, th))
                bits = list(d[p + 1:p + 17])
                cnt = sum(bits)
                if cnt > 256:
                    raise ValueError('a DHT names more than 256 symbols')
                code = 0
                for l, b in enumerate(bits, 1):
                    code += b
                    if code > (1 << l):
                        raise ValueError('a DHT over-subscribes the code space')
                    code <<= 1
                if p + 17 + cnt > e:
                    raise ValueError('bad DHT segment')
                out['huff'][(tc, th)] = (bits, list(d[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif m == 0xDD:
            if L != 4:
                raise ValueError('bad DRI segment')
            out['restart_interval'] = _u16(d, p)
        elif m == 0xEE:
            if L >= 14 and d[p:p + 5] == b'Adobe':
                out['adobe_transform'] = d[p + 11]
        elif m == 0xDA:
            if sof is None:
                raise ValueError('SOS before SOF')
            ns = d[p] if L >= 3 else 0
            if L != 6 + 2 * ns:
                raise ValueError('bad SOS segment')
            if ns != out['ncomp']:
                raise ValueError('several scans are refused (this one holds %d of %d components)' % (ns, out['ncomp']))
            td, ta = [], []
            for c in range(ns):
                if d[p + 1 + 2 * c] != out['comps'][c][0]:
                    raise ValueError('several scans or a scan out of component order')
                td.append(d[p + 2 + 2 * c] >> 4)
                ta.append(d[p + 2 + 2 * c] & 15)
            ss, se, a = d[p + 1 + 2 * ns], d[p + 2 + 2 * ns], d[p + 3 + 2 * ns]
            if (ss, se, a) != (0, 63, 0):
                raise ValueError('a scan with Ss %d, Se %d, Ah/Al %d: progressive parameters are refused' % (ss, se, a))
            for c in range(ns):
                if td[c] > 1 or ta[c] > 1:
                    raise ValueError('Huffman table index above 1')
                if (0, td[c]) not in out['huff'] or (1, ta[c]) not in out['huff']:
                    raise ValueError('a Huffman table the scan references is not defined')
                if out['comps'][c][3] not in out['quant']:
                    raise ValueError('a quant table a component references is not defined')
            if out['ncomp'] == 3 and out['adobe_transform'] not in (None, 1):
                raise ValueError('Adobe transform %d on a 3-component file is refused (YCbCr only)' % out['adobe_transform'])
            hmax, vmax = out['comps'][0][1], out['comps'][0][2]
            mx, my = -(-out['width'] // (8 * hmax)), -(-out['height'] // (8 * vmax))
            ri = out['restart_interval'] or mx * my
            out.update(td=td, ta=ta, hmax=hmax, vmax=vmax, mcus_x=mx, mcus_y=my, blocks_per_mcu=sum(c[1] * c[2] for c in out['comps']),
                       n_intervals=-(-mx * my // ri), scan_offset=e, scan_length=n - e)
            return out
        i = e


def _decoder_table(bits, vals):
    """16-bit prefix -> length << 8 | symbol (0: no such code)."""
    t = np.zeros(65536, np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            if k < len(vals):
                t[code << (16 - l):(code + 1) << (16 - l)] = (l << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return t.tolist()


def _intervals(scan, n_int):
    """Split the scan bytes at its RSTn markers; the last interval runs to the file's end."""
    pos, out, start = 0, [], 0
    n = len(scan)
    while pos + 1 < n:
        if scan[pos] == 0xFF and 0xD0 <= scan[pos + 1] <= 0xD7:
            if scan[pos + 1] != 0xD0 + (len(out) & 7):
                raise ValueError('corrupt: RST%d where RST%d belongs' % (scan[pos + 1] - 0xD0, len(out) & 7))
            out.append(scan[start:pos])
            start = pos + 2
            pos += 2
        else:
            pos += 1
    out.append(scan[start:])
    if len(out) != n_int:
        raise ValueError('corrupt: %d restart intervals, the header implies %d' % (len(out), n_int))
    return out


def _real_bytes(iv):
    """The interval's entropy-coded bytes up to the first marker, unstuffed."""
    out = bytearray()
    i, n = 0, len(iv)
    while i < n:
        b = iv[i]
        if b == 0xFF:
            if i + 1 < n and iv[i + 1] == 0:
                out.append(0xFF)
                i += 2
                continue
            break
        out.append(b)
        i += 1
    return bytes(out)


def coefficients(data):
    h = parse(data)
    d = bytes(data)
    scan = d[h['scan_offset']:]
    dct = [_decoder_table(*h['huff'][(0, t)]) for t in h['td']]
    act = [_decoder_table(*h['huff'][(1, t)]) for t in h['ta']]
    mcus = h['mcus_x'] * h['mcus_y']
    ri = h['restart_interval'] or mcus
    plan = [c for c, comp in enumerate(h['comps']) for _ in range(comp[1] * comp[2])]
    out = np.zeros((mcus * len(plan), 64), np.int16)
    zz = ZIGZAG.tolist()
    for iv, raw in enumerate(_intervals(scan, h['n_intervals'])):
        real = _real_bytes(raw)
        total = 8 * len(real)
        stream = np.unpackbits(np.frombuffer(real + b'\0' * 40, np.uint8))
        # 16-bit windows at every bit position, computed once
        w = np.zeros(len(stream) - 16, np.int64)
        for k in range(16):
            w = (w << 1) | stream[k:len(stream) - 16 + k]
        w = w.tolist()
        pos = 0
        pred = [0] * h['ncomp']
        for m in range(iv * ri, min(mcus, (iv + 1) * ri)):
            for k, c in enumerate(plan):
                e = dct[c][w[pos]]
                if e == 0:
                    raise ValueError('corrupt: a code that is not in the DC table')
                pos += e >> 8
                s = e & 255
                if s > 11:
                    raise ValueError('corrupt: a DC category above 11')
                if s:
                    v = w[pos] >> (16 - s)
                    pos += s
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                    pred[c] += v
                blk = out[m * len(plan) + k]
                blk[0] = np.int16(((pred[c] + 32768) & 65535) - 32768)
                j = 1
                tab = act[c]
                while j < 64:
                    e = tab[w[pos]]
                    if e == 0:
                        raise ValueError('corrupt: a code that is not in the AC table')
                    pos += e >> 8
                    r, s = (e >> 4) & 15, e & 15
                    if s == 0:
                        if r != 15:
                            break
                        j += 16
                        continue
                    j += r
                    v = w[pos] >> (16 - s)
                    pos += s
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                    if j > 63:
                        raise ValueError('corrupt: a run past coefficient 63')
                    blk[zz[j]] = v
                    j += 1
                if pos > total:
                    raise ValueError('corrupt: interval %d ends before its MCUs do' % iv)
        if total - pos >= 8:
            raise ValueError('corrupt: interval %d holds %d bits more than its MCUs' % (iv, total - pos))
    return out


def _idct_pass(c, shift):
    """jidctint.c: one pass over the last axis of c (int64 [..., 8])."""
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[..., i] for i in range(8))
    z1 = (c2 + c6) * FIX['c0_541']
    t2 = z1 - c6 * FIX['c1_847']
    t3 = z1 + c2 * FIX['c0_765']
    t0 = (c0 + c4) << 13
    t1 = (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = c7, c5, c3, c1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * FIX['c1_175']
    a0, a1, a2, a3 = a0 * FIX['c0_298'], a1 * FIX['c2_053'], a2 * FIX['c3_072'], a3 * FIX['c1_501']
    z1, z2, z3, z4 = -z1 * FIX['c0_899'], -z2 * FIX['c2_562'], -z3 * FIX['c1_961'] + z5, -z4 * FIX['c0_390'] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(t10 + a3 + r) >> shift, (t11 + a2 + r) >> shift, (t12 + a1 + r) >> shift, (t13 + a0 + r) >> shift,
                     (t13 - a0 + r) >> shift, (t12 - a1 + r) >> shift, (t11 - a2 + r) >> shift, (t10 - a3 + r) >> shift], axis=-1)


RANGE_LIMIT = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.uint8)


def idct(blocks, q):
    """i16 [n, 64] quantised, natural order; q: [64] natural -> u8 [n, 8, 8]."""
    c = (blocks.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    ws = _idct_pass(c.transpose(0, 2, 1), 11).transpose(0, 2, 1)           # columns
    px = _idct_pass(ws, 18)                                                # rows
    return RANGE_LIMIT[px & 1023]


def planes(data):
    """Each component's samples over its true down-sampled size."""
    h = parse(data)
    coef = coefficients(data)
    H, W, mx, my, bpm = h['height'], h['width'], h['mcus_x'], h['mcus_y'], h['blocks_per_mcu']
    coef = coef.reshape(my, mx, bpm, 64)
    out, k0 = [], 0
    for (_, hs, vs, tq) in h['comps']:
        s = idct(coef[:, :, k0:k0 + hs * vs].reshape(-1, 64), h['quant'][tq]).reshape(my, mx, vs, hs, 8, 8)
        s = s.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
        out.append(s[:-(-H * vs // h['vmax']), :-(-W * hs // h['hmax'])])
        k0 += hs * vs
    return h, out


def _up_h(p, fancy):
    """Double the columns: int64 [R, C] of weight-w samples -> (this * 3 + neighbour), not yet scaled."""
    if not fancy:
        return p * 4, p * 4
    last = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    return 3 * p + last, 3 * p + nxt


def upsample(p, hs, vs, H, W):
    """libjpeg's fancy up-sampling of a chroma plane (1x1 sampled) below hs x vs luma; plain replication at a down-sampled width <= 2."""
    p = p.astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:H, :W]
    fancy = p.shape[1] > 2
    if vs == 1:
        even, odd = _up_h(p, fancy)
        out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
        out[:, 0::2], out[:, 1::2] = (even + 1) >> 2, (odd + 2) >> 2
        return out[:H, :W]
    if not fancy:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:H, :W]
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    rows[0::2], rows[1::2] = 3 * p + above, 3 * p + below
    even, odd = _up_h(rows, True)
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (even + 8) >> 4, (odd + 7) >> 4
    return out[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def decode(data):
    h, pl = planes(data)
    H, W = h['height'], h['width']
    y = pl[0].astype(np.int64)
    if h['ncomp'] == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb = upsample(pl[1], h['hmax'], h['vmax'], H, W) - 128
    cr = upsample(pl[2], h['hmax'], h['vmax'], H, W) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)
