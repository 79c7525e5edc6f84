"""The definition of progressive (SOF2) decoding in deepdish_amd.jpeg (parse(..., progressive=True), JpegDecoder(..., progressive=True)):
a numpy restatement of libjpeg's jdphuff.c and of jdinput.c's per-scan geometry, on top of tests/jpeg_dec_ref.py.  A progressive file ends
in the same quantised coefficients, in the same blocks, as a baseline file; the IDCT, up-sampling and colour stages are that file's and
tests/jpeg_scaled_ref.py's, unchanged.  tests/test_jpeg_prog_ref.py holds it to Pillow byte for byte; tests/test_jpeg_prog_host.py and
tests/test_gpu_jpeg_progressive.py hold the parser, the shared statements and the kernels to it.

    parse(file_bytes) -> dict                     the baseline header's keys, and 'scans': one dict per SOS, in file order
    coefficients(file_bytes) -> i16 [blocks, 64]  jpeg_dec_ref.coefficients' layout: natural order, blocks in MCU order
    decode(file_bytes, s=1) -> u8 [ceil(H / s), ceil(W / s), 3] BGR

A baseline file is handed to jpeg_dec_ref.  What is refused raises ValueError with the reason's word (REFUSALS) in front; damaged entropy
data raises ValueError('corrupt ...').

Per scan (jdinput.c per_scan_setup): a scan of several components walks the frame's MCUs, each component's hs x vs blocks at their place
in the MCU; a scan of one component walks that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order -- not the MCU-padded
grid, whose other blocks such a scan never touches -- and its restart interval counts blocks.  The DRI in force is the one last read in
front of the scan; the Huffman tables are those the DHT segments in front of the scan left in the four slots of each class.

Values no valid file holds, stated here because the kernel has to do something defined with them: a coefficient v of a first scan is
stored as the low 16 bits of v << Al, two's complement; a DC predictor wraps at 32 bits; a refinement adds or subtracts 1 << Al in
16 bits, wrapping.  A DC category above 11, an AC-refinement magnitude category other than 1, a run that passes Se, an EOB run that
outlives its restart interval and bits taken from beyond the interval are corrupt."""
import numpy as np

import jpeg_dec_ref
import jpeg_scaled_ref
from jpeg_dec_ref import _decoder_table, _fix, _intervals, _real_bytes, _u16
from jpeg_ref import ZIGZAG

MAX_SCANS, MAX_TABLES = 64, 32
REFUSALS = ('progressive', 'ac_components', 'ac_before_dc', 'first_ah', 'refinement', 'incomplete', 'capacity')


def _i16(v):
    return ((int(v) + 32768) & 65535) - 32768


def parse(data):
    d = bytes(data)
    n = len(d)
    try:
        return jpeg_dec_ref.parse(d)
    except ValueError as e:
        if 'progressive' not in str(e):
            raise
        baseline_refusal = e
    out = {'quant': {}, 'restart_interval': 0, 'adobe_transform': None, 'scans': []}
    slots, n_tables = {}, 0
    state = None                     # per component and zigzag index: the Al delivered so far (-1: nothing) and the level of the scan that did
    i = 2
    while i + 4 <= n:                # to EOI, or to the end of a file that has none: what the scans delivered decides
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
            break
        L = _u16(d, i + 2)
        if L < 2 or i + 2 + L > n:
            raise ValueError('truncated: a segment length runs past the file')
        p, e = i + 4, i + 2 + L
        if 0xC0 <= m <= 0xCF and m not in (0xC2, 0xC4, 0xC8):
            if m == 0xC6:
                raise ValueError('progressive: differential progressive files (SOF6) are refused')
            raise baseline_refusal
        if m == 0xC2:
            if state is not None:
                raise ValueError('a second SOF segment')
            if L < 8:
                raise ValueError('truncated SOF segment')
            if d[p] != 8:
                raise ValueError('%d-bit precision is refused (8 only)' % d[p])
            H, W, nc = _u16(d, p + 1), _u16(d, p + 3), d[p + 5]
            if not (1 <= H <= jpeg_dec_ref.MAX_SIDE and 1 <= W <= jpeg_dec_ref.MAX_SIDE):
                raise ValueError('size %d x %d: 1 .. %d either way' % (W, H, jpeg_dec_ref.MAX_SIDE))
            if nc not in (1, 3):
                raise ValueError('%d components are refused (1 or 3)' % nc)
            if L != 8 + 3 * nc:
                raise ValueError('truncated SOF segment')
            comps = [(d[p + 6 + 3 * c], d[p + 7 + 3 * c] >> 4, d[p + 7 + 3 * c] & 15, d[p + 8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]
            elif (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                raise ValueError('sampling %s is refused (4:4:4, 4:2:2, 4:2:0)' % ', '.join('%dx%d' % (c[1], c[2]) for c in comps))
            if any(c[3] > 3 for c in comps):
                raise ValueError('quant table index above 3')
            hmax, vmax = comps[0][1], comps[0][2]
            mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
            out.update(height=H, width=W, ncomp=nc, comps=comps, sof=m, hmax=hmax, vmax=vmax, mcus_x=mx, mcus_y=my,
                       blocks_per_mcu=sum(c[1] * c[2] for c in comps))
            state = np.full((nc, 64, 2), -1, np.int64)
        elif m == 0xDB:
            while p < e:
                if d[p] >> 4:
                    raise ValueError('16-bit quant tables are refused')
                tq = d[p] & 15
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
                if tc > 1 or th > 3:
                    raise ValueError('DHT class %d id %d: four tables per class' % (tc, th))
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
                if n_tables >= MAX_TABLES:
                    raise ValueError('capacity: more than %d Huffman tables' % MAX_TABLES)
                slots[(tc, th)] = (n_tables, bits, list(d[p + 17:p + 17 + cnt]))
                n_tables += 1
                p += 17 + cnt
        elif m == 0xDD:
            if L != 4:
                raise ValueError('bad DRI segment')
            out['restart_interval'] = _u16(d, p)
        elif m == 0xEE:
            if L >= 14 and d[p:p + 5] == b'Adobe':
                out['adobe_transform'] = d[p + 11]
        elif m == 0xDA:
            if state is None:
                raise ValueError('SOS before SOF')
            ns = d[p] if L >= 3 else 0
            if ns < 1 or ns > 4 or L != 6 + 2 * ns:
                raise ValueError('bad SOS segment')
            if ns > out['ncomp']:
                raise ValueError('scans: a scan of %d components in a file of %d' % (ns, out['ncomp']))
            ids = [c[0] for c in out['comps']]
            cs, td, ta = [], [], []
            for k in range(ns):
                if d[p + 1 + 2 * k] not in ids:
                    raise ValueError('scans: a scan names a component the frame does not hold')
                c = ids.index(d[p + 1 + 2 * k])
                if cs and c <= cs[-1]:
                    raise ValueError('scans: a scan out of component order')
                cs.append(c)
                td.append(d[p + 2 + 2 * k] >> 4)
                ta.append(d[p + 2 + 2 * k] & 15)
            ss, se, ah, al = d[p + 1 + 2 * ns], d[p + 2 + 2 * ns], d[p + 3 + 2 * ns] >> 4, d[p + 3 + 2 * ns] & 15
            if ss > se or se > 63 or (ss == 0 and se != 0) or al > 13 or ah > 13:
                raise ValueError('bad SOS segment: Ss %d, Se %d, Ah %d, Al %d' % (ss, se, ah, al))
            if ss > 0 and ns != 1:
                raise ValueError('ac_components: an AC scan of %d components' % ns)
            if len(out['scans']) >= MAX_SCANS:
                raise ValueError('capacity: more than %d scans' % MAX_SCANS)
            level = 0
            for c in cs:
                if ss > 0 and state[c, 0, 0] < 0:
                    raise ValueError('ac_before_dc: an AC scan of component %d before its DC scan' % c)
                have = state[c, ss:se + 1, 0]
                if (have != have[0]).any():
                    raise ValueError('refinement: a band whose coefficients stand at different bits')
                if have[0] < 0:
                    if ah != 0:
                        raise ValueError('first_ah: the first scan of a band with Ah %d' % ah)
                elif ah != have[0] or al != ah - 1:
                    raise ValueError('refinement: Ah %d, Al %d on a band that stands at bit %d' % (ah, al, have[0]))
                level = max(level, int(state[c, ss:se + 1, 1].max()) + 1)
            for k, c in enumerate(cs):
                if (ss == 0 and ah == 0 and (0, td[k]) not in slots) or (ss > 0 and (1, ta[k]) not in slots):
                    raise ValueError('a Huffman table the scan references is not defined')
                if td[k] > 3 or ta[k] > 3:
                    raise ValueError('Huffman table index above 3')
                state[c, ss:se + 1, 0] = al
                state[c, ss:se + 1, 1] = level
            q = e                                                            # the entropy-coded bytes end in front of the next marker
            while q < n and not (d[q] == 0xFF and q + 1 < n and d[q + 1] != 0 and d[q + 1] != 0xFF and not 0xD0 <= d[q + 1] <= 0xD7):
                q += 1
            if ns > 1:
                bw, bh = out['mcus_x'], out['mcus_y']
            else:
                _, hs, vs, _ = out['comps'][cs[0]]
                bw = -(-(-(-out['width'] * hs // out['hmax'])) // 8)
                bh = -(-(-(-out['height'] * vs // out['vmax'])) // 8)
            units = bw * bh
            ri = out['restart_interval'] or units
            out['scans'].append(dict(comps=cs, ss=ss, se=se, ah=ah, al=al, restart_interval=out['restart_interval'], start=e, end=q, level=level,
                                     bw=bw, bh=bh, units=units, n_intervals=-(-units // ri),
                                     dc=[slots[(0, t)] if (0, t) in slots else None for t in td],
                                     ac=[slots[(1, t)] if (1, t) in slots else None for t in ta]))
            i = q
            continue
        i = e
    if state is None:
        raise ValueError('truncated: the file ends before an SOF segment')
    for c in range(out['ncomp']):
        if out['comps'][c][3] not in out['quant']:
            raise ValueError('a quant table a component references is not defined')
    if out['ncomp'] == 3 and out['adobe_transform'] not in (None, 1):
        raise ValueError('Adobe transform %d on a 3-component file is refused (YCbCr only)' % out['adobe_transform'])
    if (state[:, :, 0] != 0).any():
        raise ValueError('incomplete: the scans end with coefficients not delivered to bit 0 (libjpeg would smooth or zero-fill; this build refuses)')
    out['n_tables'] = n_tables
    out['n_levels'] = 1 + max(s['level'] for s in out['scans'])
    return out


class _Bits:
    def __init__(self, real):
        self.total = 8 * len(real)
        stream = np.unpackbits(np.frombuffer(real + b'\0' * 40, np.uint8))
        w = np.zeros(len(stream) - 16, np.int64)
        for k in range(16):
            w = (w << 1) | stream[k:len(stream) - 16 + k]
        self.w = w.tolist()
        self.pos = 0

    def symbol(self, tab, what):
        if self.pos > self.total:
            raise ValueError('corrupt: the interval ends before its blocks do')
        e = tab[self.w[self.pos]]
        if e == 0:
            raise ValueError('corrupt: a code that is not in the %s table' % what)
        self.pos += e >> 8
        return e & 255

    def take(self, s):
        if self.pos > self.total:
            raise ValueError('corrupt: the interval ends before its blocks do')
        v = self.w[self.pos] >> (16 - s)
        self.pos += s
        return v

    def extend(self, s):
        v = self.take(s)
        return v - ((1 << s) - 1) if v < (1 << (s - 1)) else v


def block_index(h, c, bx, by):
    """Where block (bx, by) of component c lies in the MCU-interleaved coefficient array."""
    _, hs, vs, _ = h['comps'][c]
    base = sum(k[1] * k[2] for k in h['comps'][:c])
    return ((by // vs) * h['mcus_x'] + bx // hs) * h['blocks_per_mcu'] + base + (by % vs) * hs + bx % hs


def _scan(h, sc, d, out, tables):
    zz = ZIGZAG.tolist()
    ss, se, ah, al = sc['ss'], sc['se'], sc['ah'], sc['al']
    units = sc['units']
    ri = sc['restart_interval'] or units
    p1 = 1 << al
    for iv, raw in enumerate(_intervals(d[sc['start']:sc['end']], sc['n_intervals'])):
        b = _Bits(_real_bytes(raw))
        pred = [0] * h['ncomp']
        eobrun = 0
        for u in range(iv * ri, min(units, (iv + 1) * ri)):
            if len(sc['comps']) > 1:
                ux, uy = u % h['mcus_x'], u // h['mcus_x']
                blocks = [(k, c, block_index(h, c, ux * h['comps'][c][1] + x, uy * h['comps'][c][2] + y))
                          for k, c in enumerate(sc['comps']) for y in range(h['comps'][c][2]) for x in range(h['comps'][c][1])]
            else:
                blocks = [(0, sc['comps'][0], block_index(h, sc['comps'][0], u % sc['bw'], u // sc['bw']))]
            for k, c, bi in blocks:
                blk = out[bi]
                if ss == 0 and ah == 0:                                     # DC first
                    s = b.symbol(tables[sc['dc'][k][0]], 'DC')
                    if s > 11:
                        raise ValueError('corrupt: a DC category above 11')
                    if s:
                        pred[c] = (pred[c] + b.extend(s)) & 0xFFFFFFFF
                    blk[0] = _i16((pred[c] << al) & 0xFFFF)
                elif ss == 0:                                               # DC refinement
                    if b.take(1):
                        blk[0] = _i16(int(blk[0]) | p1)
                elif ah == 0:                                               # AC first
                    if eobrun > 0:
                        eobrun -= 1
                    else:
                        tab = tables[sc['ac'][k][0]]
                        j = ss
                        while j <= se:
                            rs = b.symbol(tab, 'AC')
                            r, s = rs >> 4, rs & 15
                            if s:
                                j += r
                                v = b.extend(s)
                                if j > se:
                                    raise ValueError('corrupt: a run past Se')
                                blk[zz[j]] = _i16((v << al) & 0xFFFF)
                            elif r == 15:
                                j += 15
                            else:
                                eobrun = (1 << r) + (b.take(r) if r else 0) - 1
                                break
                            j += 1
                else:                                                       # AC refinement
                    j = ss
                    if eobrun == 0:
                        tab = tables[sc['ac'][k][0]]
                        while j <= se:
                            rs = b.symbol(tab, 'AC')
                            r, s = rs >> 4, rs & 15
                            if s:
                                if s != 1:
                                    raise ValueError('corrupt: a refinement of magnitude category %d' % s)
                                s = p1 if b.take(1) else -p1
                            elif r != 15:
                                eobrun = (1 << r) + (b.take(r) if r else 0)
                                break
                            while j <= se:
                                v = int(blk[zz[j]])
                                if v:
                                    if b.take(1) and not (v & p1):
                                        blk[zz[j]] = _i16(v + (p1 if v >= 0 else -p1))
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                j += 1
                            if s:
                                if j > se:
                                    raise ValueError('corrupt: a run past Se')
                                blk[zz[j]] = _i16(s)
                            j += 1
                    if eobrun > 0:
                        while j <= se:
                            v = int(blk[zz[j]])
                            if v and b.take(1) and not (v & p1):
                                blk[zz[j]] = _i16(v + (p1 if v >= 0 else -p1))
                            j += 1
                        eobrun -= 1
                if b.pos > b.total:
                    raise ValueError('corrupt: interval %d ends before its blocks do' % iv)
        if eobrun:
            raise ValueError('corrupt: an EOB run that outlives its restart interval')
        if b.total - b.pos >= 8:
            raise ValueError('corrupt: interval %d holds %d bits more than its blocks' % (iv, b.total - b.pos))


def coefficients(data):
    d = bytes(data)
    h = parse(d)
    if 'scans' not in h:
        return jpeg_dec_ref.coefficients(d)
    tables = {}
    for sc in h['scans']:
        for t in sc['dc'] + sc['ac']:
            if t is not None and t[0] not in tables:
                tables[t[0]] = _decoder_table(t[1], t[2])
    out = np.zeros((h['mcus_x'] * h['mcus_y'] * h['blocks_per_mcu'], 64), np.int16)
    for sc in h['scans']:
        _scan(h, sc, d, out, tables)
    return out


def decode(data, s=1):
    """The baseline ref's stages (s = 1) and the scaled ref's (2, 4, 8) over this file's coefficients."""
    d = bytes(data)
    h = parse(d)
    if 'scans' not in h:
        return jpeg_scaled_ref.decode(d, s)
    if s not in jpeg_scaled_ref.SCALES:
        raise ValueError('scale %r is none of 1, 2, 4, 8' % (s,))
    H, W, mx, my, bpm = h['height'], h['width'], h['mcus_x'], h['mcus_y'], h['blocks_per_mcu']
    coef = coefficients(d).reshape(my, mx, bpm, 64)
    pl, k0 = [], 0
    for (_, hs, vs, tq) in h['comps']:
        n, rows, cols = jpeg_scaled_ref.plane_size(H, W, hs, vs, h['hmax'], h['vmax'], s)
        p = jpeg_scaled_ref.idct_reduced(coef[:, :, k0:k0 + hs * vs].reshape(-1, 64), h['quant'][tq], n).reshape(my, mx, vs, hs, n, n)
        pl.append(p.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * n, mx * hs * n)[:rows, :cols])
        k0 += hs * vs
    oh, ow = -(-H // s), -(-W // s)
    y = pl[0].astype(np.int64)
    if h['ncomp'] == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    if s == 1:
        cb, cr = (jpeg_dec_ref.upsample(p, h['hmax'], h['vmax'], H, W) - 128 for p in pl[1:])
    else:
        cb, cr = (p.astype(np.int64) - 128 if p.shape == (oh, ow) else jpeg_scaled_ref._up_h2v1(p, s < 8 and p.shape[1] > 2)[:, :ow] - 128 for p in pl[1:])
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)
