"""Progressive (SOF2) files with scan scripts Pillow cannot write: test-side numpy only.  Takes the quantised coefficients of a baseline
file (tests/jpeg_dec_ref.py) and a script, and restates libjpeg's jcphuff.c: DC first and refinement scans, AC first scans with EOB runs,
AC refinement scans with their buffered correction bits.  tests/test_jpeg_prog_ref.py validates every file it writes against Pillow -- it
must decode there to exactly the pixels of the baseline file it came from -- before anything else is compared with it.

    write(baseline_file, script, eob_cap=0x7FFF, tables='scan') -> bytes
    script: a list of scans (comps, ss, se, ah, al) or (comps, ss, se, ah, al, restart_interval); comps a tuple of component indices;
            the interval counts MCUs in a scan of several components and blocks in a scan of one (0 / absent: none).
    eob_cap: the longest EOB run one EOBn symbol may carry (libjpeg's is 0x7FFF): a smaller one cuts runs into several symbols.
    tables: 'scan' -- every scan gets Huffman tables of its own in front of it, made from the symbols it uses, in a slot that changes from
            scan to scan; 'shared' -- one DC and one AC table in front of the first scan hold every scan's symbols.

A table holds all its symbols at one length, the shortest that leaves the all-ones code free.  A scan of one component covers the
component's own ceil(w_c / 8) x ceil(h_c / 8) blocks, so what the baseline file held in the MCU padding beyond them is not carried over;
no pixel depends on it.  The script is written as given: one that a decoder must refuse is written all the same."""
import numpy as np

import jpeg_dec_ref
from jpeg_ref import ZIGZAG

def script_default(nc):
    """libjpeg's default script (jcparam.c jpeg_simple_progression): what Pillow writes."""
    if nc == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
            ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def script_spectral(nc):
    """(a) spectral selection only."""
    all_c = tuple(range(nc))
    return [(all_c, 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for a, b in ((1, 5), (6, 63)) for c in range(nc)]


def script_narrow(nc):
    """(b) narrow bands: AC 1-1, 2-9, 10-63."""
    all_c = tuple(range(nc))
    return [(all_c, 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in range(nc) for a, b in ((1, 1), (2, 9), (10, 63))]


def script_deep(nc):
    """(c) Al = 3 refined one bit per scan down to 0, the DC refinements interleaved."""
    all_c = tuple(range(nc))
    out = [(all_c, 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in range(nc)]
    for al in (2, 1, 0):
        out += [(all_c, 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in range(nc)]
    return out


def script_dc_each(nc):
    """(d) DC scans one component at a time, first and refinement."""
    return ([((c,), 0, 0, 0, 1) for c in range(nc)] + [((c,), 1, 63, 0, 0) for c in range(nc)] + [((c,), 0, 0, 1, 0) for c in reversed(range(nc))])


SCRIPTS = {'default': script_default, 'spectral': script_spectral, 'narrow': script_narrow, 'deep': script_deep, 'dc_each': script_dc_each}


def _category(v):
    return int(v).bit_length()


def _scan_blocks(h, comps):
    """The scan's units, each a list of (component, block index into the coefficient array)."""
    mx, my, bpm = h['mcus_x'], h['mcus_y'], h['blocks_per_mcu']
    base = np.cumsum([0] + [c[1] * c[2] for c in h['comps']]).tolist()
    if len(comps) > 1:
        return [[(c, m * bpm + base[c] + k) for c in comps for k in range(h['comps'][c][1] * h['comps'][c][2])] for m in range(mx * my)]
    c = comps[0]
    _, hs, vs, _ = h['comps'][c]
    bw = -(-(-(-h['width'] * hs // h['hmax'])) // 8)
    bh = -(-(-(-h['height'] * vs // h['vmax'])) // 8)
    return [[(c, ((by // vs) * mx + bx // hs) * bpm + base[c] + (by % vs) * hs + bx % hs)] for by in range(bh) for bx in range(bw)]


class _Tokens:
    """One restart interval's symbols and raw bits, in order, with jcphuff.c's EOB-run state."""

    def __init__(self, eob_cap):
        self.out, self.eobrun, self.be, self.cap = [], 0, [], eob_cap

    def sym(self, cls, s):
        self.out.append((cls, s))

    def bits(self, v, n):
        if n:
            self.out.append((2, int(v) & ((1 << n) - 1), n))

    def flush_eobrun(self):
        if self.eobrun:
            n = self.eobrun.bit_length() - 1
            self.sym(1, n << 4)
            self.bits(self.eobrun, n)
            self.eobrun = 0
            for b in self.be:
                self.bits(b, 1)
            self.be = []


def _encode_unit(t, coef, blocks, ss, se, ah, al, last_dc):
    zz = ZIGZAG.tolist()
    for c, bi in blocks:
        blk = coef[bi]
        if ss == 0 and ah == 0:
            v = int(blk[0]) >> al
            diff = v - last_dc[c]
            last_dc[c] = v
            n = _category(abs(diff))
            t.sym(0, n)
            t.bits(diff if diff >= 0 else diff - 1, n)
        elif ss == 0:
            t.bits((int(blk[0]) >> al) & 1, 1)
        elif ah == 0:
            r = 0
            for k in range(ss, se + 1):
                v = int(blk[zz[k]])
                a = abs(v) >> al
                if a == 0:
                    r += 1
                    continue
                t.flush_eobrun()
                while r > 15:
                    t.sym(1, 0xF0)
                    r -= 16
                n = _category(a)
                t.sym(1, (r << 4) + n)
                t.bits(a if v >= 0 else ~a, n)
                r = 0
            if r > 0:
                t.eobrun += 1
                if t.eobrun == t.cap:
                    t.flush_eobrun()
        else:
            absv = [abs(int(blk[zz[k]])) >> al for k in range(ss, se + 1)]
            eob = max([k for k, a in zip(range(ss, se + 1), absv) if a == 1], default=0)
            r, br = 0, []
            for k, a in zip(range(ss, se + 1), absv):
                if a == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    t.flush_eobrun()
                    t.sym(1, 0xF0)
                    r -= 16
                    for b in br:
                        t.bits(b, 1)
                    br = []
                if a > 1:
                    br.append(a & 1)
                    continue
                t.flush_eobrun()
                t.sym(1, (r << 4) + 1)
                t.bits(0 if int(blk[zz[k]]) < 0 else 1, 1)
                for b in br:
                    t.bits(b, 1)
                br, r = [], 0
            if r > 0 or br:
                t.eobrun += 1
                t.be += br
                if t.eobrun == t.cap or len(t.be) > 937:          # jcphuff.c: MAX_CORR_BITS - DCTSIZE2 + 1
                    t.flush_eobrun()


def _table(symbols):
    """-> (bits[16], vals, {symbol: (code, length)}): every symbol at one length, the all-ones code left free."""
    vals = sorted(symbols)
    L = max(1, len(vals).bit_length())
    bits = [0] * 16
    bits[L - 1] = len(vals)
    return bits, vals, {s: (i, L) for i, s in enumerate(vals)}


def _dht(cls, slot, bits, vals):
    body = bytes([cls << 4 | slot]) + bytes(bits) + bytes(vals)
    return b'\xff\xc4' + (2 + len(body)).to_bytes(2, 'big') + body


def _pack(tokens, codes):
    acc, n, out = 0, 0, bytearray()
    for t in tokens:
        if t[0] == 2:
            v, k = t[1], t[2]
        else:
            v, k = codes[t[0]][t[1]]
        acc, n = (acc << k) | v, n + k
        while n >= 8:
            n -= 8
            byte = (acc >> n) & 255
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        acc &= (1 << n) - 1
    if n:
        byte = ((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 255
        out.append(byte)
        if byte == 0xFF:
            out.append(0)
    return bytes(out)


def write(baseline_file, script, eob_cap=0x7FFF, tables='scan'):
    d = bytes(baseline_file)
    h = jpeg_dec_ref.parse(d)
    coef = jpeg_dec_ref.coefficients(d)
    out = bytearray(b'\xff\xd8')
    for tq, q in sorted(h['quant'].items()):
        out += b'\xff\xdb\x00\x43' + bytes([tq]) + bytes(q[ZIGZAG].astype(np.uint8).tolist())
    nc = h['ncomp']
    out += b'\xff\xc2' + (8 + 3 * nc).to_bytes(2, 'big') + b'\x08' + h['height'].to_bytes(2, 'big') + h['width'].to_bytes(2, 'big') + bytes([nc])
    for (cid, hs, vs, tq) in h['comps']:
        out += bytes([cid, hs << 4 | vs, tq])
    dri = 0
    scans = []
    for sc in script:
        comps, ss, se, ah, al = sc[:5]
        ri = sc[5] if len(sc) > 5 else 0
        units = _scan_blocks(h, comps)
        step = ri or len(units)
        intervals = []
        for u0 in range(0, len(units), step):
            t = _Tokens(eob_cap)
            last_dc = [0] * nc
            for blocks in units[u0:u0 + step]:
                _encode_unit(t, coef, blocks, ss, se, ah, al, last_dc)
            t.flush_eobrun()
            intervals.append(t.out)
        used = [set(), set()]
        for iv in intervals:
            for t in iv:
                if t[0] != 2:
                    used[t[0]].add(t[1])
        scans.append((sc, intervals, used))
    shared = [{}, {}]
    if tables == 'shared':
        for cls in (0, 1):
            every = set().union(*[used[cls] for _, _, used in scans])
            if every:
                bits, vals, shared[cls] = _table(every)
                out += _dht(cls, 0, bits, vals)
    for sc, intervals, used in scans:
        comps, ss, se, ah, al = sc[:5]
        ri = sc[5] if len(sc) > 5 else 0
        codes = shared
        slot = 0 if tables == 'shared' else len(out) % 4            # any of the four slots: the decoder goes by what stands in front of the scan
        for cls in (0, 1):
            if used[cls] and tables != 'shared':
                codes = list(codes)
                bits, vals, codes[cls] = _table(used[cls])
                out += _dht(cls, slot, bits, vals)
        if ri != dri:
            out += b'\xff\xdd\x00\x04' + ri.to_bytes(2, 'big')
            dri = ri
        out += b'\xff\xda' + (6 + 2 * len(comps)).to_bytes(2, 'big') + bytes([len(comps)])
        for c in comps:
            out += bytes([h['comps'][c][0], slot << 4 | slot])
        out += bytes([ss, se, ah << 4 | al])
        for k, iv in enumerate(intervals):
            if k:
                out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
            out += _pack(iv, codes)
    out += b'\xff\xd9'
    return bytes(out)
