// The statements of the baseline JPEG decoder that run on the card, as __host__ __device__ code: the bit reader, the Huffman decoder,
// one restart interval's MCUs, and jidctint.c's accurate-integer IDCT.  csrc/jpeg_dec.hip runs them in its kernels;
// scripts/jpeg_decode_check.cpp runs the same statements on the host under the address and undefined-behaviour sanitizers, over
// truncated and damaged files, before the card sees any.  The progressive scans' statements (jdphuff.c) stand at the end, with their own
// bounds; scripts/jpeg_prog_check.cpp runs those.
//
// The bounds are part of the design:
//   - the bit reader never reads at or beyond the interval's end: it yields zero bits there and counts them (`phantom`);
//   - the coefficient index is checked against 63 before every store, and every store lands in the block being decoded;
//   - a code that is not in the table ends the interval;
//   - the MCU loop runs the interval's MCU count, the block loop the MCU's block count, and every pass of the coefficient loop advances
//     the index: no input can make a lane loop without end.
// Arithmetic is 32-bit; what can wrap on hostile coefficients is computed in uint32_t.
#pragma once
#include <cstdint>
#include "jpeg_dec_plan.h"                     // JPD_HD; the scales and jpd_plane, which the call plan needs as well

struct JpdBits {
    const uint8_t *p;
    uint32_t pos, end;       // next byte, one past the interval's last
    uint64_t acc;            // the low n bits are unread
    int n, phantom;          // phantom: how many of them were made up past the end (they are the lowest)
};

JPD_HD void jpd_bits_open(JpdBits &b, const uint8_t *p, uint32_t start, uint32_t end) {
    b.p = p, b.pos = start < end ? start : end, b.end = end, b.acc = 0, b.n = 0, b.phantom = 0;
}

// At least 33 unread bits afterwards.  A 0xFF followed by 0x00 is a stuffed 0xFF; followed by anything else, or by the end, it is a
// marker, and the interval's data ends in front of it.  Four bytes that lie inside the interval and hold no 0xFF are taken in one load
// (a lane's time is the latency of its dependent loads); everything else goes byte by byte.
JPD_HD void jpd_bits_fill(JpdBits &b) {
    while (b.n <= 32) {
        if (b.pos + 4 <= b.end && b.pos + 4 > b.pos) {
            uint32_t w;
            __builtin_memcpy(&w, b.p + b.pos, 4);
            w = __builtin_bswap32(w);
            if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {          // no byte of w is 0xFF
                b.acc = (b.acc << 32) | w;
                b.n += 32;
                b.pos += 4;
                continue;
            }
        }
        uint32_t v = 0;
        if (b.pos < b.end) {
            v = b.p[b.pos];
            if (v == 0xFF) {
                if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) b.pos += 2;
                else {
                    b.pos = b.end;
                    v = 0;
                    b.phantom += 8;
                }
            } else
                ++b.pos;
        } else
            b.phantom += 8;
        b.acc = (b.acc << 8) | v;
        b.n += 8;
    }
}

JPD_HD uint32_t jpd_peek16(const JpdBits &b) { return (uint32_t)(b.acc >> (b.n - 16)) & 0xFFFFu; }          // n >= 16

JPD_HD uint32_t jpd_take(JpdBits &b, int s) {                                                     // 1 <= s <= 16 <= n
    b.n -= s;
    return (uint32_t)(b.acc >> b.n) & ((1u << s) - 1);
}

// The next symbol, or -1 for a code the table does not hold.
JPD_HD int jpd_symbol(JpdBits &b, const dd_jpeg_huff &h) {
    if (b.n < 16) jpd_bits_fill(b);
    const uint32_t w = jpd_peek16(b);
    const uint32_t e = h.look[w >> 8];
    if (e) {
        b.n -= (int)(e >> 8);
        return (int)(e & 255);
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(w >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int k = h.valoff[l] + code;
            if (k < 0 || k >= h.nvals) return -1;
            b.n -= l;
            return h.vals[k];
        }
    }
    return -1;
}

// A coefficient of category s (1 .. 15) from its s bits (Annex F's EXTEND).
JPD_HD int jpd_extend(JpdBits &b, int s) {
    if (b.n < 16) jpd_bits_fill(b);
    const uint32_t v = jpd_take(b, s);
    return v < (1u << (s - 1)) ? (int)v - (int)((1u << s) - 1) : (int)v;
}

// The MCUs [mcu0, mcu0 + n_mcu) of one restart interval, whose bytes are scan[start .. end): quantised coefficients, natural order, into
// coef[(mcu * blocks_per_mcu + k) * 64 ..], which the caller has zeroed.  Returns DD_JPEG_ST_OK or DD_JPEG_ST_DATA.
JPD_HD int jpd_decode_interval(const dd_jpeg_info &r, const uint8_t *scan, uint32_t start, uint32_t end, int mcu0, int n_mcu, int16_t *coef) {
    JpdBits b;
    jpd_bits_open(b, scan, start, end);
    uint32_t pred[3] = {0, 0, 0};
    const int bpm = r.blocks_per_mcu, ny = bpm == 1 ? 1 : bpm - 2;
    for (int m = 0; m < n_mcu; ++m) {
        for (int k = 0; k < bpm; ++k) {
            const int c = k < ny ? 0 : k - ny + 1;
            int16_t *blk = coef + ((size_t)(mcu0 + m) * bpm + k) * 64;
            const int s = jpd_symbol(b, r.huff[r.td[c] & 1]);
            if (s < 0 || s > 11) return DD_JPEG_ST_DATA;
            if (s) pred[c] += (uint32_t)jpd_extend(b, s);
            blk[0] = (int16_t)(uint16_t)pred[c];
            const dd_jpeg_huff &ac = r.huff[2 + (r.ta[c] & 1)];
            for (int j = 1; j < 64; ++j) {
                const int rs = jpd_symbol(b, ac);
                if (rs < 0) return DD_JPEG_ST_DATA;
                const int run = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    if (run != 15) break;
                    j += 15;
                    continue;
                }
                j += run;
                const int v = jpd_extend(b, sz);
                if (j > 63) return DD_JPEG_ST_DATA;
                blk[JPD_ZIGZAG[j]] = (int16_t)v;
            }
            if (b.n < b.phantom) return DD_JPEG_ST_DATA;          // bits were taken from beyond the interval's end
        }
    }
    // what is left must be the padding of the last byte, and behind it a marker or the end
    if (b.n - b.phantom >= 8) return DD_JPEG_ST_DATA;
    if (b.pos < b.end && !(b.p[b.pos] == 0xFF && (b.pos + 1 >= b.end || b.p[b.pos + 1] != 0))) return DD_JPEG_ST_DATA;
    return DD_JPEG_ST_OK;
}

// ---- one entropy-coded segment decoded by several lanes (DD_JPEGDEC_SPLIT; jpeg_split_entropy_k and scripts/jpeg_split_check.cpp run these
// statements).  The segment's bytes are cut into subsequences of 1 << log2b bytes; subsequence i owns the symbols (a Huffman code with its
// extra bits) whose first bit lies in bytes [i << log2b, (i + 1) << log2b).  A lane decodes its subsequence from a start state -- a guess
// at first, its predecessor's end state later -- and the rounds repeat until no end state changes: Huffman data falls into step by itself.
// The bounds, beside the bit reader's:
//   - a span's loop takes one symbol per pass and ends at the first symbol boundary at or behind its limit, which is at most the data's end;
//   - a block index at or above the frame's block count is never stored;
//   - a speculative decode (JPD_SPAN_COUNT) stores no coefficient at all.

// Where a decode stands: the first unread bit is bit `bit` (0: the most significant) of the data byte at `pos` of the stuffed stream (the
// 0xFF of a stuffed pair, never its 0x00), in block k of the MCU, before coefficient j (0: the block's DC symbol comes next).
struct JpdState {
    uint32_t pos;
    uint32_t kj;             // bit | k << 3 | j << 8, or JPD_STATE_UNKNOWN: the decode that should have led here met an error
};
constexpr uint32_t JPD_STATE_UNKNOWN = 0xFFFFFFFFu;
constexpr int JPD_SPAN_COUNT = 0, JPD_SPAN_WRITE = 1;

JPD_HD bool jpd_state_eq(const JpdState &a, const JpdState &b) { return a.pos == b.pos && a.kj == b.kj; }

// Where the entropy-coded data of scan[0 .. len) ends for jpd_bits_fill: at the first 0xFF that no 0x00 follows, else at len.  In front of
// that every 0xFF starts a stuffed pair.  (A lane of jpeg_split_entropy_k asks this of its own bytes; the least answer is the segment's.)
JPD_HD bool jpd_marker_at(const uint8_t *scan, uint32_t p, uint32_t len) { return scan[p] == 0xFF && !(p + 1 < len && scan[p + 1] == 0); }

// The first data byte at or behind p (p >= 1 or p == 0): p itself unless it is the 0x00 of a stuffed pair.
JPD_HD uint32_t jpd_data_byte(const uint8_t *scan, uint32_t p, uint32_t end) { return p > 0 && p < end && scan[p] == 0 && scan[p - 1] == 0xFF ? p + 1 : p; }

// The guess subsequence i starts from: its first byte, bit 0, the DC symbol of an MCU's first block.
JPD_HD JpdState jpd_span_guess(const uint8_t *scan, uint32_t i, int log2b, uint32_t end) {
    JpdState s;
    s.pos = jpd_data_byte(scan, i << log2b, end), s.kj = 0;
    return s;
}

// JpdBits with a limit: `over` counts how many of the unread bits came from bytes at or behind `lim` (they are the lowest; phantom bits are
// among them), so the next unread bit lies in front of lim exactly when b.n > over.  lim <= b.end.
struct JpdSpanBits {
    JpdBits b;
    uint32_t lim;
    int over;
};

// jpd_bits_fill, keeping `over`: at least 33 unread bits afterwards, so that jpd_symbol and jpd_extend behind it never fill themselves.
JPD_HD void jpd_span_fill(JpdSpanBits &s) {
    JpdBits &b = s.b;
    while (b.n <= 32) {
        if (b.pos + 4 <= b.end && b.pos + 4 > b.pos) {
            uint32_t w;
            __builtin_memcpy(&w, b.p + b.pos, 4);
            w = __builtin_bswap32(w);
            if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {          // no byte of w is 0xFF
                const uint32_t front = b.pos >= s.lim ? 0u : s.lim - b.pos >= 4u ? 4u : s.lim - b.pos;
                b.acc = (b.acc << 32) | w;
                b.n += 32;
                s.over += 8 * (4 - (int)front);
                b.pos += 4;
                continue;
            }
        }
        uint32_t v = 0;
        const bool behind = b.pos >= s.lim;
        if (b.pos < b.end) {
            v = b.p[b.pos];
            if (v == 0xFF) {
                if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) b.pos += 2;
                else {
                    b.pos = b.end;
                    v = 0;
                    b.phantom += 8;
                }
            } else
                ++b.pos;
        } else
            b.phantom += 8;
        b.acc = (b.acc << 8) | v;
        b.n += 8;
        if (behind) s.over += 8;
    }
}

// What one decode of a subsequence found (JPD_SPAN_COUNT): how many blocks begin in it, and the wrap-around sum of the DC differences it
// holds per component -- associative, and what jpd_decode_interval's (int16_t)(uint16_t)pred keeps of its 32-bit predictor.
struct JpdSpanSums {
    uint32_t blocks;
    uint16_t dc[3];
};

// Decodes from state `st` to the first symbol boundary at or behind byte `lim` (lim <= end, the data's end as jpd_marker_at gives it) and
// leaves that state in st; JPD_STATE_UNKNOWN after a code the table does not hold, a DC category above 11 or a coefficient behind 63.
//   JPD_SPAN_COUNT  fills `sums`, also in front of an error; stores nothing.
//   JPD_SPAN_WRITE  the caller knows the truth: `blk` is the index of the first block that begins here (a block under way at st is
//                   blk - 1), pred the DC predictors in front of it, n_blocks the frame's block count.  Stores into coef, which the caller
//                   has zeroed, what jpd_decode_interval stores.  Returns true when block n_blocks - 1 ends here and what is left behind it
//                   is the padding of the last byte -- jpd_decode_interval's DD_JPEG_ST_OK -- and stops there; nothing is stored at or
//                   behind block n_blocks.
// The statements are jpd_decode_interval's, one symbol per pass: ZRL adds 16, a run is checked against 63 only where a coefficient follows,
// a block without EOB ends at j = 64.
JPD_HD bool jpd_decode_span(const dd_jpeg_info &r, const dd_jpeg_huff *huff, const uint8_t *scan, uint32_t end, uint32_t lim, JpdState &st, const int mode, JpdSpanSums &sums,
                            int16_t *coef, uint32_t blk, uint32_t n_blocks, const uint32_t *pred) {
    sums.blocks = 0, sums.dc[0] = sums.dc[1] = sums.dc[2] = 0;
    if (st.kj == JPD_STATE_UNKNOWN || st.pos >= lim) return false;          // nothing of this subsequence is left: the state passes through
    const int bpm = r.blocks_per_mcu, ny = bpm == 1 ? 1 : bpm - 2;
    int k = (int)((st.kj >> 3) & 31), j = (int)(st.kj >> 8);
    if (k >= bpm || j > 63) return false;
    const uint32_t tsel = (uint32_t)(r.td[0] & 1) | (uint32_t)(r.ta[0] & 1) << 1 | (uint32_t)(r.td[1] & 1) << 2 | (uint32_t)(r.ta[1] & 1) << 3 | (uint32_t)(r.td[2] & 1) << 4 |
                          (uint32_t)(r.ta[2] & 1) << 5;                      // the record is read here, not once a symbol
    JpdSpanBits s;
    jpd_bits_open(s.b, scan, st.pos, end);
    s.lim = lim, s.over = 0;
    jpd_span_fill(s);
    s.b.n -= (int)(st.kj & 7);
    JpdBits &b = s.b;
    // per component: the DC predictor (JPD_SPAN_WRITE) or the sum of the differences met (JPD_SPAN_COUNT), in scalars, not in an indexed array
    uint32_t a0 = 0, a1 = 0, a2 = 0, begun = 0;
    if (mode == JPD_SPAN_WRITE) a0 = pred[0], a1 = pred[1], a2 = pred[2];
    int16_t *cur = nullptr;                                                 // the block under way, where it may be stored
    if (mode == JPD_SPAN_WRITE && j > 0 && blk >= 1 && blk - 1 < n_blocks) cur = coef + (size_t)(blk - 1) * 64;
    bool known = true, done = false;
    for (;;) {
        jpd_span_fill(s);
        if (b.n <= s.over) break;                                           // the next symbol belongs to the subsequence behind
        const int c = k < ny ? 0 : k - ny + 1;
        if (j == 0) {
            if (mode == JPD_SPAN_WRITE && blk >= n_blocks) {                // surplus bits: jpd_decode_interval has stopped in front of them
                known = false;
                break;
            }
            const int sy = jpd_symbol(b, huff[(tsel >> (2 * c)) & 1]);
            if (sy < 0 || sy > 11) {
                known = false;
                break;
            }
            const uint32_t diff = sy ? (uint32_t)jpd_extend(b, sy) : 0u;
            const uint32_t a = (c == 0 ? a0 : c == 1 ? a1 : a2) + diff;
            if (c == 0) a0 = a;
            else if (c == 1) a1 = a;
            else a2 = a;
            if (mode == JPD_SPAN_WRITE) {
                cur = coef + (size_t)blk * 64;
                cur[0] = (int16_t)(uint16_t)a;
                ++blk;
            } else
                ++begun;
            j = 1;
        } else {
            const int rs = jpd_symbol(b, huff[2 + ((tsel >> (2 * c + 1)) & 1)]);
            if (rs < 0) {
                known = false;
                break;
            }
            const int run = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                j = run != 15 ? 64 : j + 16;
            } else {
                j += run;
                const int v = jpd_extend(b, sz);
                if (j > 63) {
                    known = false;
                    break;
                }
                if (mode == JPD_SPAN_WRITE && cur) cur[JPD_ZIGZAG[j]] = (int16_t)v;
                ++j;
            }
        }
        if (j >= 64) {                                                      // the block ends
            if (mode == JPD_SPAN_WRITE && blk == n_blocks) {                // it was the frame's last: jpd_decode_interval's closing tests
                known = false;
                // bits from beyond the end; more than the last byte's padding; data bytes not yet taken (in front of `end` there is no marker)
                done = !(b.n < b.phantom) && !(b.n - b.phantom >= 8) && !(b.pos < b.end);
                break;
            }
            j = 0;
            if (++k == bpm) k = 0;
        }
    }
    if (mode == JPD_SPAN_COUNT) sums.blocks = begun, sums.dc[0] = (uint16_t)a0, sums.dc[1] = (uint16_t)a1, sums.dc[2] = (uint16_t)a2;
    if (!known) {
        st.kj = JPD_STATE_UNKNOWN;
        return done;
    }
    // the cursor: over - n bits behind the first data byte at or behind lim
    uint32_t q = jpd_data_byte(scan, lim, end);
    int behind = s.over - b.n;
    for (; behind >= 8 && q < end; behind -= 8) q += scan[q] == 0xFF ? 2 : 1;
    if (q >= end) q = end, behind = 0;                                      // past the data: no subsequence starts there
    st.pos = q, st.kj = (uint32_t)behind | ((uint32_t)k << 3) | ((uint32_t)j << 8);
    return false;
}

// The RSTn marker (0 .. 7) at scan[p], p + 1 < len, or -1.
JPD_HD int jpd_rst_at(const uint8_t *scan, uint32_t p) { return scan[p] == 0xFF && scan[p + 1] >= 0xD0 && scan[p + 1] <= 0xD7 ? scan[p + 1] - 0xD0 : -1; }

// ---- jidctint.c (jpeg_idct_islow): 13-bit constants, the column pass descaled by 11, the row pass by 18.

JPD_HD int32_t jpd_sar(uint32_t x, int n) { return (int32_t)x >> n; }

template <int S, int SHIFT>
JPD_HD void jpd_idct8(int32_t *d) {
    typedef uint32_t U;
    const U c0 = (U)d[0], c1 = (U)d[S], c2 = (U)d[2 * S], c3 = (U)d[3 * S], c4 = (U)d[4 * S], c5 = (U)d[5 * S], c6 = (U)d[6 * S], c7 = (U)d[7 * S];
    U z1 = (c2 + c6) * 4433u;
    const U t2 = z1 - c6 * 15137u, t3 = z1 + c2 * 6270u;
    const U t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    U a0 = c7, a1 = c5, a2 = c3, a3 = c1;
    z1 = a0 + a3;
    U z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const U z5 = (z3 + z4) * 9633u;
    a0 *= 2446u, a1 *= 16819u, a2 *= 25172u, a3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995;
    z3 = z3 * (U)-16069 + z5;
    z4 = z4 * (U)-3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    const U r = 1u << (SHIFT - 1);
    d[0] = jpd_sar(t10 + a3 + r, SHIFT), d[7 * S] = jpd_sar(t10 - a3 + r, SHIFT);
    d[S] = jpd_sar(t11 + a2 + r, SHIFT), d[6 * S] = jpd_sar(t11 - a2 + r, SHIFT);
    d[2 * S] = jpd_sar(t12 + a1 + r, SHIFT), d[5 * S] = jpd_sar(t12 - a1 + r, SHIFT);
    d[3 * S] = jpd_sar(t13 + a0 + r, SHIFT), d[4 * S] = jpd_sar(t13 - a0 + r, SHIFT);
}

// libjpeg's range-limit table behind the IDCT, addressed through & 1023: the sample + 128, clamped, with the table's wrap.
JPD_HD int jpd_range_limit(int32_t v) {
    const int i = v & 1023;
    return i < 128 ? 128 + i : i < 512 ? 255 : i < 896 ? 0 : i - 896;
}

// 64 dequantised coefficients (natural order) in d -> 64 samples 0 .. 255 in d.
JPD_HD void jpd_idct(int32_t (&d)[64]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) jpd_idct8<8, 11>(&d[c]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; ++r) jpd_idct8<1, 18>(&d[8 * r]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; ++i) d[i] = jpd_range_limit(d[i]);
}

// jdcolor.c: YCbCr -> B, G, R with FIX(x) = int(x * 65536 + 0.5), packed B | G << 8 | R << 16.
JPD_HD uint32_t jpd_bgr(int y, int cb, int cr) {
    cb -= 128, cr -= 128;
    int r = y + ((91881 * cr + 32768) >> 16);
    int b = y + ((116130 * cb + 32768) >> 16);
    int g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    r = r < 0 ? 0 : r > 255 ? 255 : r;
    g = g < 0 ? 0 : g > 255 ? 255 : g;
    b = b < 0 ? 0 : b > 255 ? 255 : b;
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}

// ---- decoding at 1/2, 1/4 and 1/8 scale: jpd_scale_ok and jpd_plane (csrc/jpeg_dec_plan.h) say what n x n samples a block becomes; these are
// the transforms.

// jidctred.c (CONST_BITS 13, PASS1_BITS 2).  The column pass is exact in 64 bits for every int16 coefficient times an 8-bit quantiser, so
// what it hands to the row pass fits 32 bits; the row pass wraps like jpd_idct8, which the range limit's & 1023 does not see.

// jpeg_idct_4x4: terms 0, 1, 2, 3, 5, 6, 7 of rows and columns; term 4 is not read.  Descaled by 12, then by 19.
JPD_HD void jpd_idct4(const int32_t (&d)[64], int (&o)[16]) {
    typedef int64_t L;
    typedef uint32_t U;
    int32_t ws[4][8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) {
        if (c == 4) continue;
        const L t0 = (L)d[c] * 16384, t2 = (L)d[16 + c] * 15137 - (L)d[48 + c] * 6270;
        const L z1 = d[56 + c], z2 = d[40 + c], z3 = d[24 + c], z4 = d[8 + c];
        const L o0 = z2 * 11893 + z4 * 8697 - z1 * 1730 - z3 * 17799;
        const L o2 = z3 * 7373 + z4 * 20995 - z1 * 4176 - z2 * 4926;
        ws[0][c] = (int32_t)((t0 + t2 + o2 + 2048) >> 12), ws[3][c] = (int32_t)((t0 + t2 - o2 + 2048) >> 12);
        ws[1][c] = (int32_t)((t0 - t2 + o0 + 2048) >> 12), ws[2][c] = (int32_t)((t0 - t2 - o0 + 2048) >> 12);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 4; ++r) {
        const U t0 = (U)ws[r][0] << 14, t2 = (U)ws[r][2] * 15137u - (U)ws[r][6] * 6270u;
        const U z1 = (U)ws[r][7], z2 = (U)ws[r][5], z3 = (U)ws[r][3], z4 = (U)ws[r][1];
        const U o0 = z2 * 11893u + z4 * 8697u - z1 * 1730u - z3 * 17799u;
        const U o2 = z3 * 7373u + z4 * 20995u - z1 * 4176u - z2 * 4926u;
        const U k = 1u << 18;
        o[4 * r] = jpd_range_limit(jpd_sar(t0 + t2 + o2 + k, 19)), o[4 * r + 3] = jpd_range_limit(jpd_sar(t0 + t2 - o2 + k, 19));
        o[4 * r + 1] = jpd_range_limit(jpd_sar(t0 - t2 + o0 + k, 19)), o[4 * r + 2] = jpd_range_limit(jpd_sar(t0 - t2 - o0 + k, 19));
    }
}

// jpeg_idct_2x2: terms 0, 1, 3, 5, 7.  Descaled by 13, then by 20.
JPD_HD void jpd_idct2(const int32_t (&d)[64], int (&o)[4]) {
    typedef int64_t L;
    typedef uint32_t U;
    int32_t ws[2][8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) {
        if (c != 0 && !(c & 1)) continue;
        const L t10 = (L)d[c] * 32768;
        const L t0 = (L)d[40 + c] * 6967 + (L)d[8 + c] * 29692 - (L)d[56 + c] * 5906 - (L)d[24 + c] * 10426;
        ws[0][c] = (int32_t)((t10 + t0 + 4096) >> 13), ws[1][c] = (int32_t)((t10 - t0 + 4096) >> 13);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 2; ++r) {
        const U t10 = (U)ws[r][0] << 15;
        const U t0 = (U)ws[r][5] * 6967u + (U)ws[r][1] * 29692u - (U)ws[r][7] * 5906u - (U)ws[r][3] * 10426u;
        const U k = 1u << 19;
        o[2 * r] = jpd_range_limit(jpd_sar(t10 + t0 + k, 20)), o[2 * r + 1] = jpd_range_limit(jpd_sar(t10 - t0 + k, 20));
    }
}

// jpeg_idct_1x1: the dequantised DC term, descaled by 3.
JPD_HD int jpd_idct1(int32_t dc) { return jpd_range_limit(jpd_sar((uint32_t)dc + 4u, 3)); }

// ---- progressive scans (libjpeg's jdphuff.c; tests/jpeg_prog_ref.py is the definition).  One restart interval of one scan: its units
// [unit0, unit0 + n_units) -- MCUs of the frame for a scan of several components, the component's own blocks in raster order for a scan of
// one -- from bytes[start .. end) into the frame's coefficient buffer, which keeps the baseline layout.  The bounds, beside the bit reader's:
//   - the unit loop runs n_units, the block loop the unit's block count; every pass of a coefficient loop advances k, which stops at Se <= 63;
//   - a block's address comes from the record alone (parsed and checked on the host), never from the entropy-coded bytes;
//   - an EOB run only ever counts down, once per block.
// What no valid file holds is defined all the same: a first scan stores the low 16 bits of v << Al, a DC predictor wraps at 32 bits, a
// refinement adds or subtracts 1 << Al in 16 bits, wrapping.  Shifts by Al (0 .. 13) are done in uint32_t.

JPD_HD int jpd_bit(JpdBits &b) {
    if (b.n < 16) jpd_bits_fill(b);
    return (int)jpd_take(b, 1);
}

// An EOBn symbol's run: 2^r blocks and r more bits, 1 .. 32767.
JPD_HD int jpd_eobrun(JpdBits &b, int r) {
    int run = 1 << r;
    if (r) {
        if (b.n < 16) jpd_bits_fill(b);
        run += (int)jpd_take(b, r);
    }
    return run;
}

// A coefficient that is already non-zero, passed over by an AC refinement scan: one correction bit, and the coefficient is only read
// when that bit is set.
JPD_HD void jpd_refine_nonzero(JpdBits &b, int16_t *at, int p1) {
    if (!jpd_bit(b)) return;
    const int v = *at;
    if (!(v & p1)) *at = (int16_t)(uint16_t)((uint32_t)v + (uint32_t)(v >= 0 ? p1 : -p1));
}

// Bit k: the block's coefficient at zigzag index k (1 .. 63) is non-zero.  An AC refinement scan asks this of every coefficient it passes;
// 63 loads that do not depend on each other, in front of the block's serial walk, in place of one dependent load per coefficient.
JPD_HD uint64_t jpd_nonzero_mask(const int16_t *blk) {
    uint64_t nz = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < 64; ++k) nz |= (uint64_t)(blk[JPD_ZIGZAG[k]] != 0) << k;
    return nz;
}

// One block of the scan.  dc, ac: the tables the scan kind reads (the others may be NULL).  Returns DD_JPEG_ST_OK or DD_JPEG_ST_DATA.
JPD_HD int jpd_prog_block(JpdBits &b, int ss, int se, int ah, int al, const dd_jpeg_huff *dc, const dd_jpeg_huff *ac, int16_t *blk, uint32_t &pred, int &eobrun) {
    const int p1 = 1 << al;
    if (ss == 0) {
        if (ah == 0) {                                                      // DC, first scan
            const int s = jpd_symbol(b, *dc);
            if (s < 0 || s > 11) return DD_JPEG_ST_DATA;
            if (s) pred += (uint32_t)jpd_extend(b, s);
            blk[0] = (int16_t)(uint16_t)(pred << al);
        } else if (jpd_bit(b))                                              // DC, refinement
            blk[0] = (int16_t)((uint16_t)blk[0] | (uint16_t)p1);
        return DD_JPEG_ST_OK;
    }
    if (ah == 0) {                                                          // AC, first scan
        if (eobrun > 0) {
            --eobrun;
            return DD_JPEG_ST_OK;
        }
        for (int k = ss; k <= se; ++k) {
            const int rs = jpd_symbol(b, *ac);
            if (rs < 0) return DD_JPEG_ST_DATA;
            const int r = rs >> 4, s = rs & 15;
            if (s) {
                k += r;
                const uint32_t v = (uint32_t)jpd_extend(b, s);
                if (k > se) return DD_JPEG_ST_DATA;
                blk[JPD_ZIGZAG[k]] = (int16_t)(uint16_t)(v << al);
            } else if (r == 15)
                k += 15;
            else {
                eobrun = jpd_eobrun(b, r) - 1;
                break;
            }
        }
        return DD_JPEG_ST_OK;
    }
    int k = ss;                                                             // AC, refinement
    const uint64_t nz = jpd_nonzero_mask(blk);                              // as the scan found the block: what it adds it does not pass again
    if (eobrun == 0) {
        for (; k <= se; ++k) {
            const int rs = jpd_symbol(b, *ac);
            if (rs < 0) return DD_JPEG_ST_DATA;
            int r = rs >> 4, s = rs & 15;
            if (s) {
                if (s != 1) return DD_JPEG_ST_DATA;
                s = jpd_bit(b) ? p1 : -p1;                                  // the new coefficient's sign comes in front of the correction bits
            } else if (r != 15) {
                eobrun = jpd_eobrun(b, r);
                break;                                                      // the rest of this block is the run's first
            }
            for (; k <= se; ++k) {                                          // pass r coefficients that are still zero, refining the others on the way
                if ((nz >> k) & 1) jpd_refine_nonzero(b, blk + JPD_ZIGZAG[k], p1);
                else if (--r < 0) break;
            }
            if (s) {
                if (k > se) return DD_JPEG_ST_DATA;
                blk[JPD_ZIGZAG[k]] = (int16_t)(uint16_t)(uint32_t)s;                          // at the position the run lands on
            }
        }
    }
    if (eobrun > 0) {
        for (; k <= se; ++k)
            if ((nz >> k) & 1) jpd_refine_nonzero(b, blk + JPD_ZIGZAG[k], p1);
        --eobrun;
    }
    return DD_JPEG_ST_OK;
}

// Where block (bx, by) of component c lies in the MCU-interleaved coefficient buffer (chroma is sampled 1 x 1: csrc/jpeg_parse.h).
JPD_HD size_t jpd_block_at(const dd_jpeg_info &r, int c, int bx, int by) {
    const int hs = c ? 1 : r.hmax, vs = c ? 1 : r.vmax;
    const int base = c ? r.hmax * r.vmax + c - 1 : 0;
    return ((size_t)(by / vs) * r.mcus_x + bx / hs) * r.blocks_per_mcu + base + (by % vs) * hs + bx % hs;
}

JPD_HD int jpd_prog_decode_interval(const dd_jpeg_info &r, const dd_jpeg_scan &sc, const dd_jpeg_huff *pool, const uint8_t *bytes, uint32_t start, uint32_t end, int unit0,
                                    int n_units, int16_t *coef) {
    JpdBits b;
    jpd_bits_open(b, bytes, start, end);
    uint32_t pred[3] = {0, 0, 0};
    int eobrun = 0;
    const int ss = sc.ss & 63, se = sc.se & 63, ah = sc.ah & 15, al = sc.al & 15;
    if (sc.blocks_x < 1) return DD_JPEG_ST_DATA;
    const dd_jpeg_huff *ac = sc.ac >= 0 && sc.ac < DD_JPEG_MAX_TABLES ? pool + sc.ac : nullptr;
    if (ss > 0 && !ac) return DD_JPEG_ST_DATA;
    const bool mcus = sc.ncomp > 1;
    for (int u = 0; u < n_units; ++u) {
        const int ux = (unit0 + u) % sc.blocks_x, uy = (unit0 + u) / sc.blocks_x;
        for (int k = 0; k < (mcus ? sc.ncomp : 1) && k < 3; ++k) {
            const int c = sc.comp[k] >= 0 && sc.comp[k] < 3 ? sc.comp[k] : 0;
            const dd_jpeg_huff *dc = sc.dc[k] >= 0 && sc.dc[k] < DD_JPEG_MAX_TABLES ? pool + sc.dc[k] : nullptr;
            if (ss == 0 && ah == 0 && !dc) return DD_JPEG_ST_DATA;
            const int hs = mcus && c == 0 ? r.hmax : 1, vs = mcus && c == 0 ? r.vmax : 1;
            for (int y = 0; y < vs; ++y)
                for (int x = 0; x < hs; ++x) {
                    int16_t *blk = coef + jpd_block_at(r, c, ux * hs + x, uy * vs + y) * 64;
                    if (jpd_prog_block(b, ss, se, ah, al, dc, ac, blk, pred[c], eobrun) != DD_JPEG_ST_OK) return DD_JPEG_ST_DATA;
                    if (b.n < b.phantom) return DD_JPEG_ST_DATA;          // bits were taken from beyond the interval's end
                }
        }
    }
    if (eobrun) return DD_JPEG_ST_DATA;                                     // an EOB run that outlives its interval
    if (b.n - b.phantom >= 8) return DD_JPEG_ST_DATA;
    if (b.pos < b.end && !(b.p[b.pos] == 0xFF && (b.pos + 1 >= b.end || b.p[b.pos + 1] != 0))) return DD_JPEG_ST_DATA;
    return DD_JPEG_ST_OK;
}
