// The header of a baseline JPEG file, SOI .. the first SOS, into a fixed-size dd_jpeg_info (include/deepdish_hip.h).  Plain C++, no
// device, no allocation: shared by dd_jpeg_parse (csrc/jpeg_dec.hip) and the stand-alone sanitizer check
// (scripts/jpeg_decode_check.cpp).  These bytes come from a network: every read is checked against the length, the work is bounded by
// the header, and the entropy-coded bytes are not walked.  jpd_parse_scans, at the end, reads progressive (SOF2) files as well, for the
// handles that ask for them (dd_jpeg_parse_scans, scripts/jpeg_prog_check.cpp): it walks the whole file, bounded by its length.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/deepdish_hip.h"
#include "jpeg_tables.h"

constexpr int JPD_MAX_SIDE = 8192;

// natural (row-major) index of the k-th coefficient in zigzag order
static const uint8_t JPD_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define JPD_REFUSE(code, ...)                      \
    do {                                           \
        std::snprintf(msg, msgcap, __VA_ARGS__);   \
        o->reason = (code);                        \
        return (code);                             \
    } while (0)

// One DHT table at d[p .. e): Annex C's code assignment, then the kernel's look-up form.  Returns the bytes taken, or 0 after a refusal.
// The table at d[p .. e), p + 17 <= e, into *h; the class and slot byte has been read by the caller.
static inline size_t jpd_huffman_build(const uint8_t *d, size_t p, size_t e, dd_jpeg_huff *h, dd_jpeg_info *o, char *msg, size_t msgcap) {
    std::memset(h, 0, sizeof(*h));
    int count = 0;
    uint32_t code = 0;
    for (int l = 1; l <= 16; ++l) {
        const int b = d[p + l];
        h->bits[l - 1] = (uint8_t)b;
        count += b;
        code += (uint32_t)b;
        if (code > (1u << l)) {
            std::snprintf(msg, msgcap, "dd_jpeg_parse: a Huffman table over-subscribes the code space at length %d", l);
            o->reason = DD_JPEG_R_HUFFMAN;
            return 0;
        }
        code <<= 1;
    }
    if (count > 256) {
        std::snprintf(msg, msgcap, "dd_jpeg_parse: a Huffman table names %d symbols (at most 256)", count);
        o->reason = DD_JPEG_R_HUFFMAN;
        return 0;
    }
    if (p + 17 + (size_t)count > e) {
        std::snprintf(msg, msgcap, "dd_jpeg_parse: a DHT segment shorter than its %d symbols", count);
        o->reason = DD_JPEG_R_SEGMENT;
        return 0;
    }
    for (int i = 0; i < count; ++i) h->vals[i] = d[p + 17 + i];
    h->nvals = count;
    code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int b = h->bits[l - 1];
        h->valoff[l] = k - (int)code;
        for (int i = 0; i < b; ++i, ++k, ++code)
            if (l <= 8) {
                const uint32_t first = code << (8 - l), n = 1u << (8 - l);
                for (uint32_t j = 0; j < n && first + j < 256; ++j) h->look[first + j] = (uint16_t)((l << 8) | h->vals[k]);
            }
        h->maxcode[l] = b ? (int)code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = -1;
    h->defined = 1;
    return 17 + (size_t)count;
}

static inline size_t jpd_huffman(const uint8_t *d, size_t p, size_t e, dd_jpeg_info *o, char *msg, size_t msgcap) {
    if (p + 17 > e) {
        std::snprintf(msg, msgcap, "dd_jpeg_parse: a DHT segment shorter than its table");
        o->reason = DD_JPEG_R_SEGMENT;
        return 0;
    }
    const int tc = d[p] >> 4, th = d[p] & 15;
    if (tc > 1 || th > 1) {
        std::snprintf(msg, msgcap, "dd_jpeg_parse: Huffman table class %d id %d (baseline holds ids 0 and 1 of classes 0 and 1)", tc, th);
        o->reason = DD_JPEG_R_HUFFMAN;
        return 0;
    }
    return jpd_huffman_build(d, p, e, &o->huff[tc * 2 + th], o, msg, msgcap);
}

// DD_JPEGDEC_STD_TABLES: ITU-T T.81 Annex K.3's table for class tc (0 DC, 1 AC) and slot th (0 luminance, 1 chrominance) into *h, in the
// same look-up form a DHT segment gives -- what libjpeg-turbo's jstdhuff.c puts into every slot 0 / 1 a file leaves undefined (UVC cameras
// in MJPG mode and MJPG AVI frames carry no DHT at all).
static inline void jpd_huffman_std(int tc, int th, dd_jpeg_huff *h, dd_jpeg_info *o, char *msg, size_t msgcap) {
    uint8_t seg[1 + 16 + 162];
    const uint8_t *bits = tc ? (th ? JP_AC_CHROMA_BITS : JP_AC_LUMA_BITS) : (th ? JP_DC_CHROMA_BITS : JP_DC_LUMA_BITS);
    const uint8_t *vals = tc ? (th ? JP_AC_CHROMA_VALS : JP_AC_LUMA_VALS) : JP_DC_VALS;
    const size_t nv = tc ? 162 : 12;
    seg[0] = (uint8_t)(tc << 4 | th);
    std::memcpy(seg + 1, bits, 16);
    std::memcpy(seg + 17, vals, nv);
    (void)jpd_huffman_build(seg, 0, 17 + nv, h, o, msg, msgcap);
}

// Returns DD_JPEG_R_OK or the reason (also o->reason); msg gets the text.  flags: 0, or DD_JPEGDEC_STD_TABLES: at the SOS every DC / AC slot
// 0 or 1 that a component references and the file has not defined receives the Annex K.3 table of that slot; defined slots are untouched.
static inline int jpd_parse(const uint8_t *d, size_t n, dd_jpeg_info *o, char *msg, size_t msgcap, int flags = 0) {
    std::memset(o, 0, sizeof(*o));
    if (msgcap) msg[0] = 0;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) JPD_REFUSE(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated or not a JPEG file: no SOI marker in %zu bytes", n);
    bool have_sof = false;
    int adobe = -1, comp_id[3] = {0, 0, 0};
    size_t i = 2;
    for (;;) {
        if (i + 4 > n) JPD_REFUSE(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated: the file ends at byte %zu before an SOS segment", n);
        if (d[i] != 0xFF) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: no marker at offset %zu", i);
        const int m = d[i + 1];
        if (m == 0xFF) {
            ++i;
            continue;
        }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
            i += 2;
            continue;
        }
        if (m == 0xD9) JPD_REFUSE(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated: EOI at offset %zu before an SOS segment", i);
        const size_t L = ((size_t)d[i + 2] << 8) | d[i + 3];
        if (L < 2 || i + 2 + L > n) JPD_REFUSE(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated: the segment at offset %zu has a length of %zu, past the file's %zu bytes", i, L, n);
        size_t p = i + 4;
        const size_t e = i + 2 + L;
        if (m == 0xC2 || m == 0xC6) JPD_REFUSE(DD_JPEG_R_PROGRESSIVE, "dd_jpeg_parse: progressive files (SOF%d) are refused", m - 0xC0);
        if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) JPD_REFUSE(DD_JPEG_R_LOSSLESS, "dd_jpeg_parse: lossless files (SOF%d) are refused", m - 0xC0);
        if (m == 0xC5) JPD_REFUSE(DD_JPEG_R_LOSSLESS, "dd_jpeg_parse: hierarchical files (SOF5) are refused");
        if (m == 0xC9 || m == 0xCA || m == 0xCC || m == 0xCD || m == 0xCE) JPD_REFUSE(DD_JPEG_R_ARITHMETIC, "dd_jpeg_parse: arithmetic coding (marker 0x%02X) is refused", m);
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a second SOF segment");
            if (L < 8) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOF segment of %zu bytes", L);
            if (d[p] != 8) JPD_REFUSE(DD_JPEG_R_PRECISION, "dd_jpeg_parse: %d-bit precision is refused (8 only)", d[p]);
            const int H = (d[p + 1] << 8) | d[p + 2], W = (d[p + 3] << 8) | d[p + 4], nc = d[p + 5];
            if (H < 1 || W < 1 || H > JPD_MAX_SIDE || W > JPD_MAX_SIDE) JPD_REFUSE(DD_JPEG_R_SIZE, "dd_jpeg_parse: size %d x %d (1 .. %d either way)", W, H, JPD_MAX_SIDE);
            if (nc != 1 && nc != 3) JPD_REFUSE(DD_JPEG_R_COMPONENTS, "dd_jpeg_parse: %d components are refused (1 or 3)", nc);
            if (L != 8 + 3 * (size_t)nc) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOF segment of %zu bytes for %d components", L, nc);
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = d[p + 6 + 3 * c];
                o->hs[c] = d[p + 7 + 3 * c] >> 4;
                o->vs[c] = d[p + 7 + 3 * c] & 15;
                o->tq[c] = d[p + 8 + 3 * c];
                if (o->tq[c] > 3) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: component %d names quant table %d (0 .. 3)", c, o->tq[c]);
            }
            if (nc == 1) o->hs[0] = o->vs[0] = 1;           // a lone component's factors only scale the MCU: libjpeg ignores them
            else {
                const bool luma = o->vs[0] >= 1 && o->vs[0] <= 2 && o->hs[0] >= o->vs[0] && o->hs[0] <= 2;
                if (!luma || o->hs[1] != 1 || o->vs[1] != 1 || o->hs[2] != 1 || o->vs[2] != 1)
                    JPD_REFUSE(DD_JPEG_R_SAMPLING, "dd_jpeg_parse: sampling %dx%d, %dx%d, %dx%d is refused (4:4:4, 4:2:2 and 4:2:0 only)", o->hs[0], o->vs[0], o->hs[1],
                               o->vs[1], o->hs[2], o->vs[2]);
            }
            o->height = H, o->width = W, o->ncomp = nc, o->sof = m;
            have_sof = true;
        } else if (m == 0xDB) {
            while (p < e) {
                if (d[p] >> 4) JPD_REFUSE(DD_JPEG_R_PRECISION, "dd_jpeg_parse: 16-bit quant tables are refused (precision field %d)", d[p] >> 4);
                const int tq = d[p] & 15;
                if (tq > 3 || p + 65 > e) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a DQT segment with table id %d and %zu bytes left", tq, e - p);
                for (int k = 0; k < 64; ++k) o->quant[tq][JPD_ZIGZAG[k]] = d[p + 1 + k];
                o->quant_defined[tq] = 1;
                p += 65;
            }
        } else if (m == 0xC4) {
            while (p < e) {
                const size_t took = jpd_huffman(d, p, e, o, msg, msgcap);
                if (!took) return o->reason;
                p += took;
            }
        } else if (m == 0xDD) {
            if (L != 4) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a DRI segment of %zu bytes", L);
            o->restart_interval = (d[p] << 8) | d[p + 1];
        } else if (m == 0xEE) {
            if (L >= 14 && std::memcmp(d + p, "Adobe", 5) == 0) adobe = d[p + 11];
        } else if (m == 0xDA) {
            if (!have_sof) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOS segment before any SOF");
            const int ns = L >= 3 ? d[p] : 0;
            if (ns < 1 || ns > 4 || L != 6 + 2 * (size_t)ns) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOS segment of %zu bytes for %d components", L, ns);
            if (ns != o->ncomp) JPD_REFUSE(DD_JPEG_R_SCANS, "dd_jpeg_parse: several scans are refused (the first holds %d of %d components)", ns, o->ncomp);
            for (int c = 0; c < ns; ++c) {
                if (d[p + 1 + 2 * c] != comp_id[c]) JPD_REFUSE(DD_JPEG_R_SCANS, "dd_jpeg_parse: several scans, or a scan out of component order, are refused");
                o->td[c] = d[p + 2 + 2 * c] >> 4;
                o->ta[c] = d[p + 2 + 2 * c] & 15;
            }
            const int ss = d[p + 1 + 2 * ns], se = d[p + 2 + 2 * ns], a = d[p + 3 + 2 * ns];
            if (ss != 0 || se != 63 || a != 0) JPD_REFUSE(DD_JPEG_R_PROGRESSIVE, "dd_jpeg_parse: a scan with Ss %d, Se %d, Ah/Al 0x%02X: progressive parameters are refused", ss, se, a);
            for (int c = 0; c < ns; ++c) {
                if (o->td[c] > 1 || o->ta[c] > 1) JPD_REFUSE(DD_JPEG_R_HUFFMAN, "dd_jpeg_parse: component %d names Huffman tables %d / %d (0 and 1 only)", c, o->td[c], o->ta[c]);
                if (flags & DD_JPEGDEC_STD_TABLES) {
                    if (!o->huff[o->td[c]].defined) jpd_huffman_std(0, o->td[c], &o->huff[o->td[c]], o, msg, msgcap);
                    if (!o->huff[2 + o->ta[c]].defined) jpd_huffman_std(1, o->ta[c], &o->huff[2 + o->ta[c]], o, msg, msgcap);
                }
                if (!o->huff[o->td[c]].defined || !o->huff[2 + o->ta[c]].defined)
                    JPD_REFUSE(DD_JPEG_R_UNDEFINED, "dd_jpeg_parse: component %d references a Huffman table the file does not define", c);
                if (!o->quant_defined[o->tq[c]]) JPD_REFUSE(DD_JPEG_R_UNDEFINED, "dd_jpeg_parse: component %d references quant table %d, which the file does not define", c, o->tq[c]);
            }
            if (o->ncomp == 3 && adobe != -1 && adobe != 1) JPD_REFUSE(DD_JPEG_R_COMPONENTS, "dd_jpeg_parse: Adobe transform %d on 3 components is refused (YCbCr only)", adobe);
            o->hmax = o->hs[0], o->vmax = o->vs[0];
            o->mcus_x = (o->width + 8 * o->hmax - 1) / (8 * o->hmax);
            o->mcus_y = (o->height + 8 * o->vmax - 1) / (8 * o->vmax);
            o->blocks_per_mcu = o->ncomp == 1 ? 1 : o->hmax * o->vmax + 2;
            const int mcus = o->mcus_x * o->mcus_y;                       // at most 1024 * 1024
            const int ri = o->restart_interval ? o->restart_interval : mcus;
            o->n_intervals = (mcus + ri - 1) / ri;
            if (e > 0x7fffffffu || n - e > 0x7fffffffu) JPD_REFUSE(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a file of %zu bytes (below 2 GiB)", n);
            o->scan_offset = (int32_t)e;
            o->scan_length = (int32_t)(n - e);
            return DD_JPEG_R_OK;
        }
        i = e;
    }
}

// ---- progressive files (SOF2): the frame into *o, the scan script into *S (include/deepdish_hip.h; tests/jpeg_prog_ref.py parse is the
// definition).  A baseline file, and every file jpd_parse refuses for another reason than its being progressive, gives jpd_parse's answer
// and S->n_scans 0.  The whole file is walked: entropy-coded bytes are skipped to the next marker that is neither RSTn nor a stuffed FF 00,
// so the work is bounded by the file's length and the scan cap.

#define JPD_REFUSE_S(code, ...)                    \
    do {                                           \
        std::snprintf(msg, msgcap, __VA_ARGS__);   \
        o->reason = (code);                        \
        S->n_scans = 0;                            \
        return (code);                             \
    } while (0)

// flags: jpd_parse's, for the baseline files only; a progressive file with an undefined table is refused whatever they say.
static inline int jpd_parse_scans(const uint8_t *d, size_t n, dd_jpeg_info *o, dd_jpeg_scans *S, char *msg, size_t msgcap, int flags = 0) {
    S->n_scans = S->n_tables = S->n_levels = S->reserved = 0;
    std::memset(S->level_base, 0, sizeof(S->level_base));
    if (jpd_parse(d, n, o, msg, msgcap, flags) != DD_JPEG_R_PROGRESSIVE) return o->reason;
    // jpd_parse has checked SOI and every segment in front of the SOF2 (or of the scan with progressive parameters in a baseline frame)
    char base_msg[320];
    std::snprintf(base_msg, sizeof(base_msg), "%s", msg);
    std::memset(o, 0, sizeof(*o));
    bool have_sof = false;
    int adobe = -1, comp_id[3] = {0, 0, 0}, slot[2][4], dri = 0;
    int8_t al_at[3][64], level_at[3][64];                 // per coefficient: the Al delivered so far (-1: nothing), the level of the scan that did
    for (int c = 0; c < 2; ++c)
        for (int t = 0; t < 4; ++t) slot[c][t] = -1;
    std::memset(al_at, -1, sizeof(al_at));
    std::memset(level_at, -1, sizeof(level_at));
    size_t i = 2;
    while (i + 4 <= n) {
        if (d[i] != 0xFF) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: no marker at offset %zu", i);
        const int m = d[i + 1];
        if (m == 0xFF) {
            ++i;
            continue;
        }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
            i += 2;
            continue;
        }
        if (m == 0xD9) break;
        const size_t L = ((size_t)d[i + 2] << 8) | d[i + 3];
        if (L < 2 || i + 2 + L > n) JPD_REFUSE_S(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated: the segment at offset %zu has a length of %zu, past the file's %zu bytes", i, L, n);
        size_t p = i + 4;
        const size_t e = i + 2 + L;
        if (m == 0xC6) JPD_REFUSE_S(DD_JPEG_R_PROGRESSIVE, "dd_jpeg_parse: differential progressive files (SOF6, a hierarchical mode) are refused");
        if (m >= 0xC0 && m <= 0xCF && m != 0xC2 && m != 0xC4 && m != 0xC8) JPD_REFUSE_S(DD_JPEG_R_PROGRESSIVE, "%s", base_msg);        // a baseline frame with progressive scan parameters
        if (m == 0xC2) {
            if (have_sof) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a second SOF segment");
            if (L < 8) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOF segment of %zu bytes", L);
            if (d[p] != 8) JPD_REFUSE_S(DD_JPEG_R_PRECISION, "dd_jpeg_parse: %d-bit precision is refused (8 only)", d[p]);
            const int H = (d[p + 1] << 8) | d[p + 2], W = (d[p + 3] << 8) | d[p + 4], nc = d[p + 5];
            if (H < 1 || W < 1 || H > JPD_MAX_SIDE || W > JPD_MAX_SIDE) JPD_REFUSE_S(DD_JPEG_R_SIZE, "dd_jpeg_parse: size %d x %d (1 .. %d either way)", W, H, JPD_MAX_SIDE);
            if (nc != 1 && nc != 3) JPD_REFUSE_S(DD_JPEG_R_COMPONENTS, "dd_jpeg_parse: %d components are refused (1 or 3)", nc);
            if (L != 8 + 3 * (size_t)nc) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOF segment of %zu bytes for %d components", L, nc);
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = d[p + 6 + 3 * c];
                o->hs[c] = d[p + 7 + 3 * c] >> 4;
                o->vs[c] = d[p + 7 + 3 * c] & 15;
                o->tq[c] = d[p + 8 + 3 * c];
                if (o->tq[c] > 3) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: component %d names quant table %d (0 .. 3)", c, o->tq[c]);
            }
            if (nc == 1) o->hs[0] = o->vs[0] = 1;
            else {
                const bool luma = o->vs[0] >= 1 && o->vs[0] <= 2 && o->hs[0] >= o->vs[0] && o->hs[0] <= 2;
                if (!luma || o->hs[1] != 1 || o->vs[1] != 1 || o->hs[2] != 1 || o->vs[2] != 1)
                    JPD_REFUSE_S(DD_JPEG_R_SAMPLING, "dd_jpeg_parse: sampling %dx%d, %dx%d, %dx%d is refused (4:4:4, 4:2:2 and 4:2:0 only)", o->hs[0], o->vs[0], o->hs[1],
                                 o->vs[1], o->hs[2], o->vs[2]);
            }
            o->height = H, o->width = W, o->ncomp = nc, o->sof = m;
            o->hmax = o->hs[0], o->vmax = o->vs[0];
            o->mcus_x = (W + 8 * o->hmax - 1) / (8 * o->hmax);
            o->mcus_y = (H + 8 * o->vmax - 1) / (8 * o->vmax);
            o->blocks_per_mcu = nc == 1 ? 1 : o->hmax * o->vmax + 2;
            have_sof = true;
        } else if (m == 0xDB) {
            while (p < e) {
                if (d[p] >> 4) JPD_REFUSE_S(DD_JPEG_R_PRECISION, "dd_jpeg_parse: 16-bit quant tables are refused (precision field %d)", d[p] >> 4);
                const int tq = d[p] & 15;
                if (tq > 3 || p + 65 > e) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a DQT segment with table id %d and %zu bytes left", tq, e - p);
                for (int k = 0; k < 64; ++k) o->quant[tq][JPD_ZIGZAG[k]] = d[p + 1 + k];
                o->quant_defined[tq] = 1;
                p += 65;
            }
        } else if (m == 0xC4) {
            while (p < e) {
                if (p + 17 > e) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a DHT segment shorter than its table");
                const int tc = d[p] >> 4, th = d[p] & 15;
                if (tc > 1 || th > 3) JPD_REFUSE_S(DD_JPEG_R_HUFFMAN, "dd_jpeg_parse: Huffman table class %d id %d (ids 0 .. 3 of classes 0 and 1)", tc, th);
                if (S->n_tables >= DD_JPEG_MAX_TABLES) JPD_REFUSE_S(DD_JPEG_R_CAPACITY, "dd_jpeg_parse: more than %d Huffman tables in one file", DD_JPEG_MAX_TABLES);
                const size_t took = jpd_huffman_build(d, p, e, &S->pool[S->n_tables], o, msg, msgcap);
                if (!took) {
                    S->n_scans = 0;
                    return o->reason;
                }
                slot[tc][th] = S->n_tables++;
                p += took;
            }
        } else if (m == 0xDD) {
            if (L != 4) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a DRI segment of %zu bytes", L);
            dri = (d[p] << 8) | d[p + 1];
        } else if (m == 0xEE) {
            if (L >= 14 && std::memcmp(d + p, "Adobe", 5) == 0) adobe = d[p + 11];
        } else if (m == 0xDA) {
            if (!have_sof) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOS segment before any SOF");
            const int ns = L >= 3 ? d[p] : 0;
            if (ns < 1 || ns > 4 || L != 6 + 2 * (size_t)ns) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: an SOS segment of %zu bytes for %d components", L, ns);
            if (ns > o->ncomp) JPD_REFUSE_S(DD_JPEG_R_SCANS, "dd_jpeg_parse: a scan of %d components in a file of %d", ns, o->ncomp);
            if (S->n_scans >= DD_JPEG_MAX_SCANS) JPD_REFUSE_S(DD_JPEG_R_CAPACITY, "dd_jpeg_parse: more than %d scans in one file", DD_JPEG_MAX_SCANS);
            dd_jpeg_scan *sc = &S->scan[S->n_scans];
            std::memset(sc, 0, sizeof(*sc));
            int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
            for (int k = 0; k < ns; ++k) {
                int c = 0;
                while (c < o->ncomp && comp_id[c] != d[p + 1 + 2 * k]) ++c;
                if (c == o->ncomp) JPD_REFUSE_S(DD_JPEG_R_SCANS, "dd_jpeg_parse: a scan names component id %d, which the frame does not hold", d[p + 1 + 2 * k]);
                if (k && c <= sc->comp[k - 1]) JPD_REFUSE_S(DD_JPEG_R_SCANS, "dd_jpeg_parse: a scan out of component order");
                sc->comp[k] = c;
                td[k] = d[p + 2 + 2 * k] >> 4, ta[k] = d[p + 2 + 2 * k] & 15;
            }
            const int ss = d[p + 1 + 2 * ns], se = d[p + 2 + 2 * ns], ah = d[p + 3 + 2 * ns] >> 4, al = d[p + 3 + 2 * ns] & 15;
            if (ss > se || se > 63 || (ss == 0 && se != 0) || al > 13 || ah > 13)
                JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a scan with Ss %d, Se %d, Ah %d, Al %d", ss, se, ah, al);
            if (ss > 0 && ns != 1) JPD_REFUSE_S(DD_JPEG_R_AC_COMPONENTS, "dd_jpeg_parse: an AC scan (Ss %d) of %d components (one at a time)", ss, ns);
            int level = 0;
            for (int k = 0; k < ns; ++k) {
                const int c = sc->comp[k];
                if (ss > 0 && al_at[c][0] < 0) JPD_REFUSE_S(DD_JPEG_R_AC_BEFORE_DC, "dd_jpeg_parse: an AC scan of component %d before its DC scan", c);
                const int have = al_at[c][ss];
                for (int j = ss; j <= se; ++j) {
                    if (al_at[c][j] != have) JPD_REFUSE_S(DD_JPEG_R_REFINEMENT, "dd_jpeg_parse: a scan over coefficients %d .. %d of component %d, which stand at different bits", ss, se, c);
                    if (level_at[c][j] + 1 > level) level = level_at[c][j] + 1;
                }
                if (have < 0) {
                    if (ah != 0) JPD_REFUSE_S(DD_JPEG_R_FIRST_AH, "dd_jpeg_parse: the first scan of coefficients %d .. %d of component %d has Ah %d (0)", ss, se, c, ah);
                } else if (ah != have || al != ah - 1)
                    JPD_REFUSE_S(DD_JPEG_R_REFINEMENT, "dd_jpeg_parse: a scan with Ah %d, Al %d over coefficients %d .. %d of component %d, which stand at bit %d", ah, al, ss, se,
                                 c, have);
            }
            if (level >= DD_JPEG_MAX_LEVELS) JPD_REFUSE_S(DD_JPEG_R_CAPACITY, "dd_jpeg_parse: a scan at level %d (below %d)", level, DD_JPEG_MAX_LEVELS);
            sc->ac = -1;
            for (int k = 0; k < 3; ++k) sc->dc[k] = -1;
            for (int k = 0; k < ns; ++k) {
                const int c = sc->comp[k];
                if (td[k] > 3 || ta[k] > 3) JPD_REFUSE_S(DD_JPEG_R_HUFFMAN, "dd_jpeg_parse: component %d names Huffman tables %d / %d (0 .. 3)", c, td[k], ta[k]);
                if (ss == 0 && ah == 0) {
                    if (slot[0][td[k]] < 0) JPD_REFUSE_S(DD_JPEG_R_UNDEFINED, "dd_jpeg_parse: component %d references DC table %d, which no DHT in front of the scan defines", c, td[k]);
                    sc->dc[k] = slot[0][td[k]];
                } else if (ss > 0) {
                    if (slot[1][ta[k]] < 0) JPD_REFUSE_S(DD_JPEG_R_UNDEFINED, "dd_jpeg_parse: component %d references AC table %d, which no DHT in front of the scan defines", c, ta[k]);
                    sc->ac = slot[1][ta[k]];
                }
                for (int j = ss; j <= se; ++j) al_at[c][j] = (int8_t)al, level_at[c][j] = (int8_t)level;
            }
            size_t q = e;                                  // the entropy-coded bytes end in front of the next marker
            while (q < n && !(d[q] == 0xFF && q + 1 < n && d[q + 1] != 0 && d[q + 1] != 0xFF && !(d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7))) ++q;
            if (q > 0x7fffffffu) JPD_REFUSE_S(DD_JPEG_R_SEGMENT, "dd_jpeg_parse: a file of %zu bytes (below 2 GiB)", n);
            sc->offset = (int32_t)e, sc->length = (int32_t)(q - e);
            sc->ncomp = ns, sc->ss = ss, sc->se = se, sc->ah = ah, sc->al = al, sc->restart_interval = dri, sc->level = level;
            if (ns > 1) sc->blocks_x = o->mcus_x, sc->blocks_y = o->mcus_y;
            else {
                const int c = sc->comp[0];
                const int wc = (o->width * o->hs[c] + o->hmax - 1) / o->hmax, hc = (o->height * o->vs[c] + o->vmax - 1) / o->vmax;
                sc->blocks_x = (wc + 7) / 8, sc->blocks_y = (hc + 7) / 8;
            }
            const int units = sc->blocks_x * sc->blocks_y, ri = dri ? dri : units;          // at most 1024 * 1024 units
            sc->n_intervals = (units + ri - 1) / ri;
            if (level + 1 > S->n_levels) S->n_levels = level + 1;
            ++S->n_scans;
            i = q;
            continue;
        }
        i = e;
    }
    if (!have_sof) JPD_REFUSE_S(DD_JPEG_R_TRUNCATED, "dd_jpeg_parse: truncated: the file ends at byte %zu before an SOF segment", n);
    for (int c = 0; c < o->ncomp; ++c)
        if (!o->quant_defined[o->tq[c]]) JPD_REFUSE_S(DD_JPEG_R_UNDEFINED, "dd_jpeg_parse: component %d references quant table %d, which the file does not define", c, o->tq[c]);
    if (o->ncomp == 3 && adobe != -1 && adobe != 1) JPD_REFUSE_S(DD_JPEG_R_COMPONENTS, "dd_jpeg_parse: Adobe transform %d on 3 components is refused (YCbCr only)", adobe);
    for (int c = 0; c < o->ncomp; ++c)
        for (int j = 0; j < 64; ++j)
            if (al_at[c][j] != 0)
                JPD_REFUSE_S(DD_JPEG_R_INCOMPLETE,
                             "dd_jpeg_parse: the %d scans end with coefficient %d of component %d %s: an incomplete progressive file is refused (libjpeg would smooth or "
                             "zero-fill it)",
                             S->n_scans, j, c, al_at[c][j] < 0 ? "never sent" : "short of bit 0");
    return DD_JPEG_R_OK;
}
