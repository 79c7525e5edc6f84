// The header of a baseline JPEG file, SOI .. the first SOS, into a fixed-size dd_jpeg_info (include/deepdish_hip.h).  Plain C++, no
// device, no allocation: shared by dd_jpeg_parse (csrc/jpeg_dec.hip) and the stand-alone sanitizer check
// (scripts/jpeg_decode_check.cpp).  These bytes come from a network: every read is checked against the length, the work is bounded by
// the header, and the entropy-coded bytes are not walked.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/deepdish_hip.h"

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
    dd_jpeg_huff *h = &o->huff[tc * 2 + th];
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

// Returns DD_JPEG_R_OK or the reason (also o->reason); msg gets the text.
static inline int jpd_parse(const uint8_t *d, size_t n, dd_jpeg_info *o, char *msg, size_t msgcap) {
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
