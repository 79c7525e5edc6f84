// The JPEG decoder's call plan: everything the host decides about one call before anything is queued, as plain C++ -- no device, no
// allocation, an error code plus a message buffer -- so that csrc/jpeg_dec.hip runs it in front of its launches and
// scripts/jpeg_plan_check.cpp runs the same statements on the host under the sanitizers, over forged records.
//
// jd_plan_call takes the records (and scan scripts) csrc/jpeg_parse.h made of the files, in whatever state another thread left them, and
//   - gives every live file its place in the interval arrays (interval_base; a progressive file's scans get their own, and every level
//     its lanes: level_base), its pixel path and scale (path) and, under DD_JPEGDEC_SPLIT, its subsequence size (reserved);
//   - holds everything the kernels index with to the decoder's buffers: scan bytes within the bytes uploaded, scan and level counts within
//     dd_jpeg_scans, and for a DD_JPEGDEC_ANY_SIZE decoder sides, MCU counts, blocks and planes within the strides of JdGeom;
//   - returns in JdCall what the launches are sized by.
// After it has returned DD_OK the kernels may trust those fields; after anything else nothing is queued.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "jpeg_parse.h"

#if defined(__HIPCC__)
#define JPD_HD __host__ __device__ __forceinline__
#define JD_HD __host__ __device__ inline
#else
#define JPD_HD inline
#define JD_HD inline
#endif

// ---- decoding at 1/2, 1/4 and 1/8 scale (libjpeg's scale_num / scale_denom, Pillow's Image.draft; tests/jpeg_scaled_ref.py is the
// definition).  The entropy decoder and the coefficients are the full-size ones; every 8 x 8 block is transformed straight to n x n
// samples, n chosen per component.

JPD_HD bool jpd_scale_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }

// jdmaster.c: a component sampled hs x vs below hmax x vmax turns its blocks into n x n samples at scale 1 / s -- 8 / s, doubled while
// that still divides what the most densely sampled component gets, so that 4:2:0 chroma needs no up-sampling at any s >= 2 -- and its
// plane, before cropping to the output, holds rows x cols samples of an h x w file.
struct JpdPlane {
    int n, rows, cols;
};

JPD_HD JpdPlane jpd_plane(int h, int w, int hs, int vs, int hmax, int vmax, int s) {
    const int m = 8 / s;
    JpdPlane p;
    p.n = m;
    while (p.n < 8 && (hmax * m) % (hs * p.n * 2) == 0 && (vmax * m) % (vs * p.n * 2) == 0) p.n *= 2;
    p.rows = (int)(((long long)h * vs * p.n + vmax * 8 - 1) / (vmax * 8));
    p.cols = (int)(((long long)w * hs * p.n + hmax * 8 - 1) / (hmax * 8));
    return p;
}

// f(std::integral_constant<int, S>()) for the scale denominator s: the one place where a scale known at run time picks a kernel's template
// argument.
template <class F>
inline int jd_with_scale(int s, F &&f) {
    switch (s) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        default: return f(std::integral_constant<int, 8>());
    }
}

// What the pixel stage of a DD_JPEGDEC_ANY_SIZE decoder launches, per log2 of the scale: whether a file of the call has that scale, the
// most LDS such a file needs, whether one takes DD_JPEGDEC_PLANES.  A named type: it crosses to csrc/jpeg_dec_any.hip.
struct JdPerScale {
    size_t lds_at[4];
    bool any_at[4], planes_at[4];
};

namespace {

constexpr int JD_T = 256;                      // threads per workgroup (markers, split entropy, pixels)
constexpr int JD_LDS_MAX = 64 * 1024;          // a band's planes; what every kernel may use without asking
constexpr int JD_SPLIT_MAX_SUB = 2048;         // subsequences of a file: 28 bytes of LDS each, beside the file's four Huffman tables

// ------------------------------------------------------------------------------------------------ geometry

struct JdGeom {
    int H, W, max_bands;
    long long coef_stride;                     // int16 per frame: the largest accepted sampling's blocks
    long long plane_stride;                    // bytes per frame of the HBM planes
};

// One MCU row of a file as the pixel stage holds it: planes Y [yrows][Wy], Cb and Cr [crows][Wc], lds bytes in all.
struct JdBand {
    int Wy, Wc, yrows, crows, halo;
    size_t lds;
};

JD_HD JdBand jd_band(int W, int ncomp, int hs, int vs) {
    JdBand b;
    const int mx = (W + 8 * hs - 1) / (8 * hs);
    b.Wy = mx * 8 * hs, b.Wc = mx * 8;
    b.yrows = 8 * vs;
    b.halo = ncomp == 3 && vs == 2 ? 1 : 0;
    b.crows = ncomp == 3 ? 8 + 2 * b.halo : 0;
    b.lds = (size_t)b.yrows * b.Wy + 2 * (size_t)b.crows * b.Wc;
    return b;
}

// The same at scale 1 / s.  At s >= 2 a band is still one MCU row, 8 * vs / s output rows; every component's rows coincide with the
// luma's (4:2:0 chroma keeps blocks of twice the luma's side, jpd_plane), so there is no halo.
JD_HD JdBand jd_band(int W, int ncomp, int hs, int vs, int s) {
    if (s == 1) return jd_band(W, ncomp, hs, vs);
    JdBand b;
    const int mx = (W + 8 * hs - 1) / (8 * hs);
    const int ny = 8 / s, nc = jpd_plane(1, 1, 1, 1, hs, vs, s).n;
    b.Wy = mx * hs * ny, b.Wc = mx * nc;
    b.yrows = vs * ny;
    b.halo = 0;
    b.crows = ncomp == 3 ? nc : 0;
    b.lds = (size_t)b.yrows * b.Wy + 2 * (size_t)b.crows * b.Wc;
    return b;
}

#define JD_PLAN_REQUIRE(cond, code, ...)              \
    do {                                              \
        if (!(cond)) {                                \
            std::snprintf(msg, msgcap, __VA_ARGS__);  \
            return (code);                            \
        }                                             \
    } while (0)

// The buffers of a decoder of h x w: jd_geometry's strides are monotone in h and w, so a file that fits the sides fits them.
inline int jd_geometry(int h, int w, const char *who, JdGeom *g, char *msg, size_t msgcap) {
    JD_PLAN_REQUIRE(h >= 1 && w >= 1 && h <= JPD_MAX_SIDE && w <= JPD_MAX_SIDE, DD_E_ARG, "%s: a %d x %d frame (h, w: 1 .. %d either way)", who, w, h, JPD_MAX_SIDE);
    g->H = h, g->W = w;
    g->max_bands = (h + 7) / 8;
    const long long b8w = (w + 7) / 8, b8h = (h + 7) / 8, b16w = (w + 15) / 16, b16h = (h + 15) / 16;
    long long blocks = 3 * b8w * b8h;                                            // 4:4:4
    if (4 * b16w * b8h > blocks) blocks = 4 * b16w * b8h;                       // 4:2:2
    if (6 * b16w * b16h > blocks) blocks = 6 * b16w * b16h;                     // 4:2:0
    g->coef_stride = blocks * 64;
    g->plane_stride = 3 * (16 * b16w) * (16 * b16h);                            // every sampling's planes fit in three padded ones
    return DD_OK;
}

// ------------------------------------------------------------------------------------------------ the two packed record fields

// dd_jpeg_info.path: DD_JPEGDEC_LDS / _PLANES in bits 0 .. 7 and, for a DD_JPEGDEC_ANY_SIZE decoder, the log2 of the file's scale in
// bits 8 .. 15 (0 otherwise).  dd_jpeg_info.reserved: 0, or the log2 of the subsequence size of a file jpeg_split_entropy_k decodes.
JD_HD constexpr int jd_path_pack(int path, int scale_log2) { return path | scale_log2 << 8; }
JD_HD constexpr int jd_path_of(int packed) { return packed & 0xff; }
JD_HD constexpr int jd_path_scale_log2(int packed) { return (packed >> 8) & 0xff; }
JD_HD constexpr int jd_scale_log2(int s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : 3; }
inline int jd_split_log2_of(const dd_jpeg_info &r) { return r.reserved; }

// ------------------------------------------------------------------------------------------------ the plan

// What a decoder is, as far as planning goes.
struct JdConfig {
    JdGeom g;                                  // DD_JPEGDEC_ANY_SIZE: g.H x g.W is the largest file accepted
    int scale;                                 // the scale denominator; DD_JPEGDEC_ANY_SIZE: the smallest of a call
    int flags;                                 // DD_JPEGDEC_*
    int split_log2;                            // DD_JPEGDEC_SPLIT: log2 of the subsequence size ...
    bool split_auto;                           // ... and whether a file may double it (DD_JPEGDEC_SPLIT_BYTES fixes it)
    int max_frames;
    size_t max_bytes;
    int lanes;                                 // 0, or DD_JPEGDEC_LANES: intervals per wave of the entropy kernels, for A/B runs
    bool has(int flag) const { return (flags & flag) != 0; }
};

// What the launches of one call are sized by.
struct JdCall {
    long long total;                           // restart intervals of the baseline files: lanes of jpeg_entropy_k
    long long ptotal;                          // restart intervals of all scans of the progressive files
    long long level_total[DD_JPEG_MAX_LEVELS]; // lanes of jpeg_prog_entropy_k per level
    int max_scans, n_levels;                   // the most scans and levels a progressive file of the call has; 0: none
    int n_split, max_sub;                      // files routed to jpeg_split_entropy_k; the most subsequences one of them has
    size_t lds;                                // the pixel kernel's LDS, and whether a file takes DD_JPEGDEC_PLANES ...
    bool any_planes;
    JdPerScale per_scale;                      // ... and the same per scale, for a DD_JPEGDEC_ANY_SIZE decoder
    bool any;                                  // a file to decode at all
};

// Intervals per wave of jpeg_entropy_k / jpeg_prog_entropy_k: a lane decodes serially, so few intervals are spread over many waves (one
// per SIMD and more: 256 CUs of 4 SIMDs), and only a call with very many intervals fills its waves.
inline int jd_lanes_per_wave(long long intervals, int lanes) {
    int per = 64;
    while (per > 1 && intervals / per < 2048) per >>= 1;
    return lanes ? lanes : per;
}

inline long long jd_split_subs(long long scan_length, int log2) { return (scan_length + (1ll << log2) - 1) >> log2; }

// DD_JPEGDEC_SPLIT: the log2 of the subsequence size for a scan of this length: the decoder's, doubled -- where DD_JPEGDEC_SPLIT_BYTES did
// not fix it -- until every lane of the workgroup has at most one subsequence (see the README's table), and in any case until the file's
// states fit the kernel's LDS.
inline int jd_split_sub_log2(long long scan_length, int log2, bool split_auto) {
    if (split_auto)
        while (jd_split_subs(scan_length, log2) > JD_T) ++log2;
    while (jd_split_subs(scan_length, log2) > JD_SPLIT_MAX_SUB) ++log2;
    return log2;
}

// Is there anything for jpeg_split_entropy_k, for jpeg_entropy_k, for jpeg_prog_markers_k and jpeg_prog_entropy_k?  A call of progressive
// files alone, or of split files alone, has no baseline interval left for a lane of jpeg_entropy_k.
inline bool jd_call_has_split(const JdCall &c) { return c.n_split != 0; }
inline bool jd_call_has_progressive(const JdCall &c) { return c.max_scans != 0; }
inline bool jd_call_has_baseline_lanes(const JdCall &c) { return (c.total || !jd_call_has_progressive(c)) && !(c.n_split && c.total == c.n_split); }

// recs: n records from the parser, with status and file_offset set; scans: NULL, or their n scan scripts; scales: NULL, or one scale
// denominator per file.  Fills the records' and scans' decoder fields and *out; DD_OK, or the error with its text in msg.
inline int jd_plan_call(const JdConfig &cfg, dd_jpeg_info *recs, dd_jpeg_scans *scans, size_t n_bytes, int n, const int *scales, JdCall *out, char *msg, size_t msgcap) {
    JD_PLAN_REQUIRE(n >= 1 && n <= cfg.max_frames, DD_E_CAPACITY, "jpeg decoder: %d frames in a call (1 .. %d)", n, cfg.max_frames);
    JD_PLAN_REQUIRE(n_bytes <= cfg.max_bytes, DD_E_CAPACITY, "jpeg decoder: %zu bytes of files in a call (at most %zu)", n_bytes, cfg.max_bytes);
    JD_PLAN_REQUIRE(!scans || cfg.has(DD_JPEGDEC_PROGRESSIVE), DD_E_STATE, "jpeg decoder: scan scripts for a decoder that was not made to take progressive files");
    JD_PLAN_REQUIRE(!scales || cfg.has(DD_JPEGDEC_ANY_SIZE), DD_E_STATE, "jpeg decoder: a scale per file for a decoder that was not made with DD_JPEGDEC_ANY_SIZE");
    const JdGeom &g = cfg.g;
    JdCall c{};
    for (int i = 0; i < n; ++i) {
        dd_jpeg_info &r = recs[i];
        r.interval_base = (int32_t)c.total;
        r.reserved = 0;
        if (scans) {
            dd_jpeg_scans &S = scans[i];
            for (int l = 0; l < DD_JPEG_MAX_LEVELS; ++l) S.level_base[l] = (int32_t)c.level_total[l];
            if (r.status != DD_JPEG_ST_OK || r.sof != 0xC2) S.n_scans = S.n_levels = 0;
        }
        if (r.status != DD_JPEG_ST_OK) {
            r.n_intervals = 0;
            continue;
        }
        if (scans && scans[i].n_scans) {                                    // a progressive file: its scans take the place of the record's one
            dd_jpeg_scans &S = scans[i];
            JD_PLAN_REQUIRE(S.n_scans <= DD_JPEG_MAX_SCANS && S.n_levels <= DD_JPEG_MAX_LEVELS, DD_E_ARG, "jpeg decoder: file %d: %d scans at %d levels", i, S.n_scans, S.n_levels);
            for (int k = 0; k < S.n_scans; ++k) {
                dd_jpeg_scan &sc = S.scan[k];
                JD_PLAN_REQUIRE(r.file_offset >= 0 && sc.offset >= 0 && sc.length >= 0 && (size_t)r.file_offset + (size_t)sc.offset + (size_t)sc.length <= n_bytes, DD_E_ARG,
                                "jpeg decoder: scan %d of file %d lies outside the %zu bytes given", k, i, n_bytes);
                JD_PLAN_REQUIRE(sc.level >= 0 && sc.level < S.n_levels && sc.n_intervals >= 1, DD_E_ARG, "jpeg decoder: scan %d of file %d: level %d, %d intervals", k, i, sc.level,
                                sc.n_intervals);
                sc.interval_base = (int32_t)c.ptotal;
                c.ptotal += sc.n_intervals;
                c.level_total[sc.level] += sc.n_intervals;
            }
            JD_PLAN_REQUIRE(c.ptotal <= 0x7fffffffll, DD_E_CAPACITY, "jpeg decoder: more than 2^31 restart intervals in a call");
            c.max_scans = S.n_scans > c.max_scans ? S.n_scans : c.max_scans;
            c.n_levels = S.n_levels > c.n_levels ? S.n_levels : c.n_levels;
            r.n_intervals = 0, r.restart_interval = 0, r.scan_offset = 0, r.scan_length = 0;          // nothing for jpeg_entropy_k
        }
        JD_PLAN_REQUIRE(r.file_offset >= 0 && (size_t)r.file_offset + (size_t)r.scan_offset + (size_t)r.scan_length <= n_bytes, DD_E_ARG,
                        "jpeg decoder: file %d lies outside the %zu bytes given", i, n_bytes);
        const int fs = scales ? scales[i] : cfg.scale;
        JD_PLAN_REQUIRE(jpd_scale_ok(fs) && fs >= cfg.scale, DD_E_ARG, "jpeg decoder: file %d at scale %d (1, 2, 4 or 8, and at least the decoder's %d)", i, fs, cfg.scale);
        const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, fs);
        const int path = b.lds <= (size_t)JD_LDS_MAX ? DD_JPEGDEC_LDS : DD_JPEGDEC_PLANES;
        r.path = path;
        if (path == DD_JPEGDEC_LDS) c.lds = b.lds > c.lds ? b.lds : c.lds;
        else c.any_planes = true;
        if (cfg.has(DD_JPEGDEC_ANY_SIZE)) {
            // these records came from put on other threads: everything the kernels index with is held to the decoder's buffers here
            const long long blocks = (long long)r.mcus_x * r.mcus_y * r.blocks_per_mcu;
            const long long crows = fs == 1 ? 8 : b.crows;                  // the planes in HBM hold no halo rows
            const long long plane_bytes = (long long)r.mcus_y * ((long long)b.yrows * b.Wy + (r.ncomp == 3 ? 2 * crows * b.Wc : 0));
            JD_PLAN_REQUIRE(r.height >= 1 && r.height <= g.H && r.width >= 1 && r.width <= g.W, DD_E_ARG, "jpeg decoder: file %d is %d x %d, the decoder holds at most %d x %d", i,
                            r.width, r.height, g.W, g.H);
            JD_PLAN_REQUIRE(r.mcus_x == (r.width + 8 * r.hmax - 1) / (8 * r.hmax) && r.mcus_y == (r.height + 8 * r.vmax - 1) / (8 * r.vmax) && r.mcus_y <= g.max_bands, DD_E_ARG,
                            "jpeg decoder: file %d: %d x %d MCUs for %d x %d pixels", i, r.mcus_x, r.mcus_y, r.width, r.height);
            JD_PLAN_REQUIRE(blocks * 64 <= g.coef_stride, DD_E_ARG, "jpeg decoder: file %d has %lld blocks, a frame's coefficients hold %lld", i, blocks, g.coef_stride / 64);
            JD_PLAN_REQUIRE(path == DD_JPEGDEC_LDS || plane_bytes <= g.plane_stride, DD_E_ARG, "jpeg decoder: file %d needs %lld bytes of planes, a frame holds %lld", i, plane_bytes,
                            g.plane_stride);
            const int lg = jd_scale_log2(fs);
            JdPerScale &ps = c.per_scale;
            ps.any_at[lg] = true;
            if (path == DD_JPEGDEC_LDS) ps.lds_at[lg] = b.lds > ps.lds_at[lg] ? b.lds : ps.lds_at[lg];
            else ps.planes_at[lg] = true;
            r.path = jd_path_pack(path, lg);
        }
        // DD_JPEGDEC_SPLIT: a baseline file that is one restart interval (no DRI, DRI 0, or a DRI of the MCU count or more) and longer than a
        // subsequence goes to jpeg_split_entropy_k; jpeg_entropy_k passes over it
        if (cfg.has(DD_JPEGDEC_SPLIT) && r.sof != 0xC2 && r.n_intervals == 1 && (long long)r.scan_length > (1ll << cfg.split_log2)) {
            const int lg = jd_split_sub_log2(r.scan_length, cfg.split_log2, cfg.split_auto);
            const int subs = (int)jd_split_subs(r.scan_length, lg);
            r.reserved = lg;
            c.max_sub = subs > c.max_sub ? subs : c.max_sub;
            ++c.n_split;
        }
        c.total += r.n_intervals;
        c.any = true;
        JD_PLAN_REQUIRE(c.total <= 0x7fffffffll, DD_E_CAPACITY, "jpeg decoder: more than 2^31 restart intervals in a call");
    }
    *out = c;
    return DD_OK;
}

}  // namespace
