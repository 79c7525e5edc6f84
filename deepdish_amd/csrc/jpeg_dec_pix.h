// The pixel stage of the JPEG decoder on the device: what its kernels do to one band (one MCU row) of one file.  A band's blocks are
// dequantised and transformed (jd_block, jd_block_scaled<N>) into sample planes Y, Cb, Cr laid out as the plan's JdBand says
// (csrc/jpeg_dec_plan.h), in LDS or -- a band too wide for LDS, DD_JPEGDEC_PLANES -- in HBM; then every output pixel is up-sampled and
// colour-converted from the planes (jd_pixel, jd_pixel_scaled<S>) and the rows are stored in order (jd_paint, jd_paint_scaled<S>).  At scale 1 the
// h2v2 filter's chroma row above and below the band comes from transforming those neighbouring chroma blocks again (the halo); at 1/2, 1/4
// and 1/8 every block goes straight to 4 x 4, 2 x 2 or 1 x 1 samples, 4:2:0 chroma is not up-sampled at all and there is no halo.
// Two translation units include this: csrc/jpeg_dec.hip, whose kernels write dense frames of the decoder's one size and scale, and
// csrc/jpeg_dec_any.hip, whose kernels write every file at its own size and scale into a slot (DD_JPEGDEC_ANY_SIZE).
#pragma once
#include "jpeg_dec_dev.h"

namespace {

// Block `blk` of a frame: dequantise and transform.  rows: -1 all eight to dst (stride bytes apart), else that one row to dst.
__device__ __forceinline__ void jd_block(const int16_t *__restrict__ coef, size_t blk, const uint16_t *__restrict__ q, uint8_t *dst, int stride, int row) {
    int32_t d[64];
    const uint4 *c4 = reinterpret_cast<const uint4 *>(coef + blk * 64);
    const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 c = c4[i], v = q4[i];
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[8 * i + 2 * j] = (int32_t)(int16_t)(cw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
            d[8 * i + 2 * j + 1] = (int32_t)(int16_t)(cw[j] >> 16) * (int32_t)(qw[j] >> 16);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) jpd_idct8<8, 11>(&d[c]);
    if (row < 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            jpd_idct8<1, 18>(&d[8 * r]);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo |= (uint32_t)jpd_range_limit(d[8 * r + i]) << (8 * i);
                hi |= (uint32_t)jpd_range_limit(d[8 * r + 4 + i]) << (8 * i);
            }
            *reinterpret_cast<uint2 *>(dst + (size_t)r * stride) = make_uint2(lo, hi);
        }
    } else {
        int32_t e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = row == 0 ? d[i] : d[56 + i];            // the halo rows: a block's first or last
        jpd_idct8<1, 18>(e);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)jpd_range_limit(e[i]) << (8 * i);
            hi |= (uint32_t)jpd_range_limit(e[4 + i]) << (8 * i);
        }
        *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
    }
}

// The blocks of MCU row `band` into planes Y [.. ][Wy], Cb and Cr [.. ][Wc]: Y's row 0 is the band's first luma row; the chroma planes'
// row 0 is the band's first chroma row when halo is 0, else the last chroma row of the band above, and row 9 the first of the band below.
__device__ __forceinline__ void jd_transform_band(const dd_jpeg_info &r, const int16_t *__restrict__ coef, int band, const JdBand &b, uint8_t *Y, uint8_t *Cb, uint8_t *Cr,
                                                  bool halo) {
    const int mx = r.mcus_x, bpm = r.blocks_per_mcu, ny = bpm == 1 ? 1 : bpm - 2, hs = r.hmax;
    const int per_mcu = bpm + (halo ? 4 : 0);
    for (int t = threadIdx.x; t < mx * per_mcu; t += JD_T) {
        const int m = t / per_mcu, k = t - m * per_mcu;
        const size_t mcu = (size_t)band * mx + m;
        if (k < ny) {
            jd_block(coef, mcu * bpm + k, r.quant[r.tq[0]], Y + (size_t)(k / hs) * 8 * b.Wy + (size_t)(m * hs + k % hs) * 8, b.Wy, -1);
        } else if (k < bpm) {
            const int c = k - ny + 1;
            jd_block(coef, mcu * bpm + k, r.quant[r.tq[c]], (c == 1 ? Cb : Cr) + (size_t)(halo ? 1 : 0) * b.Wc + (size_t)m * 8, b.Wc, -1);
        } else {
            const int h = k - bpm, c = 1 + (h & 1), below = h >> 1;
            if (below ? band + 1 >= r.mcus_y : band == 0) continue;          // the frame's edge: the filter repeats the band's own row
            const size_t nb = ((size_t)(below ? band + 1 : band - 1) * mx + m) * bpm + ny + (c - 1);
            jd_block(coef, nb, r.quant[r.tq[c]], (c == 1 ? Cb : Cr) + (size_t)(below ? 9 : 0) * b.Wc + (size_t)m * 8, b.Wc, below ? 0 : 7);
        }
    }
}

// Pixel (y, x) of the frame from planes whose row 0 is luma row y0 / chroma row c0: libjpeg's fancy up-sampling over the component's
// true size cw x ch (plain replication at cw <= 2, as jdsample.c chooses), then jdcolor.c.  Packed B | G << 8 | R << 16.
__device__ __forceinline__ uint32_t jd_pixel(const dd_jpeg_info &r, const JdBand &b, const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, int y0, int c0, int y, int x,
                                             int cw, int ch) {
    const int yy = Y[(size_t)(y - y0) * b.Wy + x];
    if (r.ncomp == 1) return (uint32_t)yy * 0x010101u;
    int cb, cr;
    if (r.hmax == 1) {
        const size_t o = (size_t)(y - c0) * b.Wc + x;
        cb = Cb[o], cr = Cr[o];
    } else {
        const int cx = x >> 1, cy = r.vmax == 2 ? y >> 1 : y;
        const size_t near = (size_t)(cy - c0) * b.Wc;
        if (cw <= 2) {
            cb = Cb[near + cx], cr = Cr[near + cx];
        } else {
            const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
            if (r.vmax == 1) {
                const int bias = (x & 1) ? 2 : 1;
                cb = (3 * Cb[near + cx] + Cb[near + nx] + bias) >> 2;
                cr = (3 * Cr[near + cx] + Cr[near + nx] + bias) >> 2;
            } else {
                const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                const size_t far = (size_t)(fy - c0) * b.Wc;
                const int bias = (x & 1) ? 7 : 8;
                cb = (3 * (3 * Cb[near + cx] + Cb[far + cx]) + 3 * Cb[near + nx] + Cb[far + nx] + bias) >> 4;
                cr = (3 * (3 * Cr[near + cx] + Cr[far + cx]) + 3 * Cr[near + nx] + Cr[far + nx] + bias) >> 4;
            }
        }
    }
    return jpd_bgr(yy, cb, cr);
}

// Rows [y_first, y_first + rows) of frame `out` from the planes.  Four pixels a thread, three dword stores, where rows are dword-aligned.
__device__ __forceinline__ void jd_paint(const dd_jpeg_info &r, const JdBand &b, const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, int y0, int c0, int y_first, int rows,
                                         uint8_t *__restrict__ out, bool vec) {
    const int W = r.width, H = r.height;
    const int cw = (W + r.hmax - 1) / r.hmax, ch = (H + r.vmax - 1) / r.vmax;
    if (vec) {
        const int qw = W >> 2;
        for (int i = threadIdx.x; i < rows * qw; i += JD_T) {
            const int row = i / qw, x = (i - row * qw) * 4, y = y_first + row;
            uint32_t p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = jd_pixel(r, b, Y, Cb, Cr, y0, c0, y, x + j, cw, ch);
            uint32_t *o = reinterpret_cast<uint32_t *>(out + ((size_t)y * W + x) * 3);
            o[0] = p[0] | (p[1] << 24);
            o[1] = (p[1] >> 8) | (p[2] << 16);
            o[2] = (p[2] >> 16) | (p[3] << 8);
        }
    } else {
        for (int i = threadIdx.x; i < rows * W; i += JD_T) {
            const int row = i / W, x = i - row * W, y = y_first + row;
            const uint32_t p = jd_pixel(r, b, Y, Cb, Cr, y0, c0, y, x, cw, ch);
            uint8_t *o = out + ((size_t)y * W + x) * 3;
            o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
        }
    }
}

// ---- 1/2, 1/4 and 1/8 scale: the same, specialised on the scale denominator S.

// Block `blk` of a frame to N x N samples at dst, rows `stride` bytes apart.  N = 8 is the full transform (4:2:0 chroma at S = 2).  dst is
// aligned to N bytes: every plane starts at a multiple of its block side and is a whole number of blocks wide.
template <int N>
__device__ __forceinline__ void jd_block_scaled(const int16_t *__restrict__ coef, size_t blk, const uint16_t *__restrict__ q, uint8_t *dst, int stride) {
    if constexpr (N == 8) {
        jd_block(coef, blk, q, dst, stride, -1);
    } else if constexpr (N == 1) {
        *dst = (uint8_t)jpd_idct1((int32_t)coef[blk * 64] * (int32_t)q[0]);
    } else {
        int32_t d[64];
        const uint4 *c4 = reinterpret_cast<const uint4 *>(coef + blk * 64);
        const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (N == 4 ? i == 4 : (i != 0 && !(i & 1))) continue;          // rows the transform does not read
            const uint4 c = c4[i], v = q4[i];
            const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d[8 * i + 2 * j] = (int32_t)(int16_t)(cw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
                d[8 * i + 2 * j + 1] = (int32_t)(int16_t)(cw[j] >> 16) * (int32_t)(qw[j] >> 16);
            }
        }
        int o[N * N];
        if constexpr (N == 4) {
            jpd_idct4(d, o);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<uint32_t *>(dst + (size_t)r * stride) = (uint32_t)o[4 * r] | ((uint32_t)o[4 * r + 1] << 8) | ((uint32_t)o[4 * r + 2] << 16) | ((uint32_t)o[4 * r + 3] << 24);
        } else {
            jpd_idct2(d, o);
#pragma unroll
            for (int r = 0; r < 2; ++r) *reinterpret_cast<uint16_t *>(dst + (size_t)r * stride) = (uint16_t)(o[2 * r] | (o[2 * r + 1] << 8));
        }
    }
}

// The blocks of MCU row `band` into planes Y [b.yrows][Wy], Cb and Cr [b.crows][Wc], whose row 0 is the band's first.
template <int S>
__device__ __forceinline__ void jd_transform_band_scaled(const dd_jpeg_info &r, const int16_t *__restrict__ coef, int band, const JdBand &b, uint8_t *Y, uint8_t *Cb,
                                                         uint8_t *Cr) {
    constexpr int NY = 8 / S;
    const int mx = r.mcus_x, bpm = r.blocks_per_mcu, ny = bpm == 1 ? 1 : bpm - 2, hs = r.hmax;
    for (int t = threadIdx.x; t < mx * bpm; t += JD_T) {
        const int m = t / bpm, k = t - m * bpm;
        const size_t blk = ((size_t)band * mx + m) * bpm + k;
        if (k < ny) {
            jd_block_scaled<NY>(coef, blk, r.quant[r.tq[0]], Y + (size_t)(k / hs) * NY * b.Wy + (size_t)(m * hs + k % hs) * NY, b.Wy);
        } else {
            const int c = k - ny + 1;
            uint8_t *dst = (c == 1 ? Cb : Cr) + (size_t)m * b.crows;
            if (b.crows == NY) jd_block_scaled<NY>(coef, blk, r.quant[r.tq[c]], dst, b.Wc);
            else jd_block_scaled<2 * NY>(coef, blk, r.quant[r.tq[c]], dst, b.Wc);           // 4:2:0
        }
    }
}

// Pixel x of plane row `row` (the components' rows coincide).  Only 4:2:2 chroma is up-sampled: jdsample.c's h2v1 fancy filter over the
// plane's true width cw, plain replication at cw <= 2 and at S = 8, where libjpeg turns the filter off.  Packed B | G << 8 | R << 16.
template <int S>
__device__ __forceinline__ uint32_t jd_pixel_scaled(const dd_jpeg_info &r, const JdBand &b, const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, int row, int x, int cw) {
    const int yy = Y[(size_t)row * b.Wy + x];
    if (r.ncomp == 1) return (uint32_t)yy * 0x010101u;
    const size_t o = (size_t)row * b.Wc;
    int cb, cr;
    if (b.Wc == b.Wy) {
        cb = Cb[o + x], cr = Cr[o + x];
    } else {
        const int cx = x >> 1;
        if (S == 8 || cw <= 2) {
            cb = Cb[o + cx], cr = Cr[o + cx];
        } else {
            const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), bias = (x & 1) ? 2 : 1;
            cb = (3 * Cb[o + cx] + Cb[o + nx] + bias) >> 2;
            cr = (3 * Cr[o + cx] + Cr[o + nx] + bias) >> 2;
        }
    }
    return jpd_bgr(yy, cb, cr);
}

// Rows [y_first, y_first + rows) of the oh x ow frame `out` from planes whose row `row0` is output row y_first.
template <int S>
__device__ __forceinline__ void jd_paint_scaled(const dd_jpeg_info &r, const JdBand &b, const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, int row0, int y_first, int rows,
                                                int ow, uint8_t *__restrict__ out, bool vec) {
    const int cw = r.ncomp == 3 ? jpd_plane(r.height, r.width, 1, 1, r.hmax, r.vmax, S).cols : 0;
    if (vec) {
        const int qw = ow >> 2;
        for (int i = threadIdx.x; i < rows * qw; i += JD_T) {
            const int row = i / qw, x = (i - row * qw) * 4;
            uint32_t p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = jd_pixel_scaled<S>(r, b, Y, Cb, Cr, row0 + row, x + j, cw);
            uint32_t *o = reinterpret_cast<uint32_t *>(out + ((size_t)(y_first + row) * ow + x) * 3);
            o[0] = p[0] | (p[1] << 24);
            o[1] = (p[1] >> 8) | (p[2] << 16);
            o[2] = (p[2] >> 16) | (p[3] << 8);
        }
    } else {
        for (int i = threadIdx.x; i < rows * ow; i += JD_T) {
            const int row = i / ow, x = i - row * ow;
            const uint32_t p = jd_pixel_scaled<S>(r, b, Y, Cb, Cr, row0 + row, x, cw);
            uint8_t *o = out + ((size_t)(y_first + row) * ow + x) * 3;
            o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
        }
    }
}

}  // namespace
