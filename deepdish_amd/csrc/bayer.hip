// 8-bit raw sensor frames -> BGR u8, what a machine-vision or CSI camera delivers before any colour processing -> what the pipeline reads:
//   * raw8_to_bgr_k    the stand-alone converter, cv2.cvtColor(frame, COLOR_Bayer??2BGR) / COLOR_GRAY2BGR
//   * raw8_resize_k    convert + cv2.flip(frame, 0) + cv2.resize(frame, input_size) in one launch (the ingest ring's transform)
// One byte per pixel.  A Bayer mosaic (layouts 6 RGGB, 7 GRBG, 8 GBRG, 9 BGGR: the sensor's top-left 2 x 2 block read row by row) is
// demosaiced by OpenCV's published bilinear rule, restated -- OpenCV itself is absent, so parity with it is unpinned like every other cv2
// arithmetic here; tests/bayer_ref.py is the numpy restatement the kernels are held to bit for bit:
//   out(x, y) = D(clamp(x, 1, W - 2), clamp(y, 1, H - 2)): the outer ring of pixels repeats its inner neighbour, corners included, and
//   only the evaluation point is clamped, so no tap leaves the frame (W, H >= 3, either may be odd).  At an interior site D is
//     R or B site:  its own colour the sample, G = (N + S + W + E + 2) >> 2, the opposite colour = (NW + NE + SW + SE + 2) >> 2
//     G site:       G the sample, the colour of its horizontal neighbours (W + E + 1) >> 1, of its vertical ones (N + S + 1) >> 1
// Layout 10 is 8-bit monochrome (GREY / Y800): B = G = R = the sample, any W, H >= 1.
// No white balance, gamma or colour matrix, no 10 / 12 / 16-bit or packed mosaics, no edge-aware interpolation.
#include <climits>
#include <cstdlib>
#include "common.h"
#include "resize_lane_dev.h"

namespace {

constexpr int RAW_RGGB = 6, RAW_GRBG = 7, RAW_GBRG = 8, RAW_BGGR = 9, RAW_GRAY = 10;     // the ingest ring's pixel_format codes, continued

// Where the red sample of the top-left block sits: site (x, y) is red when ((x ^ RX) | (y ^ RY)) & 1 == 0, blue when both are 1.
template <int LAYOUT> struct BayerAt {
    static constexpr int RX = (LAYOUT == RAW_GRBG || LAYOUT == RAW_BGGR) ? 1 : 0;
    static constexpr int RY = (LAYOUT == RAW_GBRG || LAYOUT == RAW_BGGR) ? 1 : 0;
};

// D at one interior site from the column sums around it: vl, vc, vr = N + S of the columns left of, at and right of the site, h = W + E,
// c the sample; px, py = the site's column and row parity relative to the red sample.  -> B | G << 8 | R << 16.
__device__ __forceinline__ uint32_t bayer_site(int vl, int vc, int vr, int h, int c, int px, int py) {
    int b, g, r;
    if (px == py) {                                              // a red (0, 0) or blue (1, 1) site
        g = (vc + h + 2) >> 2;
        const int opp = (vl + vr + 2) >> 2;
        r = py ? opp : c; b = py ? c : opp;
    } else {                                                     // a green site: on a red row (py 0) its horizontal neighbours are red
        g = c;
        const int hor = (h + 1) >> 1, ver = (vc + 1) >> 1;
        r = py ? ver : hor; b = py ? hor : ver;
    }
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}

__device__ __forceinline__ int raw_byte(const u4v &v, int i) { return (int)((v[i >> 2] >> (8 * (i & 3))) & 255u); }

// Two 16-bit lanes per word: the even bytes (pixels 0, 2 of a dword) or the odd ones (pixels 1, 3).  In a mosaic row the even columns are all
// one kind of site and the odd columns the other, so a word of either is two sites of one kind; no sum passes 4 * 255 + 2, so nothing carries
// from one lane into the other, and a shifted sum is masked back to its byte.
constexpr uint32_t PK = 0x00ff00ffu;
__device__ __forceinline__ uint32_t pk_even(uint32_t w) { return w & PK; }
__device__ __forceinline__ uint32_t pk_odd(uint32_t w) { return (w >> 8) & PK; }
__device__ __forceinline__ uint32_t pk_prev(uint32_t cur, uint32_t prev) { return (cur << 16) | (prev >> 16); }      // lanes (prev's high, cur's low)
__device__ __forceinline__ uint32_t pk_next(uint32_t cur, uint32_t next) { return (cur >> 16) | (next << 16); }      // lanes (cur's high, next's low)

// Sixteen pixels of the row whose three source rows are t, m, b (16 bytes each; lo / hi: the byte left of and right of them, bits 0-7 t,
// 8-15 m, 16-23 b), PY the row's parity relative to the red sample; the lane starts at an even column.  first / last: the lane holds the
// frame's column 0 / W - 1, which repeats its inner neighbour.  Three 16-byte stores at o.
template <int LAYOUT, int PY>
__device__ __forceinline__ void bayer_row16(const u4v &t, const u4v &m, const u4v &b, uint32_t lo, uint32_t hi, bool first, bool last,
                                            uint8_t *__restrict__ o) {
    // N + S and the sample per column, even and odd columns apart; index 0 is the dword left of the lane (its last odd column is what is
    // read of it), index 5 the dword right of it (its first even column)
    uint32_t ve[6], vo[6], ce[6], co[6];
    ve[0] = ce[0] = 0; vo[5] = co[5] = 0;
    vo[0] = ((lo & 255u) + ((lo >> 16) & 255u)) << 16; co[0] = ((lo >> 8) & 255u) << 16;
    ve[5] = (hi & 255u) + ((hi >> 16) & 255u); ce[5] = (hi >> 8) & 255u;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        ve[d + 1] = pk_even(t[d]) + pk_even(b[d]); vo[d + 1] = pk_odd(t[d]) + pk_odd(b[d]);
        ce[d + 1] = pk_even(m[d]); co[d + 1] = pk_odd(m[d]);
    }
    constexpr bool EVEN_IS_RB = BayerAt<LAYOUT>::RX == PY;       // the even columns are the row's red / blue sites, the odd ones green; or the reverse
    uint32_t w[12];
#pragma unroll
    for (int d = 1; d <= 4; ++d) {
        uint32_t be, ge, re, bo, go, ro;                         // B, G, R of pixels 0, 2 (e) and 1, 3 (o) of the dword, a byte per 16-bit lane
        if constexpr (EVEN_IS_RB) {
            const uint32_t cw = pk_prev(co[d], co[d - 1]), vw = pk_prev(vo[d], vo[d - 1]);       // the columns west of the even ones
            const uint32_t cross = ((ve[d] + cw + co[d] + 0x00020002u) >> 2) & PK, diag = ((vw + vo[d] + 0x00020002u) >> 2) & PK;
            ge = cross; re = PY ? diag : ce[d]; be = PY ? ce[d] : diag;
            const uint32_t hor = ((ce[d] + pk_next(ce[d], ce[d + 1]) + 0x00010001u) >> 1) & PK, ver = ((vo[d] + 0x00010001u) >> 1) & PK;
            go = co[d]; ro = PY ? ver : hor; bo = PY ? hor : ver;
        } else {
            const uint32_t hor = ((pk_prev(co[d], co[d - 1]) + co[d] + 0x00010001u) >> 1) & PK, ver = ((ve[d] + 0x00010001u) >> 1) & PK;
            ge = ce[d]; re = PY ? ver : hor; be = PY ? hor : ver;
            const uint32_t cn = pk_next(ce[d], ce[d + 1]), vn = pk_next(ve[d], ve[d + 1]);       // the columns east of the odd ones
            const uint32_t cross = ((vo[d] + ce[d] + cn + 0x00020002u) >> 2) & PK, diag = ((ve[d] + vn + 0x00020002u) >> 2) & PK;
            go = cross; ro = PY ? diag : co[d]; bo = PY ? co[d] : diag;
        }
        const uint32_t bg = be | (ge << 8), rb = re | (bo << 8), gr = go | (ro << 8);        // B0 G0 B2 G2, R0 B1 R2 B3, G1 R1 G3 R3
        w[3 * d - 3] = (bg & 0xffffu) | (rb << 16);              // B0 G0 R0 B1
        w[3 * d - 2] = (gr & 0xffffu) | (bg & 0xffff0000u);      // G1 R1 B2 G2
        w[3 * d - 1] = (rb >> 16) | (gr & 0xffff0000u);          // R2 B3 G3 R3
    }
    if (first) w[0] = (w[0] >> 24) | ((w[1] & 0xffffu) << 8) | (w[0] & 0xff000000u);                   // pixel 0 = pixel 1
    if (last) w[11] = (w[11] & 0xffu) | ((w[10] >> 16) << 8) | ((w[11] & 0xffu) << 24);               // pixel 15 = pixel 14
    u4v *op = reinterpret_cast<u4v *>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u4v q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = w[4 * k + j];
        op[k] = q;
    }
}

// grid (ceil(items / 256), batch); src has a pitch and a frame stride, dst is dense [batch][H][W][3]; all addressing in 64 bits.
// WIDE: W % 16 == 0 and every row of both sides 16-byte aligned (the launcher checks) -- an item is 16 pixels of a row pair: the four
// source rows it needs as 16-byte loads plus their two halo bytes, 2 x three 16-byte stores; 1 byte read and 3 written per pixel, the
// rest is cache hits on the neighbouring rows.  Otherwise an item is one pixel, byte by byte: any W and H.
template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(256) void raw8_to_bgr_k(const uint8_t *__restrict__ src, int H, int W, int pitch, int64_t frame_stride,
                                                     uint8_t *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t *f = src + (size_t)blockIdx.y * (size_t)frame_stride;
    uint8_t *o = dst + (size_t)blockIdx.y * ((size_t)H * W * 3);
    if constexpr (LAYOUT == RAW_GRAY) {
        const int ipr = WIDE ? W >> 4 : W;                       // items per row
        if (i >= H * ipr) return;
        const int y = i / ipr, bx = i - y * ipr;
        const uint8_t *row = f + (size_t)y * (size_t)pitch;
        uint8_t *q = o + (size_t)y * W * 3;
        if constexpr (WIDE) {
            const u4v s = *reinterpret_cast<const u4v *>(row + 16 * (size_t)bx);
            u4v *op = reinterpret_cast<u4v *>(q + 48 * (size_t)bx);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                u4v d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = 16 * w + 4 * j;
                    d[j] = (uint32_t)raw_byte(s, k / 3) | ((uint32_t)raw_byte(s, (k + 1) / 3) << 8) | ((uint32_t)raw_byte(s, (k + 2) / 3) << 16) |
                           ((uint32_t)raw_byte(s, (k + 3) / 3) << 24);
                }
                op[w] = d;
            }
        } else {
            const uint8_t g = row[bx];
            q += (size_t)bx * 3;
            q[0] = g; q[1] = g; q[2] = g;
        }
    } else if constexpr (WIDE) {
        const int ipr = W >> 4;                                  // items per row pair
        if (i >= ((H + 1) >> 1) * ipr) return;
        const int by = i / ipr, bx = i - by * ipr, x0 = 16 * bx;
        // rows b0 .. b0 + 3 hold the three rows around both evaluation rows (clamp(2 by + j, 1, H - 2) - 1 - b0 is 0 or 1)
        const int b0 = min(max(2 * by - 1, 0), max(H - 4, 0));
        const int xl = max(x0 - 1, 0), xr = min(x0 + 16, W - 1);
        u4v r[4];
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t *row = f + (size_t)min(b0 + k, H - 1) * (size_t)pitch;
            r[k] = *reinterpret_cast<const u4v *>(row + x0);
            lo[k] = row[xl]; hi[k] = row[xr];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int y = 2 * by + j;
            if (y >= H) break;
            const int cy = min(max(y, 1), H - 2);
            const bool up = cy - 1 - b0 != 0;                    // the evaluation row's three rows are r[1 .. 3], else r[0 .. 2]
            const u4v t = up ? r[1] : r[0], m = up ? r[2] : r[1], b = up ? r[3] : r[2];
            const uint32_t l3 = up ? lo[1] | (lo[2] << 8) | (lo[3] << 16) : lo[0] | (lo[1] << 8) | (lo[2] << 16);
            const uint32_t h3 = up ? hi[1] | (hi[2] << 8) | (hi[3] << 16) : hi[0] | (hi[1] << 8) | (hi[2] << 16);
            uint8_t *q = o + ((size_t)y * W + x0) * 3;
            if ((cy ^ BayerAt<LAYOUT>::RY) & 1) bayer_row16<LAYOUT, 1>(t, m, b, l3, h3, x0 == 0, x0 + 16 == W, q);
            else bayer_row16<LAYOUT, 0>(t, m, b, l3, h3, x0 == 0, x0 + 16 == W, q);
        }
    } else {
        if (i >= H * W) return;
        const int y = i / W, x = i - y * W;
        const int cy = min(max(y, 1), H - 2), cx = min(max(x, 1), W - 2);
        const uint8_t *m = f + (size_t)cy * (size_t)pitch + cx, *t = m - pitch, *b = m + pitch;
        const uint32_t p = bayer_site(t[-1] + b[-1], t[0] + b[0], t[1] + b[1], m[-1] + m[1], m[0], (cx ^ BayerAt<LAYOUT>::RX) & 1,
                                      (cy ^ BayerAt<LAYOUT>::RY) & 1);
        uint8_t *q = o + ((size_t)y * W + x) * 3;
        q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8); q[2] = (uint8_t)(p >> 16);
    }
}

// The taps of a dense W x H mosaic at `f`, demosaiced in the stored frame: pixels (sx, r) and (sx + 1, r) evaluate at clamped sites whose
// 3 x 3 windows lie in rows cy - 1 .. cy + 1 and the four columns c0 .. c0 + 3 -- one unaligned dword per row (W >= 4; three bytes when
// W == 3), never a byte outside the frame.
template <int LAYOUT>
struct BayerTaps {
    const uint8_t *__restrict__ f;
    int H, W;
    __device__ __forceinline__ void operator()(int r, int sx, bool second, uint32_t &t0, uint32_t &t1) const {
        const int cy = min(max(r, 1), H - 2);
        const int c0 = min(max(sx - 1, 0), max(W - 4, 0));
        const int cx0 = min(max(sx, 1), W - 2), cx1 = min(max(sx + 1, 1), W - 2);
        const uint8_t *m = f + (size_t)cy * W + c0;
        uint32_t wt, wm, wb;
        if (W >= 4) {
            wt = *reinterpret_cast<const u32u *>(m - W); wm = *reinterpret_cast<const u32u *>(m); wb = *reinterpret_cast<const u32u *>(m + W);
        } else {
            wt = (uint32_t)m[-W] | ((uint32_t)m[1 - W] << 8) | ((uint32_t)m[2 - W] << 16);
            wm = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16);
            wb = (uint32_t)m[W] | ((uint32_t)m[W + 1] << 8) | ((uint32_t)m[W + 2] << 16);
        }
        const int py = (cy ^ BayerAt<LAYOUT>::RY) & 1;
        int v[4], c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (int)((wt >> (8 * k)) & 255u) + (int)((wb >> (8 * k)) & 255u);
            c[k] = (int)((wm >> (8 * k)) & 255u);
        }
        const bool a = cx0 - 1 - c0 != 0;                        // the site's window is columns c0 + 1 .. c0 + 3, else c0 .. c0 + 2
        t0 = a ? bayer_site(v[1], v[2], v[3], c[1] + c[3], c[2], (cx0 ^ BayerAt<LAYOUT>::RX) & 1, py)
               : bayer_site(v[0], v[1], v[2], c[0] + c[2], c[1], (cx0 ^ BayerAt<LAYOUT>::RX) & 1, py);
        if (second) {
            const bool a1 = cx1 - 1 - c0 != 0;
            t1 = a1 ? bayer_site(v[1], v[2], v[3], c[1] + c[3], c[2], (cx1 ^ BayerAt<LAYOUT>::RX) & 1, py)
                    : bayer_site(v[0], v[1], v[2], c[0] + c[2], c[1], (cx1 ^ BayerAt<LAYOUT>::RX) & 1, py);
        } else t1 = t0;
    }
};

// The taps of a dense W x H monochrome frame at `f`: two adjacent bytes, one load where the row has both.
struct GrayTaps {
    const uint8_t *__restrict__ f;
    int W;
    __device__ __forceinline__ void operator()(int r, int sx, bool second, uint32_t &t0, uint32_t &t1) const {
        const uint8_t *p = f + (size_t)r * W + sx;
        if (second) { const uint32_t y = *reinterpret_cast<const u16u *>(p); t0 = (y & 255u) * 0x010101u; t1 = (y >> 8) * 0x010101u; }
        else t0 = t1 = (uint32_t)p[0] * 0x010101u;
    }
};

// yuv_resize_lane (resize_lane_dev.h) over those taps: the bytes of raw8_to_bgr_k followed by crop_resize, in one launch.
template <int LAYOUT, int NPX>
__global__ __launch_bounds__(256) void raw8_resize_k(const uint8_t *__restrict__ src, int H, int W, int flip, int oh, int ow,
                                                     uint8_t *__restrict__ out) {
    const uint8_t *f = src + (size_t)blockIdx.y * ((size_t)H * W);
    if constexpr (LAYOUT == RAW_GRAY) {
        const GrayTaps tap{f, W};
        yuv_resize_lane<NPX>(tap, H, W, flip, oh, ow, out);
    } else {
        const BayerTaps<LAYOUT> tap{f, H, W};
        yuv_resize_lane<NPX>(tap, H, W, flip, oh, ow, out);
    }
}

template <int LAYOUT>
int raw8_to_bgr_launch(hipStream_t s, bool wide, dim3 grid, const uint8_t *src, int H, int W, int pitch, int64_t frame_stride, uint8_t *dst) {
    if (wide) hipLaunchKernelGGL((raw8_to_bgr_k<LAYOUT, true>), grid, dim3(256), 0, s, src, H, W, pitch, frame_stride, dst);
    else hipLaunchKernelGGL((raw8_to_bgr_k<LAYOUT, false>), grid, dim3(256), 0, s, src, H, W, pitch, frame_stride, dst);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

template <int LAYOUT>
int raw8_resize_launch(hipStream_t s, bool quad, dim3 grid, const uint8_t *src, int H, int W, int flip, int oh, int ow, uint8_t *out) {
    if (quad) hipLaunchKernelGGL((raw8_resize_k<LAYOUT, 4>), grid, dim3(256), 0, s, src, H, W, flip, oh, ow, out);
    else hipLaunchKernelGGL((raw8_resize_k<LAYOUT, 1>), grid, dim3(256), 0, s, src, H, W, flip, oh, ow, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace

namespace ddk {

// layout 6 .. 9 Bayer, 10 gray; pitch / frame_stride 0 = dense (see dd_raw8_to_bgr).  The caller has checked layout, sizes and pitch.
int raw8_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t frame_stride, uint8_t *dst) {
    if (batch <= 0) return DD_OK;
    if (pitch == 0) pitch = W;
    if (frame_stride == 0) frame_stride = (int64_t)pitch * H;
    const bool wide = W % 16 == 0 && pitch % 16 == 0 && frame_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const int items = layout == RAW_GRAY ? H * (wide ? W / 16 : W) : wide ? ((H + 1) / 2) * (W / 16) : H * W;
    const dim3 grid(dd_ceil_div(items, 256), batch);
    switch (layout) {
    case RAW_RGGB: return raw8_to_bgr_launch<RAW_RGGB>(s, wide, grid, src, H, W, pitch, frame_stride, dst);
    case RAW_GRBG: return raw8_to_bgr_launch<RAW_GRBG>(s, wide, grid, src, H, W, pitch, frame_stride, dst);
    case RAW_GBRG: return raw8_to_bgr_launch<RAW_GBRG>(s, wide, grid, src, H, W, pitch, frame_stride, dst);
    case RAW_BGGR: return raw8_to_bgr_launch<RAW_BGGR>(s, wide, grid, src, H, W, pitch, frame_stride, dst);
    default: return raw8_to_bgr_launch<RAW_GRAY>(s, wide, grid, src, H, W, pitch, frame_stride, dst);
    }
}

// n dense frames [H][W] -> BGR [n][oh][ow][3], rows read bottom-up when `flip`.
int raw8_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int layout, int flip, int oh, int ow, uint8_t *out) {
    if (n <= 0) return DD_OK;
    const bool quad = ow % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const dim3 grid(dd_ceil_div(oh * (quad ? ow / 4 : ow), 256), n);
    switch (layout) {
    case RAW_RGGB: return raw8_resize_launch<RAW_RGGB>(s, quad, grid, src, H, W, flip, oh, ow, out);
    case RAW_GRBG: return raw8_resize_launch<RAW_GRBG>(s, quad, grid, src, H, W, flip, oh, ow, out);
    case RAW_GBRG: return raw8_resize_launch<RAW_GBRG>(s, quad, grid, src, H, W, flip, oh, ow, out);
    case RAW_BGGR: return raw8_resize_launch<RAW_BGGR>(s, quad, grid, src, H, W, flip, oh, ow, out);
    default: return raw8_resize_launch<RAW_GRAY>(s, quad, grid, src, H, W, flip, oh, ow, out);
    }
}

}  // namespace ddk

extern "C" {

// Every argument is checked before ctx is touched: a bad call is answered with a code on a machine without a GPU.
int dd_raw8_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t frame_stride, uint8_t *dst,
                   void *stream) {
    DD_REQUIRE(layout >= RAW_RGGB && layout <= RAW_GRAY, DD_E_ARG,
               "dd_raw8_to_bgr: layout %d is none of 6 (RGGB), 7 (GRBG), 8 (GBRG), 9 (BGGR), 10 (gray)", layout);
    DD_REQUIRE(batch >= 0 && batch <= 65535, DD_E_ARG, "dd_raw8_to_bgr: batch %d outside 0..65535", batch);
    const int least = layout == RAW_GRAY ? 1 : 3;
    DD_REQUIRE(W >= least, DD_E_ARG, "dd_raw8_to_bgr: W %d below %d%s", W, least, least == 3 ? " (a demosaiced site needs both neighbours)" : "");
    DD_REQUIRE(H >= least, DD_E_ARG, "dd_raw8_to_bgr: H %d below %d%s", H, least, least == 3 ? " (a demosaiced site needs both neighbours)" : "");
    DD_REQUIRE((int64_t)H * W <= INT_MAX - 256, DD_E_ARG, "dd_raw8_to_bgr: H %d x W %d is more pixels than a launch indexes", H, W);
    DD_REQUIRE(pitch == 0 || pitch >= W, DD_E_ARG, "dd_raw8_to_bgr: pitch %d below W %d", pitch, W);
    const int64_t p = pitch ? pitch : W, extent = p * (H - 1) + W;
    DD_REQUIRE(frame_stride == 0 || frame_stride >= extent, DD_E_ARG, "dd_raw8_to_bgr: frame_stride %lld below a frame's %lld bytes",
               (long long)frame_stride, (long long)extent);
    DD_REQUIRE(ctx, DD_E_ARG, "dd_raw8_to_bgr: NULL ctx");
    DD_DEVICE(ctx);
    if (batch == 0) return DD_OK;
    DD_REQUIRE(src && dst, DD_E_ARG, "dd_raw8_to_bgr: NULL argument");
    return ddk::raw8_to_bgr(dd_pick_stream(ctx, stream), src, batch, H, W, layout, pitch, frame_stride, dst);
}

}  // extern "C"
