// 4:2:0 YUV (NV12 / I420) -> BGR u8, what a decoder hands out -> what the pipeline reads (u8, integer arithmetic, HBM-bound):
//   * yuv420_to_bgr_k   the stand-alone converter, cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420)
//   * yuv420_resize_k   convert + cv2.flip(frame, 0) + cv2.resize(frame, input_size) in one launch (the ingest ring's transform)
// The arithmetic is OpenCV's published BT.601 fixed-point form (20 fractional bits), restated -- OpenCV itself is absent, so parity with
// it is unpinned like every other cv2 arithmetic here; tests/yuv_ref.py is the numpy restatement the kernels are held to bit for bit.
//   NV12: H rows of luma, then H/2 rows of interleaved U,V pairs.   I420: H rows of luma, then the U plane, then the V plane.
// The chroma sample of pixel (x, y) is that of block (x >> 1, y >> 1): no chroma interpolation.
//
// Packed 4:2:2 (YUY2 / UYVY), what a UVC / V4L2 camera or a capture card delivers raw, with the same per-pixel arithmetic:
//   * yuv422_to_bgr_k   cv2.cvtColor(frame, COLOR_YUV2BGR_YUY2 / COLOR_YUV2BGR_UYVY); tests/yuv422_ref.py is its definition
//   * yuv422_resize_k   convert + flip + resize in one launch, the lane of yuv420_resize_k over another tap fetch
//   A row of W pixels is 2 W bytes of 4-byte macropixels, YUY2: Y0 U Y1 V, UYVY: U Y0 V Y1; both pixels of a macropixel share its chroma,
//   every row carries its own (H may be odd).
#include <climits>
#include <cstdlib>
#include "common.h"
#include "resize_lane_dev.h"

namespace {

constexpr int YUV_NV12 = 1, YUV_I420 = 2, YUV_YUY2 = 4, YUV_UYVY = 5;      // the ingest ring's pixel_format codes (3 is its JPEG ring)
constexpr int YUV_SHIFT = 20;
constexpr int YUV_CY = 1220542, YUV_CVR = 1673527, YUV_CVG = -852492, YUV_CUG = -409993, YUV_CUB = 2116026;
// rounding term and the -128 of both chroma samples folded into one constant per channel: R = (c + CVR * V + KR) >> 20 ...
constexpr int YUV_KR = (1 << (YUV_SHIFT - 1)) - 128 * YUV_CVR;
constexpr int YUV_KG = (1 << (YUV_SHIFT - 1)) - 128 * YUV_CVG - 128 * YUV_CUG;
constexpr int YUV_KB = (1 << (YUV_SHIFT - 1)) - 128 * YUV_CUB;

// Four values -> sat8(v >> 20) each, packed into a word: two v_ashr_pk_u8_i32 (D[7:0] = sat_u8(S0 >> S2), D[15:8] = sat_u8(S1 >> S2) into the
// half of D that op_sel[3] names, the other half kept) instead of twelve shift / min / max / shift / or.  Written out because hipcc's own use of
// the instruction assumes zeros in the half it keeps (image.hip, lanczos_v4_k).  Operands are ordinary VALU results: no wait states needed.
__device__ __forceinline__ uint32_t yuv_pack4(int v0, int v1, int v2, int v3) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v0), "v"(v1), "v"(YUV_SHIFT));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(r) : "v"(v2), "v"(v3), "v"(YUV_SHIFT));
    return r;
#else
    return 0;
#endif
}

// The chroma part of a 2x2 block's three channels (every product fits the 24-bit multiplier: coefficients < 2^23, samples < 2^8).
struct YuvChroma { int r, g, b; };
__device__ __forceinline__ YuvChroma yuv_chroma(int U, int V) {
    YuvChroma t;
    t.r = __mul24(V, YUV_CVR) + YUV_KR;
    t.g = __mul24(V, YUV_CVG) + __mul24(U, YUV_CUG) + YUV_KG;
    t.b = __mul24(U, YUV_CUB) + YUV_KB;
    return t;
}
__device__ __forceinline__ int yuv_luma(int Y) { return __mul24(max(Y - 16, 0), YUV_CY); }

// One pixel -> B | G << 8 | R << 16 (saturated bytes).
__device__ __forceinline__ uint32_t yuv_bgr(int Y, int U, int V) {
    const YuvChroma t = yuv_chroma(U, V);
    const int c = yuv_luma(Y);
    return yuv_pack4(c + t.b, c + t.g, c + t.r, 0);
}

// grid (ceil(items / 256), batch).  WIDE: W % 16 == 0 and every row 16-byte aligned (the launcher checks) -- an item is 16 pixels of two
// rows: two 16-byte luma loads, 16 bytes of chroma (NV12: one load, I420: 8 + 8), 2 x three 16-byte stores; 4.5 bytes of traffic per pixel
// and nothing else.  Otherwise an item is one 2x2 block, byte by byte: any even W and H.
template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(256) void yuv420_to_bgr_k(const uint8_t *__restrict__ src, int H, int W, int pitch, int64_t chroma_offset,
                                                       int64_t frame_stride, uint8_t *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ipr = WIDE ? W >> 4 : W >> 1;                      // items per row pair
    if (i >= (H >> 1) * ipr) return;
    const int by = i / ipr, bx = i - by * ipr;
    const uint8_t *f = src + (size_t)blockIdx.y * (size_t)frame_stride;
    const uint8_t *ch = f + chroma_offset;
    const int cpitch = pitch >> 1;                               // I420 chroma rows
    uint8_t *o = dst + (((size_t)blockIdx.y * H + 2 * by) * W) * 3;
    if constexpr (WIDE) {
        const uint8_t *yp = f + (size_t)(2 * by) * pitch + 16 * bx;
        const u4v y0 = *reinterpret_cast<const u4v *>(yp), y1 = *reinterpret_cast<const u4v *>(yp + pitch);
        uint32_t uw[4], vw[4];                                   // NV12: uw[j] = U V U V of pairs 2j, 2j + 1; I420: uw / vw[j] = four samples
        if constexpr (LAYOUT == YUV_NV12) {
            const u4v c = *reinterpret_cast<const u4v *>(ch + (size_t)by * pitch + 16 * bx);
#pragma unroll
            for (int j = 0; j < 4; ++j) uw[j] = c[j];
        } else {
            const uint8_t *up = ch + (size_t)by * cpitch + 8 * bx;
            const u2v u = *reinterpret_cast<const u2v *>(up), v = *reinterpret_cast<const u2v *>(up + (size_t)cpitch * (H >> 1));
            uw[0] = u[0]; uw[1] = u[1]; vw[0] = v[0]; vw[1] = v[1];
        }
        YuvChroma t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int U, V;
            if constexpr (LAYOUT == YUV_NV12) {
                U = (int)((uw[k >> 1] >> (16 * (k & 1))) & 255u);
                V = (int)((uw[k >> 1] >> (16 * (k & 1) + 8)) & 255u);
            } else {
                U = (int)((uw[k >> 2] >> (8 * (k & 3))) & 255u);
                V = (int)((vw[k >> 2] >> (8 * (k & 3))) & 255u);
            }
            t[k] = yuv_chroma(U, V);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const u4v y = r ? y1 : y0;
            int val[48];                                         // the row's 48 output values before the shift, in byte order
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int c = yuv_luma((int)((y[x >> 2] >> (8 * (x & 3))) & 255u));
                val[3 * x] = c + t[x >> 1].b; val[3 * x + 1] = c + t[x >> 1].g; val[3 * x + 2] = c + t[x >> 1].r;
            }
            u4v *op = reinterpret_cast<u4v *>(o + (size_t)r * W * 3 + 48 * bx);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                u4v q;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b = 16 * w + 4 * j;
                    q[j] = yuv_pack4(val[b], val[b + 1], val[b + 2], val[b + 3]);
                }
                op[w] = q;
            }
        }
    } else {
        const uint8_t *yp = f + (size_t)(2 * by) * pitch + 2 * bx;
        int U, V;
        if constexpr (LAYOUT == YUV_NV12) {
            const uint8_t *cp = ch + (size_t)by * pitch + 2 * bx;
            U = cp[0]; V = cp[1];
        } else {
            const uint8_t *up = ch + (size_t)by * cpitch + bx;
            U = up[0]; V = up[(size_t)cpitch * (H >> 1)];
        }
        const YuvChroma t = yuv_chroma(U, V);
        o += (size_t)(2 * bx) * 3;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const int c = yuv_luma(yp[(size_t)r * pitch + x]);
                const uint32_t p = yuv_pack4(c + t.b, c + t.g, c + t.r, 0);
                uint8_t *q = o + ((size_t)r * W + x) * 3;
                q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8); q[2] = (uint8_t)(p >> 16);
            }
    }
}

// Pixels (sx, r) and (sx + 1, r) of a dense W x H frame at `f`, converted: t0, t1 = B | G << 8 | R << 16.  `second` false: the right edge,
// both taps are pixel sx.  Two adjacent pixels are two adjacent luma bytes and at most two adjacent chroma blocks: one load each where the
// row has the bytes, never one past the row's end.
template <int LAYOUT>
__device__ __forceinline__ void yuv_tap_pair(const uint8_t *__restrict__ f, int H, int W, int r, int sx, bool second, uint32_t &t0, uint32_t &t1) {
    const uint8_t *yp = f + (size_t)r * W + sx;
    int Y0, Y1;
    if (second) { const uint32_t y = *reinterpret_cast<const u16u *>(yp); Y0 = (int)(y & 255u); Y1 = (int)(y >> 8); }
    else Y0 = Y1 = yp[0];
    int U0, V0, U1, V1;
    const uint8_t *ch = f + (size_t)H * W;
    if constexpr (LAYOUT == YUV_NV12) {
        const int cx = sx & ~1;
        const uint8_t *cp = ch + (size_t)(r >> 1) * W + cx;
        uint32_t c;
        if (cx + 4 <= W) c = *reinterpret_cast<const u32u *>(cp);
        else { c = *reinterpret_cast<const u16u *>(cp); c |= c << 16; }
        U0 = (int)(c & 255u); V0 = (int)((c >> 8) & 255u);
        U1 = (sx & 1) ? (int)((c >> 16) & 255u) : U0; V1 = (sx & 1) ? (int)(c >> 24) : V0;
    } else {
        const int cw = W >> 1, cx = sx >> 1;
        const uint8_t *up = ch + (size_t)(r >> 1) * cw + cx, *vp = up + (size_t)cw * (H >> 1);
        uint32_t u, v;
        if (cx + 2 <= cw) { u = *reinterpret_cast<const u16u *>(up); v = *reinterpret_cast<const u16u *>(vp); }
        else { u = up[0]; u |= u << 8; v = vp[0]; v |= v << 8; }
        U0 = (int)(u & 255u); V0 = (int)(v & 255u);
        U1 = (sx & 1) ? (int)(u >> 8) : U0; V1 = (sx & 1) ? (int)(v >> 8) : V0;
    }
    t0 = yuv_bgr(Y0, U0, V0);
    t1 = second ? yuv_bgr(Y1, U1, V1) : t0;
}

// The taps of a dense NV12 / I420 frame at `f`.
template <int LAYOUT>
struct Yuv420Taps {
    const uint8_t *__restrict__ f;
    int H, W;
    __device__ __forceinline__ void operator()(int r, int sx, bool second, uint32_t &t0, uint32_t &t1) const {
        yuv_tap_pair<LAYOUT>(f, H, W, r, sx, second, t0, t1);
    }
};

// Macropixel word (little-endian load of its four bytes) -> its samples.
template <int ORDER> __device__ __forceinline__ int yuv422_y0(uint32_t w) { return (int)((ORDER == YUV_YUY2 ? w : w >> 8) & 255u); }
template <int ORDER> __device__ __forceinline__ int yuv422_y1(uint32_t w) { return (int)((ORDER == YUV_YUY2 ? w >> 16 : w >> 24) & 255u); }
template <int ORDER> __device__ __forceinline__ int yuv422_u(uint32_t w) { return (int)((ORDER == YUV_YUY2 ? w >> 8 : w) & 255u); }
template <int ORDER> __device__ __forceinline__ int yuv422_v(uint32_t w) { return (int)((ORDER == YUV_YUY2 ? w >> 24 : w >> 16) & 255u); }

// The taps of a dense YUY2 / UYVY frame at `f` (rows of 2 W bytes): pixels sx and sx + 1 are one macropixel when sx is even, else the second
// half of one and the first half of the next -- which the row has whenever pixel sx + 1 exists (W is even).  Never a byte past the row.
template <int ORDER>
struct Yuv422Taps {
    const uint8_t *__restrict__ f;
    int W;
    __device__ __forceinline__ void operator()(int r, int sx, bool second, uint32_t &t0, uint32_t &t1) const {
        const uint8_t *mp = f + (size_t)r * (2 * (size_t)W) + 4 * (size_t)(sx >> 1);
        const uint32_t w0 = *reinterpret_cast<const u32u *>(mp);
        const int U0 = yuv422_u<ORDER>(w0), V0 = yuv422_v<ORDER>(w0);
        if (!(sx & 1)) {
            t0 = yuv_bgr(yuv422_y0<ORDER>(w0), U0, V0);
            t1 = second ? yuv_bgr(yuv422_y1<ORDER>(w0), U0, V0) : t0;
        } else {
            t0 = yuv_bgr(yuv422_y1<ORDER>(w0), U0, V0);
            if (second) {
                const uint32_t w1 = *reinterpret_cast<const u32u *>(mp + 4);
                t1 = yuv_bgr(yuv422_y0<ORDER>(w1), yuv422_u<ORDER>(w1), yuv422_v<ORDER>(w1));
            } else t1 = t0;
        }
    }
};

// yuv_resize_lane (resize_lane_dev.h) over those taps: convert + flip + stretch of whole dense frames in one launch.
template <int LAYOUT, int NPX>
__global__ __launch_bounds__(256) void yuv420_resize_k(const uint8_t *__restrict__ src, int H, int W, int flip, int oh, int ow,
                                                       uint8_t *__restrict__ out) {
    const Yuv420Taps<LAYOUT> tap{src + (size_t)blockIdx.y * ((size_t)H * W * 3 / 2), H, W};
    yuv_resize_lane<NPX>(tap, H, W, flip, oh, ow, out);
}

template <int ORDER, int NPX>
__global__ __launch_bounds__(256) void yuv422_resize_k(const uint8_t *__restrict__ src, int H, int W, int flip, int oh, int ow,
                                                       uint8_t *__restrict__ out) {
    const Yuv422Taps<ORDER> tap{src + (size_t)blockIdx.y * ((size_t)H * W * 2), W};
    yuv_resize_lane<NPX>(tap, H, W, flip, oh, ow, out);
}

// grid (ceil(items / 256), batch).  WIDE: W % 16 == 0 and every row of both sides 16-byte aligned (the launcher checks) -- an item is 16
// pixels of one row: two 16-byte loads (eight macropixels), three 16-byte stores; 5 bytes of traffic per pixel and nothing else.
// Otherwise an item is one macropixel, byte by byte: any even W.  Rows and frames are addressed in 64 bits.
template <int ORDER, bool WIDE>
__global__ __launch_bounds__(256) void yuv422_to_bgr_k(const uint8_t *__restrict__ src, int H, int W, int pitch, int64_t frame_stride,
                                                       uint8_t *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ipr = WIDE ? W >> 4 : W >> 1;                      // items per row
    if (i >= H * ipr) return;
    const int y = i / ipr, bx = i - y * ipr;
    const uint8_t *row = src + (size_t)blockIdx.y * (size_t)frame_stride + (size_t)y * (size_t)pitch;
    uint8_t *o = dst + (((size_t)blockIdx.y * H + y) * W) * 3;
    if constexpr (WIDE) {
        const u4v *sp = reinterpret_cast<const u4v *>(row + 32 * (size_t)bx);
        const u4v m0 = sp[0], m1 = sp[1];
        int val[48];                                             // the 48 output values before the shift, in byte order
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t w = k < 4 ? m0[k & 3] : m1[k & 3];
            const YuvChroma t = yuv_chroma(yuv422_u<ORDER>(w), yuv422_v<ORDER>(w));
            const int c0 = yuv_luma(yuv422_y0<ORDER>(w)), c1 = yuv_luma(yuv422_y1<ORDER>(w));
            val[6 * k] = c0 + t.b; val[6 * k + 1] = c0 + t.g; val[6 * k + 2] = c0 + t.r;
            val[6 * k + 3] = c1 + t.b; val[6 * k + 4] = c1 + t.g; val[6 * k + 5] = c1 + t.r;
        }
        u4v *op = reinterpret_cast<u4v *>(o + 48 * (size_t)bx);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            u4v q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = 16 * w + 4 * j;
                q[j] = yuv_pack4(val[b], val[b + 1], val[b + 2], val[b + 3]);
            }
            op[w] = q;
        }
    } else {
        const uint8_t *mp = row + 4 * (size_t)bx;
        const uint32_t w = (uint32_t)mp[0] | ((uint32_t)mp[1] << 8) | ((uint32_t)mp[2] << 16) | ((uint32_t)mp[3] << 24);
        const YuvChroma t = yuv_chroma(yuv422_u<ORDER>(w), yuv422_v<ORDER>(w));
        const int c0 = yuv_luma(yuv422_y0<ORDER>(w)), c1 = yuv_luma(yuv422_y1<ORDER>(w));
        const uint32_t p0 = yuv_pack4(c0 + t.b, c0 + t.g, c0 + t.r, 0), p1 = yuv_pack4(c1 + t.b, c1 + t.g, c1 + t.r, 0);
        uint8_t *q = o + 6 * (size_t)bx;
        q[0] = (uint8_t)p0; q[1] = (uint8_t)(p0 >> 8); q[2] = (uint8_t)(p0 >> 16);
        q[3] = (uint8_t)p1; q[4] = (uint8_t)(p1 >> 8); q[5] = (uint8_t)(p1 >> 16);
    }
}

}  // namespace

namespace ddk {

// pitch / chroma_offset / frame_stride: 0 means dense (see dd_yuv420_to_bgr).  The caller has checked layout, even sizes and pitch.
int yuv420_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t chroma_offset,
                  int64_t frame_stride, uint8_t *dst) {
    if (batch <= 0) return DD_OK;
    if (pitch == 0) pitch = W;
    if (chroma_offset == 0) chroma_offset = (int64_t)pitch * H;
    if (frame_stride == 0) frame_stride = chroma_offset + (layout == YUV_NV12 ? (int64_t)pitch : (int64_t)(pitch / 2) * 2) * (H / 2);
    const bool wide = W % 16 == 0 && pitch % 16 == 0 && chroma_offset % 16 == 0 && frame_stride % 16 == 0 &&
                      ((int64_t)(pitch / 2) * (H / 2)) % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const dim3 grid(dd_ceil_div((H / 2) * (wide ? W / 16 : W / 2), 256), batch), block(256);
    if (layout == YUV_NV12) {
        if (wide) hipLaunchKernelGGL((yuv420_to_bgr_k<YUV_NV12, true>), grid, block, 0, s, src, H, W, pitch, chroma_offset, frame_stride, dst);
        else hipLaunchKernelGGL((yuv420_to_bgr_k<YUV_NV12, false>), grid, block, 0, s, src, H, W, pitch, chroma_offset, frame_stride, dst);
    } else {
        if (wide) hipLaunchKernelGGL((yuv420_to_bgr_k<YUV_I420, true>), grid, block, 0, s, src, H, W, pitch, chroma_offset, frame_stride, dst);
        else hipLaunchKernelGGL((yuv420_to_bgr_k<YUV_I420, false>), grid, block, 0, s, src, H, W, pitch, chroma_offset, frame_stride, dst);
    }
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// n dense frames [H * 3 / 2][W] -> BGR [n][oh][ow][3], rows read bottom-up when `flip`.
int yuv420_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int layout, int flip, int oh, int ow, uint8_t *out) {
    if (n <= 0) return DD_OK;
    const bool quad = ow % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const dim3 grid(dd_ceil_div(oh * (quad ? ow / 4 : ow), 256), n), block(256);
    if (layout == YUV_NV12) {
        if (quad) hipLaunchKernelGGL((yuv420_resize_k<YUV_NV12, 4>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
        else hipLaunchKernelGGL((yuv420_resize_k<YUV_NV12, 1>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
    } else {
        if (quad) hipLaunchKernelGGL((yuv420_resize_k<YUV_I420, 4>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
        else hipLaunchKernelGGL((yuv420_resize_k<YUV_I420, 1>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
    }
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// order 4 YUY2, 5 UYVY; pitch / frame_stride 0 = dense (see dd_yuv422_to_bgr).  The caller has checked order, sizes and pitch.
int yuv422_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int order, int pitch, int64_t frame_stride, uint8_t *dst) {
    if (batch <= 0) return DD_OK;
    if (pitch == 0) pitch = 2 * W;
    if (frame_stride == 0) frame_stride = (int64_t)pitch * H;
    const bool wide = W % 16 == 0 && pitch % 16 == 0 && frame_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const dim3 grid(dd_ceil_div(H * (wide ? W / 16 : W / 2), 256), batch), block(256);
    if (order == YUV_YUY2) {
        if (wide) hipLaunchKernelGGL((yuv422_to_bgr_k<YUV_YUY2, true>), grid, block, 0, s, src, H, W, pitch, frame_stride, dst);
        else hipLaunchKernelGGL((yuv422_to_bgr_k<YUV_YUY2, false>), grid, block, 0, s, src, H, W, pitch, frame_stride, dst);
    } else {
        if (wide) hipLaunchKernelGGL((yuv422_to_bgr_k<YUV_UYVY, true>), grid, block, 0, s, src, H, W, pitch, frame_stride, dst);
        else hipLaunchKernelGGL((yuv422_to_bgr_k<YUV_UYVY, false>), grid, block, 0, s, src, H, W, pitch, frame_stride, dst);
    }
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// n dense frames [H][W][2] -> BGR [n][oh][ow][3], rows read bottom-up when `flip`.
int yuv422_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int order, int flip, int oh, int ow, uint8_t *out) {
    if (n <= 0) return DD_OK;
    const bool quad = ow % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const dim3 grid(dd_ceil_div(oh * (quad ? ow / 4 : ow), 256), n), block(256);
    if (order == YUV_YUY2) {
        if (quad) hipLaunchKernelGGL((yuv422_resize_k<YUV_YUY2, 4>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
        else hipLaunchKernelGGL((yuv422_resize_k<YUV_YUY2, 1>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
    } else {
        if (quad) hipLaunchKernelGGL((yuv422_resize_k<YUV_UYVY, 4>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
        else hipLaunchKernelGGL((yuv422_resize_k<YUV_UYVY, 1>), grid, block, 0, s, src, H, W, flip, oh, ow, out);
    }
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

extern "C" {

int dd_yuv420_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t chroma_offset,
                     int64_t frame_stride, uint8_t *dst, void *stream) {
    DD_REQUIRE(ctx, DD_E_ARG, "dd_yuv420_to_bgr: NULL ctx");
    DD_REQUIRE(layout == YUV_NV12 || layout == YUV_I420, DD_E_ARG, "dd_yuv420_to_bgr: layout %d is neither 1 (NV12) nor 2 (I420)", layout);
    DD_REQUIRE(batch >= 0 && batch <= 65535, DD_E_ARG, "dd_yuv420_to_bgr: batch %d outside 0..65535", batch);
    DD_REQUIRE(W >= 2 && W % 2 == 0, DD_E_ARG, "dd_yuv420_to_bgr: W %d must be even and positive (4:2:0 chroma)", W);
    DD_REQUIRE(H >= 2 && H % 2 == 0, DD_E_ARG, "dd_yuv420_to_bgr: H %d must be even and positive (4:2:0 chroma)", H);
    DD_REQUIRE(pitch == 0 || pitch >= W, DD_E_ARG, "dd_yuv420_to_bgr: pitch %d below W %d", pitch, W);
    DD_REQUIRE(layout != YUV_I420 || pitch % 2 == 0, DD_E_ARG, "dd_yuv420_to_bgr: pitch %d must be even for I420 (chroma rows use pitch / 2)", pitch);
    const int64_t p = pitch ? pitch : W;
    DD_REQUIRE(chroma_offset == 0 || chroma_offset >= p * (H - 1) + W, DD_E_ARG, "dd_yuv420_to_bgr: chroma_offset %lld inside the luma plane",
               (long long)chroma_offset);
    const int64_t co = chroma_offset ? chroma_offset : p * H;
    const int64_t extent = layout == YUV_NV12 ? co + p * (H / 2 - 1) + W : co + (p / 2) * (H / 2) + (p / 2) * (H / 2 - 1) + W / 2;
    DD_REQUIRE(frame_stride == 0 || frame_stride >= extent, DD_E_ARG, "dd_yuv420_to_bgr: frame_stride %lld below a frame's %lld bytes",
               (long long)frame_stride, (long long)extent);
    DD_DEVICE(ctx);
    if (batch == 0) return DD_OK;
    DD_REQUIRE(src && dst, DD_E_ARG, "dd_yuv420_to_bgr: NULL argument");
    return ddk::yuv420_to_bgr(dd_pick_stream(ctx, stream), src, batch, H, W, layout, pitch, chroma_offset, frame_stride, dst);
}

// Every argument is checked before ctx is touched: a bad call is answered with a code on a machine without a GPU.
int dd_yuv422_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int order, int pitch, int64_t frame_stride, uint8_t *dst,
                     void *stream) {
    DD_REQUIRE(order == YUV_YUY2 || order == YUV_UYVY, DD_E_ARG, "dd_yuv422_to_bgr: order %d is neither 4 (YUY2) nor 5 (UYVY)", order);
    DD_REQUIRE(batch >= 0 && batch <= 65535, DD_E_ARG, "dd_yuv422_to_bgr: batch %d outside 0..65535", batch);
    DD_REQUIRE(W >= 2 && W % 2 == 0, DD_E_ARG, "dd_yuv422_to_bgr: W %d must be even and positive (4:2:2 macropixels)", W);
    DD_REQUIRE(H >= 1, DD_E_ARG, "dd_yuv422_to_bgr: H %d must be positive", H);
    DD_REQUIRE((int64_t)H * (W / 2) <= INT_MAX - 256, DD_E_ARG, "dd_yuv422_to_bgr: H %d x W %d is more macropixels than a launch indexes", H, W);
    DD_REQUIRE(pitch == 0 || pitch >= 2 * (int64_t)W, DD_E_ARG, "dd_yuv422_to_bgr: pitch %d below 2 W = %lld", pitch, 2 * (long long)W);
    const int64_t p = pitch ? pitch : 2 * (int64_t)W, extent = p * (H - 1) + 2 * (int64_t)W;
    DD_REQUIRE(p <= INT_MAX, DD_E_ARG, "dd_yuv422_to_bgr: W %d needs a pitch above INT_MAX", W);
    DD_REQUIRE(frame_stride == 0 || frame_stride >= extent, DD_E_ARG, "dd_yuv422_to_bgr: frame_stride %lld below a frame's %lld bytes",
               (long long)frame_stride, (long long)extent);
    DD_REQUIRE(ctx, DD_E_ARG, "dd_yuv422_to_bgr: NULL ctx");
    DD_DEVICE(ctx);
    if (batch == 0) return DD_OK;
    DD_REQUIRE(src && dst, DD_E_ARG, "dd_yuv422_to_bgr: NULL argument");
    return ddk::yuv422_to_bgr(dd_pick_stream(ctx, stream), src, batch, H, W, order, pitch, frame_stride, dst);
}

}  // extern "C"
