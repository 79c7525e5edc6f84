// The convert + flip + stretch lane shared by the resize kernels of yuv.hip and bayer.hip, and the byte types their loads and stores use.
#pragma once
#include <cstdint>
#include "resize_dev.h"

namespace {

typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint16_t u16u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));

// Convert + flip + stretch of whole dense frames: every source tap is converted to saturated BGR bytes first, then the arithmetic of
// crop_resize_k / crop_resize4_k (image.hip) runs on those bytes -- lin_coeff, 11-bit coefficients, the exact-2x INTER_AREA shortcut --
// so the result is what the stand-alone converter followed by crop_resize gives, byte for byte, without the BGR frame ever reaching HBM.
// grid (ceil(oh * (ow / NPX) / 256), n); a lane owns NPX (4: ow % 4 == 0, twelve bytes leave as three dwords; or 1) output pixels of a row.
// `tap(r, sx, second, t0, t1)` gives pixels (sx, r) and (sx + 1, r) of frame blockIdx.y, converted; `out` is [n][oh][ow][3].
template <int NPX, class Taps>
__device__ __forceinline__ void yuv_resize_lane(const Taps &tap, int H, int W, int flip, int oh, int ow, uint8_t *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int qpr = ow / NPX;
    if (q >= oh * qpr) return;
    const int dy = q / qpr, dx0 = (q - dy * qpr) * NPX;
    uint8_t *o = out + (((size_t)blockIdx.y * oh + dy) * ow + dx0) * 3;
    const bool area = W == 2 * ow && H == 2 * oh;                // exact 2x decimation: INTER_AREA shortcut
    int sy, ya0 = 0, ya1 = 0, sy1;
    if (area) { sy = 2 * dy; sy1 = sy + 1; }
    else { lin_coeff(dy, oh, H, sy, ya0, ya1); sy1 = min(sy + 1, H - 1); }
    // flip: row y of the (virtually) flipped BGR frame is stored row H-1-y, whose chroma is that of the STORED row (convert, then flip)
    const int r0 = flip ? H - 1 - sy : sy, r1 = flip ? H - 1 - sy1 : sy1;
    uint8_t px[NPX][3];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        int sx, xa0 = 0, xa1 = 0;
        bool second = true;
        if (area) sx = 2 * (dx0 + i);
        else { lin_coeff(dx0 + i, ow, W, sx, xa0, xa1); second = sx + 1 <= W - 1; }      // at the right edge both taps are pixel sx
        uint32_t t00, t01, t10, t11;
        tap(r0, sx, second, t00, t01);
        tap(r1, sx, second, t10, t11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int p00 = (int)((t00 >> (8 * c)) & 255u), p01 = (int)((t01 >> (8 * c)) & 255u);
            const int p10 = (int)((t10 >> (8 * c)) & 255u), p11 = (int)((t11 >> (8 * c)) & 255u);
            if (area) {
                px[i][c] = (uint8_t)((p00 + p01 + p10 + p11 + 2) >> 2);
            } else {
                const int h0 = p00 * xa0 + p01 * xa1;            // scale 2^11
                const int h1 = p10 * xa0 + p11 * xa1;
                const int v = (((ya0 * (h0 >> 4)) >> 16) + ((ya1 * (h1 >> 4)) >> 16) + 2) >> 2;
                px[i][c] = (uint8_t)min(max(v, 0), 255);
            }
        }
    }
    if constexpr (NPX == 4) {
        const uint8_t *b = &px[0][0];
        uint32_t *ow32 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            ow32[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
    } else {
        o[0] = px[0][0]; o[1] = px[0][1]; o[2] = px[0][2];
    }
}

}  // namespace
