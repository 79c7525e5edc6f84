// Device-side pieces of the cv2.resize restatement shared by the resize kernels of image.hip and yuv.hip.
#pragma once
#include <cmath>

namespace {

// ------------------------------------------------------------------ cv2 INTER_LINEAR on u8
// OpenCV resize.cpp: coordinates in float, coefficients rounded to 11-bit shorts.
__device__ __forceinline__ void lin_coeff(int d, int dst, int src, int &s, int &a0, int &a1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)((d + 0.5) * scale - 0.5);
    int si = (int)floorf(f);
    f -= (float)si;
    if (si < 0) { f = 0.f; si = 0; }
    if (si >= src - 1) { f = 0.f; si = src - 1; }
    s = si;
    a0 = (int)rintf((1.f - f) * 2048.f);
    a1 = (int)rintf(f * 2048.f);
}

struct CropBox { int sx, sy, cw, ch, frame, flip, swap_rb, r2; };   // cw <= 0 marks a box the reference rejects; flip: rows read bottom-up (cv2.flip(frame, 0));
                                                                    // swap_rb: channels written in reverse order (a BGR frame resampled into the RGB a detector reads)

}  // namespace
