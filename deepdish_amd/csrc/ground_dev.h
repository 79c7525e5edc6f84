// Ground-plane unprojection of one image point, shared by the host entry and by ground_points_k (csrc/ground.hip).
// Floating-point contraction is off from here to the end of the including file: host and device then perform the same IEEE f64
// operations in the same order and agree bit for bit (tests/topdown_ref.py restates this order).
//
// Rectilinear camera at (0, 0, e), heading 0, tilt t (0 looks straight down, 90 deg at the horizon, towards +Y), roll r:
//   a = (u - cx) / fx              b = -(v - cy) / fy           the camera-frame ray (a, b, -1)
//   a' = cos r * a - sin r * b     b' = sin r * a + cos r * b   Rz(r)^T
//   den = cos t - sin t * b'                                    minus the ray's world Z after Rx(t)^T
//   X = e * a' / den               Y = e * (cos t * b' + sin t) / den
// den <= 0: the ray never reaches the ground -> (NaN, NaN); so does a non-finite input or result.  The NaN is one fixed quiet NaN.
#pragma once
#pragma clang fp contract(off)

// A camera as dd_ground_camera writes it: the trigonometry is done there, once.  Nine doubles: with no cosine or sine left to the kernel,
// fx, fy, cx, cy, e and the two pairs are nine independent numbers.
enum { GC_FX = 0, GC_FY, GC_CX, GC_CY, GC_E, GC_COS_T, GC_SIN_T, GC_COS_R, GC_SIN_R, GC_DOUBLES };

__host__ __device__ static inline void ground_from_image(const double *__restrict__ cam, double u, double v, double &X, double &Y) {
    const double a = (u - cam[GC_CX]) / cam[GC_FX];
    const double b = -(v - cam[GC_CY]) / cam[GC_FY];
    const double ar = cam[GC_COS_R] * a - cam[GC_SIN_R] * b;
    const double br = cam[GC_SIN_R] * a + cam[GC_COS_R] * b;
    const double den = cam[GC_COS_T] - cam[GC_SIN_T] * br;
    const double x = cam[GC_E] * ar / den;
    const double y = cam[GC_E] * (cam[GC_COS_T] * br + cam[GC_SIN_T]) / den;
    const bool ok = __builtin_isfinite(u) && __builtin_isfinite(v) && den > 0.0 && __builtin_isfinite(x) && __builtin_isfinite(y);
    X = ok ? x : __builtin_nan("");
    Y = ok ? y : __builtin_nan("");
}
