// Top-down view: image points -> metres on the ground plane (deepdish.py:592-611, :1088-1097 cam.spaceFromImage), a camera per point.
// The arithmetic is ground_dev.h, the same for the host loop and for the kernel.
//   ground_points_k   one lane per point, grid-stride.  A point is one 16-byte load and one 16-byte store.  Camera indices are uniform in
//                     runs (a stream's points lie behind one another), so a wave takes its first waiting lane's index, reads that camera
//                     through the scalar path (one 64-byte and one 8-byte scalar load) and serves every lane that shares it; one turn
//                     per distinct camera in the wave.  No LDS, no atomics.  An index outside the table reads nothing and yields NaN.
#include <cmath>
#include "common.h"
#include "ground_dev.h"

static_assert(GC_DOUBLES == DD_GROUND_CAMERA_DOUBLES, "the camera record of ground_dev.h and of the public header");

namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_BLOCKS_PER_CU = 8;      // the grid's cap: 2048 workgroups on 256 CUs, further points by the grid's stride

typedef double gp_f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(GP_THREADS) void ground_points_k(const double *__restrict__ cams, int n_cams, const int *__restrict__ cam_index,
                                                               const gp_f64x2 *__restrict__ points, gp_f64x2 *__restrict__ out, long long n) {
    const long long stride = (long long)gridDim.x * GP_THREADS;
    for (long long i = (long long)blockIdx.x * GP_THREADS + threadIdx.x; i < n; i += stride) {
        const int ci = cam_index ? cam_index[i] : 0;
        const gp_f64x2 p = points[i];
        gp_f64x2 r = {__builtin_nan(""), __builtin_nan("")};
        const bool valid = ci >= 0 && ci < n_cams;
        unsigned long long waiting = __ballot(valid);                 // the same in every lane: a scalar loop, one camera per turn
        while (waiting) {
            const int c = __builtin_amdgcn_readlane(ci, __builtin_ctzll(waiting));
            // The address is formed from a copy of c the optimiser cannot see through: inside `ci == c` it would otherwise put the lane's own
            // ci in c's place, and the nine doubles would come as per-lane vector loads instead of two scalar loads.
            int cu = c;
            asm volatile("" : "+s"(cu));
            const bool mine = valid && ci == c;
            if (mine) {
                double X, Y;
                ground_from_image(cams + (size_t)cu * GC_DOUBLES, p.x, p.y, X, Y);
                r.x = X; r.y = Y;
            }
            waiting &= ~__ballot(mine);
        }
        out[i] = r;
    }
}

bool gp_finite(double v) { return std::isfinite(v); }

}  // namespace

extern "C" {

int dd_ground_camera(double f_mm, double sensor_w_mm, double sensor_h_mm, int image_w, int image_h, double elevation_m, double tilt_deg,
                     double roll_deg, double *out) {
    DD_REQUIRE(out, DD_E_ARG, "dd_ground_camera: NULL argument");
    DD_REQUIRE(gp_finite(f_mm) && gp_finite(sensor_w_mm) && gp_finite(sensor_h_mm) && gp_finite(elevation_m) && gp_finite(tilt_deg) && gp_finite(roll_deg),
               DD_E_ARG, "dd_ground_camera: a non-finite value (f %g mm, sensor %g x %g mm, elevation %g m, tilt %g deg, roll %g deg)", f_mm, sensor_w_mm,
               sensor_h_mm, elevation_m, tilt_deg, roll_deg);
    DD_REQUIRE(f_mm > 0 && sensor_w_mm > 0 && sensor_h_mm > 0, DD_E_ARG, "dd_ground_camera: focal length %g mm and sensor %g x %g mm must be positive", f_mm,
               sensor_w_mm, sensor_h_mm);
    DD_REQUIRE(image_w > 0 && image_h > 0, DD_E_ARG, "dd_ground_camera: a %d x %d image", image_w, image_h);
    DD_REQUIRE(elevation_m > 0, DD_E_ARG, "dd_ground_camera: elevation %g m must be positive", elevation_m);
    const double t = tilt_deg * (M_PI / 180.0), r = roll_deg * (M_PI / 180.0);
    out[GC_FX] = f_mm / sensor_w_mm * image_w;
    out[GC_FY] = f_mm / sensor_h_mm * image_h;
    out[GC_CX] = image_w / 2.0;
    out[GC_CY] = image_h / 2.0;
    out[GC_E] = elevation_m;
    out[GC_COS_T] = std::cos(t); out[GC_SIN_T] = std::sin(t);
    out[GC_COS_R] = std::cos(r); out[GC_SIN_R] = std::sin(r);
    return DD_OK;
}

// cams: f64 [n_cams][9] as dd_ground_camera writes them; cam_index: int32 [n] or NULL (camera 0); points, out: f64 [n][2], sharing no
// byte.  on_device = 0: host arrays, computed here (ctx may be NULL), a camera index outside the table is DD_E_ARG before
// anything is written.  on_device = 1: all four arrays on the device, ground_points_k queued on `stream` (NULL: the context's); an index
// outside the table yields NaN for that point.
int dd_ground_from_image(dd_ctx *ctx, const double *cams, int n_cams, const int32_t *cam_index, const double *points, long long n, double *out,
                         int on_device, void *stream) {
    DD_REQUIRE(n >= 0 && n_cams > 0, DD_E_ARG, "dd_ground_from_image: %lld points, %d cameras", n, n_cams);
    if (n == 0) return DD_OK;
    DD_REQUIRE(cams && points && out, DD_E_ARG, "dd_ground_from_image: NULL argument");
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(points), b = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)n * 16;
        DD_REQUIRE(a + bytes <= b || b + bytes <= a, DD_E_ARG, "dd_ground_from_image: out overlaps points (it is written out of place)");
    }
    if (!on_device) {
        if (cam_index)
            for (long long i = 0; i < n; ++i)
                DD_REQUIRE(cam_index[i] >= 0 && cam_index[i] < n_cams, DD_E_ARG, "dd_ground_from_image: point %lld names camera %d of %d", i, cam_index[i], n_cams);
        for (long long i = 0; i < n; ++i) {
            double X, Y;
            ground_from_image(cams + (size_t)(cam_index ? cam_index[i] : 0) * GC_DOUBLES, points[2 * i], points[2 * i + 1], X, Y);
            out[2 * i] = X; out[2 * i + 1] = Y;
        }
        return DD_OK;
    }
    DD_REQUIRE(ctx, DD_E_ARG, "dd_ground_from_image: device arrays and no context");
    DD_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(cams) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(cam_index) & 3) == 0, DD_E_ARG, "dd_ground_from_image: points and out must be 16-byte aligned on the device");
    DD_DEVICE(ctx);
    hipStream_t s = dd_pick_stream(ctx, stream);
    const long long blocks = std::min<long long>((n + GP_THREADS - 1) / GP_THREADS, (long long)dd_cu_count(ctx->device) * GP_BLOCKS_PER_CU);
    hipLaunchKernelGGL(ground_points_k, dim3((unsigned)blocks), dim3(GP_THREADS), 0, s, cams, n_cams, cam_index, reinterpret_cast<const gp_f64x2 *>(points),
                       reinterpret_cast<gp_f64x2 *>(out), n);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // extern "C"
