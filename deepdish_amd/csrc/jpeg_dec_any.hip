// The pixel stage of the JPEG decoder for a DD_JPEGDEC_ANY_SIZE decoder: files of any size up to the decoder's, each at its own scale, each
// written into the top-left corner of a uniform slot.  csrc/jpeg_dec.hip describes the stages in front of this one; the call plan
// (csrc/jpeg_dec_plan.h) has decided every file's path and scale, has held its record to the decoder's strides, and says which scales
// occur (JdPerScale).  The kernels here are those of csrc/jpeg_dec.hip's pixel stage with the scale a template argument at 1 as well, a
// slot pitch, and a test that passes over the files of another scale; the device functions are shared (csrc/jpeg_dec_pix.h).  They have
// a translation unit of their own because they are a separate family of eight kernels that only this option launches.
#include "common.h"
#include "jpeg_dec_dev.h"
#include "jpeg_dec_pix.h"
#include "jpeg_dec_plan.h"

namespace {

// A record's path holds the path and the log2 of the file's scale (jd_path_pack); the frame is the top-left ceil(h / S) x ceil(w / S) of a
// slot of OH x OW whose rows are OW * 3 bytes apart.  The planes and the coefficients keep the file's own dense layout inside the
// decoder's strides, which bound every accepted file's (the plan checks that on the host).

template <int S>
__device__ __forceinline__ bool jd_any_mine(const dd_jpeg_info &r, int path) {
    return r.path == jd_path_pack(path, jd_scale_log2(S));
}

// Rows [y_first, y_first + rows) of the file's ow pixels wide frame at `out`, rows `pitch` bytes apart, from planes whose row 0 is output
// row y0 (luma) / chroma row c0 (S = 1 only).  Dword stores where `vec` says the slot allows them and ow is a multiple of four.
template <int S>
__device__ __forceinline__ void jd_paint_any(const dd_jpeg_info &r, const JdBand &b, const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, int y0, int c0, int y_first, int rows,
                                             int ow, uint8_t *__restrict__ out, size_t pitch, bool vec) {
    int cw, ch = 0;
    if constexpr (S == 1) cw = (r.width + r.hmax - 1) / r.hmax, ch = (r.height + r.vmax - 1) / r.vmax;
    else cw = r.ncomp == 3 ? jpd_plane(r.height, r.width, 1, 1, r.hmax, r.vmax, S).cols : 0;
    auto pixel = [&](int y, int x) -> uint32_t {
        if constexpr (S == 1) return jd_pixel(r, b, Y, Cb, Cr, y0, c0, y, x, cw, ch);
        else return jd_pixel_scaled<S>(r, b, Y, Cb, Cr, y - y0, x, cw);
    };
    if (vec && (ow & 3) == 0) {
        const int qw = ow >> 2;
        for (int i = threadIdx.x; i < rows * qw; i += JD_T) {
            const int row = i / qw, x = (i - row * qw) * 4, y = y_first + row;
            uint32_t p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = pixel(y, x + j);
            uint32_t *o = reinterpret_cast<uint32_t *>(out + (size_t)y * pitch + (size_t)x * 3);
            o[0] = p[0] | (p[1] << 24);
            o[1] = (p[1] >> 8) | (p[2] << 16);
            o[2] = (p[2] >> 16) | (p[3] << 8);
        }
    } else {
        for (int i = threadIdx.x; i < rows * ow; i += JD_T) {
            const int row = i / ow, x = i - row * ow, y = y_first + row;
            const uint32_t p = pixel(y, x);
            uint8_t *o = out + (size_t)y * pitch + (size_t)x * 3;
            o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
        }
    }
}

template <int S>
__global__ __launch_bounds__(JD_T) void jpeg_planes_any_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                          uint8_t *__restrict__ planes) {
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || !jd_any_mine<S>(r, DD_JPEGDEC_PLANES) || band >= r.mcus_y) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, S);
    const int crows = S == 1 ? 8 : b.crows;                    // the planes in HBM hold no halo rows
    uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * crows * b.Wc;
    const int16_t *c = coef + (size_t)f * g.coef_stride;
    if constexpr (S == 1) jd_transform_band(r, c, band, b, Y + (size_t)band * b.yrows * b.Wy, Cb + (size_t)band * crows * b.Wc, Cr + (size_t)band * crows * b.Wc, false);
    else jd_transform_band_scaled<S>(r, c, band, b, Y + (size_t)band * b.yrows * b.Wy, Cb + (size_t)band * crows * b.Wc, Cr + (size_t)band * crows * b.Wc);
}

// One workgroup per band of a frame.  OH x OW: the slot; vec: its rows and its base are dword-aligned.
template <int S>
__global__ __launch_bounds__(JD_T) void jpeg_pixels_any_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                          const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, int OH, int OW, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t jd_lds[];
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || band >= r.mcus_y) return;
    const bool lds = jd_any_mine<S>(r, DD_JPEGDEC_LDS);
    if (!lds && !jd_any_mine<S>(r, DD_JPEGDEC_PLANES)) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, S);
    const int oh = (r.height + S - 1) / S, ow = (r.width + S - 1) / S;
    const int y_first = band * b.yrows, rows = min(b.yrows, oh - y_first);
    if (rows <= 0 || oh > OH || ow > OW) return;
    const size_t pitch = (size_t)OW * 3;
    uint8_t *frame = out + (size_t)f * OH * pitch;
    if (lds) {
        uint8_t *Y = jd_lds, *Cb = Y + (size_t)b.yrows * b.Wy, *Cr = Cb + (size_t)b.crows * b.Wc;
        if constexpr (S == 1) jd_transform_band(r, coef + (size_t)f * g.coef_stride, band, b, Y, Cb, Cr, b.halo != 0);
        else jd_transform_band_scaled<S>(r, coef + (size_t)f * g.coef_stride, band, b, Y, Cb, Cr);
        __syncthreads();
        jd_paint_any<S>(r, b, Y, Cb, Cr, y_first, band * 8 - b.halo, y_first, rows, ow, frame, pitch, vec != 0);
    } else {
        const int crows = S == 1 ? 8 : b.crows;
        const uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * crows * b.Wc;
        jd_paint_any<S>(r, b, Y, Cb, Cr, 0, 0, y_first, rows, ow, frame, pitch, vec != 0);
    }
}

}  // namespace

namespace ddk {

// One launch pair per scale that occurs in the call: jpeg_planes_any_k<S> where a file of that scale takes DD_JPEGDEC_PLANES, then
// jpeg_pixels_any_k<S> with the most LDS a file of that scale needs.  n files, max_bands workgroups each; each launch passes over the
// other scales' files.  OH x OW: the slot.
int jpegdec_pixels_any(hipStream_t s, int n, int max_bands, long long coef_stride, long long plane_stride, const JdPerScale &per_scale, const dd_jpeg_info *recs,
                       const int *mark, const int16_t *coef, uint8_t *planes, uint8_t *out_dev, int OH, int OW) {
    JdGeom g{};
    g.max_bands = max_bands, g.coef_stride = coef_stride, g.plane_stride = plane_stride;
    const unsigned grid = (unsigned)n * (unsigned)max_bands;
    const int vec = (OW & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0;
    for (int lg = 0; lg < 4; ++lg) {
        if (!per_scale.any_at[lg]) continue;
        const int rc = jd_with_scale(1 << lg, [&](auto scale) -> int {
            constexpr int S = decltype(scale)::value;
            if (per_scale.planes_at[lg]) {
                hipLaunchKernelGGL(jpeg_planes_any_k<S>, dim3(grid), dim3(JD_T), 0, s, recs, g, mark, coef, planes);
                DD_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(jpeg_pixels_any_k<S>, dim3(grid), dim3(JD_T), per_scale.lds_at[lg], s, recs, g, mark, coef, planes, out_dev, OH, OW, vec);
            DD_LAUNCH_CHECK();
            return DD_OK;
        });
        if (rc != DD_OK) return rc;
    }
    return DD_OK;
}

}  // namespace ddk
