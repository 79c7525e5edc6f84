// Letterboxed detector input: Pillow's Lanczos resize to an aspect-preserving size, pasted into a constant canvas, in one launch.
//   geometry   yolo3/utils.py:18-28 letterbox_image (= tools/yolo.py:141-151): s = min(w / W, h / H), new = int(W s) x int(H s), pasted at
//              ((w - new_w) // 2, (h - new_h) // 2) -- same double arithmetic, same truncation
//   pixels     Image.new('RGB', (w, h), (pad,) * 3).paste(Image.fromarray(rgb).resize((new_w, new_h), Image.LANCZOS), (off_x, off_y)), byte
//              for byte: the integer arithmetic of lanczos_h_k / lanczos_v_k (image.hip) on the same coefficient tables; an axis whose size
//              does not change is copied (Pillow skips that pass)
// The filter (the YOLOv5 adaptor's Lanczos, not the YOLOv3 plugin's bicubic) is this build's choice.  Scalar ALU only.
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <algorithm>
#include "common.h"
#include "lanczos_tab.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;       // Pillow Resample.c
constexpr int LB_THREADS = 256;
// LDS a workgroup of letterbox_lanczos_k may take for its band of horizontally resampled source rows.  A CU has 160 KiB: two workgroups
// fit beside each other at the budget, more when the band is smaller.
constexpr int LB_LDS_BUDGET = 64 * 1024;
constexpr int LB_MAX_ROWS = 16;                  // canvas rows per workgroup at most: small canvases still spread over several workgroups
constexpr int LB_VPAD_ROWS = 8;                  // canvas rows per workgroup of letterbox_v_pad_k

struct LbP {
    const uint8_t *src;        // letterbox_lanczos_k: frames [H][W][src_c]; letterbox_v_pad_k: rows [H][new_w][src_c] (the horizontal pass's result)
    uint8_t *dst;              // canvases [h][w][3]
    size_t src_frame, dst_frame;      // bytes per frame on either side
    int H, W, src_c, swap_rb;
    int h, w, new_h, new_w, off_x, off_y, pad;
    const int *bh, *kh;        // horizontal bounds / coefficients, NULL when new_w == W
    const int *bv, *kv;        // vertical, NULL when new_h == H
    int ksh, ksv;
    int rows, rows_cap;        // canvas rows per workgroup; source rows the LDS band has room for
    int pitch, base;           // LDS band: bytes per row; canvas byte that column 0 of a band row stands for (a multiple of 16 below off_x * 3)
};

typedef uint32_t lb_u32u __attribute__((aligned(1)));      // a dword at any byte address (whole pixels of a row: never past the frame)

__device__ __forceinline__ int lb_clip8(int a) { return min(max(a >> PRECISION_BITS, 0), 255); }

// Four bytes -> one word.  hipcc (ROCm 7.2) turns clamp | clamp << 8 ... into v_ashr_pk_u8_i32 and corrupts bytes 2-3 (image.hip,
// lanczos_v4_k): the bytes stay opaque to the pattern matcher.
__device__ __forceinline__ uint32_t lb_pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// Canvas rows r0 .. r1 - 1 of one frame, whole rows: padding left and right of the picture, padding rows above and below it, the vertical
// pass (or the copy) in between.  One work item = VEC consecutive canvas bytes (VEC > 1: the row length and the canvas address are multiples
// of VEC, so an item never straddles rows and its store is aligned).  LDS: the taps come from the workgroup's band of rows (band row 0 =
// source row s_lo), else from `mid` in memory.  Every canvas byte of the rows is stored exactly once.
template <int VEC, bool LDS>
__device__ __forceinline__ void lb_store_rows(const LbP &P, const uint8_t *band, int s_lo, const uint8_t *mid, uint8_t *out, int r0, int r1) {
    const int rowb = P.w * 3, x0b = P.off_x * 3, x1b = x0b + P.new_w * 3;
    const int ipr = rowb / VEC;
    const int items = (r1 - r0) * ipr;
    for (int it = threadIdx.x; it < items; it += LB_THREADS) {
        const int rr = it / ipr;
        const int r = r0 + rr, b = (it - rr * ipr) * VEC;
        const int yy = r - P.off_y;
        uint32_t o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (uint32_t)P.pad;
        if (yy >= 0 && yy < P.new_h && b + VEC > x0b && b < x1b) {
            const bool resample = P.bv != nullptr;
            const int ymin = resample ? P.bv[2 * yy] : yy, n = resample ? P.bv[2 * yy + 1] : 1;
            const int *k = resample ? P.kv + (size_t)yy * P.ksv : nullptr;
            int acc[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] = resample ? 1 << (PRECISION_BITS - 1) : 0;
            for (int y = 0; y < n; ++y) {
                const int kv = resample ? k[y] : 1;
                if constexpr (LDS) {
                    const uint8_t *p = band + (ymin - s_lo + y) * P.pitch + (b - P.base);
                    if constexpr (VEC == 1) {
                        acc[0] += (int)p[0] * kv;
                    } else {
#pragma unroll
                        for (int q = 0; q < VEC / 4; ++q) {
                            const uint32_t v = reinterpret_cast<const uint32_t *>(p)[q];
                            acc[4 * q + 0] += (int)(v & 255u) * kv;
                            acc[4 * q + 1] += (int)((v >> 8) & 255u) * kv;
                            acc[4 * q + 2] += (int)((v >> 16) & 255u) * kv;
                            acc[4 * q + 3] += (int)(v >> 24) * kv;
                        }
                    }
                } else {
                    const uint8_t *row = mid + (size_t)(ymin + y) * P.new_w * P.src_c;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const int e = b + j - x0b;
                        if (e >= 0 && b + j < x1b) {
                            const int px = e / 3, ch = e - px * 3;
                            acc[j] += (int)row[(size_t)px * P.src_c + (P.swap_rb ? 2 - ch : ch)] * kv;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (b + j >= x0b && b + j < x1b) o[j] = (uint32_t)(resample ? lb_clip8(acc[j]) : acc[j]);
        }
        uint8_t *d = out + (size_t)r * rowb + b;
        if constexpr (VEC == 1) {
            d[0] = (uint8_t)o[0];
        } else if constexpr (VEC == 4) {
            *reinterpret_cast<uint32_t *>(d) = lb_pack4(o[0], o[1], o[2], o[3]);
        } else {
            uint4 v;
            v.x = lb_pack4(o[0], o[1], o[2], o[3]); v.y = lb_pack4(o[4], o[5], o[6], o[7]);
            v.z = lb_pack4(o[8], o[9], o[10], o[11]); v.w = lb_pack4(o[12], o[13], o[14], o[15]);
            *reinterpret_cast<uint4 *>(d) = v;
        }
    }
}

// grid (bands, frames), 256 threads.  A workgroup owns P.rows canvas rows of one frame: it resamples horizontally (or copies) the source
// rows its vertical windows need into LDS, 3 bytes per pixel laid out at the canvas's byte alignment, and after one barrier runs the
// vertical pass out of LDS and stores its canvas rows whole.  A band that lies in the top or bottom padding only stores `pad`.
template <int VEC>
__global__ __launch_bounds__(LB_THREADS) void letterbox_lanczos_k(const LbP P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lb_band[];
    const size_t f = blockIdx.y;
    const int r0 = blockIdx.x * P.rows, r1 = min(r0 + P.rows, P.h);
    const uint8_t *src = P.src + f * P.src_frame;
    const int yy_lo = max(r0 - P.off_y, 0), yy_hi = min(r1 - P.off_y, P.new_h);
    int s_lo = 0;
    if (yy_lo < yy_hi) {                                          // block-uniform
        int s_hi;
        if (P.bv) { s_lo = P.bv[2 * yy_lo]; s_hi = P.bv[2 * (yy_hi - 1)] + P.bv[2 * (yy_hi - 1) + 1]; }      // windows move down with yy
        else { s_lo = yy_lo; s_hi = yy_hi; }
        const int nrows = min(s_hi - s_lo, P.rows_cap);           // the plan sized rows_cap from the same table: never the smaller
        const int lead = P.off_x * 3 - P.base;
        for (int idx = threadIdx.x; idx < nrows * P.new_w; idx += LB_THREADS) {
            const int r = idx / P.new_w, xx = idx - r * P.new_w;
            const uint8_t *row = src + (size_t)(s_lo + r) * P.W * P.src_c;
            int a0, a1, a2;
            if (P.bh) {
                const int xmin = P.bh[2 * xx], n = P.bh[2 * xx + 1];
                const int *k = P.kh + (size_t)xx * P.ksh;
                const uint8_t *q = row + (size_t)xmin * P.src_c;
                a0 = a1 = a2 = 1 << (PRECISION_BITS - 1);
                int x = 0;
                if (P.src_c == 3) {                                   // four taps = twelve bytes = three (unaligned) dwords instead of twelve byte loads
                    for (; x + 4 <= n; x += 4) {
                        const uint32_t w0 = *reinterpret_cast<const lb_u32u *>(q + x * 3), w1 = *reinterpret_cast<const lb_u32u *>(q + x * 3 + 4),
                                       w2 = *reinterpret_cast<const lb_u32u *>(q + x * 3 + 8);
                        const int k0 = k[x], k1 = k[x + 1], k2 = k[x + 2], k3 = k[x + 3];
                        a0 += (int)(w0 & 255u) * k0 + (int)(w0 >> 24) * k1 + (int)((w1 >> 16) & 255u) * k2 + (int)((w2 >> 8) & 255u) * k3;
                        a1 += (int)((w0 >> 8) & 255u) * k0 + (int)(w1 & 255u) * k1 + (int)(w1 >> 24) * k2 + (int)((w2 >> 16) & 255u) * k3;
                        a2 += (int)((w0 >> 16) & 255u) * k0 + (int)((w1 >> 8) & 255u) * k1 + (int)(w2 & 255u) * k2 + (int)(w2 >> 24) * k3;
                    }
                } else {                                              // one pixel = one dword
                    for (; x < n; ++x) {
                        const uint32_t w0 = *reinterpret_cast<const lb_u32u *>(q + x * 4);
                        const int kv = k[x];
                        a0 += (int)(w0 & 255u) * kv;
                        a1 += (int)((w0 >> 8) & 255u) * kv;
                        a2 += (int)((w0 >> 16) & 255u) * kv;
                    }
                }
                for (; x < n; ++x) {
                    const int kv = k[x];
                    a0 += q[x * P.src_c + 0] * kv;
                    a1 += q[x * P.src_c + 1] * kv;
                    a2 += q[x * P.src_c + 2] * kv;
                }
                a0 = lb_clip8(a0); a1 = lb_clip8(a1); a2 = lb_clip8(a2);
            } else {
                const uint8_t *q = row + (size_t)xx * P.src_c;
                a0 = q[0]; a1 = q[1]; a2 = q[2];
            }
            if (P.swap_rb) { const int t = a0; a0 = a2; a2 = t; }
            uint8_t *o = lb_band + r * P.pitch + lead + xx * 3;
            o[0] = (uint8_t)a0; o[1] = (uint8_t)a1; o[2] = (uint8_t)a2;
        }
    }
    __syncthreads();
    lb_store_rows<VEC, true>(P, lb_band, s_lo, nullptr, P.dst + f * P.dst_frame, r0, r1);
}

// The second form's last launch: vertical pass + paste + pad, the taps read from memory.  grid (bands, frames).
template <int VEC>
__global__ __launch_bounds__(LB_THREADS) void letterbox_v_pad_k(const LbP P) {
    const size_t f = blockIdx.y;
    const int r0 = blockIdx.x * P.rows, r1 = min(r0 + P.rows, P.h);
    lb_store_rows<VEC, false>(P, nullptr, 0, P.src + f * P.src_frame, P.dst + f * P.dst_frame, r0, r1);
}

struct LbPlan { int new_w = 0, new_h = 0, off_x = 0, off_y = 0, path = 0, rows = 0, rows_cap = 0, pitch = 0, base = 0; bool one_launch = false; };

std::mutex g_plan_mu;
std::map<std::tuple<int, int, int, int>, LbPlan> g_plans;      // (H, W, h, w)

}  // namespace

extern "C" int dd_letterbox_geometry(int W, int H, int net_w, int net_h, int *new_w, int *new_h, int *off_x, int *off_y) {
    DD_REQUIRE(W > 0 && H > 0 && net_w > 0 && net_h > 0, DD_E_ARG, "dd_letterbox_geometry: sizes must be positive (%d x %d into %d x %d)", W, H, net_w, net_h);
    const double sw = net_w * 1.0 / W, sh = net_h * 1.0 / H;      // yolo3/utils.py:22-23
    const double s = sw < sh ? sw : sh;
    const int nw = (int)(W * s), nh = (int)(H * s);
    DD_REQUIRE(nw > 0 && nh > 0, DD_E_ARG, "dd_letterbox_geometry: %d x %d into %d x %d leaves a %d x %d picture (Pillow: height and width must be > 0)",
               W, H, net_w, net_h, nw, nh);
    if (new_w) *new_w = nw;
    if (new_h) *new_h = nh;
    if (off_x) *off_x = (net_w - nw) / 2;                         // :27; never negative: W s <= net_w
    if (off_y) *off_y = (net_h - nh) / 2;
    return DD_OK;
}

namespace ddk {

// The one decision of the letterbox launch, from the geometry and the process's DD_LETTERBOX_FUSED switch alone.  Host only.
static int letterbox_plan(int H, int W, int h, int w, LbPlan *out) {
    static const bool fused_off = getenv("DD_LETTERBOX_FUSED") && atoi(getenv("DD_LETTERBOX_FUSED")) == 0;
    std::lock_guard<std::mutex> lk(g_plan_mu);
    const auto key = std::make_tuple(H, W, h, w);
    auto it = g_plans.find(key);
    if (it == g_plans.end()) {
        LbPlan pl;
        const int rc = dd_letterbox_geometry(W, H, w, h, &pl.new_w, &pl.new_h, &pl.off_x, &pl.off_y);
        if (rc != DD_OK) return rc;
        pl.base = (pl.off_x * 3) & ~15;
        pl.pitch = (pl.off_x * 3 - pl.base + pl.new_w * 3 + 15) & ~15;
        // source rows the band of `rows` canvas rows needs, the most over all bands, from the vertical table itself
        std::vector<int> bounds;
        if (pl.new_h != H) bounds = make_table(H, pl.new_h).bounds;
        auto band_rows = [&](int rows) {
            int most = 0;
            for (int r0 = 0; r0 < h; r0 += rows) {
                const int lo = std::max(r0 - pl.off_y, 0), hi = std::min(std::min(r0 + rows, h) - pl.off_y, pl.new_h);
                if (lo >= hi) continue;
                most = std::max(most, bounds.empty() ? hi - lo : bounds[2 * (hi - 1)] + bounds[2 * (hi - 1) + 1] - bounds[2 * lo]);
            }
            return most;
        };
        int rows = std::min(LB_MAX_ROWS, h);
        while (rows > 1 && (size_t)band_rows(rows) * pl.pitch > (size_t)LB_LDS_BUDGET) --rows;
        pl.rows = rows;
        pl.rows_cap = band_rows(rows);
        const bool fits = (size_t)pl.rows_cap * pl.pitch <= (size_t)LB_LDS_BUDGET;
        pl.path = (pl.new_w == W && pl.new_h == H) ? 0 : (fits && !fused_off) ? 1 : 2;
        pl.one_launch = fits && !fused_off;                       // a copy (path 0) is letterbox_v_pad_k alone otherwise
        if (!pl.one_launch) pl.rows = std::min(LB_VPAD_ROWS, h);
        it = g_plans.emplace(key, pl).first;
    }
    *out = it->second;
    return DD_OK;
}

// `batch` frames [H][W][src_c] -> canvases [h][w][3].  tmp: batch * H * new_w * 3 bytes, used by the two-launch form only.
int resize_lanczos_letterbox(hipStream_t s, int device, const uint8_t *src, int batch, int H, int W, int src_c, int swap_rb, uint8_t *dst, int h, int w,
                             int pad, uint8_t *tmp) {
    LbPlan pl;
    int rc = letterbox_plan(H, W, h, w, &pl);
    if (rc != DD_OK) return rc;
    DD_REQUIRE(batch <= 65535, DD_E_CAPACITY, "resize_lanczos_letterbox: %d frames in one launch (<= 65535)", batch);
    DevTable th{0, nullptr, nullptr}, tv{0, nullptr, nullptr};
    if (pl.new_w != W && (rc = get_table(device, W, pl.new_w, &th)) != DD_OK) return rc;
    if (pl.new_h != H && (rc = get_table(device, H, pl.new_h, &tv)) != DD_OK) return rc;
    LbP P;
    P.src = src; P.dst = dst;
    P.src_frame = (size_t)H * W * src_c; P.dst_frame = (size_t)h * w * 3;
    P.H = H; P.W = W; P.src_c = src_c; P.swap_rb = swap_rb;
    P.h = h; P.w = w; P.new_h = pl.new_h; P.new_w = pl.new_w; P.off_x = pl.off_x; P.off_y = pl.off_y; P.pad = pad;
    P.bh = th.bounds; P.kh = th.kk; P.ksh = th.ksize;
    P.bv = tv.bounds; P.kv = tv.kk; P.ksv = tv.ksize;
    P.rows = pl.rows; P.rows_cap = pl.rows_cap; P.pitch = pl.pitch; P.base = pl.base;
    const int rowb = w * 3;
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    const int vec = (rowb % 16 == 0 && (a & 15) == 0) ? 16 : (rowb % 4 == 0 && (a & 3) == 0) ? 4 : 1;     // the widest store every row start allows
    const dim3 grid((unsigned)dd_ceil_div(h, pl.rows), (unsigned)batch);
    if (pl.one_launch) {
        const size_t lds = (size_t)pl.rows_cap * pl.pitch;
        if (vec == 16) hipLaunchKernelGGL(letterbox_lanczos_k<16>, grid, dim3(LB_THREADS), lds, s, P);
        else if (vec == 4) hipLaunchKernelGGL(letterbox_lanczos_k<4>, grid, dim3(LB_THREADS), lds, s, P);
        else hipLaunchKernelGGL(letterbox_lanczos_k<1>, grid, dim3(LB_THREADS), lds, s, P);
        DD_LAUNCH_CHECK();
        return DD_OK;
    }
    if (pl.new_w != W) {                                          // the dense horizontal pass: [H][W][src_c] -> tmp [H][new_w][3], channels in order
        DD_REQUIRE(tmp, DD_E_ARG, "resize_lanczos_letterbox: the two-launch form needs an intermediate");
        if ((rc = resize_lanczos(s, device, src, H, W, src_c, swap_rb, tmp, H, pl.new_w, tmp, batch)) != DD_OK) return rc;
        P.src = tmp; P.src_frame = (size_t)H * pl.new_w * 3; P.src_c = 3; P.swap_rb = 0;
    }
    if (vec == 16) hipLaunchKernelGGL(letterbox_v_pad_k<16>, grid, dim3(LB_THREADS), 0, s, P);
    else if (vec == 4) hipLaunchKernelGGL(letterbox_v_pad_k<4>, grid, dim3(LB_THREADS), 0, s, P);
    else hipLaunchKernelGGL(letterbox_v_pad_k<1>, grid, dim3(LB_THREADS), 0, s, P);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

extern "C" {

int dd_resize_lanczos_letterbox_plan(dd_ctx *ctx, int H, int W, int src_c, int swap_rb, int h, int w, int batch, int *path, int *rows_per_block) {
    (void)ctx; (void)swap_rb;                                     // the decision depends on neither a device nor the channel order
    DD_REQUIRE(batch > 0 && H > 0 && W > 0 && h > 0 && w > 0, DD_E_ARG, "dd_resize_lanczos_letterbox_plan: bad argument");
    DD_REQUIRE(src_c == 3 || src_c == 4, DD_E_ARG, "dd_resize_lanczos_letterbox_plan: src_c must be 3 or 4");
    LbPlan pl;
    const int rc = ddk::letterbox_plan(H, W, h, w, &pl);
    if (rc != DD_OK) return rc;
    if (path) *path = pl.path;
    if (rows_per_block) *rows_per_block = pl.rows;
    return DD_OK;
}

int dd_resize_lanczos_letterbox(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int src_c, int swap_rb, uint8_t *dst, int h, int w, int pad,
                                void *stream) {
    DD_REQUIRE(ctx && src && dst && batch > 0 && H > 0 && W > 0 && h > 0 && w > 0, DD_E_ARG, "dd_resize_lanczos_letterbox: bad argument");
    DD_REQUIRE(src_c == 3 || src_c == 4, DD_E_ARG, "dd_resize_lanczos_letterbox: src_c must be 3 or 4");
    DD_REQUIRE(pad >= 0 && pad <= 255, DD_E_ARG, "dd_resize_lanczos_letterbox: pad %d (0 .. 255)", pad);
    DD_DEVICE(ctx);
    LbPlan pl;
    int rc = ddk::letterbox_plan(H, W, h, w, &pl);
    if (rc != DD_OK) return rc;
    uint8_t *tmp = nullptr;
    if (pl.path == 2 && pl.new_w != W) {
        if ((rc = ctx->scratch[3].reserve((size_t)batch * H * pl.new_w * 3 + 64)) != DD_OK) return rc;
        tmp = ctx->scratch[3].as<uint8_t>();
    }
    return ddk::resize_lanczos_letterbox(dd_pick_stream(ctx, stream), ctx->device, src, batch, H, W, src_c, swap_rb, dst, h, w, pad, tmp);
}

}  // extern "C"
