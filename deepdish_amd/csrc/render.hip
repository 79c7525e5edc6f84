// Annotated output frames: the overlay of deepdish.py:295-408,1187-1207 (count line, track paths, crossing segments, detection and track
// boxes, text) painted over frames that live in HBM, one launch for all requested streams.
//   rectangle   Pillow's ImageDraw.rectangle(outline=...), byte for byte: the two horizontal edges, and the two vertical edges over rows
//               min(y0 + 1, y1) .. max(y0 + 1, y1) (Draw.c draws them from y0 + 1 to y1 as lines: a box with y1 == y0 also colours row y0 + 1)
//   fill        Pillow's ImageDraw.rectangle(fill=...) without outline, byte for byte: every pixel x0 <= x <= x1, y0 <= y <= y1
//               (fills and lines of even width are accepted only after dd_render_record_set(r, DD_RENDER_RECORDS_2))
//   line        this build's rule, exact integers: a capsule of width w (1 .. 15, odd or even) around the segment a-b -- with d = b - a,
//               L2 = d.d, t = (p - a).d, c = (p - a) x d: t <= 0: 4 |p - a|^2 <= w^2;  t >= L2: 4 |p - b|^2 <= w^2;  else 4 c^2 <= w^2 L2
//   mask        Pillow's ImageDraw.draw_bitmap (what ImageDraw.text ends in): per channel t = dst (255 - m) + ink m + 128, ((t >> 8) + t) >> 8,
//               the coverage m read from a u8 atlas in HBM
// Painter's order: a workgroup owns one 64 x 16 tile of one output frame, loads it once, walks that stream's records in order (staged
// through LDS 256 at a time, the ones whose box misses the tile skipped by a ballot) and stores it once.  Integer ALU only.
#include <algorithm>
#include <mutex>
#include "common.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE_W = 64, RD_TILE_H = 16;       // 16 lanes x 4 pixels wide, 16 rows: one wave = 4 rows
constexpr int RD_CHUNK = 256;                       // records staged in LDS at a time: one per thread
constexpr int RD_COORD_MIN = -8192, RD_COORD_MAX = 8191, RD_MAX_SIDE = 8192, RD_MAX_WIDTH = 15;
enum { RD_RECT = 0, RD_LINE = 1, RD_MASK = 2, RD_FILL = 3 };

struct RdRec { int kind, x0, y0, x1, y1, arg, ink, pad; };      // rect, fill: corners; line: a, b, arg = width; mask: x, y, w, h, arg = atlas offset; ink = B | G << 8 | R << 16

struct RdP {
    const uint8_t *frames;     // [*][H][W][3]
    uint8_t *out;              // [n][H][W][3]
    const int *streams;        // [n] source frame of output frame i
    const RdRec *recs;
    const int *rec_off;        // [n + 1]
    const uint8_t *atlas;
    int H, W;
};

typedef uint32_t rd_u32x3 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ uint32_t rd_blend(uint32_t dst, uint32_t ink, uint32_t m) {
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t t = ((dst >> (8 * c)) & 255u) * (255u - m) + ((ink >> (8 * c)) & 255u) * m + 128u;
        o |= ((((t >> 8) + t) >> 8) & 255u) << (8 * c);
    }
    return o;
}

// One record over the lane's four pixels (x .. x + 3, y); px[j] = B | G << 8 | R << 16.
__device__ __forceinline__ void rd_apply(const RdRec &r, const uint8_t *__restrict__ atlas, int x, int y, uint32_t (&px)[4]) {
    if (r.kind == RD_RECT) {
        const int ylo = min(r.y0 + 1, r.y1), yhi = max(r.y0 + 1, r.y1);
        const bool hrow = y == r.y0 || y == r.y1, vrow = y >= ylo && y <= yhi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x + j;
            if ((hrow && xx >= r.x0 && xx <= r.x1) || (vrow && (xx == r.x0 || xx == r.x1))) px[j] = (uint32_t)r.ink;
        }
    } else if (r.kind == RD_LINE) {
        // coordinates lie in [-8192, 8191], pixels in [0, 8191]: |p - a| < 2^15, |d| < 2^14, so t and c fit 32 bits and their squares 64
        const int dx = r.x1 - r.x0, dy = r.y1 - r.y0;
        const long long L2 = (long long)dx * dx + (long long)dy * dy, w2 = (long long)r.arg * r.arg;
        const int py = y - r.y0, qy = y - r.y1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pxx = x + j - r.x0, qx = x + j - r.x1;
            const long long t = (long long)pxx * dx + (long long)py * dy;
            bool in;
            if (t <= 0) in = 4 * ((long long)pxx * pxx + (long long)py * py) <= w2;
            else if (t >= L2) in = 4 * ((long long)qx * qx + (long long)qy * qy) <= w2;
            else { const long long c = (long long)pxx * dy - (long long)py * dx; in = 4 * c * c <= w2 * L2; }
            if (in) px[j] = (uint32_t)r.ink;
        }
    } else if (r.kind == RD_FILL) {
        if (y >= r.y0 && y <= r.y1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j >= r.x0 && x + j <= r.x1) px[j] = (uint32_t)r.ink;
        }
    } else {
        const int my = y - r.y0;
        if (my >= 0 && my < r.y1) {
            const uint8_t *row = atlas + (size_t)r.arg + (size_t)my * r.x1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int mx = x + j - r.x0;
                if (mx >= 0 && mx < r.x1) px[j] = rd_blend(px[j], (uint32_t)r.ink, row[mx]);
            }
        }
    }
}

// grid (tiles across, tiles down, output frames), 256 threads.  DWORDS: rows and both frame arrays are dword-aligned and W is a multiple of 4,
// so a lane's four pixels are three aligned dwords; else every byte moves on its own.
template <bool DWORDS>
__global__ __launch_bounds__(RD_THREADS) void render_k(const RdP P) {
    __shared__ RdRec recs[RD_CHUNK];
    __shared__ unsigned long long hits[RD_CHUNK / 64];
    const int i = blockIdx.z;
    const int tx0 = blockIdx.x * RD_TILE_W, ty0 = blockIdx.y * RD_TILE_H;
    const int x = tx0 + (threadIdx.x & 15) * 4, y = ty0 + (threadIdx.x >> 4);
    const size_t frame = (size_t)P.H * P.W * 3;
    const uint8_t *src = P.frames + (size_t)P.streams[i] * frame + ((size_t)y * P.W + x) * 3;
    uint8_t *dst = P.out + (size_t)i * frame + ((size_t)y * P.W + x) * 3;
    const bool live = y < P.H && x < P.W;
    const int nx = live ? min(4, P.W - x) : 0;      // DWORDS: 0 or 4
    uint32_t px[4] = {0, 0, 0, 0};
    if (live) {
        if constexpr (DWORDS) {
            const rd_u32x3 v = *reinterpret_cast<const rd_u32x3 *>(src);
            px[0] = v.x & 0xffffffu; px[1] = (v.x >> 24) | ((v.y & 0xffffu) << 8); px[2] = (v.y >> 16) | ((v.z & 0xffu) << 16); px[3] = v.z >> 8;
        } else {
            for (int j = 0; j < nx; ++j) px[j] = (uint32_t)src[3 * j] | ((uint32_t)src[3 * j + 1] << 8) | ((uint32_t)src[3 * j + 2] << 16);
        }
    }
    const int r0 = P.rec_off[i], r1 = P.rec_off[i + 1];
    const int tx1 = min(tx0 + RD_TILE_W, P.W) - 1, ty1 = min(ty0 + RD_TILE_H, P.H) - 1;      // the tile, inclusive
    for (int base = r0; base < r1; base += RD_CHUNK) {                                         // block-uniform
        const int n = min(RD_CHUNK, r1 - base);
        bool hit = false;
        if ((int)threadIdx.x < n) {
            const RdRec r = P.recs[base + threadIdx.x];
            recs[threadIdx.x] = r;
            int bx0, by0, bx1, by1;
            if (r.kind == RD_RECT) { bx0 = r.x0; bx1 = r.x1; by0 = min(r.y0, r.y1); by1 = max(r.y0 + 1, r.y1); }
            else if (r.kind == RD_LINE) {
                const int e = (r.arg + 1) / 2;
                bx0 = min(r.x0, r.x1) - e; bx1 = max(r.x0, r.x1) + e; by0 = min(r.y0, r.y1) - e; by1 = max(r.y0, r.y1) + e;
            } else if (r.kind == RD_FILL) { bx0 = r.x0; bx1 = r.x1; by0 = r.y0; by1 = r.y1; }
            else { bx0 = r.x0; by0 = r.y0; bx1 = r.x0 + r.x1 - 1; by1 = r.y0 + r.y1 - 1; }
            hit = bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0;
        }
        const unsigned long long m = __ballot(hit);
        if ((threadIdx.x & 63) == 0) hits[threadIdx.x >> 6] = m;
        __syncthreads();
        for (int w = 0; w < RD_CHUNK / 64; ++w) {
            const unsigned long long hw = hits[w];
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hw), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(hw >> 32));
            unsigned long long mm = (unsigned long long)lo | ((unsigned long long)hi << 32);      // the same in every lane: a scalar loop
            while (mm) {
                const int k = __builtin_ctzll(mm);
                mm &= mm - 1;
                rd_apply(recs[w * 64 + k], P.atlas, x, y, px);
            }
        }
        __syncthreads();
    }
    if (live) {
        if constexpr (DWORDS) {
            rd_u32x3 v;
            v.x = px[0] | (px[1] << 24); v.y = (px[1] >> 8) | (px[2] << 16); v.z = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<rd_u32x3 *>(dst) = v;
        } else {
            for (int j = 0; j < nx; ++j) { dst[3 * j] = (uint8_t)px[j]; dst[3 * j + 1] = (uint8_t)(px[j] >> 8); dst[3 * j + 2] = (uint8_t)(px[j] >> 16); }
        }
    }
}

}  // namespace

struct dd_render {
    dd_ctx *ctx = nullptr;
    int H = 0, W = 0;
    std::vector<uint8_t> atlas_host;       // every mask put so far, back to back: what a grown device atlas is refilled from
    uint8_t *d_atlas = nullptr;
    size_t atlas_cap = 0;
    DevBuf d_recs;                         // one draw's records, offsets and stream list
    PinBuf h_recs;                         // ... staged here
    hipEvent_t copied = nullptr;           // the last draw's copy out of h_recs
    bool copy_pending = false;
    int record_set = DD_RENDER_RECORDS_1;  // what dd_render_draw accepts: kinds 0 .. 2 with odd widths, or (2) also kind 3 and even widths
    std::mutex mu;
};

extern "C" {

int dd_render_create(dd_ctx *ctx, int frame_h, int frame_w, dd_render **out) {
    DD_REQUIRE(ctx && out, DD_E_ARG, "dd_render_create: NULL argument");
    DD_REQUIRE(frame_h > 0 && frame_w > 0 && frame_h <= RD_MAX_SIDE && frame_w <= RD_MAX_SIDE, DD_E_ARG,
               "dd_render_create: a %d x %d canvas (1 .. %d either way)", frame_w, frame_h, RD_MAX_SIDE);
    dd_render *r = new dd_render();
    r->ctx = ctx; r->H = frame_h; r->W = frame_w;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->copied, hipEventDisableTiming);
    if (e != hipSuccess) { delete r; DD_HIP(e); }
    *out = r;
    return DD_OK;
}

int dd_render_destroy(dd_render *r) {
    if (!r) return DD_OK;
    if (r->d_atlas) (void)hipFree(r->d_atlas);
    if (r->copy_pending) (void)hipEventSynchronize(r->copied);
    if (r->copied) (void)hipEventDestroy(r->copied);
    r->d_recs.release();
    r->h_recs.release();
    delete r;
    return DD_OK;
}

// Which records dd_render_draw accepts from now on.  A renderer starts with DD_RENDER_RECORDS_1 (rectangle outlines, lines of odd width, masks) and
// refuses everything else, as it always has; DD_RENDER_RECORDS_2 adds the filled rectangle (kind 3) and lines of even width.
int dd_render_record_set(dd_render *r, int record_set) {
    DD_REQUIRE(r, DD_E_ARG, "dd_render_record_set: NULL argument");
    DD_REQUIRE(record_set == DD_RENDER_RECORDS_1 || record_set == DD_RENDER_RECORDS_2, DD_E_ARG, "dd_render_record_set: record set %d (1 or 2)", record_set);
    std::lock_guard<std::mutex> lk(r->mu);
    r->record_set = record_set;
    return DD_OK;
}

// A coverage mask, u8 [h][w] on the host, appended to the atlas; *offset_out is what a mask record names.  The copy has completed on return.
int dd_render_put_mask(dd_render *r, const uint8_t *mask_host, int w, int h, int *offset_out) {
    DD_REQUIRE(r && mask_host && offset_out, DD_E_ARG, "dd_render_put_mask: NULL argument");
    DD_REQUIRE(w > 0 && h > 0 && w <= RD_MAX_SIDE && h <= RD_MAX_SIDE, DD_E_ARG, "dd_render_put_mask: a %d x %d mask (1 .. %d either way)", w, h, RD_MAX_SIDE);
    DD_DEVICE(r->ctx);
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t off = r->atlas_host.size(), bytes = (size_t)w * h;
    DD_REQUIRE(off + bytes <= (size_t)0x7fffffff, DD_E_CAPACITY, "dd_render_put_mask: the atlas holds %zu bytes, %zu more do not fit 2^31", off, bytes);
    r->atlas_host.insert(r->atlas_host.end(), mask_host, mask_host + bytes);
    if (off + bytes > r->atlas_cap) {          // grow: kernels of earlier draws may still read the old one
        DD_HIP(hipDeviceSynchronize());
        uint8_t *bigger = nullptr;
        const size_t cap = std::max((size_t)1 << 20, 2 * (off + bytes));
        DD_HIP(hipMalloc(&bigger, cap));
        if (r->d_atlas) (void)hipFree(r->d_atlas);
        r->d_atlas = bigger; r->atlas_cap = cap;
        DD_HIP(hipMemcpy(r->d_atlas, r->atlas_host.data(), off + bytes, hipMemcpyHostToDevice));
    } else {
        DD_HIP(hipMemcpy(r->d_atlas + off, mask_host, bytes, hipMemcpyHostToDevice));
    }
    *offset_out = (int)off;
    return DD_OK;
}

// frames_dev: u8 [n_frames][H][W][3] BGR on the device; output frame i = frame streams_host[i] (all < n_frames) under records
// prim_off_host[i] .. prim_off_host[i + 1] - 1 of prims_host (8 int32 each: kind, four coordinates, arg, ink, 0), painted in order.
// out_dev: u8 [n][H][W][3], no byte shared with frames_dev.  Every record is checked here; the kernel trusts them.
int dd_render_draw(dd_render *r, const uint8_t *frames_dev, int n_frames, const int *streams_host, int n, const int32_t *prims_host,
                   const int *prim_off_host, uint8_t *out_dev, void *stream) {
    DD_REQUIRE(r && frames_dev && streams_host && prim_off_host && out_dev && n > 0 && n_frames > 0, DD_E_ARG, "dd_render_draw: bad argument");
    DD_REQUIRE(n <= 65535, DD_E_CAPACITY, "dd_render_draw: %d frames in one launch (<= 65535)", n);
    const size_t frame = (size_t)r->H * r->W * 3;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(frames_dev), b = reinterpret_cast<uintptr_t>(out_dev);
        DD_REQUIRE(a + frame * n_frames <= b || b + frame * n <= a, DD_E_ARG, "dd_render_draw: the output overlaps the source frames (it is written out of place)");
    }
    DD_REQUIRE(prim_off_host[0] == 0, DD_E_ARG, "dd_render_draw: the first record offset is %d, not 0", prim_off_host[0]);
    for (int i = 0; i < n; ++i) {
        DD_REQUIRE(streams_host[i] >= 0 && streams_host[i] < n_frames, DD_E_ARG, "dd_render_draw: stream %d of %d frames", streams_host[i], n_frames);
        DD_REQUIRE(prim_off_host[i + 1] >= prim_off_host[i], DD_E_ARG, "dd_render_draw: record offsets decrease at frame %d", i);
    }
    const int total = prim_off_host[n];
    DD_REQUIRE(total == 0 || prims_host, DD_E_ARG, "dd_render_draw: %d records and no array", total);
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t atlas_used = r->atlas_host.size();
    const bool wide = r->record_set == DD_RENDER_RECORDS_2;
    for (int k = 0; k < total; ++k) {
        const int32_t *q = prims_host + (size_t)k * 8;
        DD_REQUIRE(q[0] >= RD_RECT && q[0] <= (wide ? RD_FILL : RD_MASK), DD_E_ARG, "dd_render_draw: record %d has kind %d", k, q[0]);
        if (q[0] == RD_MASK) {
            DD_REQUIRE(q[1] >= RD_COORD_MIN && q[1] <= RD_COORD_MAX && q[2] >= RD_COORD_MIN && q[2] <= RD_COORD_MAX, DD_E_ARG,
                       "dd_render_draw: record %d lies at (%d, %d), outside %d .. %d", k, q[1], q[2], RD_COORD_MIN, RD_COORD_MAX);
            DD_REQUIRE(q[3] > 0 && q[4] > 0 && q[3] <= RD_MAX_SIDE && q[4] <= RD_MAX_SIDE && q[5] >= 0 && (size_t)q[5] + (size_t)q[3] * q[4] <= atlas_used, DD_E_ARG,
                       "dd_render_draw: record %d names a %d x %d mask at atlas byte %d of %zu", k, q[3], q[4], q[5], atlas_used);
        } else {
            for (int c = 1; c <= 4; ++c)
                DD_REQUIRE(q[c] >= RD_COORD_MIN && q[c] <= RD_COORD_MAX, DD_E_ARG, "dd_render_draw: record %d has coordinate %d, outside %d .. %d", k, q[c],
                           RD_COORD_MIN, RD_COORD_MAX);
            if (q[0] == RD_RECT || q[0] == RD_FILL)
                DD_REQUIRE(q[3] >= q[1] && q[4] >= q[2], DD_E_ARG, "dd_render_draw: record %d is a rectangle with x1 < x0 or y1 < y0 (%d, %d, %d, %d)", k, q[1], q[2], q[3], q[4]);
            if (q[0] == RD_LINE)
                DD_REQUIRE(q[5] >= 1 && q[5] <= RD_MAX_WIDTH && (wide || (q[5] & 1)), DD_E_ARG, "dd_render_draw: record %d has line width %d (%s1 .. %d)", k, q[5],
                           wide ? "" : "odd, ", RD_MAX_WIDTH);
        }
    }
    DD_DEVICE(r->ctx);
    hipStream_t s = dd_pick_stream(r->ctx, stream);
    // device block: [records | offsets n + 1 | streams n], staged in pinned memory and sent as one copy; the staging block is rewritten
    // only after the previous draw's copy has left it
    const size_t rec_bytes = (size_t)total * sizeof(RdRec), need = rec_bytes + (size_t)(2 * n + 1) * sizeof(int);
    if (r->copy_pending) { DD_HIP(hipEventSynchronize(r->copied)); r->copy_pending = false; }
    if (need > r->d_recs.cap) DD_HIP(hipStreamSynchronize(s));      // an earlier draw on this stream may still read the block that reserve() frees
    int rc;
    if ((rc = r->d_recs.reserve(need)) != DD_OK) return rc;
    if ((rc = r->h_recs.reserve(need)) != DD_OK) return rc;
    char *h = r->h_recs.as<char>(), *d = r->d_recs.as<char>();
    if (total) memcpy(h, prims_host, rec_bytes);
    memcpy(h + rec_bytes, prim_off_host, (size_t)(n + 1) * sizeof(int));
    memcpy(h + rec_bytes + (size_t)(n + 1) * sizeof(int), streams_host, (size_t)n * sizeof(int));
    DD_HIP(hipMemcpyAsync(d, h, need, hipMemcpyHostToDevice, s));
    DD_HIP(hipEventRecord(r->copied, s));
    r->copy_pending = true;
    RdP P;
    P.frames = frames_dev; P.out = out_dev;
    P.recs = reinterpret_cast<const RdRec *>(d);
    P.rec_off = reinterpret_cast<const int *>(d + rec_bytes);
    P.streams = P.rec_off + n + 1;
    P.atlas = r->d_atlas;
    P.H = r->H; P.W = r->W;
    const dim3 grid((unsigned)dd_ceil_div(r->W, RD_TILE_W), (unsigned)dd_ceil_div(r->H, RD_TILE_H), (unsigned)n);
    const bool dwords = r->W % 4 == 0 && (reinterpret_cast<uintptr_t>(frames_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0;
    if (dwords) hipLaunchKernelGGL(render_k<true>, grid, dim3(RD_THREADS), 0, s, P);
    else hipLaunchKernelGGL(render_k<false>, grid, dim3(RD_THREADS), 0, s, P);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // extern "C"
