// Frame ingest ring: the step in front of the hot path (SURVEY.md section 8 f, n1).
//
// Replaces the CPU side of Pipeline.capture (deepdish.py:837-878): frames arrive in host memory
// (cv2.VideoCapture), are optionally flipped (cv2.flip(frame, 0), :864) and stretched to the pipeline's
// input size (cv2.resize(frame, input_size), :867, INTER_LINEAR) before they reach the detector.  Here a
// decoder writes raw frames of S streams straight into a pinned slot; submit() queues the host->device
// copy on a private copy stream followed by the flip + resize on the GPU (the crop_resize_k restatement of
// cv2.resize; skipped when sizes match and no flip is asked), and the consumer stream waits on an event,
// never on the host.  With >= 2 slots the upload of step t+1 overlaps the kernels of step t.
//
// A slot may also hold what a decoder produces itself, 4:2:0 YUV (NV12 or I420, 1.5 bytes per pixel instead of 3): half the bytes cross
// the link, and the conversion to BGR (csrc/yuv.hip) happens on the copy stream -- fused with the flip + resize in one launch
// (yuv420_resize_k), or, with DD_INGEST_YUV_FUSED=0, as convert-into-a-staging-buffer then crop_resize (the same bytes, for A/B runs).
// The consumer always receives BGR.
//
// A slot may also hold packed 4:2:2 YUV, what a UVC / V4L2 camera (YUY2) or a capture card (UYVY) delivers raw: 2 bytes per pixel, any
// height, an even width.  The same three forms on the copy stream: yuv422_to_bgr straight into the slot's output without a transform,
// yuv422_resize_k fused, or with DD_INGEST_YUV_FUSED=0 convert-into-the-staging-buffer then crop_resize.
//
// A slot may also hold 8-bit raw sensor frames, what a machine-vision or CSI camera delivers before any colour processing: a Bayer mosaic
// (RGGB, GRBG, GBRG, BGGR) or monochrome, 1 byte per pixel, a third of BGR (dd_ingest_create_raw8).  The same three forms on the copy stream
// (csrc/bayer.hip): raw8_to_bgr straight into the slot's output without a transform, raw8_resize_k fused, or with DD_INGEST_YUV_FUSED=0
// convert-into-the-staging-buffer then crop_resize.
//
// A slot may also hold baseline JPEG files, what a camera or the reference's frame_%06d.jpg sequence delivers (a tenth or less of the raw
// bytes): put() copies a stream's file into the slot's pinned arena and parses its header on the calling thread, submit() uploads the
// bytes in use and the records and decodes on the copy stream (csrc/jpeg_dec.hip) -- into the slot's output, or into a staging buffer
// in front of crop_resize when a flip or a resize is asked.  Each stream carries a status; a bad file costs its neighbours nothing.
// Such a ring may decode at 1/2, 1/4 or 1/8 scale (dd_ingest_create_jpeg_scaled): src_h x src_w stays what every file must state, the
// decoder writes ceil(src_h / scale) x ceil(src_w / scale) frames, and it is that size the staging buffer has and crop_resize starts from.
// A ring made with DD_JPEGDEC_ANY_SIZE takes files of any size up to src_h x src_w, each at its own scale (the ring's, or Pillow's draft rule
// per file): put() records the file's size and scale, and submit() always decodes into the staging buffer -- uniform slots of the largest
// frame, each file in its slot's top-left corner -- builds one crop box per stream from its record, uploads the boxes through the slot's
// pinned memory and lets crop_resize stretch each to dst, as the reference's cv2.resize(frame, self.input_size) does whatever the camera sent.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "common.h"

struct dd_ingest {
    dd_ctx *ctx = nullptr;
    int slots = 0, S = 0, sh = 0, sw = 0, dh = 0, dw = 0, flip = 0;
    int format = 0;                         // 0 BGR, 1 NV12, 2 I420, 3 JPEG files, 4 YUY2, 5 UYVY, 6 .. 9 Bayer RGGB GRBG GBRG BGGR, 10 gray
    int jh = 0, jw = 0;                     // the frames in front of the flip + resize: sh x sw, or a JPEG ring's scaled decode
    bool transform = false, own_out = false, fused = true;
    uint8_t *d_stage = nullptr;             // YUV, two-launch form only: the converted BGR frames [S][sh][sw][3]
    hipStream_t copy = nullptr;
    std::vector<uint8_t *> h_raw, d_raw, d_out;
    std::vector<hipEvent_t> ready, done;
    std::vector<char> used, submitted;      // done[slot] / ready[slot] has been recorded at least once
    void *d_boxes = nullptr;                // S full-frame CropBox records
    size_t raw_bytes = 0, out_bytes = 0;
    // JPEG slots: h_raw[slot] is the arena; per slot the records and the status in pinned memory, the status on the device, the arena's
    // fill and whether the slot was submitted since it was last reset
    dd_jpegdec *dec = nullptr;
    std::vector<dd_jpeg_info *> h_recs;
    std::vector<dd_jpeg_scans *> h_scans;     // beside the records, in a ring that takes progressive files (dd_ingest_create_jpeg_ex); else empty
    std::vector<int *> h_status, d_status;
    std::vector<size_t> fill;
    std::vector<char> stale;
    // DD_JPEGDEC_ANY_SIZE: per slot and stream what put() learnt, (width, height, scale) and the scale alone as the decoder takes it, and the
    // crop boxes in pinned memory on their way to d_boxes
    int jflags = 0, jscale = 1;
    bool any_size = false, auto_scale = false;
    std::vector<std::vector<int>> sizes, scales;
    std::vector<int *> h_boxes;
    std::mutex mu;
};

constexpr int INGEST_JPEG = 3, INGEST_YUY2 = 4, INGEST_UYVY = 5;
constexpr int INGEST_RGGB = 6, INGEST_GRAY = 10;         // raw 8-bit: 6 .. 9 the Bayer mosaics, 10 monochrome
static bool ingest_is_422(int format) { return format == INGEST_YUY2 || format == INGEST_UYVY; }
static bool ingest_is_raw8(int format) { return format >= INGEST_RGGB && format <= INGEST_GRAY; }

static int ingest_create(const char *who, dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip,
                         int pixel_format, dd_ingest **out, size_t jpeg_slot_bytes = 0, int jpeg_scale = 1, int jpeg_flags = 0, bool raw8 = false) {
    DD_REQUIRE(ctx && out && slots > 0 && n_streams > 0 && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, DD_E_ARG,
               "%s: bad argument", who);
    DD_REQUIRE((pixel_format >= 0 && pixel_format <= 2) || ingest_is_422(pixel_format) || (pixel_format == INGEST_JPEG && jpeg_slot_bytes) ||
               (raw8 && ingest_is_raw8(pixel_format)), DD_E_ARG,
               "%s: pixel_format %d is none of 0 (BGR), 1 (NV12), 2 (I420), 4 (YUY2), 5 (UYVY)", who, pixel_format);
    if (pixel_format == 1 || pixel_format == 2) {
        DD_REQUIRE(src_w % 2 == 0, DD_E_ARG, "%s: src_w %d must be even for 4:2:0 frames", who, src_w);
        DD_REQUIRE(src_h % 2 == 0, DD_E_ARG, "%s: src_h %d must be even for 4:2:0 frames", who, src_h);
        DD_REQUIRE(n_streams <= 65535, DD_E_ARG, "%s: n_streams %d above 65535", who, n_streams);
    }
    if (ingest_is_422(pixel_format)) {
        DD_REQUIRE(src_w % 2 == 0, DD_E_ARG, "%s: src_w %d must be even for 4:2:2 frames", who, src_w);
        DD_REQUIRE(n_streams <= 65535, DD_E_ARG, "%s: n_streams %d above 65535", who, n_streams);
    }
    if (ingest_is_raw8(pixel_format)) DD_REQUIRE(n_streams <= 65535, DD_E_ARG, "%s: n_streams %d above 65535", who, n_streams);
    const bool any_size = pixel_format == INGEST_JPEG && (jpeg_flags & DD_JPEGDEC_ANY_SIZE) != 0;
    const bool auto_scale = any_size && jpeg_scale == 0;        // the draft rule per file; the slots are sized for scale 1
    if (auto_scale) jpeg_scale = 1;
    DD_REQUIRE(jpeg_scale == 1 || jpeg_scale == 2 || jpeg_scale == 4 || jpeg_scale == 8, DD_E_ARG, "%s: scale %d is none of 1, 2, 4, 8", who, jpeg_scale);
    DD_HIP(hipSetDevice(ctx->device));
    dd_ingest *g = new dd_ingest();
    g->ctx = ctx; g->slots = slots; g->S = n_streams; g->sh = src_h; g->sw = src_w; g->dh = dst_h; g->dw = dst_w;
    g->flip = flip != 0;
    g->jh = (src_h + jpeg_scale - 1) / jpeg_scale, g->jw = (src_w + jpeg_scale - 1) / jpeg_scale;
    g->transform = g->flip || g->jh != dst_h || g->jw != dst_w || any_size;      // any size: always through the staging buffer and crop_resize
    g->jflags = jpeg_flags, g->jscale = jpeg_scale, g->any_size = any_size, g->auto_scale = auto_scale;
    g->format = pixel_format;
    g->raw_bytes = pixel_format ? (size_t)n_streams * src_h * src_w * 3 / 2 : (size_t)n_streams * src_h * src_w * 3;
    if (pixel_format == INGEST_JPEG) g->raw_bytes = jpeg_slot_bytes;
    if (ingest_is_422(pixel_format)) g->raw_bytes = (size_t)n_streams * src_h * src_w * 2;
    if (ingest_is_raw8(pixel_format)) g->raw_bytes = (size_t)n_streams * src_h * src_w;
    g->own_out = g->transform || pixel_format != 0;          // BGR without a transform: the uploaded frames are the output
    g->fused = !(getenv("DD_INGEST_YUV_FUSED") && atoi(getenv("DD_INGEST_YUV_FUSED")) == 0);
    if (pixel_format == INGEST_JPEG) g->fused = false;      // decode into the staging buffer, then crop_resize
    g->out_bytes = (size_t)n_streams * dst_h * dst_w * 3;
    DD_HIP(hipStreamCreateWithFlags(&g->copy, hipStreamNonBlocking));
    for (int i = 0; i < slots; ++i) {
        uint8_t *h = nullptr, *d = nullptr, *o = nullptr;
        DD_HIP(hipHostMalloc(reinterpret_cast<void **>(&h), g->raw_bytes, hipHostMallocDefault));
        if (pixel_format != INGEST_JPEG) DD_HIP(hipMalloc(reinterpret_cast<void **>(&d), g->raw_bytes + 64));       // the decoder holds the files' device twin
        if (g->own_out) DD_HIP(hipMalloc(reinterpret_cast<void **>(&o), g->out_bytes + 64));
        else o = d;
        hipEvent_t r, dn;
        DD_HIP(hipEventCreateWithFlags(&r, hipEventDisableTiming));
        DD_HIP(hipEventCreateWithFlags(&dn, hipEventDisableTiming));
        g->h_raw.push_back(h); g->d_raw.push_back(d); g->d_out.push_back(o);
        g->ready.push_back(r); g->done.push_back(dn); g->used.push_back(0); g->submitted.push_back(0);
    }
    if (g->format && g->transform && !g->fused)
        DD_HIP(hipMalloc(reinterpret_cast<void **>(&g->d_stage), (size_t)n_streams * g->jh * g->jw * 3 + 64));
    if (g->transform && !(g->format && g->fused)) {
        std::vector<int> boxes((size_t)n_streams * 8, 0);
        for (int z = 0; z < n_streams; ++z) {
            int *b = boxes.data() + (size_t)z * 8;
            b[0] = 0; b[1] = 0; b[2] = g->jw; b[3] = g->jh; b[4] = z; b[5] = g->flip;
        }
        DD_HIP(hipMalloc(&g->d_boxes, boxes.size() * sizeof(int)));
        DD_HIP(hipMemcpy(g->d_boxes, boxes.data(), boxes.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    if (pixel_format == INGEST_JPEG) {
        if (int rc = dd_jpegdec_create_ex(ctx, src_h, src_w, jpeg_scale, jpeg_flags, n_streams, (int64_t)jpeg_slot_bytes, &g->dec)) return rc;
        for (int i = 0; i < slots; ++i) {
            dd_jpeg_info *r = nullptr;
            int *hs = nullptr, *ds = nullptr;
            DD_HIP(hipHostMalloc(reinterpret_cast<void **>(&r), (size_t)n_streams * sizeof(dd_jpeg_info), hipHostMallocDefault));
            DD_HIP(hipHostMalloc(reinterpret_cast<void **>(&hs), (size_t)n_streams * sizeof(int), hipHostMallocDefault));
            DD_HIP(hipMalloc(reinterpret_cast<void **>(&ds), (size_t)n_streams * sizeof(int)));
            g->h_recs.push_back(r); g->h_status.push_back(hs); g->d_status.push_back(ds);
            if (jpeg_flags & DD_JPEGDEC_PROGRESSIVE) {
                dd_jpeg_scans *sc = nullptr;
                DD_HIP(hipHostMalloc(reinterpret_cast<void **>(&sc), (size_t)n_streams * sizeof(dd_jpeg_scans), hipHostMallocDefault));
                memset(sc, 0, (size_t)n_streams * sizeof(dd_jpeg_scans));
                g->h_scans.push_back(sc);
            }
            g->fill.push_back(0); g->stale.push_back(1);
            if (any_size) {
                int *hb = nullptr;
                DD_HIP(hipHostMalloc(reinterpret_cast<void **>(&hb), (size_t)n_streams * 8 * sizeof(int), hipHostMallocDefault));
                g->h_boxes.push_back(hb);
                g->sizes.emplace_back((size_t)n_streams * 3, 0);
                g->scales.emplace_back((size_t)n_streams, jpeg_scale);
            }
        }
    }
    *out = g;
    return DD_OK;
}

// A JPEG slot before its first put after a submit: wait until the last upload has left it, then empty it.  Caller holds g->mu.
static int ingest_jpeg_reset(dd_ingest *g, int slot) {
    if (!g->stale[slot]) return DD_OK;
    if (g->submitted[slot]) DD_HIP(hipEventSynchronize(g->ready[slot]));
    for (int z = 0; z < g->S; ++z) {
        memset(&g->h_recs[slot][z], 0, offsetof(dd_jpeg_info, quant));      // the scalar fields; the next parse rewrites the tables
        g->h_recs[slot][z].status = DD_JPEG_ST_NO_FRAME;
    }
    if (g->any_size) std::fill(g->sizes[slot].begin(), g->sizes[slot].end(), 0);
    g->fill[slot] = 0;
    g->stale[slot] = 0;
    return DD_OK;
}

extern "C" {

int dd_ingest_create_jpeg(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int64_t slot_bytes,
                          dd_ingest **out) {
    DD_REQUIRE(slot_bytes >= 1, DD_E_ARG, "dd_ingest_create_jpeg: slot_bytes %lld", (long long)slot_bytes);
    return ingest_create("dd_ingest_create_jpeg", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, INGEST_JPEG, out, (size_t)slot_bytes);
}

int dd_ingest_create_jpeg_scaled(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int scale, int64_t slot_bytes,
                                 dd_ingest **out) {
    DD_REQUIRE(slot_bytes >= 1, DD_E_ARG, "dd_ingest_create_jpeg_scaled: slot_bytes %lld", (long long)slot_bytes);
    return ingest_create("dd_ingest_create_jpeg_scaled", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, INGEST_JPEG, out, (size_t)slot_bytes, scale);
}

int dd_ingest_create_jpeg_ex(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int scale, int flags, int64_t slot_bytes,
                             dd_ingest **out) {
    DD_REQUIRE(slot_bytes >= 1, DD_E_ARG, "dd_ingest_create_jpeg_ex: slot_bytes %lld", (long long)slot_bytes);
    return ingest_create("dd_ingest_create_jpeg_ex", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, INGEST_JPEG, out, (size_t)slot_bytes, scale, flags);
}

int dd_ingest_jpeg_put(dd_ingest *g, int slot, int stream, const uint8_t *data_host, int64_t n) {
    DD_REQUIRE(g && data_host && slot >= 0 && slot < g->slots && stream >= 0 && stream < g->S && n >= 1 && n <= 0x7fffffffll, DD_E_ARG,
               "dd_ingest_jpeg_put: bad argument");
    DD_REQUIRE(g->format == INGEST_JPEG, DD_E_STATE, "dd_ingest_jpeg_put: the ring does not hold JPEG files");
    DD_DEVICE(g->ctx);
    size_t at;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        if (int rc = ingest_jpeg_reset(g, slot)) return rc;
        at = (g->fill[slot] + 63) & ~(size_t)63;
        DD_REQUIRE(at + (size_t)n <= g->raw_bytes, DD_E_CAPACITY, "dd_ingest_jpeg_put: a file of %lld bytes at offset %zu of a slot of %zu bytes", (long long)n, at,
                   g->raw_bytes);
        g->fill[slot] = at + (size_t)n;
    }
    // the copy and the parse run outside the lock: decoder threads share that work.  A stream's record belongs to the thread that puts it.
    memcpy(g->h_raw[slot] + at, data_host, (size_t)n);
    dd_jpeg_info *rec = &g->h_recs[slot][stream];
    ddk::jpegdec_parse(g->h_raw[slot] + at, (size_t)n, g->sh, g->sw, rec, g->h_scans.empty() ? nullptr : &g->h_scans[slot][stream], g->jflags);
    rec->file_offset = (int64_t)at;
    if (g->any_size) {                                          // a refused header leaves zeros; a file too large keeps what it stated
        int *sz = &g->sizes[slot][(size_t)stream * 3];
        sz[0] = sz[1] = sz[2] = 0;
        if (rec->status == DD_JPEG_ST_OK || rec->status == DD_JPEG_ST_SIZE) {
            const int sc = g->auto_scale ? dd_jpeg_draft_scale(rec->width, rec->height, g->dw, g->dh) : g->jscale;
            sz[0] = rec->width, sz[1] = rec->height, sz[2] = sc;
            g->scales[slot][stream] = sc;
        }
    }
    return DD_OK;
}

int dd_ingest_source_sizes(dd_ingest *g, int slot, int *sizes_host) {
    DD_REQUIRE(g && sizes_host && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_source_sizes: bad argument");
    DD_REQUIRE(g->any_size, DD_E_STATE, "dd_ingest_source_sizes: the ring was not made with DD_JPEGDEC_ANY_SIZE");
    memcpy(sizes_host, g->sizes[slot].data(), (size_t)g->S * 3 * sizeof(int));
    return DD_OK;
}

int dd_ingest_status(dd_ingest *g, int slot, int *status_host) {
    DD_REQUIRE(g && status_host && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_status: bad argument");
    DD_REQUIRE(g->format == INGEST_JPEG, DD_E_STATE, "dd_ingest_status: the ring does not hold JPEG files");
    DD_REQUIRE(g->submitted[slot], DD_E_STATE, "dd_ingest_status: slot %d was never submitted", slot);
    DD_DEVICE(g->ctx);
    DD_HIP(hipEventSynchronize(g->ready[slot]));
    memcpy(status_host, g->h_status[slot], (size_t)g->S * sizeof(int));
    return DD_OK;
}

int dd_ingest_create(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip,
                     dd_ingest **out) {
    return ingest_create("dd_ingest_create", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, 0, out);
}

int dd_ingest_create_format(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip,
                            int pixel_format, dd_ingest **out) {
    return ingest_create("dd_ingest_create_format", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, pixel_format, out);
}

// Layout and sizes are checked before ctx is touched: a bad call is answered with a code on a machine without a GPU.
int dd_ingest_create_raw8(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int layout,
                          dd_ingest **out) {
    DD_REQUIRE(ingest_is_raw8(layout), DD_E_ARG, "dd_ingest_create_raw8: layout %d is none of 6 (RGGB), 7 (GRBG), 8 (GBRG), 9 (BGGR), 10 (gray)",
               layout);
    if (layout != INGEST_GRAY) {
        DD_REQUIRE(src_w >= 3, DD_E_ARG, "dd_ingest_create_raw8: src_w %d below 3 (a demosaiced site needs both neighbours)", src_w);
        DD_REQUIRE(src_h >= 3, DD_E_ARG, "dd_ingest_create_raw8: src_h %d below 3 (a demosaiced site needs both neighbours)", src_h);
    }
    DD_REQUIRE((int64_t)src_h * src_w <= INT_MAX - 256, DD_E_ARG, "dd_ingest_create_raw8: src_h %d x src_w %d is more pixels than a launch indexes",
               src_h, src_w);
    return ingest_create("dd_ingest_create_raw8", ctx, slots, n_streams, src_h, src_w, dst_h, dst_w, flip, layout, out, 0, 1, 0, true);
}

int dd_ingest_destroy(dd_ingest *g) {
    if (!g) return DD_OK;
    (void)hipStreamSynchronize(g->copy);
    for (int i = 0; i < g->slots; ++i) {
        (void)hipHostFree(g->h_raw[i]);
        if (g->own_out) (void)hipFree(g->d_out[i]);
        if (g->d_raw[i]) (void)hipFree(g->d_raw[i]);
        (void)hipEventDestroy(g->ready[i]);
        (void)hipEventDestroy(g->done[i]);
    }
    if (g->d_boxes) (void)hipFree(g->d_boxes);
    if (g->d_stage) (void)hipFree(g->d_stage);
    for (dd_jpeg_scans *sc : g->h_scans) (void)hipHostFree(sc);
    for (int *hb : g->h_boxes) (void)hipHostFree(hb);
    for (size_t i = 0; i < g->h_recs.size(); ++i) {
        (void)hipHostFree(g->h_recs[i]);
        (void)hipHostFree(g->h_status[i]);
        (void)hipFree(g->d_status[i]);
    }
    if (g->dec) (void)dd_jpegdec_destroy(g->dec);
    (void)hipStreamDestroy(g->copy);
    delete g;
    return DD_OK;
}

int dd_ingest_host_slot(dd_ingest *g, int slot, uint8_t **host_ptr, int64_t *n_bytes) {
    DD_REQUIRE(g && host_ptr && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_host_slot: bad argument");
    DD_REQUIRE(g->format != INGEST_JPEG, DD_E_STATE, "dd_ingest_host_slot: a JPEG ring's slots are filled through dd_ingest_jpeg_put");
    *host_ptr = g->h_raw[slot];
    if (n_bytes) *n_bytes = (int64_t)g->raw_bytes;
    return DD_OK;
}

// The host may refill a pinned slot once its previous upload has left it.
int dd_ingest_wait_uploaded(dd_ingest *g, int slot) {
    DD_REQUIRE(g && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_wait_uploaded: bad slot");
    DD_DEVICE(g->ctx);
    if (g->submitted[slot]) DD_HIP(hipEventSynchronize(g->ready[slot]));
    return DD_OK;
}

int dd_ingest_submit(dd_ingest *g, int slot) {
    DD_REQUIRE(g && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_submit: bad slot");
    DD_DEVICE(g->ctx);
    if (g->format == INGEST_JPEG) {
        std::lock_guard<std::mutex> lk(g->mu);
        if (int rc = ingest_jpeg_reset(g, slot)) return rc;                         // a submit without a put: every stream reports "no frame"
        if (g->used[slot]) DD_HIP(hipStreamWaitEvent(g->copy, g->done[slot], 0));
        uint8_t *dst = g->transform ? g->d_stage : g->d_out[slot];
        if (g->any_size) {                                      // one box per stream from its record: the file's own frame in its staging slot
            int *hb = g->h_boxes[slot];
            for (int z = 0; z < g->S; ++z) {
                const dd_jpeg_info &r = g->h_recs[slot][z];
                const int sc = g->scales[slot][z], ok = r.status == DD_JPEG_ST_OK && sc >= 1;
                const int ow = ok ? (r.width + sc - 1) / sc : 0, oh = ok ? (r.height + sc - 1) / sc : 0;
                int *b = hb + (size_t)z * 8;
                b[0] = 0, b[1] = g->flip ? g->jh - oh : 0, b[2] = ow, b[3] = oh, b[4] = z, b[5] = g->flip, b[6] = 0, b[7] = 0;      // crop_resize flips within the slot
            }
            DD_HIP(hipMemcpyAsync(g->d_boxes, hb, (size_t)g->S * 8 * sizeof(int), hipMemcpyHostToDevice, g->copy));
        }
        int rc = ddk::jpegdec_launch(g->dec, g->h_recs[slot], g->h_scans.empty() ? nullptr : g->h_scans[slot], g->h_raw[slot], g->fill[slot], g->S, dst, g->d_status[slot],
                                     g->copy, nullptr, g->any_size ? g->scales[slot].data() : nullptr);
        if (rc == DD_OK && g->transform) rc = ddk::crop_resize(g->copy, g->d_stage, g->jh, g->jw, g->d_boxes, g->S, g->dh, g->dw, g->d_out[slot]);
        if (rc != DD_OK) return rc;
        DD_HIP(hipMemcpyAsync(g->h_status[slot], g->d_status[slot], (size_t)g->S * sizeof(int), hipMemcpyDeviceToHost, g->copy));
        DD_HIP(hipEventRecord(g->ready[slot], g->copy));
        g->submitted[slot] = 1;
        g->stale[slot] = 1;
        return DD_OK;
    }
    if (g->used[slot]) DD_HIP(hipStreamWaitEvent(g->copy, g->done[slot], 0));       // the previous consumer of this slot
    DD_HIP(hipMemcpyAsync(g->d_raw[slot], g->h_raw[slot], g->raw_bytes, hipMemcpyHostToDevice, g->copy));
    if (g->format) {
        const bool packed = ingest_is_422(g->format), raw8 = ingest_is_raw8(g->format);
        auto convert = [&](uint8_t *dst) {
            if (raw8) return ddk::raw8_to_bgr(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, 0, 0, dst);
            return packed ? ddk::yuv422_to_bgr(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, 0, 0, dst)
                          : ddk::yuv420_to_bgr(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, 0, 0, 0, dst);
        };
        int rc;
        if (!g->transform) {                                    // the converter writes straight into the slot's output
            rc = convert(g->d_out[slot]);
        } else if (g->fused && raw8) {
            rc = ddk::raw8_resize(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, g->flip, g->dh, g->dw, g->d_out[slot]);
        } else if (g->fused) {
            rc = packed ? ddk::yuv422_resize(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, g->flip, g->dh, g->dw, g->d_out[slot])
                        : ddk::yuv420_resize(g->copy, g->d_raw[slot], g->S, g->sh, g->sw, g->format, g->flip, g->dh, g->dw, g->d_out[slot]);
        } else {                                                // one staging buffer serves every slot: the copy stream runs them in order
            rc = convert(g->d_stage);
            if (rc == DD_OK) rc = ddk::crop_resize(g->copy, g->d_stage, g->sh, g->sw, g->d_boxes, g->S, g->dh, g->dw, g->d_out[slot]);
        }
        if (rc != DD_OK) return rc;
    } else if (g->transform) {
        int rc = ddk::crop_resize(g->copy, g->d_raw[slot], g->sh, g->sw, g->d_boxes, g->S, g->dh, g->dw, g->d_out[slot]);
        if (rc != DD_OK) return rc;
    }
    DD_HIP(hipEventRecord(g->ready[slot], g->copy));
    g->submitted[slot] = 1;
    return DD_OK;
}

int dd_ingest_acquire(dd_ingest *g, int slot, void *consumer_stream, const uint8_t **frames_dev) {
    DD_REQUIRE(g && frames_dev && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_acquire: bad argument");
    DD_DEVICE(g->ctx);
    DD_HIP(hipStreamWaitEvent(dd_pick_stream(g->ctx, consumer_stream), g->ready[slot], 0));
    *frames_dev = g->d_out[slot];
    return DD_OK;
}

int dd_ingest_release(dd_ingest *g, int slot, void *consumer_stream) {
    DD_REQUIRE(g && slot >= 0 && slot < g->slots, DD_E_ARG, "dd_ingest_release: bad slot");
    DD_DEVICE(g->ctx);
    DD_HIP(hipEventRecord(g->done[slot], dd_pick_stream(g->ctx, consumer_stream)));
    g->used[slot] = 1;
    return DD_OK;
}

}  // extern "C"
