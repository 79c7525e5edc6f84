// Shared host-side plumbing for libdeepdish_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/deepdish_hip.h"

void dd_set_error(const char *fmt, ...);

#define DD_HIP(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            dd_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,            \
                         hipGetErrorString(e_));                                  \
            return DD_E_HIP;                                                      \
        }                                                                         \
    } while (0)

#define DD_REQUIRE(cond, code, ...)                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            dd_set_error(__VA_ARGS__);                                            \
            return (code);                                                        \
        }                                                                         \
    } while (0)

#define DD_LAUNCH_CHECK() DD_HIP(hipGetLastError())

// Every entry point that launches or allocates selects its context's device first: a fresh host thread starts on
// device 0 whatever device the handle was created on.
#define DD_DEVICE(ctx) DD_HIP(hipSetDevice((ctx)->device))

// Growable device scratch buffer (never shrinks; growth happens outside graph capture).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return DD_OK;
        if (p) { DD_HIP(hipFree(p)); p = nullptr; cap = 0; }
        size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
        DD_HIP(hipMalloc(&p, want));
        cap = want;
        return DD_OK;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return DD_OK;
        if (p) { DD_HIP(hipHostFree(p)); p = nullptr; cap = 0; }
        size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
        DD_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return DD_OK;
    }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

// One-time per-device set-up inside a launcher (hipFuncSetAttribute is a per-device property): run(device) returns
// true to exactly one caller per device, which does the set-up while the others wait for it.
#include <atomic>
#include <mutex>
struct DevOnce {
    std::atomic<uint64_t> done{0};
    std::mutex mu;
    template <class F> int run(int device, F &&f) {
        const uint64_t bit = 1ull << (device & 63);
        if (done.load(std::memory_order_acquire) & bit) return DD_OK;
        std::lock_guard<std::mutex> lk(mu);
        if (done.load(std::memory_order_relaxed) & bit) return DD_OK;
        const int rc = f();
        if (rc == DD_OK) done.fetch_or(bit, std::memory_order_release);
        return rc;
    }
};

struct dd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf scratch[4];     // general per-call scratch (index by purpose inside one call)
    PinBuf pin[2];
};

static inline hipStream_t dd_pick_stream(dd_ctx *ctx, void *stream) {
    return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
}

// Switches from the environment.  dd_env_int: the number a variable holds, `def` when it is not set; dd_env_set: present at all.  A call site keeps
// its own convention on top ("0 turns off": dd_env_int(X, 1) != 0; "non-zero turns on": dd_env_int(X, 0) != 0) and its own lifetime (`static` = once
// per process).
static inline int dd_env_int(const char *name, int def) {
    const char *v = getenv(name);
    return v ? atoi(v) : def;
}
static inline bool dd_env_set(const char *name) { return getenv(name) != nullptr; }

static inline int dd_ceil_div(int a, int b) { return (a + b - 1) / b; }

// Compute units of a device (cached; 256 on MI355X): what the persistent one-workgroup-per-CU launches size their grids by.
static inline int dd_cu_count(int device) {
    static std::atomic<int> cache[64];
    int n = cache[device & 63].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
        cache[device & 63].store(n, std::memory_order_relaxed);
    }
    return n;
}

// XCD-aware block order (MI355X: 8 XCDs, each with a private 4 MiB L2; workgroups are dealt round-robin
// over them).  Maps the hardware's linear workgroup id to a logical id such that every XCD works on one
// contiguous 1/8 of the logical range: neighbouring tiles (shared halo rows, shared weight panels) then
// hit in the same L2 instead of being fetched by up to 8 of them.  Bijective for any count.
__device__ __forceinline__ unsigned dd_xcd_remap(unsigned id, unsigned n) {
    const unsigned q = n >> 3, r = n & 7u, xcd = id & 7u, slot = id >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

struct JdPerScale;                              // csrc/jpeg_dec_plan.h

// ---- kernel launchers shared between the flat C ABI and the tracker / pipeline handles ----
namespace ddk {
int kf_initiate(hipStream_t s, double *means, double *covs, const int *slots, const double *xyah, int n);
int kf_predict(hipStream_t s, double *means, double *covs, const int *slots, int n);
int kf_project(hipStream_t s, const double *means, const double *covs, const int *slots, int n,
               double *pm, double *pc);
int kf_update(hipStream_t s, double *means, double *covs, const int *slots, const double *xyah, int n);
int kf_gate(hipStream_t s, const double *means, const double *covs, const int *slots, int n,
            const double *xyah, int n_det, int only_position, double *out_d2);
int iou_cost(hipStream_t s, const double *tlwh_t, const int *tsu, int n_t, const double *tlwh_d, int n_d,
             double *out);
int normalize_rows(hipStream_t s, const float *in, float *out, int n);   // rows of 128 f32
// gallery rows are pre-normalised; target t owns rows [row_start[t], row_start[t]+row_count[t])
int cosine_nn_cost(hipStream_t s, const float *gallery_n, const long long *row_start, const int *row_count,
                   int n_t, const float *feats_n, int n_d, double *out, int ld_out);
int euclidean_nn_cost(hipStream_t s, const float *gallery, const long long *row_start, const int *row_count,
                      int n_t, const float *feats, int n_d, double *out, int ld_out);   // rows NOT normalised
int nms(hipStream_t s, const double *boxes, const double *keys, int k, double thr, int mode,
        int *out_idx, int *out_n, void *scratch, size_t scratch_bytes);
size_t nms_scratch_bytes(int k);
int nms_ex(hipStream_t s, const void *boxes, const void *keys, int k, double thr, int mode, int max_keep, int *out_idx,
           int *out_n, void *scratch, size_t scratch_bytes);
int nms_batched_small(hipStream_t s, const double *boxes, const double *keys, const int *d_offsets, int n_problems,
                      double thr, int mode, int *out_idx, int *out_n);
int nms_batched_small_streams(hipStream_t s, const double *boxes, const double *keys, const int *d_offsets, int n_problems,
                              const double *d_thrs, int mode, int *out_idx, int *out_n);   // one threshold per problem
// tracker fused kernels
int crop_box_host(const int64_t *b, int ph, int pw, int H, int W, int *sx, int *sy, int *cw, int *ch);
int crop_box_host_f64(const double *b, int ph, int pw, int H, int W, int *sx, int *sy, int *cw, int *ch);
// d_boxes: device array of {sx, sy, cw, ch, frame, 0, 0, 0} int32 records
int crop_resize(hipStream_t s, const uint8_t *frames, int H, int W, const void *d_boxes, int n, int oh, int ow, uint8_t *out);
// 4:2:0 YUV -> BGR (yuv.hip); layout 1 NV12, 2 I420; pitch / chroma_offset / frame_stride 0 = dense
int yuv420_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t chroma_offset,
                  int64_t frame_stride, uint8_t *dst);
// the same + cv2.flip(frame, 0) + INTER_LINEAR stretch of n dense frames in one launch: the bytes of yuv420_to_bgr then crop_resize
int yuv420_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int layout, int flip, int oh, int ow, uint8_t *out);
// packed 4:2:2 YUV -> BGR (yuv.hip); order 4 YUY2, 5 UYVY; pitch / frame_stride 0 = dense; and its convert + flip + stretch of n dense frames
int yuv422_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int order, int pitch, int64_t frame_stride, uint8_t *dst);
int yuv422_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int order, int flip, int oh, int ow, uint8_t *out);
// 8-bit raw sensor frames -> BGR (bayer.hip); layout 6 RGGB, 7 GRBG, 8 GBRG, 9 BGGR, 10 gray; pitch / frame_stride 0 = dense; and its convert +
// flip + stretch of n dense frames
int raw8_to_bgr(hipStream_t s, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t frame_stride, uint8_t *dst);
int raw8_resize(hipStream_t s, const uint8_t *src, int n, int H, int W, int layout, int flip, int oh, int ow, uint8_t *out);
// the JPEG decoder's two halves (jpeg_dec.hip), as the ingest ring drives them: a header into a record with the status a decoder of h x w
// gives it (returned too; the reason is left in dd_last_error), and upload + kernels for n records without a host wait
// scans / scans_host: NULL, or (a decoder made with DD_JPEGDEC_PROGRESSIVE) where each file's scan script goes, kept like the records
// flags: the decoder's DD_JPEGDEC_* (0: every file must be h x w and define its tables); scales: NULL, or one scale denominator per file
// (a decoder made with DD_JPEGDEC_ANY_SIZE)
int jpegdec_parse(const uint8_t *file, size_t n, int h, int w, dd_jpeg_info *rec, dd_jpeg_scans *scans, int flags = 0);
int jpegdec_launch(dd_jpegdec *dec, dd_jpeg_info *recs_host, dd_jpeg_scans *scans_host, const uint8_t *bytes_host, size_t n_bytes, int n, uint8_t *out_dev, int *status_dev,
                   hipStream_t s, hipEvent_t uploaded, const int *scales = nullptr);
// csrc/jpeg_dec_any.hip: the pixel stage of a DD_JPEGDEC_ANY_SIZE decoder; per_scale: the call plan's (csrc/jpeg_dec_plan.h)
int jpegdec_pixels_any(hipStream_t s, int n, int max_bands, long long coef_stride, long long plane_stride, const JdPerScale &per_scale, const dd_jpeg_info *recs,
                       const int *mark, const int16_t *coef, uint8_t *planes, uint8_t *out_dev, int OH, int OW);
int resize_lanczos(hipStream_t s, int device, const uint8_t *src, int H, int W, int src_c, int swap_rb, uint8_t *dst,
                   int h, int w, uint8_t *tmp, int batch);
size_t ssd_post_scratch_bytes(int n_anchors, int batch);
int ssd_postprocess(hipStream_t s, const float *raw, const float *anchors, int n_anchors, int n_classes, int max_det,
                    float score_thr, float iou_thr, float *boxes, float *classes, float *scores, int *count, int batch,
                    void *scratch, size_t scratch_bytes);
size_t ssd_post_decoded_scratch_bytes(int n_anchors, int batch);
int ssd_postprocess_decoded(hipStream_t s, const float *d_boxes, const float *d_score, const int *d_cls, const float *d_keys,
                            int n_anchors, int max_det, float score_thr, float iou_thr, float *boxes, float *classes, float *scores,
                            int *count, int batch, void *scratch, size_t scratch_bytes);
int ssd_regular_nms_raw(hipStream_t s, const float *raw, const float *anchors, int n_anchors, int n_classes, int max_det, int per_class,
                        float score_thr, float iou_thr, float *boxes, float *classes, float *scores, int *count, int batch);
int ssd_regular_nms_u8(hipStream_t s, const uint8_t *box_q, const uint8_t *cls_q, int cls_stride, const uint8_t *lut, const float *quant4,
                       const float *anchors, int n_anchors, int n_classes, int max_det, int per_class, float score_thr, float iou_thr,
                       float *boxes, float *classes, float *scores, int *count, int batch);
int ssd_finish(hipStream_t s, const float *boxes, const float *cls, const float *scores, int batch, int max_det, double conf,
               double iou_thr, double img_w, double img_h, double *out_boxes, int *out_cls, double *out_scores, int *out_n);
// YOLOv5 (post.hip): rows over the threshold per image, from the raw head or from the Detect layers' decoded rows; stretch or letterbox
int yolov5_decode(hipStream_t s, const float *raw, int n_rows, int n_cls, float thr, float img_w, float img_h, float *out_boxes,
                  float *out_scores, int *out_cls, int cap, int *out_n, int batch, void *scratch);
int yolov5_select(hipStream_t s, const float *boxes4, const float *conf, const int *cls, int n_rows, float thr, float img_w, float img_h,
                  float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n, int batch);
int yolov5_decode_letterbox(hipStream_t s, const float *raw, int n_rows, int n_cls, float thr, int img_w, int img_h, int net_w, int net_h,
                            float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n, int batch, void *scratch);
int yolov5_select_letterbox(hipStream_t s, const float *boxes4, const float *conf, const int *cls, int n_rows, float thr, int img_w, int img_h,
                            int net_w, int net_h, float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n, int batch);
int yolov5_pack(hipStream_t s, const float *boxes, const float *scores, const int *cls, const int *n_rows, int cap, int batch, float *packed);
int resize_lanczos_letterbox(hipStream_t s, int device, const uint8_t *src, int batch, int H, int W, int src_c, int swap_rb, uint8_t *dst, int h, int w,
                             int pad, uint8_t *tmp);
// what the batched pipeline launches on streams of its own: retained feature rows (featrows.hip), frame compaction (gather.hip), MOG2 (mog2.hip)
int feature_rows_carry(hipStream_t s, const float *fresh, const float *store, float *out, float *store_new, const int *d_table, int n_entries);
int gather_frames(hipStream_t s, const uint8_t *src, long long frame_bytes, const int *d_idx, int n, uint8_t *dst);
int mog2_apply_streams(dd_mog2 *m, hipStream_t s, const uint8_t *frames, const uint8_t *present_host, double learning_rate, uint8_t *mask,
                       uint8_t *masked);
int mog2_reset_streams(dd_mog2 *m, hipStream_t s, const int *streams_host, int n);
int mask_box_count(hipStream_t s, const uint8_t *mask, int H, int W, const int *d_boxes, const int *d_box_stream, int K, int *d_counts);
// non-zero bytes of whole mask planes (gate.hip): d_streams int32 [n] or NULL = planes 0 .. n - 1; d_counts int32 [n]
int mask_stream_count(hipStream_t s, const uint8_t *mask, int H, int W, const int *d_streams, int n, int *d_counts);
// a group of trackers sharing one pool (tracker.hip): every stream's tracker of a pipeline, stepped together in three phases
int tracker_group_create(dd_ctx *ctx, int n, double max_cos, double max_iou, int max_age, int n_init, int budget, int tcap,
                         int gcap, dd_tracker **out);
int tracker_group_set_metric(dd_tracker *any, int metric);
int tracker_group_set_association(dd_tracker *any, int where);
long long tracker_group_stream_param_launches(const dd_tracker *any);
int tracker_set_params(dd_tracker *t, const double *max_cos, const double *max_iou, const int *max_age, const int *n_init);
int tracker_reset(dd_tracker *t);
int trackers_predict(dd_tracker **ts, int S);
int trackers_update_begin(dd_tracker **ts, int S, const double *tlwh_host, const float *feats, int feats_on_device,
                          const int *det_off);
int trackers_update_match(dd_tracker **ts, int S);
int trackers_update_end(dd_tracker **ts, int S);
int tracker_read_host(dd_tracker *t, int which, int64_t *ints6_host, double *means_host);
// stream snapshots: one tracker's tables out (tracker_export) and in (reserve, then import, then flush), and the gallery kernels (snapshot.hip)
struct TrackerPoolView {
    float *const *d_arenas;
    double *d_means, *d_covs, max_cos, max_iou;
    int arena_shift, metric, budget, tcap, max_age, n_init;
    bool upd_inflight;
};
struct TrackView { int64_t id; int state, tsu, hits, age, last_det, slot, slot_total, n_rows, n_chunks; const int *chunks; };
struct TrackLoad { int64_t id; int state, tsu, hits, age, last_det, slot_total, n_rows; const double *mean; };
void tracker_pool_view(dd_tracker *t, TrackerPoolView *v);
int tracker_export(dd_tracker *t, int64_t *next_id, std::vector<TrackView> &live, std::vector<TrackView> &dead);
int tracker_pool_reserve_chunks(dd_tracker *any, size_t n);
int tracker_import(dd_tracker *t, int64_t next_id, const TrackLoad *tracks, int n_live, int n_dead, std::vector<int> &slots_out,
                   std::vector<int> &chunks_out);
int tracker_gallery_flush(dd_tracker *any, hipStream_t s);
int chunk_rows_gather(hipStream_t s, float *const *d_arenas, int arena_shift, const int *d_chunks, const int *d_table, int n_entries,
                      float *dense, const double *means, const double *covs, double *state);
int chunk_rows_scatter(hipStream_t s, float *const *d_arenas, int arena_shift, const int *d_chunks, const int *d_table, int n_entries,
                       const float *dense, double *means, double *covs, const double *state);
int mog2_stream_planes(dd_mog2 *m, int stream, void **rec, void **m2, void **nm, long long **nframes, int *history, float *var_threshold,
                       int *detect_shadows);
void pyset_difference_order(const std::vector<int> &a, const std::vector<int> &b, std::vector<int> &out);
int lsap(const double *cost, int nr, int nc, int *rows, int *cols);   // host; returns pair count or -1
int gather_state(hipStream_t s, const double *means, const double *covs, const int *slots, int n,
                 double *out_means, double *out_covs);
// the association decision of one stream (tracker.py:95-133 _match): host form (tracker.hip) and one wave per stream (assoc.hip).
// matches: (row, det) pairs flattened.  app / iou: [T][n] row-major; state / tsu: per row.
void match_decide_host(const double *app, const double *iou, int T, int n, const int *state, const int *tsu, double max_cos,
                       double max_iou, int max_age, std::vector<int> &matches, std::vector<int> &un_rows, std::vector<int> &un_dets);
size_t assoc_out_ints(int T, int n);   // ints one stream's decision takes in assoc_match's output
int assoc_match(hipStream_t s, const double *cost, const int *row_state, const int *row_tsu, const int *desc, int n_streams,
                double max_cos, double max_iou, int max_age, int *out);
// the same with the three values per decided stream: par_d f64 [n_streams][2] = max_cos, max_iou; par_age int [n_streams] (device)
int assoc_match_streams(hipStream_t s, const double *cost, const int *row_state, const int *row_tsu, const int *desc, int n_streams,
                        const double *par_d, const int *par_age, int *out);
}  // namespace ddk
