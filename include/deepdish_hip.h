/* deepdish_hip.h -- C ABI of libdeepdish_hip.so (MI355X / gfx950 only).
 *
 * The upstream project (AdaptiveCity/deepdish) is pure Python and has NO FFI: its
 * hot path is a set of duck-typed Python plugin objects.  This header is therefore
 * the boundary a maintainer would bind with ctypes; every entry
 * point cites the reference interface (file:line, relative to the upstream tree)
 * whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (DD_E_*); the message of the
 *     last error on the calling thread is dd_last_error().  Nothing throws.
 *   - pointers are DEVICE pointers unless the parameter name ends in _host.
 *   - matrices are dense row-major; f64 = double, f32 = float, boxes are tlwh
 *     (top-left x, top-left y, width, height) unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the context's own stream).
 *     Calls only enqueue work; the caller synchronises, except for *_host outputs,
 *     which are complete on return.
 *   - the library never takes ownership of caller memory.
 */
#ifndef DEEPDISH_HIP_H
#define DEEPDISH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_OK            0
#define DD_E_ARG        -1   /* bad argument (NULL, negative size, capacity exceeded) */
#define DD_E_HIP        -2   /* a HIP runtime call failed */
#define DD_E_STATE      -3   /* call order / handle state */
#define DD_E_CAPACITY   -4   /* a fixed capacity (tracks, boxes, batch) would be exceeded */

#define DD_FEATURE_DIM 128   /* re-ID feature length, tools/freeze_model.py:139-147 */

typedef struct dd_ctx dd_ctx;
typedef struct dd_tracker dd_tracker;
typedef struct dd_net dd_net;
typedef struct dd_pipeline dd_pipeline;

const char *dd_last_error(void);
int dd_version(void);

/* One context per (thread, device): owns a stream and scratch memory.  The reference
 * runs the detector and the encoder on different pool threads (deepdish.py:935,1008);
 * give each its own context. */
int dd_ctx_create(int device, dd_ctx **out);
int dd_ctx_destroy(dd_ctx *ctx);
int dd_ctx_stream(dd_ctx *ctx, void **out_stream);
int dd_ctx_sync(dd_ctx *ctx);

/* ---------------------------------------------------------------- Kalman filter (f64)
 * State layout: means[slot][8] = (cx, cy, a, h, vx, vy, va, vh), covs[slot][8][8].
 * `slots` selects rows of the state arrays (NULL = rows 0..n-1). */

/* deep_sort/kalman_filter.py:55-86  KalmanFilter.initiate */
int dd_kf_initiate(dd_ctx *ctx, double *means, double *covs, const int *slots,
                   const double *xyah, int n, void *stream);
/* deep_sort/kalman_filter.py:88-123  KalmanFilter.predict (Track.predict, track.py:113-125) */
int dd_kf_predict(dd_ctx *ctx, double *means, double *covs, const int *slots, int n, void *stream);
/* deep_sort/kalman_filter.py:125-152  KalmanFilter.project -> proj_mean[n][4], proj_cov[n][4][4] */
int dd_kf_project(dd_ctx *ctx, const double *means, const double *covs, const int *slots, int n,
                  double *proj_mean, double *proj_cov, void *stream);
/* deep_sort/kalman_filter.py:154-186  KalmanFilter.update; pair i updates slots[i] with xyah[i] */
int dd_kf_update(dd_ctx *ctx, double *means, double *covs, const int *slots,
                 const double *xyah, int n, void *stream);
/* deep_sort/kalman_filter.py:188-229  KalmanFilter.gating_distance for every (track, detection):
 * out_d2[n][n_det] squared Mahalanobis distance; only_position != 0 uses (cx, cy) only. */
int dd_kf_gate(dd_ctx *ctx, const double *means, const double *covs, const int *slots, int n,
               const double *xyah, int n_det, int only_position, double *out_d2, void *stream);

/* ---------------------------------------------------------------- cost matrices */

/* deep_sort/iou_matching.py:7-39 iou + :42-81 iou_cost: out[n_t][n_d] = 1 - IoU (no +1 pixel).
 * rows with tsu[i] > 1 are filled with 1e5 (tsu may be NULL). */
int dd_iou_cost(dd_ctx *ctx, const double *tlwh_t, const int *tsu, int n_t,
                const double *tlwh_d, int n_d, double *out, void *stream);

/* deep_sort/nn_matching.py:31-54,78-96,156-177: per target t, min over its gallery rows of
 * (1 - a.b) with a, b L2-normalised in f32; result widened to f64 as nn_matching.py:174-176.
 * Target t owns gallery rows [offsets[t], offsets[t+1]).  out[n_t][n_d]. */
int dd_cosine_nn_cost(dd_ctx *ctx, const float *gallery, const int *offsets_host, int n_t,
                      const float *feats, int n_d, double *out, void *stream);

/* deep_sort/nn_matching.py:5-28,57-75: the "euclidean" metric -- per target t, min over its gallery rows g of
 * max(0, |g|^2 + |q|^2 - 2 g.q) in f32 (a SQUARED distance), widened to f64.  Same contract as dd_cosine_nn_cost;
 * gallery and feats are used as they are, NOT normalised. */
int dd_euclidean_nn_cost(dd_ctx *ctx, const float *gallery, const int *offsets_host, int n_t,
                         const float *feats, int n_d, double *out, void *stream);

/* deep_sort/preprocessing.py:6-73 non_max_suppression (greedy, +1 pixel, inter/area_other > thr).
 * `keys` is the sort key (scores, or y2 when the reference is called with scores=None).
 * out_idx[k] receives the surviving indices in pick order, *out_n their number (both device).
 * Equal keys: the higher original index first.  A NaN key ranks as the largest key (np.argsort places it last, so the reference
 * picks it first); it is treated as +inf, so NaN keys -- and a NaN beside a +inf key -- tie and go by index.  k <= 4096. */
int dd_nms(dd_ctx *ctx, const double *tlwh, const double *keys, int k, double max_overlap,
           int *out_idx, int *out_n, void *stream);

/* tools/ssd_mobilenet.py:59-98 nms_boxes for ONE class: xyxy boxes, IoU with +1 on the
 * intersection only, keep while IoU <= thr. Same outputs as dd_nms. */
int dd_nms_ssd(dd_ctx *ctx, const double *xyxy, const double *scores, int k, double iou_thr,
               int *out_idx, int *out_n, void *stream);

/* scipy.optimize.linear_sum_assignment as called at deep_sort/linear_assignment.py:58
 * (scipy is a third-party dependency of the reference; rectangular shortest-augmenting-path,
 * Crouse 2016).  Host code.  row_ind/col_ind get min(nr,nc) pairs sorted by row. */
int dd_lsap_host(const double *cost_host, int nr, int nc, int *row_ind_host, int *col_ind_host);

/* Iteration order of Python's list(set(a) - set(b)) for small non-negative ints (CPython 3.10 set
 * layout): deep_sort/linear_assignment.py:140 feeds that order into the IoU stage (tracker.py:120-123),
 * where it decides new-track-id order under cost ties.  Host code; exported for tests. */
int dd_pyset_difference_order_host(const int *a_host, int na, const int *b_host, int nb, int *out_host,
                                   int *out_n_host);

/* The same solver on the device, one wave64 per problem, all problems in ONE launch: scipy.optimize.linear_sum_assignment as called at
 * deep_sort/linear_assignment.py:58, with dd_lsap_host's choices under ties (pair for pair the same result).  cost_dev: device memory;
 * problem p is the row-major nr_host[p] x nc_host[p] matrix at element offset offset_host[p].  rows_host / cols_host receive the
 * min(nr, nc) pairs of every problem, sorted by row, problem after problem.  A shape above DD_ASSOC_DEVICE_MAX in either dimension, an
 * empty shape, an infeasible matrix or a NaN / -inf cost is DD_E_ARG, the message naming the first such problem. */
#define DD_ASSOC_DEVICE_MAX 256
int dd_lsap_batch(dd_ctx *ctx, const double *cost_dev, const int *nr_host, const int *nc_host, const int64_t *offset_host,
                  int n_problems, int *rows_host, int *cols_host);

/* The association decision of one tracker update, for parity tests: deep_sort/tracker.py:95-133 _match, i.e. matching_cascade over the
 * confirmed tracks (deep_sort/linear_assignment.py:78-141; each level min_cost_matching, :11-75, costs above the threshold clamped to
 * threshold + 1e-5 at :57), then min_cost_matching on the IoU costs for the unconfirmed tracks and the confirmed ones missed once
 * (tracker.py:117-123).  app / iou: [T][n] f64 row-major, the appearance cost after gating and the IoU cost; state_host / tsu_host: per
 * track row, state (1 Tentative, 2 Confirmed) and time_since_update.  where = 0: the host code on HOST matrices (no GPU, ctx may be NULL);
 * where = 1: the device code (csrc/assoc.hip) on DEVICE matrices, T and n at most DD_ASSOC_DEVICE_MAX.  Out, in the order the reference
 * builds them: matches_host [min(T, n)][2] (track row, detection), un_rows_host [T] (unmatched tracks), un_dets_host [n] (unmatched
 * detections) and their counts. */
int dd_match_cascade(dd_ctx *ctx, int where, const double *app, const double *iou, int T, int n, const int *state_host,
                     const int *tsu_host, double max_cos, double max_iou, int max_age, int *matches_host, int *n_matches_host,
                     int *un_rows_host, int *n_un_rows_host, int *un_dets_host, int *n_un_dets_host);

/* ---------------------------------------------------------------- tracker (state in HBM)
 * deep_sort/tracker.py:40-138 Tracker + track.py:67-196 Track state machine +
 * linear_assignment.py:11-190 (threshold, LSAP, cascade, gating) + nn_matching.py:137-154
 * partial_fit.  Kalman state and the appearance gallery live in device memory; the integer
 * book-keeping (ids, states, hits, age, time_since_update) lives on the host.
 * nn_budget <= 0 is the reference's budget=None (deepdish.py:515): a track keeps EVERY sample it was ever matched
 * with -- galleries grow in 32-row chunks from a pool shared by the group and are bounded by device memory only
 * (DD_E_CAPACITY when an allocation fails, never a silent overwrite).  nn_budget = B keeps the last B samples
 * (nn_matching.py:150-153).  gallery_capacity is a sizing hint: the rows per track the chunk table starts with. */
int dd_tracker_create(dd_ctx *ctx, double max_cosine_distance, double max_iou_distance,
                      int max_age, int n_init, int nn_budget /* <=0: None */,
                      int track_capacity, int gallery_capacity, dd_tracker **out);
/* deep_sort/nn_matching.py:5-28,57-75 (metric chosen at :126-132): dd_tracker_create with the metric named -- 0 = "cosine"
 * (what dd_tracker_create means), 1 = "euclidean"; any other value is DD_E_ARG.  Under the euclidean metric matching_threshold bounds
 * the minimum squared distance, and features are associated and stored in the gallery as given (no L2 normalisation anywhere). */
int dd_tracker_create_metric(dd_ctx *ctx, int metric, double matching_threshold, double max_iou_distance,
                             int max_age, int n_init, int nn_budget /* <=0: None */,
                             int track_capacity, int gallery_capacity, dd_tracker **out);
int dd_tracker_destroy(dd_tracker *trk);
/* tracker.py:51-57 */
int dd_tracker_predict(dd_tracker *trk);
/* tracker.py:59-93.  tlwh_host[n][4] f64; feats[n][128] f32 on device when feats_on_device,
 * else on the host. */
int dd_tracker_update(dd_tracker *trk, const double *tlwh_host, const float *feats,
                      int feats_on_device, int n);
/* which: 0 = tracker.tracks, 1 = tracker.deleted_tracks (tracker.py:80-81) */
int dd_tracker_count(dd_tracker *trk, int which, int *out_n_host);
/* Any output pointer may be NULL.  ints6[n][6] = (track_id, state, time_since_update, hits, age,
 * index of the detection that updated or founded the track in the last update, else -1);
 * means[n][8], covs[n][64]. */
int dd_tracker_read(dd_tracker *trk, int which, int64_t *ints6_host, double *means_host,
                    double *covs_host);
/* Per-track calls the host makes between two updates (deepdish/framerecords.py:133-165 via deepdish.py:1047):
 * dd_tracker_track_update = Track.update(kf, detection) (deep_sort/track.py:127-152) for one live track -- Kalman
 * update with the box, feature (128 f32, host or device) appended to the track's gallery, hits += 1,
 * time_since_update = 0, Tentative -> Confirmed at n_init hits; the mirrored mean is refreshed (synchronises).
 * dd_tracker_track_set = host assignment to track.state (1 Tentative, 2 Confirmed) and track.time_since_update
 * (< 0: unchanged).  dd_tracker_remove = the host reassigned tracker.tracks without these ids. */
int dd_tracker_track_update(dd_tracker *t, int64_t track_id, const double *tlwh_host, const float *feat, int feat_on_device);
int dd_tracker_track_predict(dd_tracker *t, int64_t track_id);   /* Track.predict(kf), deep_sort/track.py:113-125, one track */
int dd_tracker_track_set(dd_tracker *t, int64_t track_id, int state, int time_since_update);
int dd_tracker_remove(dd_tracker *t, const int64_t *track_ids_host, int n);
int dd_tracker_next_id(dd_tracker *trk, int64_t *out_host);
/* Rows of tracker.tracks reassigned by the host (deepdish.py:1047) are not supported: the
 * identity pass-through of framerecords.py:183 is the only behaviour reproduced. */

/* last association, for parity tests: app_host / iou_host [rows][cols] = the appearance cost matrix (nn_matching.py:156-177
 * after gate_cost_matrix, linear_assignment.py:181-189: gated entries 1e5; rows of unconfirmed tracks unspecified) and the
 * IoU cost matrix (iou_matching.py:42-81) of the last update; rows = tracks before that update, cols = detections. */
int dd_tracker_last_cost(dd_tracker *trk, double *app_host, double *iou_host, int cap, int *rows_host, int *cols_host);
/* matches[m][2] = (track row, detection), in update order */
int dd_tracker_last_matches(dd_tracker *trk, int *pairs_host, int cap, int *out_m_host);
/* Where Tracker._match (deep_sort/tracker.py:95-133: matching cascade, linear_assignment.py:78-141, and the assignments it solves, :11-75)
 * is decided for the tracker's GROUP (the trackers of a pipeline share it): 0 = on the host from the cost matrices (the default), 1 = on
 * the device, one wave per stream behind the association kernel, only the three lists coming back.  The decisions are the same.  A group
 * update in which any stream has more than DD_ASSOC_DEVICE_MAX tracks or detections runs whole on the host path; a stream whose device
 * decision stops (NaN / -inf cost) is decided by the host code.  DD_E_STATE while an update of the group is in flight. */
int dd_tracker_set_association(dd_tracker *trk, int where);
/* Group-wide counts since creation (any pointer may be NULL): group updates decided on the device, group updates decided on the host,
 * streams of device-decided updates that fell back to the host code, and the bytes the decisions copied device-to-host (the cost matrices
 * under host association; the lists, plus the matrices of streams that fell back, under device association). */
int dd_tracker_association_stats(dd_tracker *trk, long long *device_updates_host, long long *host_updates_host,
                                 long long *fallback_streams_host, long long *d2h_bytes_host);

/* ---------------------------------------------------------------- crops
 * tools/generate_detections.py:40-84 extract_image_patch for every box (integer box math on the
 * host side of the call, bilinear u8 resample as cv2.resize INTER_LINEAR on the device).
 * frame: u8 [H][W][3] BGR.  boxes_host: int64 tlwh [n][4] exactly as the reference receives them.
 * out: u8 [n][ph][pw][3].  valid_host[i] = 0 where the reference would return None. */
int dd_crop_resize(dd_ctx *ctx, const uint8_t *frame, int H, int W, const int64_t *boxes_host,
                   int n, int ph, int pw, uint8_t *out, int *valid_host, void *stream);
/* The same for float boxes (f64 [n][4] tlwh): generate_detections.py:64-74 evaluated in floating point with one
 * truncation at `astype(np.int)` -- what happens upstream when a box comes from a CVAT annotation
 * (deepdish/framerecords.py:109-118 feeds annotation boxes to the encoder). */
int dd_crop_resize_f64(dd_ctx *ctx, const uint8_t *frame, int H, int W, const double *boxes_host, int n, int ph,
                       int pw, uint8_t *out, int *valid_host, void *stream);

/* tools/generate_detections.py:86-116 DummyImageEncoder (mode 0: channel-mean of 16x8 patches, -128,
 * L2-normalised) and ConstantImageEncoder (mode 1: e0): the reference's model-free test encoders.
 * patches u8 [n][16][8][3] -> out f32 [n][128]. */
int dd_fake_encode(dd_ctx *ctx, const uint8_t *patches, int n, int mode, float *out, void *stream);

/* PIL Image.resize(LANCZOS) of an RGB(A) u8 image as tools/ssd_mobilenet.py:54-57 and
 * tools/yolov5.py:99 call it (stretch, no letterbox).  src u8 [H][W][src_c] (first 3 channels
 * used, optionally swapped BGR->RGB), dst u8 [h][w][3]. */
int dd_resize_lanczos(dd_ctx *ctx, const uint8_t *src, int H, int W, int src_c, int swap_rb,
                      uint8_t *dst, int h, int w, void *stream);
/* The same resize of `batch` frames of one geometry, densely packed on both sides (what the batched pipeline
 * does with a step's frames: one launch, both passes through LDS when the geometry allows). */
int dd_resize_lanczos_batch(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int src_c, int swap_rb,
                            uint8_t *dst, int h, int w, void *stream);
/* Which kernels dd_resize_lanczos / dd_resize_lanczos_batch run for a geometry: the decision those calls themselves switch on (and the
 * DD_LANCZOS_* switches of the process), answered without launching anything.  src / dst: the pointers the real call would be given (only
 * their alignment, and whether they are the same, matters); tmp: the intermediate, NULL = the context's own scratch as the real call
 * reserves it (ctx may be NULL when tmp is given: nothing touches the device).  Any out pointer may be NULL.
 * *h_step: what turns src [H][W][src_c] into 3-channel rows of w pixels; *v_step: what turns those into h rows.
 * *h_ksteps / *v_ksteps: 64-byte window steps of the banded tables (1..4) for the band and fused steps, 0 for the others. */
#define DD_LANCZOS_H_NONE 0        /* w == W, 3 channels, no swap: the vertical step reads src */
#define DD_LANCZOS_H_COPY 1        /* w == W: copy_rgb_k (4 -> 3 channels and / or red-blue swap, a byte at a time) */
#define DD_LANCZOS_H_SWAP_COPY 2   /* w == W: copy_swap_rb4_k (3 channels, red-blue swap, four pixels per thread) */
#define DD_LANCZOS_H_ROW 3         /* lanczos_h_row_k (source rows staged in LDS) */
#define DD_LANCZOS_H_SCALAR 4      /* lanczos_h_k */
#define DD_LANCZOS_H_BAND_WIDE 5   /* band_resample_wide_k into the transposed intermediate */
#define DD_LANCZOS_H_BAND_NARROW 6 /* band_resample_k into the transposed intermediate */
#define DD_LANCZOS_H_FUSED 7       /* lanczos_fused_k: both passes in one launch */
#define DD_LANCZOS_V_NONE 0        /* h == H and the horizontal step wrote dst (or src is dst) */
#define DD_LANCZOS_V_MEMCPY 1      /* h == H, w == W, nothing to convert: device-to-device copy */
#define DD_LANCZOS_V_V4 2          /* lanczos_v4_k (four bytes per thread) */
#define DD_LANCZOS_V_SCALAR 3      /* lanczos_v_k */
#define DD_LANCZOS_V_BAND_WIDE 4   /* band_resample_wide_k out of the transposed intermediate */
#define DD_LANCZOS_V_BAND_NARROW 5 /* band_resample_k out of the transposed intermediate */
#define DD_LANCZOS_V_FUSED 6       /* lanczos_fused_k */
int dd_resize_lanczos_plan(dd_ctx *ctx, int H, int W, int src_c, int swap_rb, int h, int w, int batch, const void *src,
                           const void *dst, const void *tmp, int *h_step, int *v_step, int *h_ksteps, int *v_ksteps);
/* Aspect-preserving geometry of a W x H frame in a net_w x net_h canvas, as the reference's letterbox_image computes it (yolo3/utils.py:18-28 =
 * tools/yolo.py:141-151): s = min(net_w * 1.0 / W, net_h * 1.0 / H), new = int(W s) x int(H s), pasted at ((net_w - new_w) // 2,
 * (net_h - new_h) // 2) -- the same double arithmetic and truncation (49 x 7 into 64 x 64 is 63 x 9 at (0, 27)).  Host only: no context, no
 * device.  A picture of zero width or height (Pillow raises ValueError there) is DD_E_ARG.  Any out pointer may be NULL. */
int dd_letterbox_geometry(int W, int H, int net_w, int net_h, int *new_w, int *new_h, int *off_x, int *off_y);
/* Letterboxed detector input, `batch` frames in one launch: dst u8 [batch][h][w][3] = for the RGB view of each frame
 *     Image.new('RGB', (w, h), (pad,) * 3).paste(Image.fromarray(rgb).resize((new_w, new_h), Image.LANCZOS), (off_x, off_y))
 * byte for byte, with dd_letterbox_geometry(W, H, w, h)'s numbers; src_c / swap_rb as in dd_resize_lanczos.  An axis whose size does not
 * change is copied (640 x 480 into 640 x 640 is swap + paste + pad).  Every canvas byte is written once, nothing outside it.  The reference
 * letterboxes for its YOLOv3 plugin only and with bicubic; Lanczos (its YOLOv5 adaptor's filter) is this build's choice.
 * DD_LETTERBOX_FUSED=0 (read once per process) runs the two-launch form for every geometry. */
int dd_resize_lanczos_letterbox(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int src_c, int swap_rb, uint8_t *dst, int h, int w,
                                int pad, void *stream);
/* The decision dd_resize_lanczos_letterbox switches on, answered without a device (ctx may be NULL).  *path: 0 = neither axis is
 * resampled (one copy launch), 1 = letterbox_lanczos_k (both passes through LDS, one launch), 2 = two launches (the dense horizontal pass,
 * then letterbox_v_pad_k): a geometry whose one-row vertical window exceeds the kernel's 64 KiB LDS budget, or DD_LETTERBOX_FUSED=0.
 * *rows_per_block: canvas rows a workgroup of the last launch owns. */
int dd_resize_lanczos_letterbox_plan(dd_ctx *ctx, int H, int W, int src_c, int swap_rb, int h, int w, int batch, int *path, int *rows_per_block);
/* cv2.resize INTER_LINEAR stretch as tools/tflite_object_detector.py:211 */
int dd_resize_bilinear(dd_ctx *ctx, const uint8_t *src, int H, int W, int c,
                       uint8_t *dst, int h, int w, void *stream);

/* 4:2:0 YUV -> BGR: cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420) for frames already on the device (a hardware decoder's
 * surfaces).  OpenCV's published BT.601 fixed-point arithmetic restated (csrc/yuv.hip; parity with OpenCV itself is unpinned, the library
 * is absent): per pixel c = max(0, Y - 16) * 1220542, R = sat8((c + 524288 + 1673527 (V - 128)) >> 20), G = sat8((c + 524288
 * - 852492 (V - 128) - 409993 (U - 128)) >> 20), B = sat8((c + 524288 + 2116026 (U - 128)) >> 20); the chroma of pixel (x, y) is that of
 * block (x >> 1, y >> 1), no interpolation.
 * src: `batch` frames of W x H (both even) u8.  layout 1 = NV12: H rows of luma, then H/2 rows of interleaved U,V pairs; layout 2 = I420: H
 * rows of luma, then H/2 rows of U, then H/2 rows of V.  pitch: bytes per luma row, 0 = W; NV12 chroma rows use pitch, I420 chroma rows
 * pitch / 2 (pitch even).  chroma_offset: bytes from a frame's start to its chroma, 0 = pitch * H (the I420 V plane follows the U plane's
 * H/2 rows).  frame_stride: bytes between frames, 0 = dense.  dst: u8 dense [batch][H][W][3] BGR.
 * DD_E_ARG (the message names the argument) for another layout, an odd or non-positive size, a pitch below W. */
int dd_yuv420_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t chroma_offset,
                     int64_t frame_stride, uint8_t *dst, void *stream);
/* Packed 4:2:2 YUV -> BGR: cv2.cvtColor(frame, COLOR_YUV2BGR_YUY2 / COLOR_YUV2BGR_UYVY) for frames already on the device, what a UVC / V4L2
 * camera (YUY2) or an SDI / HDMI capture card (UYVY) delivers raw.  Per pixel the arithmetic of dd_yuv420_to_bgr (tests/yuv422_ref.py is the
 * definition; parity with OpenCV itself is unpinned, the library is absent).  A row of W pixels (W even) is 2 W bytes of 4-byte macropixels,
 * order 4 = YUY2: Y0 U Y1 V, order 5 = UYVY: U Y0 V Y1; the two pixels of a macropixel share its chroma, no interpolation, no vertical
 * sub-sampling (H may be odd).  pitch: bytes per row, 0 = 2 W.  frame_stride: bytes between frames, 0 = dense (pitch * H).
 * dst: u8 dense [batch][H][W][3] BGR.  DD_E_ARG (the message names the argument) for another order, an odd or non-positive W, a non-positive
 * H, a pitch below 2 W; the arguments are checked before ctx is used. */
int dd_yuv422_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int order, int pitch, int64_t frame_stride, uint8_t *dst,
                     void *stream);
/* 8-bit raw sensor frames -> BGR for frames already on the device: one byte per pixel, what a machine-vision (GigE / USB3 Vision BayerRG8 and
 * its siblings) or CSI camera delivers before any colour processing, and 8-bit monochrome.  layout 6 = RGGB, 7 = GRBG, 8 = GBRG, 9 = BGGR: the
 * sensor's top-left 2 x 2 block read row by row (cv2.cvtColor COLOR_BayerBG2BGR, _BayerGB2BGR, _BayerGR2BGR, _BayerRG2BGR in that order:
 * OpenCV names the block at (1, 1)); layout 10 = gray (COLOR_GRAY2BGR: B = G = R = the sample).  The mosaic is demosaiced by OpenCV's
 * published bilinear rule restated (csrc/bayer.hip; tests/bayer_ref.py is the definition; parity with OpenCV itself is unpinned, the library
 * is absent): out(x, y) = D(clamp(x, 1, W - 2), clamp(y, 1, H - 2)), and at an interior R or B site its own colour is the sample,
 * G = (N + S + W + E + 2) >> 2, the opposite colour (NW + NE + SW + SE + 2) >> 2; at a G site G is the sample, the colour of its horizontal
 * neighbours (W + E + 1) >> 1, of its vertical ones (N + S + 1) >> 1.  No white balance, gamma or colour matrix is applied.
 * src: `batch` frames of W x H u8 (Bayer: both >= 3, either may be odd; gray: both >= 1).  pitch: bytes per row, 0 = W.  frame_stride: bytes
 * between frames, 0 = dense (pitch * H).  dst: u8 dense [batch][H][W][3] BGR.  DD_E_ARG (the message names the argument) for another layout,
 * a size too small, a pitch below W; the arguments are checked before ctx is used. */
int dd_raw8_to_bgr(dd_ctx *ctx, const uint8_t *src, int batch, int H, int W, int layout, int pitch, int64_t frame_stride, uint8_t *dst,
                   void *stream);

/* ---------------------------------------------------------------- frame ingest
 * The CPU side of Pipeline.capture (deepdish.py:837-878): cv2.flip(frame, 0) (:864) + cv2.resize(frame,
 * input_size) (:867) on frames that a decoder put in host memory.  A ring of `slots` pinned host buffers,
 * each [n_streams][src_h][src_w][3] u8 BGR, with device twins; dd_ingest_submit queues host->device copy
 * + flip + INTER_LINEAR stretch on a private copy stream; dd_ingest_acquire makes the consumer's stream
 * wait for that slot (no host wait) and returns the device frames [n_streams][dst_h][dst_w][3];
 * dd_ingest_release marks the consumer's last use so the slot can be refilled. */
typedef struct dd_ingest dd_ingest;
typedef struct dd_jpegdec dd_jpegdec;
int dd_ingest_create(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip,
                     dd_ingest **out);
/* The same ring for slots that hold what a decoder produces: pixel_format 0 = BGR (exactly dd_ingest_create), 1 = NV12, 2 = I420 (layouts
 * as dd_yuv420_to_bgr, dense; src_h and src_w even, else DD_E_ARG naming the value).  A YUV slot and its device twin are
 * n_streams * src_h * src_w * 3 / 2 bytes -- half the bytes per frame on the host link and in pinned memory; dd_ingest_submit converts on
 * the copy stream, then flips and stretches the BGR frame as above (one launch for all three; DD_INGEST_YUV_FUSED=0, read here, selects
 * convert-into-a-staging-buffer + the BGR ring's resize launch: the same bytes).  The consumer still receives BGR
 * [n_streams][dst_h][dst_w][3]; submit / acquire / release are unchanged.
 * pixel_format 4 = YUY2, 5 = UYVY: packed 4:2:2 as dd_yuv422_to_bgr, dense (src_w even, else DD_E_ARG naming the value; src_h any positive
 * value).  Such a slot and its device twin are n_streams * src_h * src_w * 2 bytes, two thirds of BGR; the conversion, the one-launch form
 * and DD_INGEST_YUV_FUSED=0 are as for 4:2:0.  pixel_format 3 names the JPEG ring, which dd_ingest_create_jpeg makes: refused here. */
int dd_ingest_create_format(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip,
                            int pixel_format, dd_ingest **out);
/* The same ring for slots that hold 8-bit raw sensor frames, dense: layout 6 .. 9 a Bayer mosaic, 10 monochrome, as dd_raw8_to_bgr (the
 * ring's format codes continued; dd_ingest_create_format refuses them as it always has).  A slot and its device twin are
 * n_streams * src_h * src_w bytes, a third of BGR.  dd_ingest_submit converts on the copy stream: straight into the slot's output without
 * a flip or a resize, otherwise convert + flip + stretch in one launch (the mosaic is demosaiced in the stored frame, then flipped), or,
 * with DD_INGEST_YUV_FUSED=0 (read here), convert-into-a-staging-buffer + the BGR ring's resize launch: the same bytes.  DD_E_ARG naming
 * the value for another layout or a Bayer src_h / src_w below 3, checked before ctx is used.  dd_ingest_status and dd_ingest_jpeg_put on
 * such a ring are DD_E_STATE.  The consumer receives BGR [n_streams][dst_h][dst_w][3]. */
int dd_ingest_create_raw8(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int layout,
                          dd_ingest **out);
/* The same ring for slots that hold baseline JPEG files (see the JPEG decoder below): a slot is one pinned arena of slot_bytes, into which
 * dd_ingest_jpeg_put copies stream `stream`'s file at the next 64-byte-aligned offset (after waiting for the slot's previous upload, as
 * dd_ingest_wait_uploaded does) and parses its header on the calling thread; it may be called from several threads at once.  A full arena
 * is DD_E_CAPACITY.  dd_ingest_submit uploads the bytes in use and the records in one copy each and decodes on the copy stream, straight
 * into the slot's output when neither flip nor resize is asked, otherwise into one staging buffer followed by the ring's crop_resize
 * launch.  dd_ingest_status gives the slot's int32 [n_streams] DD_JPEG_ST_* once the slot's work has run (it waits for it): a stream
 * with a non-zero status costs the others nothing, and one for which nothing was put since the last submit reports DD_JPEG_ST_NO_FRAME.
 * dd_ingest_host_slot on such a ring is DD_E_STATE.  The consumer always receives BGR [n_streams][dst_h][dst_w][3].  Every put into a slot
 * must have returned before that slot's submit; a second put for a stream replaces the first (its bytes stay in the arena until the submit). */
int dd_ingest_create_jpeg(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int64_t slot_bytes,
                          dd_ingest **out);
/* The same ring decoding at 1 / scale (1, 2, 4 or 8; anything else is DD_E_ARG naming the value; see dd_jpegdec_create_scaled).  src_h x
 * src_w stays the size every file must state (DD_JPEG_ST_SIZE otherwise).  The decoder writes frames of ceil(src_h / scale) x ceil(src_w /
 * scale): straight into the slot's output when that is dst_h x dst_w and no flip is asked, otherwise into the staging buffer, which has
 * that size, followed by the ring's crop_resize launch from there to dst_h x dst_w.  scale 1 is dd_ingest_create_jpeg. */
int dd_ingest_create_jpeg_scaled(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int scale,
                                 int64_t slot_bytes, dd_ingest **out);
int dd_ingest_jpeg_put(dd_ingest *g, int slot, int stream, const uint8_t *data_host, int64_t n);
int dd_ingest_status(dd_ingest *g, int slot, int *status_host);
int dd_ingest_destroy(dd_ingest *g);
int dd_ingest_host_slot(dd_ingest *g, int slot, uint8_t **host_ptr, int64_t *n_bytes);
int dd_ingest_wait_uploaded(dd_ingest *g, int slot);    /* host may overwrite the pinned slot after this returns */
int dd_ingest_submit(dd_ingest *g, int slot);
int dd_ingest_acquire(dd_ingest *g, int slot, void *consumer_stream, const uint8_t **frames_dev);
int dd_ingest_release(dd_ingest *g, int slot, void *consumer_stream);

/* ---------------------------------------------------------------- background subtraction
 * cv2.createBackgroundSubtractorMOG2(history, varThreshold, detectShadows) (deepdish.py:889) for n_streams
 * independent streams of [height][width][3] u8 frames; every other parameter keeps OpenCV's default (5 modes,
 * backgroundRatio 0.9, varThresholdGen 9, varInit 15, varMin 4, varMax 75, complexity reduction 0.05, shadow
 * value 127, shadow threshold 0.5).  The model (101 bytes per pixel) lives in HBM inside the handle.
 * dd_mog2_apply = backSub.apply(frame, learningRate) (deepdish.py:922) for all streams in one launch:
 * frames device u8 [n_streams][H][W][3] -> mask device u8 [n_streams][H][W] (0 background, 127 shadow, 255
 * foreground); learning_rate < 0 = OpenCV's automatic 1/min(2 nframes, history).  masked_frames (optional,
 * device, same shape as frames) receives cv2.bitwise_and(frame, frame, mask=fgMask) (deepdish.py:924).
 * Calls on one handle must be issued in frame order (the model update is sequential per stream). */
typedef struct dd_mog2 dd_mog2;
int dd_mog2_create(dd_ctx *ctx, int n_streams, int height, int width, int history, double var_threshold, int detect_shadows,
                   dd_mog2 **out);
int dd_mog2_destroy(dd_mog2 *m);
int dd_mog2_apply(dd_mog2 *m, const uint8_t *frames, double learning_rate, uint8_t *mask, uint8_t *masked_frames, void *stream);
/* dd_mog2_apply for the streams with present_host[z] != 0 only (u8 [n_streams], values 0 / 1; NULL = every stream): model, mask plane
 * and masked frame of the others are neither read nor written.  OpenCV counts nframes per subtractor, so the handle keeps one frame
 * count per stream and the automatic learning rate is 1/min(2 nframes, history) of EACH listed stream.  While all counts are equal and
 * every stream is listed this is dd_mog2_apply's one launch; otherwise one launch of mog2_apply_list_k over a table of {stream, alphaT,
 * 1 - alphaT, prune} entries whose floats the host computes as dd_mog2_apply does -- the same per-pixel arithmetic either way. */
int dd_mog2_apply_streams(dd_mog2 *m, const uint8_t *frames, const uint8_t *present_host, double learning_rate, uint8_t *mask,
                          uint8_t *masked_frames, void *stream);
/* Test aid: the model of one stream as host arrays -- weight, variance f32 [5][H*W], mean f32 [5][3][H*W]
 * (zero past a pixel's mode count), nmodes u8 [H*W].  Synchronises. */
int dd_mog2_state(dd_mog2 *m, int stream_index, float *weight_host, float *variance_host, float *mean_host, uint8_t *nmodes_host);
/* The listed streams' subtractors start over, as cv2.createBackgroundSubtractorMOG2() (deepdish.py:889) leaves them in a restarted
 * process: no modes at any pixel (the plane dd_mog2_create clears, cleared again on `stream`, NULL = the context's) and a frame count
 * of 0, so the automatic learning rate 1/min(2 nframes, history) starts over too.  The other streams' models are neither read nor
 * written.  streams_host int32 [n], each 0 .. n_streams - 1 (DD_E_ARG otherwise, before anything is queued); n = 0 does nothing. */
int dd_mog2_reset_streams(dd_mog2 *m, const int *streams_host, int n, void *stream);
/* np.count_nonzero(fgMask[y:y+h, x:x+w]) (deepdish.py:957) for n_boxes boxes: mask device u8
 * [n_streams][height][width]; boxes_xywh_host int32 [n_boxes][4], already clipped to the frame as
 * deepdish.py:951-952 does (anything else is DD_E_ARG); box_stream_host int32 [n_boxes]; counts_host int32
 * [n_boxes].  Synchronises the stream. */
int dd_mask_box_count(dd_ctx *ctx, const uint8_t *mask, int n_streams, int height, int width, const int *boxes_xywh_host,
                      const int *box_stream_host, int n_boxes, int *counts_host, void *stream);
/* np.count_nonzero of whole mask planes (csrc/gate.hip, mask_stream_count_k): mask_dev device u8 [n_streams][height][width], planes
 * dense; streams_host int32 [n], each 0 .. n_streams - 1, or NULL = all of them in order (then n must be n_streams); counts_host int32
 * [n], counts_host[i] = the non-zero bytes of plane streams_host[i].  Any byte value counts: MOG2's 127 (shadow) as its 255.  Planes
 * that are not listed are not read.  An integer sum: the same ints on every call.  n = 0 does nothing; n <= 65 535.  Anything else
 * is DD_E_ARG before a launch.  Runs on the context's stream and synchronises it. */
int dd_mask_stream_count(dd_ctx *ctx, const uint8_t *mask_dev, int n_streams, int height, int width, const int *streams_host, int n,
                         int *counts_host);

/* Frame compaction (csrc/gather.hip): dst frame i = src frame idx[i] for i < n, frames of frame_bytes bytes behind one another; src_dev
 * holds n_src frames.  idx_host int32 [n] must be strictly increasing and < n_src (DD_E_ARG otherwise: checked on the host, never by a
 * faulting kernel); n = 0 is legal and launches nothing.  One launch of frames_gather_k, grid (chunks, n), 64-bit offsets; 16-byte
 * loads and stores per lane when src_dev, dst_dev and frame_bytes are multiples of 16, 4-byte ones when multiples of 4, bytes otherwise.
 * The buffers must not overlap.  Synchronises the stream. */
int dd_gather_frames(dd_ctx *ctx, const uint8_t *src_dev, int n_src, int64_t frame_bytes, const int *idx_host, int n, uint8_t *dst_dev,
                     void *stream);

/* Retained feature rows (csrc/featrows.hip; what dd_pipeline_detector_skip_streams launches once per step, deepdish.py:1003-1014): a row
 * is 128 f32.  table_host int32 [n_streams][6] = {sel, src_row, n_out, dst_out_row, n_store, dst_store_row}: stream z reads rows
 * [src_row, src_row + max(n_out, n_store)) of fresh_dev (sel 0: the encoder's output) or store_dev (sel 1: the store), and writes the
 * first n_out of them to rows_out_dev at dst_out_row (the tracker's input) and the first n_store to store_out_dev at dst_store_row (the
 * next store).  *_rows = the rows each buffer holds: every range is checked against them on the host (DD_E_ARG; never by a faulting
 * kernel), as are overlapping destination ranges and buffers that are not 16-byte aligned.  One launch of feature_rows_carry_k, one
 * block per stream that has rows (a stream with none costs nothing), 16-byte loads and stores, 64-bit offsets; n_streams = 0 is legal
 * and launches nothing.  Sources and destinations must not overlap.  Synchronises the stream. */
int dd_feature_rows_carry(dd_ctx *ctx, const float *fresh_dev, int64_t fresh_rows, const float *store_dev, int64_t store_rows,
                          float *rows_out_dev, int64_t out_rows, float *store_out_dev, int64_t store_out_rows, const int *table_host,
                          int n_streams, void *stream);

/* ---------------------------------------------------------------- networks
 * Replaces tflite_runtime.Interpreter(model_path).invoke() at tools/ssd_mobilenet.py:35-38,102-109,
 * tools/yolov5.py:71-79,107-109 and tools/generate_detections.py:153-154,169-171.  A model is an op
 * program + one weight blob compiled on the host (deepdish_amd/nets.py: MARS per
 * tools/freeze_model.py:88-157, SSD-MobileNet-v1, YOLOv5s per detectors/yolov5/yolov5s.yaml) -- the
 * analogue of the reference's .tflite file; the word layout is documented in csrc/nets.hip. */
int dd_net_create(dd_ctx *ctx, const int32_t *program_host, int n_words, const void *weights_host,
                  int64_t n_weight_bytes, int max_batch, dd_net **out);
/* The same engine with its activation buffers overlaid by lifetime (a buffer is live from its first writer to its last reader; the
 * output tensor to the end): what a pipeline that never reads intermediate tensors wants -- the reference's interpreter keeps one
 * arena per model too (tflite_runtime: `interpreter.allocate_tensors()`, tools/ssd_mobilenet.py:38).  f16 programs only; dd_net_read
 * of anything but the output tensor is DD_E_STATE. */
int dd_net_create_shared(dd_ctx *ctx, const int32_t *program_host, int n_words, const void *weights_host,
                         int64_t n_weight_bytes, int max_batch, dd_net **out);
/* device bytes of the engine's activation buffers (one number: the arena, or the sum of the per-tensor buffers) */
int dd_net_activation_bytes(dd_net *net, int64_t *out_host);
int dd_net_destroy(dd_net *net);
/* input u8 [n][in_h][in_w][3]; results stay in the net's own device tensors (dd_net_output). */
int dd_net_forward(dd_net *net, const uint8_t *input, int n, void *stream);
/* tensor < 0 selects the program's declared output.  dtype: 0 f16, 1 f32, 2 u8.  Row n of the
 * tensor starts at dev_ptr + n * h * w * cs elements. */
int dd_net_output(dd_net *net, int tensor, void **dev_ptr_host, int *h_host, int *w_host, int *c_host,
                  int *cs_host, int *dtype_host);

/* Latency mode for small batches (the reference runs ONE stream: deepdish.py:1324-1340): the kernels of a forward are
 * captured once per (input pointer, n) into a hipGraph and replayed with one launch.  Results are identical. */
int dd_net_use_graph(dd_net *net, int enable);
int dd_net_input_size(dd_net *net, int *h_host, int *w_host);   /* the model's input height / width (ssd_mobilenet.py:43, yolov5.py:79) */
int dd_net_max_batch(dd_net *net, int *out_host);
int dd_net_last_batch(dd_net *net, int *out_host);   /* images in the most recent forward */
/* Copy the first n images of a (whole, un-sliced) tensor to caller memory: n*h*w*cs elements. */
int dd_net_read(dd_net *net, int tensor, int n, void *dst, int dst_on_device, void *stream);

/* Measurement aid (not on the product path): bracket every op of the next forwards with HIP events
 * on the launch stream; read back the per-op milliseconds of the last forward. */
int dd_net_profile(dd_net *net, int enable);
int dd_net_profile_read(dd_net *net, float *ms_host, int cap, int *n_ops_host);
/* Which launch ran each op of the last forward: 0 the op's own kernel, 1 none (folded into the next op's launch),
 * 2 conv3x3_pool_rows_k, 3 conv3x3_pool_rows_k with the first layer folded in, 4 res_unit_rows_k, 5 ssd_front_k,
 * 6 conv3x3_c64_rows_k, 7 conv3x3_s2_rows_k, 8 conv_ws_k, 9 conv_ws_dw_k, 10 dwpw_rows_k, 11 SSD head with the decode in its
 * epilogue, 12 res_pair_rows_k, 13 YOLOv5 Detect head with the row reduction in its epilogue, 14 mars_ws128_k, 15 none (the op ran
 * inside the previous op's launch), 16 mars_pair64_k, 17 q_dwm_k, 18 conv3x3_c64_rows_k on 8-column strips, 19 q_front_k, 20 q_mid_k,
 * 21 q_conv_k with a residual ADD in its epilogue, 22 q_add_k, 23 stem_conv_pool_wide_k (first layer + 3x3 layer + max pool of a 64- or
 * 128-wide crop, reported on the pool op) -- so that a per-kernel time table attributes a fused launch to the kernel that ran. */
int dd_net_op_launches(dd_net *net, int32_t *codes_host, int cap, int *n_ops_host);
/* Which variant of the generic convolution launcher ran each op of the last forward (read-only, beside dd_net_op_launches, which reports 0
 * for all of them): WM | WN << 4 | MI << 8 | NI << 12 | (BK / 16) << 16 | mode << 20 | splitk << 24 -- the block tile is WM*MI*16 pixels x
 * WN*NI*16 channels in steps of BK along K; mode 0 / 1 / 2 = conv_glds_k with the general / pointwise / whole-tap fill, 3 = conv_mfma_k;
 * splitk = slices of the K axis (1 = none; > 1: conv_splitk_finish_k ran behind it).  0 for an op that took any other kernel.
 * Ops of a uint8 program (every one that launched; 0 for an op a row pipeline ran): bits 0..3 the kernel, the rest its template arguments --
 *   1 q_conv_k:       MQ << 4 (3 bits) | ROWSUM << 7 | NPF << 8 (3 bits) | PIPE << 11 | SPLIT << 12 (2 bits) | Q16N << 14 | merged heads << 15 |
 *                     magic-number division << 16 | residual ADD << 17 | launches << 18 (2 bits; 2: the merged op as one launch per predictor,
 *                     the word then describes the second)
 *   2 q_pws_k:        (K / 512) << 4 (2 bits) | MW << 6 (3 bits) | epilogue << 9 (2 bits: 0 bordered interleaved, 1 rows) | ROWSUM << 11 |
 *                     SAT << 12 (2 bits) | merged heads << 14
 *   3 q_dw_k:         launches << 8 (8 bits)
 *   4 q_dwm_k:        SAT << 4 | magic-number division << 5 | frame chunks << 8 (8 bits, saturating)
 *   5 q_dwpw_k:       (CIN / 32) << 4 (5 bits) | (COUT / 64) << 9 (4 bits) | STRIDE << 13 (2 bits) | (QTT / 64) << 15 (2 bits) |
 *                     filter form << 17 (2 bits: 0 plain, 1 row sums, 2 hi + lo, 3 dup) | SAT << 19 (2 bits) | frame chunks << 21 (7 bits, saturating)
 *   6 q_conv0_k:      HL << 4 | SAT << 5 (2 bits) | frame chunks << 8 (8 bits, saturating)
 *   7 q_add_k:        frame chunks << 8 (8 bits, saturating)
 *   8 q_ssd_decode_k
 * SAT: 0 the layer's own clamp, 1 the byte range by saturating packs, 2 also both shifts <= 8 (q_dwm_k: 0 / 1). */
int dd_net_op_variants(dd_net *net, int32_t *codes_host, int cap, int *n_ops_host);
/* Host only (no device, no context): *fits_host = 1 when a uint8 MobileNet block (3x3 depthwise of `stride` + 1x1 cin -> cout, SAME padding)
 * on an h x w source runs as one fused launch (OP_QDWPW) -- the launcher's own acceptance rule, asked by the program compiler so that it
 * never emits a fused op that dd_net_forward would refuse.  split_filter: the pointwise filter is packed as hi + lo parts. */
int dd_netq_dwpw_fits(int cin, int cout, int stride, int h, int w, int split_filter, int *fits_host);

/* TFLite_Detection_PostProcess (inside the reference's .tflite graph, tools/ssd_mobilenet.py:103-109):
 * anchor decode, sigmoid, per-class NMS, top max_det.  raw f32 [n_anchors][4+n_classes] ->
 * boxes f32 [max_det][4] (ymin,xmin,ymax,xmax normalised), classes f32, scores f32, count. */
int dd_ssd_postprocess(dd_ctx *ctx, const float *raw, const float *anchors, int n_anchors,
                       int n_classes, int max_det, float score_thr, float iou_thr,
                       float *boxes, float *classes, float *scores, int *count, void *stream);

/* The op's first stage alone, `batch` images: raw f32 [batch][n_anchors][4+n_classes] -> per anchor boxes f32 [.][4]
 * (ymin,xmin,ymax,xmax), scores (sigmoid of the best class logit, background excluded), classes int32 (id - 1, lowest
 * on ties; a NaN logit never wins, and an anchor no class wins -- every logit -inf or NaN -- gives class 0 with score 0, so the
 * class is always in [0, n_classes - 2]), keys f32 (score, or -1 below score_thr) -- and its second stage (class-agnostic NMS, top max_det) from
 * those arrays.  dd_ssd_postprocess = the two in one call for one image. */
int dd_ssd_decode(dd_ctx *ctx, const float *raw, const float *anchors, int n_anchors, int n_classes, float score_thr,
                  float *boxes, float *scores, int *classes, float *keys, int batch, void *stream);
int dd_ssd_postprocess_decoded(dd_ctx *ctx, const float *dec_boxes, const float *dec_scores, const int *dec_classes,
                               const float *dec_keys, int n_anchors, int max_det, float score_thr, float iou_thr,
                               float *boxes, float *classes, float *scores, int *count, int batch, void *stream);
/* SSD detector engines (tools/ssd_mobilenet.py:102-109): run that first stage inside the head layers' GEMM epilogues,
 * straight from the accumulators -- the [n][n_anchors][4+n_classes] head matrix is then never written (dd_net_read of
 * it is DD_E_STATE) and dd_net_ssd_decoded hands out the per-anchor arrays of the last forward ([n][n_anchors] each,
 * same bits as dd_ssd_decode on the head matrix).  anchors_host f32 [n_anchors][4] (yc, xc, h, w). */
int dd_net_ssd_decode(dd_net *net, const float *anchors_host, int n_anchors, float score_thr, int enable);
int dd_net_ssd_decoded(dd_net *net, float **boxes_dev, float **scores_dev, int **classes_dev, float **keys_dev);
/* the same arrays of the first n images of the last forward copied to host memory (any pointer may be NULL) */
int dd_net_ssd_decoded_read(dd_net *net, int n, float *boxes_host, float *scores_host, int *classes_host, float *keys_host);

/* TFLite_Detection_PostProcess as a model file with use_regular_nms = true runs it (the interpreter applies the op's options,
 * tools/ssd_mobilenet.py:100-109; kernels/detection_postprocess.cc NonMaxSuppressionMultiClassRegularHelper): for every class in
 * ascending id the anchors with score >= score_thr by descending score (equal scores: the lower anchor first), greedy NMS inside the
 * class (IoU > iou_thr suppresses, the f32 expressions of the fast path), at most detections_per_class survivors; the classes'
 * survivors merged by descending score (equal scores: the lower class first, inside a class the keep order), the first max_det rows.
 * One anchor can come out under several classes; boxes of different classes never suppress each other.  TensorFlow Lite is absent
 * from this image: restated from the op's published behaviour, parity unpinned.  Outputs as dd_ssd_postprocess for `batch` images:
 * boxes f32 [batch][max_det][4], classes f32 (id - 1), scores f32 [batch][max_det], count int32 [batch]; rows past count are zero.
 * 64 < n_anchors <= 4096, 1 <= max_det <= 64, detections_per_class >= 1, at most 256 score columns per anchor (255 classes behind a
 * background column, 256 for _decoded); anything else is DD_E_ARG.  One
 * kernel (csrc/post_regular.hip) behind three front ends:
 *   _decoded: dec_boxes f32 [batch][n_anchors][4] (ymin,xmin,ymax,xmax; 16-byte aligned) and a ready score matrix f32
 *     [batch][n_anchors][score_ld] whose column first_class_col + c holds class c (n_classes = classes, no background column);
 *   dd_ssd_postprocess_regular: the f32 head matrix raw [batch][n_anchors][4 + n_classes] (n_classes counts the background column,
 *     as in dd_ssd_postprocess); a row's box has the bits dd_ssd_decode gives its anchor, every class logit goes through the sigmoid;
 *   _u8: the uint8 head tensors of a quantised model (dd_net_ssd_heads_u8): box bytes [batch][n_anchors][4], class bytes
 *     [batch][n_anchors][cls_stride] (background first) through the graph's LOGISTIC as a 256-byte table (device), quant4_host =
 *     box scale, box zero point, score scale, score zero point: scale * (q - zero point), what dd_net_ssd_decode's uint8 stage reads. */
int dd_ssd_regular_nms_decoded(dd_ctx *ctx, const float *dec_boxes, const float *scores_in, int score_ld, int first_class_col,
                               int n_anchors, int n_classes, int max_det, int detections_per_class, float score_thr, float iou_thr,
                               float *boxes, float *classes, float *scores, int *count, int batch, void *stream);
int dd_ssd_postprocess_regular(dd_ctx *ctx, const float *raw, const float *anchors, int n_anchors, int n_classes, int max_det,
                               int detections_per_class, float score_thr, float iou_thr, float *boxes, float *classes, float *scores,
                               int *count, int batch, void *stream);
int dd_ssd_postprocess_regular_u8(dd_ctx *ctx, const uint8_t *box_q, const uint8_t *cls_q, int cls_stride, const uint8_t *logistic_table,
                                  const float *quant4_host, const float *anchors, int n_anchors, int n_classes, int max_det,
                                  int detections_per_class, float score_thr, float iou_thr, float *boxes, float *classes, float *scores,
                                  int *count, int batch, void *stream);
/* The quantised head tensors of a uint8 SSD engine where the last forward left them (tools/ssd_mobilenet.py:102-109: the two inputs of
 * the post-process op): device pointers to the box bytes [n][n_anchors][4], the class bytes [n][n_anchors][cls_stride] and the 256-byte
 * logistic table, quant4_host[4] = box scale, box zero point, score scale, score zero point, n_classes with the background column.
 * DD_E_STATE for an engine whose buffers share memory by lifetime (the tensors do not outlive the forward), DD_E_ARG for a program
 * without the uint8 SSD head. */
int dd_net_ssd_heads_u8(dd_net *net, const uint8_t **box_q_dev, const uint8_t **cls_q_dev, int *cls_stride_host,
                        const uint8_t **logistic_table_dev, float *quant4_host, int *n_anchors_host, int *n_classes_host);

/* YOLOv5 detector: tools/yolov5.py:126-128 (cls *= obj, np.argmax, confidence) inside the Detect layers' epilogues -- per row of the
 * head the decoded box (x, y, w, h: the matrix's first four columns), the confidence and the class; the f32 [rows][5 + C] matrix
 * (yolov5.py:109 `pred`) is then never written and dd_net_read of it is an error.  Needs a program compiled with the per-anchor
 * copy of the Detect weights (deepdish_amd.nets.compile_yolov5s emits it).  enable = 0 switches back. */
int dd_net_yolo_decode(dd_net *net, int enable);
/* Device pointers to what the last forward's heads wrote: boxes f32 [n][rows][4], conf f32 [n][rows], classes i32 [n][rows]
 * (a NaN product makes conf NaN and the class the first NaN's index, as np.argmax does); rows = rows per image. */
int dd_net_yolo_decoded(dd_net *net, float **boxes, float **conf, int **classes, int *rows);
/* The same, copied to the host for the first n images (any pointer may be NULL). */
int dd_net_yolo_decoded_read(dd_net *net, int n, float *boxes_host, float *conf_host, int *classes_host);

/* tools/ssd_mobilenet.py:111-150, SSDMobileNet.predict after its four get_tensor calls, for `batch` images at once:
 * NaN scrub (:111-116), score >= confidence (:119), reorder [1,0,3,2] and scale by (w,h,w,h) in f64 (:121-127),
 * per-class nms_boxes (:59-98, see dd_nms_ssd).  Inputs are the outputs of dd_ssd_postprocess (device):
 * boxes f32 [batch][max_det][4], classes f32, scores f32 [batch][max_det], max_det <= 64.  Outputs (device):
 * out_boxes f64 [batch][max_det][4] xyxy pixels, out_cls int32 (class id = label-file line - 1, :142-147),
 * out_scores f64, out_n int32 [batch].  Rows come class by class in ascending id (the reference walks a Python
 * set) and inside a class in nms_boxes' pick order. */
int dd_ssd_detections(dd_ctx *ctx, const float *boxes, const float *classes, const float *scores, int batch,
                      int max_det, double confidence, double iou_thr, double img_w, double img_h, double *out_boxes,
                      int *out_cls, double *out_scores, int *out_n, void *stream);

/* tools/yolov5.py:120-131: xywh->xyxy, cls*=obj, argmax, conf >= thr, scale to image.
 * raw f32 [n_rows][5+n_cls] -> out_boxes f32 [cap][4] xyxy pixels, out_scores, out_cls, *out_n
 * (rows in ascending row order, like np.where). */
int dd_yolov5_decode(dd_ctx *ctx, const float *raw, int n_rows, int n_cls, float thr,
                     float img_w, float img_h, float *out_boxes, float *out_scores,
                     int *out_cls, int cap, int *out_n, void *stream);

/* dd_yolov5_decode for an img_w x img_h frame that reached the net_w x net_h network through dd_resize_lanczos_letterbox: the corners,
 * normalised to the canvas, go back to frame pixels as X = (x - off_x / net_w) / (new_w / net_w) * img_w (Y likewise) in f64, rounded once
 * to f32 -- the shape of tools/yolo.py:78-86, with the integer paste offset where the reference divides by 2. (that is where the pixels
 * are).  No int(), no clipping: boxes in the padding come out negative.  A frame with the canvas's aspect gives dd_yolov5_decode's bits. */
int dd_yolov5_decode_letterbox(dd_ctx *ctx, const float *raw, int n_rows, int n_cls, float thr, int img_w, int img_h, int net_w, int net_h,
                               float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n, void *stream);

/* The forms of the two calls above that the batched pipeline launches, reachable on their own.
 * dd_yolov5_decode_batch: raw f32 [batch][n_rows][5 + n_cls] -> per image out_boxes f32 [batch][cap][4], out_scores, out_cls
 * [batch][cap], out_n [batch].  out_n[z] counts EVERY row of image z with confidence >= thr; the first min(out_n[z], cap) of them, in
 * row order, are written and nothing behind them is touched.  net_w <= 0: the stretch arithmetic of dd_yolov5_decode; net_w > 0: the
 * un-mapping of dd_yolov5_decode_letterbox (img_w, img_h whole numbers).  n_rows == 0 zeroes out_n and launches nothing.  Per-row
 * scratch (confidence and class, batch * n_rows * 8 bytes plus alignment) comes from the context.
 * dd_yolov5_select_batch: the second half alone on boxes4 f32 [batch][n_rows][4] (x, y, w, h), conf f32 and cls int32
 * [batch][n_rows] (what dd_net_yolo_decoded hands out): same outputs, same geometry switch, no scratch.
 * dd_yolov5_pack: those per-image outputs -> packed f32 rows {x1, y1, x2, y2, score, class bits} of all images behind one another,
 * image z's min(n_rows[z], cap) rows starting at the sum over the images before it; n_rows int32 [batch] (device) as out_n above.
 * Nothing is written past the total. */
int dd_yolov5_decode_batch(dd_ctx *ctx, const float *raw, int n_rows, int n_cls, float thr, float img_w, float img_h, int net_w, int net_h,
                           float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n, int batch, void *stream);
int dd_yolov5_select_batch(dd_ctx *ctx, const float *boxes4, const float *conf, const int *cls, int n_rows, float thr, float img_w,
                           float img_h, int net_w, int net_h, float *out_boxes, float *out_scores, int *out_cls, int cap, int *out_n,
                           int batch, void *stream);
int dd_yolov5_pack(dd_ctx *ctx, const float *boxes, const float *scores, const int *cls, const int *n_rows, int cap, int batch,
                   float *packed, void *stream);

/* ---------------------------------------------------------------- multi-stream hot path
 * The per-frame call sequence of the reference's Pipeline (deepdish.py:880-885 run_object_detector,
 * :940-960 box hygiene, :995 NMS, :1008 encoder, :1028-1029 tracker, :1035-1114 count line) for
 * n_streams independent streams, one frame each per step, device work batched across streams.
 * detector may be NULL (detections are then always injected).  Which detector adaptor runs is chosen like the
 * reference chooses its plugin (deepdish.py:482-502): anchors_host != NULL = SSD-MobileNet (tools/ssd_mobilenet.py:
 * resize to the net's input, forward, TFLite_Detection_PostProcess, predict tail; labels_nl line i+1 names class
 * id i, :142-147; score threshold 0.5); anchors_host == NULL = YOLOv5 (tools/yolov5.py:97-146: resize, forward with
 * the Detect decode fused, dd_yolov5_decode, label filter, xyxy -> tlwh; n_anchors = rows of the head tensor,
 * n_classes = classes; labels_nl line i names class id i, :134; score threshold 0.25; no NMS of its own -- every
 * candidate goes on to deep_sort's NMS, however many pass the threshold).
 * labels_nl: the label file's lines joined by '\n'; wanted_nl: --wanted-labels.
 * line_host: count line x1,y1,x2,y2 (deepdish.py:739-744). */
int dd_pipeline_create(dd_ctx *ctx, int n_streams, int frame_h, int frame_w, dd_net *detector,
                       const float *anchors_host, int n_anchors, int n_classes, dd_net *encoder,
                       const char *labels_nl, const char *wanted_nl, double max_cosine_distance,
                       double nms_max_overlap, double max_iou_distance, int max_age, int n_init,
                       const double *line_host, int track_capacity, int gallery_capacity, dd_pipeline **out);
int dd_pipeline_destroy(dd_pipeline *p);
/* Adaptor that consumes an SSD-type detector's output, chosen like the reference chooses its plugin class from the model
 * file name (deepdish.py:482-502): 0 = tools/ssd_mobilenet.py (default), 2 = the generic TFLite-Task adaptor
 * (tools/tflite.py:9-41 over tools/tflite_object_detector.py:180-295: cv2.resize INTER_LINEAR of the RGB frame, rows of the
 * post-process op with score >= 0.5, int() of the scaled corners, sorted by score).  Before the first step. */
int dd_pipeline_detector_adaptor(dd_pipeline *p, int adaptor);
/* Options of the TFLite_Detection_PostProcess op inside an SSD-type model file, which the reference's interpreter applies as the file
 * states them (tools/ssd_mobilenet.py:100-109: invoke() + the four output tensors of max_detections rows): rows per frame (<= 64),
 * nms_score_threshold, nms_iou_threshold (fast class-agnostic NMS).  Defaults: the stock export's 10 / 1e-8 / 0.6.  Before the first step.
 * Above 16 rows the ORDER of equal-score rows of one class is the reference's only up to its NumPy's unstable sort (tools/ssd_mobilenet.py:73
 * `s.argsort()[::-1]`: stable for <= 16 elements, unspecified beyond) -- INTEGRATION.md, "Ties inside a class". */
int dd_pipeline_ssd_options(dd_pipeline *p, int max_detections, float nms_score_threshold, float nms_iou_threshold);
/* A model file whose post-process op states use_regular_nms = true (tools/ssd_mobilenet.py:100-109: the interpreter runs what the file
 * says): the detector stage calls the per-class NMS (dd_ssd_postprocess_regular / _u8) with this detections_per_class (>= 1) instead of
 * the fast class-agnostic one; max_detections and the two thresholds stay dd_pipeline_ssd_options'.  The head layers' decode epilogue
 * keeps only the best class of an anchor, so it is switched off (dd_net_ssd_decode enable = 0): the f32 engine writes its head matrix,
 * the uint8 engine's head tensors are read where they lie.  Before the first step. */
int dd_pipeline_ssd_regular_nms(dd_pipeline *p, int detections_per_class);
/* --object-detector-skip-frames n (deepdish.py:892-893,929-938,1003-1014): the detector and the encoder run on one step in n + 1 --
 * steps 0, n + 1, 2 (n + 1), ... counted from the first step; n <= 0 = every step (the default).  A skip step runs no detector chain
 * (resize, forward, post-process, adaptor tail, host copy), no crops and no encoder: each stream reuses the last detector step's adaptor
 * output (dd_pipeline_detections returns it; injected detections passed on a skip step are ignored) through this step's box hygiene,
 * motion test and NMS, and its first min(kept boxes, feature rows of that step) boxes pair with those feature rows in order, as the
 * reference's zip() does.  Stage events add nothing to objd / feat on a skip step.  Before the first step. */
int dd_pipeline_detector_skip_frames(dd_pipeline *p, int n);
/* The same option with one counter per stream (deepdish.py:892-893,929-938,1003-1014 -- the reference is one process per camera, so its
 * skip_rem IS per camera).  n_host int32 [n_streams], every value >= 0; phase_host int32 [n_streams] with 0 <= phase[z] <= n[z], or NULL
 * (other values: DD_E_ARG).  Stream z keeps rem[z] (starts at 0) and "has a detector result" (starts false).  On a step in which z is
 * present: rem[z] > 0 and z has a result -> a skip step for z, rem[z] -= 1; otherwise a detector step for z, then rem[z] = phase[z] if
 * this was z's first detector step and a phase was given, else n[z].  A step without z moves nothing of z, its counter included.  Without
 * phase this is the reference's rule applied to each stream's own present frames.  phase is this build's addition (the reference has no
 * such option): it shortens the first cycle only, so that streams with equal n detect on different steps -- with phase[z] = z mod (n + 1)
 * every unmasked step after the first runs the detector for n_streams / (n + 1) streams instead of all or none.
 * In a step, predict, MOG2, box hygiene, the motion test (against this frame's mask), NMS, the tracker update and the count line run for
 * every present stream; the detector chain, crops and encoder for the streams on a detector step only (through the compaction of
 * dd_pipeline_step3 when those are not all streams); injected rows replace the detector's output for these and are ignored for the
 * others.  A stream on a skip step pairs its first min(kept boxes, retained rows) boxes with the rows of ITS OWN last encoder run, which
 * a store of retained rows keeps across other streams' encoder runs and steps without the stream (dd_feature_rows_carry's kernel, one
 * launch per step; the store holds the rows actually retained, twice: it is double-buffered).  The look-ahead queues the detector run
 * of the next step's detector streams, known when this step starts; nothing when there are none.  Presence masks are allowed in this
 * form.  Before the first step (DD_E_STATE after); a pipeline takes this form or dd_pipeline_detector_skip_frames(n > 0), not both
 * (DD_E_STATE). */
int dd_pipeline_detector_skip_streams(dd_pipeline *p, const int *n_host, const int *phase_host);
/* out5_host = {detector stream-steps, skip stream-steps (both summed over the steps, in either form of the option), feature_rows_carry_k
 * launches, feature rows retained now, bytes allocated for the store}: the last three are 0 without dd_pipeline_detector_skip_streams.
 * skipped_host u8 [n_streams] (may be NULL): 1 where the stream's last step was a skip step. */
int dd_pipeline_skip_stats(dd_pipeline *p, long long *out5_host, uint8_t *skipped_host);
/* Letterboxed detector input for a YOLOv5 pipeline (other detectors: DD_E_ARG -- SSD-MobileNet is trained on stretched input): the step's
 * Lanczos stretch becomes dd_resize_lanczos_letterbox with this pad value (0 .. 255; 114 is YOLOv5's own, 128 the reference's YOLOv3 canvas)
 * on the detector stream, and both decode forms un-map their boxes as dd_yolov5_decode_letterbox does.  Everything downstream sees frame
 * pixels as before.  Before the first step (DD_E_STATE after). */
int dd_pipeline_detector_letterbox(dd_pipeline *p, int pad);
/* deep_sort/nn_matching.py:5-28,57-75: the metric of the pipeline's trackers, 0 = cosine (default), 1 = euclidean (other values:
 * DD_E_ARG).  The threshold stays the max_cosine_distance given to dd_pipeline_create, as the reference hands --max-cosine-distance to
 * NearestNeighborDistanceMetric as matching_threshold whatever the metric (deepdish.py:515-516).  Before the first step (DD_E_STATE after). */
int dd_pipeline_metric(dd_pipeline *p, int metric);
/* dd_tracker_set_association for the pipeline's tracker group (deep_sort/tracker.py:95-133, deep_sort/linear_assignment.py:11-141 decided on
 * the host, 0, the default, or on the device, 1; other values: DD_E_ARG).  Between steps. */
int dd_pipeline_association(dd_pipeline *p, int where);
/* Per-stream parameters.  The reference is one process per camera, and each process has its own flags (deepdish.py:1394-1460); the
 * values dd_pipeline_create takes once hold for every stream until one of these setters gives every stream its own.  All of them: before
 * the first step (DD_E_STATE after), arrays of n_streams entries on the host, checked as a whole before anything changes (DD_E_ARG).
 * A pipeline whose entries are all equal launches exactly the kernels, with the arguments, of one built from the scalar.
 *
 * --line (deepdish.py:739-744): lines_host f64 [n_streams][4] = x1, y1, x2, y2 of each stream's count line, finite.  The crossing tests
 * of the count-line pass (:1071-1078, :1303-1312) and of dd_pipeline_overlay use the stream's own line. */
int dd_pipeline_stream_lines(dd_pipeline *p, const double *lines_host);
/* The count lines of `n` streams, out_host f64 [n][4] in the order of streams_host. */
int dd_pipeline_lines(dd_pipeline *p, const int *streams_host, int n, double *out_host);
/* --wanted-labels (deepdish.py:460-461; the adaptors' label filter, tools/ssd_mobilenet.py:204-212, tools/yolov5.py:137-145,
 * tools/tflite.py:26-41; the counters, deepdish.py:525-528): mask_host u8 [n_streams][n_wanted] of 0 / 1 over the wanted_nl list given to
 * dd_pipeline_create -- stream z detects, tracks and counts label i only where mask[z][i] = 1.  A row of zeros is legal: that stream
 * tracks and counts nothing.  The shape of dd_pipeline_counts stays [n_streams][n_wanted][4]; rows a stream does not want stay zero. */
int dd_pipeline_stream_wanted(dd_pipeline *p, const uint8_t *mask_host);
/* --max-cosine-distance, --max-iou-distance, --max-age (deepdish.py:516-517) and deep_sort's n_init (tracker.py:40-49) per stream's
 * tracker; each array is NULL (unchanged) or [n_streams].  max_cos >= 0 and max_iou >= 0, finite; max_age >= 0; n_init >= 0.  The host
 * decision reads them per tracker as it always did; decided on the device (dd_pipeline_association), a group update whose trackers do
 * not all agree launches assoc_match_streams_k, which reads the three association values per decided stream from the staging block the
 * update already uploads (no further copy), instead of assoc_match_k. */
int dd_pipeline_stream_tracker_params(dd_pipeline *p, const double *max_cos_host, const double *max_iou_host, const int *max_age_host,
                                      const int *n_init_host);
/* --nms-max-overlap (deepdish.py:995) per stream, f64 [n_streams], finite.  While every stream of a step has at most 64 candidates and
 * the step's streams do not all agree, the batched NMS launch is nms_small_streams_k, which reads one threshold per problem from the
 * block the step already uploads; beyond 64 candidates the one-call-per-stream form passes that stream's value. */
int dd_pipeline_stream_nms_overlap(dd_pipeline *p, const double *overlap_host);
/* --background-subtraction-ratio (deepdish.py:957) per stream, f64 [n_streams], each in [0, 1]: the motion test of stream z's boxes
 * compares against ratio[z].  Only after dd_pipeline_background_subtraction turned subtraction on (DD_E_STATE otherwise); turning it
 * on again resets every stream to that call's ratio.  Subtraction cannot be off for some streams only. */
int dd_pipeline_stream_motion_ratio(dd_pipeline *p, const double *ratio_host);
/* The motion gate (opt-in; this build's addition -- the reference has none, its nearest relative is the power-saving delay of
 * deepdish.py:963-969): skip the detector and the encoder for the streams where nothing moved.  threshold_host int32 [n_streams],
 * T[z] >= 0.  From then on every step, after tracker predict and MOG2 and before the detector's output is consumed, counts the
 * foreground pixels of each stream on a detector step (mask_stream_count_k, one launch, one more host wait per step) and GATES the
 * streams with count <= T[z] for this step: no detector chain (resize, forward, post-process, adaptor tail), no crops, no encoder
 * rows; the adaptor output dd_pipeline_detections returns is empty; injected rows of the stream are ignored (they stand for a detector
 * output that was not made); everything else runs as for any present stream -- box hygiene, motion test and NMS over zero candidates,
 * the tracker update with zero detections, the count line, its frame number.  The contract: with T[z] = 0 the pipeline is, step by
 * step, bit for bit the ungated one (tracks, galleries, counts, frames seen, motion mask), because an empty mask fails every box of
 * positive area at any ratio > 0 (deepdish.py:957) -- with these differences: (1) a box that the hygiene clips to w * h == 0 passes
 * the reference's test on any mask (0 >= ratio * 0) and is a detection ungated; on a gated step it does not exist; (2) the adaptor
 * output of a gated step is empty instead of holding boxes that would all have been rejected; (3) the motion test's rejected counter
 * does not count what was never made, and dd_pipeline_skip_stats' detector stream-steps exclude gated ones (they are no skip
 * stream-steps either).  T[z] > 0 is a stated approximation for noisy sensors: a stream with at most T[z] foreground pixels hands
 * its tracker nothing, whatever the detector would have found there.  No frames_next run is queued ahead by a gated pipeline (the next
 * step's detector list is not known before its mask is): the argument stays legal and the next step runs its detector itself.
 * Presence masks, background masking and dd_pipeline_reset_streams are allowed (after a reset MOG2 starts over for the stream; the
 * counts that yields decide).  The gate is a parameter of the pipeline, not stream state: snapshots do not carry it.
 * DD_E_STATE: after the first step; subtraction off; a stream's ratio equal to 0 (every box passes count >= 0, so an empty mask decides
 * nothing); either form of object_detector_skip_frames with some N > 0 -- not built: a gated step leaves no detector output for the
 * following skip steps to reuse, and the reference tests the retained boxes against the NEXT frame's mask.  The same combinations are
 * refused by the other setters once the gate is set.  DD_E_ARG: NULL, a negative threshold. */
int dd_pipeline_motion_gate(dd_pipeline *p, const int *threshold_host);
/* out2_host = {steps on which the gate ran (some stream was on a detector step), gated stream-steps summed over the steps}; count_host
 * int32 [n_streams] (may be NULL): the foreground pixels measured on the stream's last detector-eligible step, -1 before its first
 * and after its reset; gated_host u8 [n_streams] (may be NULL): whether that step was gated.  A step without the stream keeps its
 * entry.  Zeros and -1 for a pipeline without the gate. */
int dd_pipeline_gate_stats(dd_pipeline *p, long long *out2_host, int *count_host, uint8_t *gated_host);
/* The listed streams start over; the reference restarts the camera's process.  Between steps, at any time.  Afterwards each listed stream
 * is in the state of a stream of a pipeline just built with the same parameters: no tracks, no deleted list, next id 1
 * (tracker.py:40-49), its gallery chunks back in the pool; empty path store and votes (deepdish.py:519), counters zero (:525-528); no
 * detections, frame number 0, an overlay that reports "never stepped"; MOG2 model, frame count and motion-mask plane as at creation
 * (dd_mog2_reset_streams on the pipeline's stream); per-stream skip counter and phase as dd_pipeline_detector_skip_streams left them,
 * the retained detector output and encoder rows dropped.  Nothing of any other stream is read or written.  A queued look-ahead detector
 * run is discarded: the next step runs the detector itself.  streams_host int32 [n]: an index outside 0 .. n_streams - 1 or listed twice
 * is DD_E_ARG, before anything changes; n = 0 does nothing.  With dd_pipeline_detector_skip_frames(n > 0) it is DD_E_STATE, as masks are:
 * one counter for all streams cannot give one stream a fresh first detector step -- dd_pipeline_detector_skip_streams can. */
int dd_pipeline_reset_streams(dd_pipeline *p, const int *streams_host, int n);
/* out4_host = {launches of nms_small_streams_k, launches of assoc_match_streams_k, dd_pipeline_reset_streams calls that reset at least one
 * stream, streams reset}: whether the per-stream kernel variants ran. */
int dd_pipeline_stream_param_stats(dd_pipeline *p, long long *out4_host);
/* ---- stream snapshots (csrc/snapshot_fmt.h: the blob; csrc/snapshot.hip: the gallery kernels).  A stream restored from a snapshot is,
 * from its next step on, bit for bit the stream the snapshot was taken from: in the same pipeline, in another process, in a pipeline with
 * another number of streams, on another device.  Carried per stream: the tracker (tracks and deleted list in order, next id, every mean
 * and covariance, every gallery in storage order with its sample count), paths, votes, counts (by label name), frame number, the last
 * step's detections and retained adaptor output, the skip counter with the stream's retained encoder rows, and -- background != 0 and
 * subtraction on -- the MOG2 planes, frame count and motion-mask plane.  NOT carried: parameters (recorded and compared), stage timers and
 * the *_stats counters, dd_tracker_last_cost / dd_tracker_last_matches.  Slot and chunk numbers are not state: restore hands out fresh ones.
 *
 * dd_pipeline_snapshot_bytes: what dd_pipeline_snapshot of the listed streams (streams_host NULL: 0 .. n - 1) will write.
 * dd_pipeline_snapshot: a pure read between steps -- it waits for the main stream and changes nothing; a queued look-ahead run stays queued.
 * One chunk_rows_gather_k launch packs every listed gallery, mean and covariance; one copy brings them to the host. */
int dd_pipeline_snapshot_bytes(dd_pipeline *p, const int *streams_host, int n, int background, int64_t *bytes_host);
int dd_pipeline_snapshot(dd_pipeline *p, const int *streams_host, int n, int background, uint8_t *blob_host, int64_t cap, int64_t *bytes_host);
/* Entry i of the blob goes to stream streams_host[i] (NULL: stream i); n must be the blob's entry count.  Equal to dd_pipeline_reset_streams
 * of those streams followed by loading the state; a queued look-ahead run is discarded.  Everything is checked before anything changes, and
 * a restore that returns an error leaves the pipeline exactly as it was: DD_E_ARG for a stream out of range or listed twice, another n
 * than the blob has, a blob its validator refuses, a background section while subtraction is off, or a parameter of the source stream
 * that differs from the destination's (the message names the first: H, W, feature length, metric, nn_budget, detector kind, max_det,
 * labels, wanted labels, line, max_age, n_init, max_cosine_distance, max_iou_distance, nms_max_overlap, motion ratio, masking, the MOG2
 * settings, skip N and phase; floats by bit pattern); DD_E_CAPACITY for more tracks than track_capacity; DD_E_STATE with
 * dd_pipeline_detector_skip_frames(n > 0) (see dd_pipeline_reset_streams) or an update in flight. */
int dd_pipeline_restore(dd_pipeline *p, const uint8_t *blob_host, int64_t n_bytes, const int *streams_host, int n);
/* Host only: validates the blob and describes it.  info_host (may be NULL) int64 [cap_entries][8] = frames seen, tracks (live + deleted),
 * next id, gallery rows, has background, bytes, offset of the entry in the blob, 0. */
int dd_snapshot_info(const uint8_t *blob_host, int64_t n_bytes, int *n_entries_host, int64_t *info_host, int cap_entries);
/* Test aid: the gallery of one live track, rows in STORAGE order (under nn_budget the ring as it lies), and the samples appended so far. */
int dd_tracker_gallery_read(dd_tracker *t, int64_t track_id, float *rows_host, int cap_rows, int *n_rows_host, int *slot_total_host);
/* The two gallery kernels alone.  arenas_host: n_arenas device pointers, each to arena_rows rows of 128 f32 (arena_rows = 32 x a power of two);
 * chunk c is rows [32 (c mod chunks per arena), + 32) of arena c div chunks per arena.  chunks_host int32 [n_chunks]: chunk lists behind
 * one another.  table_host int64 [n_entries][3] = {offset of the entry's list in chunks_host, row count, first row in dense_dev}: row r of
 * an entry is row r mod 32 of chunk list[r div 32].  gather packs the rows into dense_dev (dense_rows rows), scatter is the inverse.
 * Every range is checked here against the stated sizes; destinations must not overlap.  Synchronous. */
int dd_chunk_rows_gather(dd_ctx *ctx, const void *const *arenas_host, int n_arenas, int64_t arena_rows, const int *chunks_host, int n_chunks,
                         const int64_t *table_host, int n_entries, float *dense_dev, int64_t dense_rows, void *stream);
int dd_chunk_rows_scatter(dd_ctx *ctx, void *const *arenas_host, int n_arenas, int64_t arena_rows, const int *chunks_host, int n_chunks,
                          const int64_t *table_host, int n_entries, const float *dense_dev, int64_t dense_rows, void *stream);
/* The pipeline's background subtractor (NULL while subtraction is off), for dd_mog2_state; it is the pipeline's: do not apply or destroy. */
int dd_pipeline_mog2(dd_pipeline *p, dd_mog2 **out);
/* frames: device u8 [n_streams][H][W][3] BGR.  inj_*: optional detections that REPLACE the detector's
 * output (it still runs): tlwh f64 rows, scores, class ids; stream s owns rows
 * [inj_offsets[s], inj_offsets[s+1]).  Blocks until the step is complete. */
int dd_pipeline_step(dd_pipeline *p, const uint8_t *frames, const double *inj_boxes_host,
                     const double *inj_scores_host, const int *inj_cls_host, const int *inj_offsets_host);
/* Same step with a look-ahead: the detector run of `frames_next` (may be NULL) is queued on the pipeline's detector
 * stream once this step has read its own detections -- the reference keeps one detector call and one encoder call
 * in flight on different frames the same way (deepdish.py:935,985,1008).  Contract: the next call must pass
 * `frames_next` as its `frames`, and the memory behind it must stay UNMODIFIED until that call returns -- the queued
 * result is matched to the next step by address, so a capture buffer that is refilled in place (a 1-slot ring) must
 * not be handed in here (pass NULL instead).  frames_next == frames is rejected (DD_E_ARG). */
int dd_pipeline_step2(dd_pipeline *p, const uint8_t *frames, const uint8_t *frames_next, const double *inj_boxes_host,
                      const double *inj_scores_host, const int *inj_cls_host, const int *inj_offsets_host);
/* dd_pipeline_step2 under per-stream presence masks: present_host u8 [n_streams] of 0 / 1 (other values: DD_E_ARG, before anything is
 * queued); NULL = every stream, and then this IS dd_pipeline_step2.  For a stream with present[z] = 0 the step does not exist: no predict,
 * no update, no count-line pass, no vote, no MOG2 update; nothing of its frame slot or of its injected rows is read and nothing of its
 * state is written -- every stream is in the state of a pipeline stepped only when it was present.  The detector's resize and forward
 * run on the present frames alone, compacted by dd_gather_frames' kernel into a buffer of n_streams frames that the first masked step
 * needing it allocates (an all-ones mask gathers nothing).  present_next_host belongs to frames_next (without frames_next: DD_E_ARG;
 * NULL = all present).  The queued look-ahead run remembers its stream list: when the next call arrives with other frames or another
 * list than announced, the run is discarded and the detector runs in that call, with the same result.  An all-zero mask is a legal
 * step that launches nothing and changes no state.  A mask on a pipeline with dd_pipeline_detector_skip_frames set is DD_E_STATE: that
 * form's skip phase is one counter per pipeline (all streams in lock-step); dd_pipeline_detector_skip_streams has one per stream and
 * takes masks. */
int dd_pipeline_step3(dd_pipeline *p, const uint8_t *frames, const uint8_t *present_host, const uint8_t *frames_next,
                      const uint8_t *present_next_host, const double *inj_boxes_host, const double *inj_scores_host,
                      const int *inj_cls_host, const int *inj_offsets_host);
/* seen_host int64 [n_streams]: the number of steps each stream was present in -- its own frame number. */
int dd_pipeline_frames_seen(dd_pipeline *p, int64_t *seen_host);
/* out3_host = {steps that carried a mask, frames_gather_k launches, streams advanced summed over all steps}: which path the steps took. */
int dd_pipeline_present_stats(dd_pipeline *p, long long *out3_host);
/* The stream the look-ahead detector run of dd_pipeline_step2 is queued on (NULL for a pipeline without a detector).  A caller whose
 * `frames_next` are still on their way to the device hands it to dd_ingest_acquire as the consumer of THAT slot: the upload of frame
 * t + 1 is then waited for by the detector run of frame t + 1 alone, not by step t's own kernels -- the reference's capture thread fills
 * the next frame while the stages work on the current one the same way (deepdish.py:837-878, FreshQueue :192-203).  A skip step
 * (dd_pipeline_detector_skip_frames) has no detector run: its main stream waits at step entry for what this stream holds, so frames
 * acquired for it are still uploaded before the step's MOG2 update reads them. */
int dd_pipeline_detector_stream(dd_pipeline *p, void **stream_out);
/* counts_host: int64 [n_streams][n_wanted][4] = poscount, negcount, intcount, delcount */
/* Background subtraction for every stream of the pipeline (deepdish.py:512,889,920-924,957): ratio =
 * --background-subtraction-ratio (reference default 0.25), ratio < 0 = --disable-background-subtraction (the state
 * a new pipeline starts in, as the reference's benchmarks run); masking = --enable-background-masking.  Each
 * step then updates the MOG2 model with the step's frames and drops detector boxes with fewer than
 * ratio * w * h moving pixels before NMS.  (Re-)enabling starts a fresh model. */
int dd_pipeline_background_subtraction(dd_pipeline *p, double ratio, int masking);
/* Foreground mask of the last step, u8 [n_streams][H][W], copied to dst (host, or device when dst_on_device);
 * dst may be NULL to read only the number of boxes the motion test has rejected so far. */
int dd_pipeline_motion_mask(dd_pipeline *p, uint8_t *dst, int dst_on_device, long long *rejected_host);
int dd_pipeline_counts(dd_pipeline *p, int64_t *counts_host);
int dd_pipeline_tracker(dd_pipeline *p, int stream, dd_tracker **out);
/* accumulated host wall time per stage (objd, nms, feat, trak as in deepdish.py's TimingInfo labels) */
int dd_pipeline_stage_seconds(dd_pipeline *p, double *out4_host, long long *steps_host);
/* GPU time per stage, as the reference names its per-frame timers (deepdish.py:975-981 objd, :1018-1021 feat, :1031-1032 trak; nms is the
 * deep_sort NMS of :995): milliseconds between HIP events recorded on the streams the stage's kernels run on, summed over the steps so far --
 * out6 = {objd (resize, detector forward, post-process, adaptor tail, host copy; on the detector stream), nms, feat (crops + encoder), trak
 * (Kalman predict, association, update, track management kernels), host (the steps' wall time outside their waits for the GPU: adaptor
 * filter, box hygiene, LSAP, count line), wall}. */
int dd_pipeline_stage_gpu_ms(dd_pipeline *p, double *out6_host, long long *steps_host);
/* What the detector adaptor returned for one stream in the last step -- the reference's object_detector.detect_image(...) result
 * (deepdish.py:935,985; tools/ssd_mobilenet.py:198-213): tlwh rows (f64), scores, class ids (index into the label file minus the
 * adaptor's label offset); with injected detections, those.  cap rows of room; n_host always gets the row count. */
int dd_pipeline_detections(dd_pipeline *p, int stream, double *boxes_host, double *scores_host, int *classes_host, int cap, int *n_host);

/* The overlay elements of the last step for `n` streams (deepdish.py:971-974,1066-1086,1122-1134: what the reference hands its renderer),
 * packed over the streams in the order of streams_host.  sizes_host int32 [n][4] is always filled: per stream the number of drawn tracks
 * (confirmed, time_since_update <= 1, in track order), of their path points together, of this step's crossing segments and of the
 * detections that went into the tracker.  The other arrays are filled when every one of them is given, with room for caps_host[4] rows
 * of each kind in all (DD_E_CAPACITY otherwise): track_ints int64 rows {track id, line of the label file that holds the voted label or
 * -1, points of its path}; track_tlbr f64 [tracks][4] (to_tlbr()); points f64 [points][2], the bottom-centre path of each track in turn;
 * cross f64 [crossings][4], the last two path points of a track that crossed the line in this step; det_tlbr f64 [detections][4];
 * counts int64 [n][n_wanted][4] as dd_pipeline_counts; line f64 [4], the count line of stream streams_host[0] (with per-stream lines,
 * dd_pipeline_lines has the others).  Host work only; between steps. */
int dd_pipeline_overlay(dd_pipeline *p, const int *streams_host, int n, int *sizes_host, const int *caps_host, int64_t *track_ints_host,
                        double *track_tlbr_host, double *points_host, double *cross_host, double *det_tlbr_host, int64_t *counts_host,
                        double *line_host);

/* ---------------------------------------------------------------- renderer (csrc/render.hip)
 * Paints primitive records over BGR frames in HBM, out of place, one launch for all requested frames.  A record is 8 int32:
 *   {0, x0, y0, x1, y1, 0, ink, 0}        rectangle outline, Pillow's ImageDraw.rectangle byte for byte (x1 >= x0, y1 >= y0)
 *   {1, ax, ay, bx, by, width, ink, 0}    line segment: the pixels within width / 2 of it (a capsule; exact integers; width odd, 1 .. 15)
 *   {2, x, y, w, h, offset, ink, 0}       mask blit: u8 coverage [h][w] at `offset` of the atlas, blended as Pillow's draw_bitmap does
 *   {3, x0, y0, x1, y1, 0, ink, 0}        filled rectangle, Pillow's ImageDraw.rectangle(fill=...) byte for byte: x0 .. x1, y0 .. y1 inclusive (x1 >= x0, y1 >= y0)
 * Kind 3 and lines of EVEN width (the same capsule rule) belong to record set 2: a renderer refuses them until dd_render_record_set(r, 2).
 * ink = B | G << 8 | R << 16; coordinates lie in -8192 .. 8191 and a canvas is at most 8192 either way (DD_E_ARG otherwise).  Records
 * are painted in the order given: a later one overwrites an earlier one. */
typedef struct dd_render dd_render;
int dd_render_create(dd_ctx *ctx, int frame_h, int frame_w, dd_render **out);
int dd_render_destroy(dd_render *r);
/* The records dd_render_draw accepts from now on: DD_RENDER_RECORDS_1 (how a renderer starts) or DD_RENDER_RECORDS_2. */
#define DD_RENDER_RECORDS_1 1
#define DD_RENDER_RECORDS_2 2
int dd_render_record_set(dd_render *r, int record_set);
/* Appends a coverage mask (host u8 [h][w]) to the atlas; offset_out is what a mask record names.  Complete on return. */
int dd_render_put_mask(dd_render *r, const uint8_t *mask_host, int w, int h, int *offset_out);
/* frames_dev: u8 [n_frames][H][W][3].  Output frame i of n is frame streams_host[i] under records prim_off_host[i] ..
 * prim_off_host[i + 1] - 1 of prims_host (prim_off_host: int32 [n + 1], from 0); a frame without records is a copy.  out_dev: u8
 * [n][H][W][3], sharing no byte with frames_dev.  Every record is checked before the launch (DD_E_ARG names the first bad one).  Queued on
 * `stream` (NULL: the context's); draws of one renderer go to one stream at a time. */
int dd_render_draw(dd_render *r, const uint8_t *frames_dev, int n_frames, const int *streams_host, int n, const int32_t *prims_host,
                   const int *prim_off_host, uint8_t *out_dev, void *stream);

/* ---------------------------------------------------------------- ground plane (csrc/ground.hip, csrc/ground_dev.h)
 * The reference's --3d mode (deepdish.py:592-611, :1088-1097): a rectilinear camera at (0, 0, elevation), heading 0, tilt 0 = looking
 * straight down, 90 degrees = at the horizon towards +Y; image pixels go to metres on the plane Z = 0.  A pixel whose ray does not reach
 * the ground (at or above the horizon), or a non-finite one, yields (NaN, NaN).
 * A camera is DD_GROUND_CAMERA_DOUBLES doubles: fx, fy, cx, cy, elevation, cos tilt, sin tilt, cos roll, sin roll. */
#define DD_GROUND_CAMERA_DOUBLES 9
/* Host only.  DD_E_ARG for a non-finite value and for a non-positive focal length, sensor side, image side or elevation. */
int dd_ground_camera(double f_mm, double sensor_w_mm, double sensor_h_mm, int image_w, int image_h, double elevation_m, double tilt_deg,
                     double roll_deg, double *out);
/* cams: f64 [n_cams][9]; cam_index: int32 [n], or NULL for camera 0; points, out: f64 [n][2], sharing no byte.  on_device = 0: host
 * arrays, computed in the call (ctx may be NULL); an index outside 0 .. n_cams - 1 is DD_E_ARG and nothing is written.  on_device = 1:
 * all arrays on the device (points and out 16-byte aligned), one launch queued on `stream` (NULL: the context's); a point with an index
 * outside the table yields NaN and reads no camera.  Host and device results agree bit for bit.  n == 0 is a no-op. */
int dd_ground_from_image(dd_ctx *ctx, const double *cams, int n_cams, const int32_t *cam_index, const double *points, long long n, double *out,
                         int on_device, void *stream);

/* ---------------------------------------------------------------- JPEG encoder (csrc/jpeg.hip)
 * The exit of the render path: BGR frames in HBM -> whole baseline JFIF files in HBM, with no raw download and no CPU encode.  It serves
 * the three places the reference turns an output frame into JPEG: cv2.imencode(".jpg", frame) for the MJPEG web stream
 * (deepdish.py:155-181), frame_%06d.jpg under --output-cvat-dir (:764-766) and the file --stream-path names.  The bytes are libjpeg's
 * for 8-bit YCbCr 4:2:0 with the Annex K tables at `quality` -- Pillow's Image.save(f, 'JPEG', quality=q, subsampling='4:2:0',
 * restart_marker_rows=r), byte for byte, header included.  The one deviation from cv2.imencode is the DRI segment and the RSTn markers
 * (an interval is restart_rows MCU rows); every decoder honours them.  Parity with OpenCV's own bytes is not pinned. */
typedef struct dd_jpeg dd_jpeg;
#define DD_JPEG_LDS     0   /* an interval's samples and coefficients stay in LDS */
#define DD_JPEG_STREAM  1   /* an interval too large for LDS: blocks are transformed again from the frame where they are needed */
/* deepdish.py:168 cv2.imencode(".jpg", frame): one encoder per frame size, quality (1 .. 100; cv2's default is 95) and restart_rows
 * (>= 1, at most 65535 MCUs in an interval); sides 1 .. 8192.  DD_E_ARG names the bad argument.  ctx may be NULL: such an encoder
 * answers dd_jpeg_header only.  No device work happens before the first dd_jpeg_encode. */
int dd_jpeg_create(dd_ctx *ctx, int h, int w, int quality, int restart_rows, dd_jpeg **out);
int dd_jpeg_destroy(dd_jpeg *enc);
/* deepdish.py:168: everything cv2.imencode writes before the scan (SOI, JFIF APP0, two DQT, SOF0, four DHT), then DRI and SOS; the same
 * for every frame of this encoder.  len_host always gets its length; buf_host (may be NULL) gets the bytes when cap suffices
 * (DD_E_CAPACITY otherwise).  Host only. */
int dd_jpeg_header(dd_jpeg *enc, uint8_t *buf_host, int cap, int *len_host);
/* Which kernel path (DD_JPEG_*) a geometry takes (deepdish.py:168 at any frame size); decided from the sizes alone, needs no device. */
int dd_jpeg_plan(int h, int w, int restart_rows, int *path_host);
/* deepdish.py:168,178-179,764-766: frames_dev u8 [n][H][W][3] BGR -> out_dev u8 [n][cap], file i at out_dev + i * cap, and lengths_dev
 * int32 [n].  lengths[i] is always the true length of file i; a file with lengths[i] <= cap is complete in its slot; one that does not
 * fit writes nothing at all, and the call returns DD_E_CAPACITY after the other frames are done.  Two launches on `stream` (NULL: the
 * context's); the call then waits for them, because the lengths decide its return value. */
int dd_jpeg_encode(dd_jpeg *enc, const uint8_t *frames_dev, int n, uint8_t *out_dev, int64_t cap, int *lengths_dev, void *stream);

/* ---------------------------------------------------------------- JPEG decoder (csrc/jpeg_parse.h, csrc/jpeg_dec.hip)
 * The entry of the ingest path for what a camera host usually holds: the frame_%06d.jpg files the reference reads under --input-cvat-dir
 * (deepdish.py:685-689, cv2.VideoCapture at :727) or an MJPEG stream.  Baseline files are decoded in HBM to BGR, libjpeg's arithmetic
 * restated (Annex F Huffman decoding, jidctint.c's accurate-integer IDCT, fancy up-sampling, jdcolor.c's YCbCr -> RGB): Pillow's
 * Image.open(f).convert('RGB') with the channels swapped, byte for byte (tests/jpeg_dec_ref.py).  Parity with OpenCV's own decode is
 * not pinned.
 * Accepted: SOF0, and SOF1 at 8 bits; 1 component, or 3 with luma sampled 1x1, 2x1 or 2x2 over 1x1 chroma; one interleaved scan; DC / AC
 * tables 0 and 1; any DRI.  Everything else is refused by name (DD_JPEG_R_*).
 * Options of dd_jpegdec_create_ex / dd_ingest_create_jpeg_ex, all off unless asked for (below): DD_JPEGDEC_PROGRESSIVE (SOF2 files),
 * DD_JPEGDEC_SPLIT (marker-less scans over many lanes), DD_JPEGDEC_ANY_SIZE (files of any size up to the decoder's, each at its own scale),
 * DD_JPEGDEC_STD_TABLES (the Annex K.3 tables where a file defines none). */
#define DD_E_FORMAT     -5   /* input data (a file) is malformed or of a kind that is refused; the message names the reason */
/* why dd_jpeg_parse refused a file (dd_jpeg_info.reason) */
#define DD_JPEG_R_OK           0
#define DD_JPEG_R_TRUNCATED    1   /* no SOI, a segment length past the file, no SOS before the end */
#define DD_JPEG_R_PROGRESSIVE  2   /* SOF2 / SOF6, or a scan with Ss, Se, Ah, Al other than 0, 63, 0, 0 */
#define DD_JPEG_R_ARITHMETIC   3   /* SOF9 and above */
#define DD_JPEG_R_LOSSLESS     4   /* SOF3 / SOF7, and hierarchical SOF5 */
#define DD_JPEG_R_PRECISION    5   /* sample precision other than 8 bits, or a 16-bit quant table */
#define DD_JPEG_R_COMPONENTS   6   /* neither 1 nor 3 components; an Adobe transform other than YCbCr on 3 */
#define DD_JPEG_R_SAMPLING     7   /* 4:4:0, 4:1:1, sub-sampled luma ... */
#define DD_JPEG_R_SCANS        8   /* a scan that does not hold every component in order */
#define DD_JPEG_R_HUFFMAN      9   /* a DHT that over-subscribes the code space, names more than 256 symbols or a table id above 1 */
#define DD_JPEG_R_UNDEFINED   10   /* a component references a table the file does not define (a Huffman slot 0 / 1: unless DD_JPEGDEC_STD_TABLES) */
#define DD_JPEG_R_SIZE        11   /* height or width of 0 or above 8192 */
#define DD_JPEG_R_SEGMENT     12   /* a segment whose content contradicts its length */
/* per-frame status of a decode (int32) */
#define DD_JPEG_ST_OK          0
#define DD_JPEG_ST_HEADER      1   /* the header was refused (dd_jpeg_parse says why); nothing is written for the frame */
#define DD_JPEG_ST_SIZE        2   /* the SOF size is not the decoder's H x W (DD_JPEGDEC_ANY_SIZE: a side is larger than it); nothing is written */
#define DD_JPEG_ST_DATA        3   /* corrupt or truncated entropy-coded data: the frame holds unspecified bytes, inside its own H x W x 3 */
#define DD_JPEG_ST_NO_FRAME    4   /* ingest ring: no file was put for this stream since the last submit; nothing is written */
/* One Huffman table: Annex C's bits / vals, and what the kernel reads: look[b] = length << 8 | symbol for the code of at most 8 bits that
 * prefixes byte b (0: none); for longer codes maxcode[l] (-1: no code of length l) and valoff[l] = index of the first symbol of length l
 * minus its code. */
typedef struct dd_jpeg_huff {
    uint8_t bits[16], vals[256];
    uint16_t look[256];
    int32_t maxcode[18], valoff[18], nvals, defined;
} dd_jpeg_huff;
/* The header of one file, SOI .. the first SOS.  Fixed size, no pointers: the decoder uploads these records as they are. */
typedef struct dd_jpeg_info {
    int32_t reason;                              /* DD_JPEG_R_* */
    int32_t height, width, ncomp, sof;           /* sof: 0xC0 or 0xC1 */
    int32_t hs[3], vs[3], tq[3], td[3], ta[3];   /* per component: sampling factors, quant table, DC and AC table */
    int32_t hmax, vmax, mcus_x, mcus_y, blocks_per_mcu;
    int32_t restart_interval;                    /* MCUs, 0: none */
    int32_t n_intervals;                         /* ceil(MCUs / interval), 1 without DRI */
    int32_t scan_offset, scan_length;            /* the entropy-coded bytes: from behind the SOS segment to the end of the file */
    int32_t quant_defined[4];
    /* filled by the decoder for its kernels; 0 from dd_jpeg_parse */
    int32_t status, path, interval_base, reserved;
    int64_t file_offset;
    uint16_t quant[4][64];                       /* natural order */
    dd_jpeg_huff huff[4];                        /* DC 0, DC 1, AC 0, AC 1 */
} dd_jpeg_info;
/* Host only, no device: parse `n` bytes of a file into *info.  DD_E_FORMAT with info->reason and a dd_last_error() text that names the
 * reason when the file is refused.  The work is bounded by the header; the entropy-coded bytes are not walked.  Every read is checked
 * against n. */
int dd_jpeg_parse(const uint8_t *file_host, int64_t n, dd_jpeg_info *info);

#define DD_JPEGDEC_LDS     0   /* jpeg_pixels_k keeps a band (one MCU row) of sample planes in LDS */
#define DD_JPEGDEC_PLANES  1   /* a band too wide for that: jpeg_planes_k writes the sample planes to HBM first */
/* Which path a frame of h x w with `ncomp` components and luma sampling hs x vs takes, how many pixel rows a band of jpeg_pixels_k holds
 * and how many bands the frame has.  Needs no device. */
int dd_jpegdec_plan(int h, int w, int ncomp, int hs, int vs, int *path_host, int *band_rows_host, int *bands_host);
/* A decoder for up to max_frames files of h x w per call, max_bytes of file data in all (sides 1 .. 8192).  It owns the coefficient
 * buffer (int16, the largest accepted sampling's blocks per frame) and the staging for records and bytes. */
int dd_jpegdec_create(dd_ctx *ctx, int h, int w, int max_frames, int64_t max_bytes, dd_jpegdec **out);
int dd_jpegdec_destroy(dd_jpegdec *dec);
/* File i is files_host[offsets[i] .. offsets[i] + lengths[i]) (a length of 0: DD_JPEG_ST_NO_FRAME).  Parses each header, uploads the
 * records and the bytes in one copy each, then launches jpeg_markers_k, jpeg_entropy_k and jpeg_pixels_k (jpeg_planes_k in front of the
 * last when a frame takes DD_JPEGDEC_PLANES) on `stream` (NULL: the context's).  out_dev u8 [n][h][w][3] BGR, status_dev int32 [n]
 * (DD_JPEG_ST_*), both valid once the stream has run.  Files may differ in tables, sampling and restart interval.  A frame with a
 * non-zero status costs its neighbours nothing.  The call returns once the uploads have left the host buffers. */
int dd_jpegdec_decode(dd_jpegdec *dec, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, int n, uint8_t *out_dev,
                      int *status_dev, void *stream);
/* Device-event times of a decode's parts (scripts/time_ingest_jpeg.py): after dd_jpegdec_profile(dec, 1) every decode records events, and
 * dd_jpegdec_profile_read waits for the last decode and gives ms_host[4] = the two uploads, jpeg_markers_k, clearing the coefficients +
 * jpeg_entropy_k, jpeg_planes_k + jpeg_pixels_k.  DD_E_STATE without a profiled decode. */
int dd_jpegdec_profile(dd_jpegdec *dec, int on);
int dd_jpegdec_profile_read(dd_jpegdec *dec, float *ms_host);
/* Decoding at 1/2, 1/4 or 1/8 scale: libjpeg's scale_num / scale_denom = 1 / scale, what Pillow's Image.draft and cv2's
 * IMREAD_REDUCED_COLOR_2 / 4 / 8 select.  A file of h x w decodes to ceil(h / scale) x ceil(w / scale), byte for byte Pillow's
 * im.draft(mode, (w // scale, h // scale)); im.convert('RGB') with the channels swapped (tests/jpeg_scaled_ref.py; parity with OpenCV's
 * reduced decode is not pinned).  Markers and entropy decoding are the full-size ones; every 8 x 8 block is transformed straight to n x n
 * samples (jidctred.c), n = 8 / scale, except 4:2:0 chroma, which keeps 2 * n and so needs no up-sampling; 4:2:2 chroma goes through the
 * h2v1 filter (replicated at scale 8).  h x w stays the size a file must state, and the status contract is dd_jpegdec_decode's; out_dev
 * is u8 [n][ceil(h / scale)][ceil(w / scale)][3], and a frame is written only inside its own bytes of it, whatever its status.
 * scale 1 is dd_jpegdec_create / dd_jpegdec_plan exactly; a scale other than 1, 2, 4, 8 is DD_E_ARG naming the value.  A band of
 * jpeg_pixels_k is 8 * vs / scale output rows and needs less LDS, so widths that take DD_JPEGDEC_PLANES at full size stay in LDS here. */
int dd_jpegdec_create_scaled(dd_ctx *ctx, int h, int w, int scale, int max_frames, int64_t max_bytes, dd_jpegdec **out);
int dd_jpegdec_plan_scaled(int h, int w, int ncomp, int hs, int vs, int scale, int *path_host, int *band_rows_host, int *bands_host);
/* The size of the frames this decoder writes: h x w, or the scaled size. */
int dd_jpegdec_output_size(dd_jpegdec *dec, int *out_h_host, int *out_w_host);
/* Pillow's draft rule: the largest of 8, 4, 2, 1 that is <= min(src_w / dst_w, src_h / dst_h) in whole numbers, 1 when that is 0: the
 * decode that is still at least dst_w x dst_h.  Returns the scale; DD_E_ARG for a side below 1.  Host only. */
int dd_jpeg_draft_scale(int src_w, int src_h, int dst_w, int dst_h);

/* ---- progressive files (SOF2), an option of the decoder.  cv2.imread, which the reference calls on images/frame_%06d.jpg
 * (deepdish.py:685-689, :727), reads them without being asked, and a CVAT directory that a tool has re-saved holds them more often than
 * not.  A progressive file ends in the same quantised coefficients as a baseline file, so only the entropy stage differs
 * (jpeg_prog_entropy_k, libjpeg's jdphuff.c restated; tests/jpeg_prog_ref.py is the definition): the pixels are libjpeg's for a complete
 * file, byte for byte Pillow's.  Nothing here changes what dd_jpeg_parse, dd_jpegdec_create(_scaled) or dd_ingest_create_jpeg(_scaled)
 * do: they refuse such a file as before (DD_JPEG_R_PROGRESSIVE, DD_JPEG_ST_HEADER).
 * Accepted: SOF2 at 8 bits with the components and samplings above; up to DD_JPEG_MAX_SCANS scans and DD_JPEG_MAX_TABLES DHT tables
 * (slots 0 .. 3 of each class, redefined between scans at will); DC scans of any subset of the components in frame order; AC scans of one
 * component; any DRI in front of any scan.  Refused by name, beside everything dd_jpeg_parse refuses: */
#define DD_JPEG_R_AC_COMPONENTS 13  /* an AC scan (Ss > 0) of more than one component */
#define DD_JPEG_R_AC_BEFORE_DC  14  /* an AC scan of a component whose DC scan has not come */
#define DD_JPEG_R_FIRST_AH      15  /* the first scan of a band with Ah other than 0 */
#define DD_JPEG_R_REFINEMENT    16  /* a refinement whose Ah is not the band's previous Al or whose Al is not Ah - 1; a band whose
                                       coefficients stand at different bits; a band sent again */
#define DD_JPEG_R_INCOMPLETE    17  /* the scans end with a coefficient of a component not delivered to bit 0: libjpeg would smooth or
                                       zero-fill such a file, this build does not imitate that */
#define DD_JPEG_R_CAPACITY      18  /* more scans or more Huffman tables than dd_jpeg_scans holds */
/* DD_JPEG_R_PROGRESSIVE stays the reason for SOF6 (differential progressive, a hierarchical mode). */
#define DD_JPEG_MAX_SCANS   64      /* libjpeg's and mozjpeg's scripts need at most 12 */
#define DD_JPEG_MAX_TABLES  32
#define DD_JPEG_MAX_LEVELS  16      /* a level lowers a band's Al by one, and Al is at most 13 */
typedef struct dd_jpeg_scan {
    int32_t offset, length;                      /* the entropy-coded bytes within the file: behind the SOS segment to the next marker that
                                                    is neither RSTn nor a stuffed FF 00 */
    int32_t ncomp, comp[3];                      /* indices into the frame's components, ascending */
    int32_t dc[3], ac;                           /* indices into dd_jpeg_scans.pool; -1 where the scan reads no such table */
    int32_t ss, se, ah, al;
    int32_t restart_interval;                    /* the DRI in force at this SOS: MCUs for a scan of several components, blocks for one; 0: none */
    int32_t blocks_x, blocks_y;                  /* the units the scan walks: the MCU grid, or one component's own ceil(w_c / 8) x ceil(h_c / 8) */
    int32_t n_intervals;
    int32_t level;                               /* one more than the highest level of an earlier scan of the same component whose band
                                                    overlaps this one; scans of one level write different coefficients */
    int32_t interval_base;                       /* filled by the decoder; 0 from dd_jpeg_parse_scans */
} dd_jpeg_scan;
typedef struct dd_jpeg_scans {
    int32_t n_scans, n_tables, n_levels, reserved;        /* n_scans 0: a baseline file, all of it in dd_jpeg_info */
    int32_t level_base[DD_JPEG_MAX_LEVELS];               /* filled by the decoder; 0 from dd_jpeg_parse_scans */
    dd_jpeg_scan scan[DD_JPEG_MAX_SCANS];
    dd_jpeg_huff pool[DD_JPEG_MAX_TABLES];                /* every DHT table of the file, in file order */
} dd_jpeg_scans;
/* dd_jpeg_parse for baseline and progressive files.  A baseline file gives exactly dd_jpeg_parse's *info and scans->n_scans 0.  For SOF2 the
 * whole file is walked (entropy-coded bytes are skipped to the next marker, every read checked against n): *info holds the frame
 * (sof 0xC2, no scan fields, no tables) and *scans the scan script.  Host only. */
int dd_jpeg_parse_scans(const uint8_t *file_host, int64_t n, dd_jpeg_info *info, dd_jpeg_scans *scans);
/* dd_jpegdec_create_scaled with flags: DD_JPEGDEC_PROGRESSIVE makes the decoder take SOF2 files too.  After jpeg_markers_k,
 * jpeg_prog_markers_k finds every scan's RSTn markers, and jpeg_prog_entropy_k runs once per level over all files of the call, one lane per
 * (scan, restart interval), into the same zeroed coefficient buffer; baseline files of the same call go through jpeg_entropy_k as ever, and
 * the pixel kernels follow unchanged.  An error in any scan is DD_JPEG_ST_DATA for that file.  flags 0 is dd_jpegdec_create_scaled
 * exactly; an unknown flag is DD_E_ARG. */
#define DD_JPEGDEC_PROGRESSIVE 1
int dd_jpegdec_create_ex(dd_ctx *ctx, int h, int w, int scale, int flags, int max_frames, int64_t max_bytes, dd_jpegdec **out);
/* After a profiled decode on such a decoder: ms_host[DD_JPEG_MAX_LEVELS] = jpeg_prog_entropy_k per level, *n_levels_host how many ran
 * (0: no progressive file in the call); dd_jpegdec_profile_read's third figure then covers both entropy kernels. */
int dd_jpegdec_profile_levels(dd_jpegdec *dec, float *ms_host, int *n_levels_host);
/* dd_ingest_create_jpeg_scaled with the same flags: a ring whose slots take progressive files as well (deepdish.py:685-689). */
int dd_ingest_create_jpeg_ex(dd_ctx *ctx, int slots, int n_streams, int src_h, int src_w, int dst_h, int dst_w, int flip, int scale, int flags,
                             int64_t slot_bytes, dd_ingest **out);
/* A flag for dd_jpegdec_create_ex and dd_ingest_create_jpeg_ex, alone or beside DD_JPEGDEC_PROGRESSIVE, at any scale: several lanes decode
 * one entropy-coded segment.  A baseline file that is a single restart interval (no DRI, DRI 0, or a DRI of the MCU count or more: what an
 * MJPEG camera, cv2.imencode and Pillow write by default) and whose scan is longer than one subsequence goes to jpeg_split_entropy_k, one
 * workgroup per file, in place of one lane of jpeg_entropy_k: the scan is cut into subsequences of DD_JPEGDEC_SPLIT_BYTES (read when the
 * handle is made: a power of two, 16 .. 4096, anything else DD_E_ARG naming the value; kept as given, only doubled for a file with more
 * than 2048 of them.  Not set: 64, doubled per file until it has at most 256 subsequences, one per lane of its workgroup), every lane
 * decodes its subsequences from a guessed state and then from its predecessor's end state until no end state changes, and a last decode
 * stores the coefficients.  The result is the sequential decode, exact on every input, and the status contract
 * is unchanged.  Files with real restart intervals, scans no longer than a subsequence and progressive files take jpeg_entropy_k and
 * jpeg_prog_entropy_k in the same call as ever; without the flag nothing changes.  dd_jpeg_info.reserved holds the log2 of a routed
 * file's subsequence size on the device (0: not routed). */
#define DD_JPEGDEC_SPLIT 2
/* Waits for the decoder's last decode; out_host[4] = files routed to jpeg_split_entropy_k in it, their subsequences, the most rounds a
 * file took (at most its subsequences + 1), and decodes of a subsequence in the rounds (the storing decode not counted).  All zeros for a
 * decoder made without DD_JPEGDEC_SPLIT. */
int dd_jpegdec_split_stats(dd_jpegdec *dec, int64_t *out_host);

/* ---- files of any size up to the decoder's, each at its own scale: a flag for dd_jpegdec_create_ex and dd_ingest_create_jpeg_ex, beside
 * the others, at any scale.  A camera fleet delivers VGA, 720p, 1080p and 4K side by side, and a camera that reconnects changes mode; the
 * reference stretches whatever arrives to its input size (cv2.resize(frame, self.input_size), deepdish.py:867).  With the flag h x w is
 * the largest file accepted: a file with 1 <= height <= h and 1 <= width <= w is DD_JPEG_ST_OK, one with either side larger is
 * DD_JPEG_ST_SIZE, writes nothing, and both sizes stand in dd_last_error().  Path (DD_JPEGDEC_LDS / _PLANES) and dword stores are
 * decided per file.  out_dev stays u8 [n][OH][OW][3], OH = ceil(h / scale), OW = ceil(w / scale), rows OW * 3 bytes apart: frame i is
 * the top-left ceil(h_i / s_i) x ceil(w_i / s_i) of its slot, and no other byte of the slot is written.  The pixels are those of a
 * decoder made for that file's own size and scale, byte for byte: jpeg_pixels_any_k<S> and jpeg_planes_any_k<S> are jpeg_pixels(_scaled)_k
 * and jpeg_planes(_scaled)_k with the pitch, the frame stride and the output size taken from the slot and the record; one launch per
 * scale that occurs in the call, each passing over the files of another scale.  The markers and entropy kernels are per record as ever.
 * On the device dd_jpeg_info.path holds the path in bits 0 .. 7 and the log2 of the file's scale in bits 8 .. 15 (only with this flag);
 * dd_jpeg_info.reserved stays the split log2.  Without the flag nothing changes. */
#define DD_JPEGDEC_ANY_SIZE 4
/* dd_jpegdec_decode with one scale denominator per file: scales int32 [n] of 1, 2, 4, 8, or NULL for the decoder's own scale in every
 * file (then this is dd_jpegdec_decode).  The decoder's own scale is the smallest a call may use -- it fixes OH x OW -- and a smaller
 * entry, or one that is none of 1, 2, 4, 8, is DD_E_ARG.  A scales array needs a decoder made with DD_JPEGDEC_ANY_SIZE (DD_E_STATE). */
int dd_jpegdec_decode_scales(dd_jpegdec *dec, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, const int *scales, int n,
                             uint8_t *out_dev, int *status_dev, void *stream);
/* The ring made with DD_JPEGDEC_ANY_SIZE: src_h x src_w is the largest file accepted.  dd_ingest_jpeg_put parses, records the file's size
 * and scale -- `scale` for every file, or, with scale 0 (accepted with this flag only), Pillow's draft rule per file,
 * dd_jpeg_draft_scale(file_w, file_h, dst_w, dst_h), the slots then being sized for scale 1 -- and dd_ingest_submit always decodes into
 * the staging buffer, n_streams * OH * OW * 3 bytes (n_streams * src_h * src_w * 3 with scale 0 or 1: the caller's to size), builds one
 * crop box per stream from its record, (0, 0, w_out, h_out) with the ring's flip, empty where the host knows the status is not OK,
 * uploads the boxes through the slot's pinned memory without a host wait and launches crop_resize from there to dst_h x dst_w.  A file of
 * exactly twice dst takes crop_resize's INTER_AREA shortcut.  dd_ingest_source_sizes: sizes_host int32 [n_streams][3] = (width, height,
 * scale) of what was put into the slot since its last submit was taken up, zeros where nothing was put or the header was refused; host
 * knowledge, no wait.  DD_E_STATE on a ring made without the flag. */
int dd_ingest_source_sizes(dd_ingest *g, int slot, int *sizes_host);

/* ---- default Huffman tables: a flag for dd_jpegdec_create_ex, dd_ingest_create_jpeg_ex and dd_jpeg_parse_flags.  UVC webcams in MJPG mode
 * and MJPG AVI frames carry no DHT segment and rely on the Annex K.3 tables; libjpeg-turbo fills every undefined slot 0 / 1 with them
 * (jstdhuff.c).  With the flag, at the SOS of a baseline file (SOF0, SOF1 at 8 bits) every DC / AC slot 0 or 1 that a component references
 * and the file has not defined receives the table of that slot -- 0 luminance, 1 chrominance -- in dd_jpeg_info.huff[], look-up form and
 * `defined` included; defined slots are untouched, and behind the parser nothing knows the difference.  Still refused as ever: a table id
 * above 1, a progressive file with an undefined table, everything else.  Without the flag such a file is DD_JPEG_R_UNDEFINED. */
#define DD_JPEGDEC_STD_TABLES 8
/* dd_jpeg_parse (scans NULL) or dd_jpeg_parse_scans (scans given) with flags: 0 or DD_JPEGDEC_STD_TABLES; anything else is DD_E_ARG. */
int dd_jpeg_parse_flags(const uint8_t *file_host, int64_t n, int flags, dd_jpeg_info *info, dd_jpeg_scans *scans);

/* ---------------------------------------------------------------- multi-GPU
 * Sum of the per-stream count vectors (pos, neg, int, del per label; deepdish.py:1141-1145).
 * The collective itself is issued by the host through torch.distributed (RCCL); this entry
 * only packs/accumulates the int64 vector on the device. */
int dd_counts_accumulate(dd_ctx *ctx, int64_t *acc, const int64_t *counts_host, int n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPDISH_HIP_H */
