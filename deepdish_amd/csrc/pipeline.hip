// Multi-stream hot path: S independent video streams advanced one frame each per step, on one GPU.
//
// One step = the four calls the reference's Pipeline makes per frame (deepdish.py upstream):
// run_object_detector :880-885 -> box hygiene :940-960 -> non_max_suppression :995 -> encoder :1008 ->
// tracker.predict/update :1028-1029 -> count-line logic :1035-1114, for every stream, with the
// device work batched ACROSS streams (one detector forward for S frames, one crop launch and one MARS
// forward for all boxes of all streams, one batched NMS launch) and four host<->device round trips
// per STEP instead of ~10 per frame.  Streams share nothing (own tracker, ids, counters), exactly as
// independent DeepDish processes would.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include "common.h"
#include "hostpool.h"
#include "host_phases.h"
#include "snapshot_fmt.h"

namespace {

constexpr int MAX_DET_DEFAULT = 10, MAX_DET_CAP = 64;          // max_detections of the stock SSD post-process op; what csrc/post.hip takes
constexpr float SSD_SCORE_THR = 1e-8f, SSD_IOU_THR = 0.6f;    // its score / NMS thresholds (dd_pipeline_ssd_options: the model file's own)
constexpr int YOLO_HOST_ROWS = 128;      // YOLOv5 rows per stream the first device-to-host copy of a step has room for (the rest, if any, follows)
enum { DET_SSD = 0, DET_YOLOV5 = 1, DET_TFLITE = 2 };
enum { CONFIRMED = 2, DELETED = 3 };
constexpr int GRAIN = 16;                // host phases: one parallel_for over the streams each -- they share nothing (hostpool.h)

// The blocks a detector run fills and the step consumes, one description each: at(base, n, max_det) = the typed pointers into a block
// of n images (on the device or in its pinned host copy), bytes(n, max_det) = what it takes.  enqueue_detector writes them and sizes its
// copy to the host by them, the step's adaptor tails read them, dd_pipeline_create reserves them.
// TFLite_Detection_PostProcess's output, which the generic TFLite adaptor takes as it is: per image max_det boxes f32 x4 (ymin, xmin,
// ymax, xmax, normalised), classes f32, scores f32; then a count per image
struct TfliteBlock {
    float *boxes, *classes, *scores;
    int *count;
    static TfliteBlock at(void *base, size_t n, size_t max_det) {
        float *b = static_cast<float *>(base), *s = b + n * max_det * 5;
        return {b, b + n * max_det * 4, s, reinterpret_cast<int *>(s + n * max_det)};
    }
    static size_t bytes(size_t n, size_t max_det) { return n * max_det * 6 * sizeof(float) + n * sizeof(int); }
};
// the SSD adaptor's tail (ssd_finish, tools/ssd_mobilenet.py:111-150): per image max_det boxes f64 x4 (tlbr, pixels), scores f64, class
// i32; then a count per image
struct SsdBlock {
    double *boxes, *scores;
    int *cls, *count;
    static SsdBlock at(void *base, size_t n, size_t max_det) {
        double *b = static_cast<double *>(base), *s = b + n * max_det * 4;
        int *c = reinterpret_cast<int *>(s + n * max_det);
        return {b, s, c, c + n * max_det};
    }
    static size_t bytes(size_t n, size_t max_det) { return n * (max_det * (4 * 8 + 8 + 4) + 4); }
};
// YOLOv5 on the device: every row of the head may pass the threshold (yolov5.py:120-145 has no limit), so max_det is the head's row
// count -- per image max_det boxes f32 x4, scores f32, classes i32; then a count per image
struct YoloBlock {
    float *boxes, *scores;
    int *cls, *count;
    static YoloBlock at(void *base, size_t n, size_t max_det) {
        float *b = static_cast<float *>(base), *s = b + n * max_det * 4;
        int *c = reinterpret_cast<int *>(s + n * max_det);
        return {b, s, c, c + n * max_det};
    }
    static size_t bytes(size_t n, size_t max_det) { return n * (max_det * 24 + 4); }
};
// YOLOv5 on the host: [n counts | pad to 64 B | rows x 24 B], the passing rows of all images packed behind one another (yolov5_pack: box
// f32 x4, score f32, class i32).  max_det = the packed rows the block has room for, over all images.  bytes() is counts + rows: the pad is
// less than the 64 B of slack its reservation adds.
struct YoloHostBlock {
    static constexpr size_t ROW = 24;
    int *count;
    float *rows;
    static size_t head(size_t n) { return (n * 4 + 63) / 64 * 64; }
    static YoloHostBlock at(void *base, size_t n, size_t /*max_det*/) {
        return {static_cast<int *>(base), reinterpret_cast<float *>(static_cast<char *>(base) + head(n))};
    }
    static size_t bytes(size_t n, size_t max_det) { return n * 4 + max_det * ROW; }
};

struct Votes {                         // track.py:78-81,147-151: label -> confidences, in first-seen order
    std::vector<int> cls;
    std::vector<int> cnt;
    std::vector<double> sum;
    void add(int c, double conf) {
        for (size_t i = 0; i < cls.size(); ++i) if (cls[i] == c) { cnt[i]++; sum[i] += conf; return; }
        cls.push_back(c); cnt.push_back(1); sum.push_back(conf);
    }
};

struct StreamState {
    dd_tracker *trk = nullptr;
    std::map<int64_t, std::vector<std::pair<double, double>>> db;    // deepdish.py:519 self.db
    std::map<int64_t, Votes> votes;
    std::vector<int64_t> counts;                                     // [n_wanted][4] pos, neg, int, del
    std::vector<int> det_cls;                                        // class of every detection of this step
    std::vector<double> det_conf;
    // per-step scratch of the host phases (kept across steps: no allocation in the steady state)
    std::vector<double> boxes0, scores0;                             // detector adaptor output: tlwh f64 rows, scores
    std::vector<int> cls0;
    std::vector<int64_t> ib;                                         // after box hygiene: int boxes, scores, classes
    std::vector<double> is;
    std::vector<int> ic, keep;
    std::vector<int64_t> ints;                                       // count line: track table rows
    std::vector<double> means;
    std::vector<double> det_tlwh;                                    // the rows that went into the tracker in this stream's last step (overlay)
    long long seen = 0;                                              // steps this stream was present in: its own frame number
    // the stream starts over (dd_pipeline_reset_streams): as a new StreamState has it, but for its tracker handle, reset in place
    void restart(size_t n_wanted) {
        dd_tracker *keep_trk = trk;
        *this = StreamState();
        trk = keep_trk;
        counts.assign(n_wanted * 4, 0);
    }
};

using ddhost::cross2;
using ddhost::seg_intersect;
using ddhost::StepPlan;

}  // namespace

struct dd_pipeline {
    dd_ctx *ctx = nullptr;
    int S = 0, H = 0, W = 0;
    dd_net *det = nullptr, *enc = nullptr;
    int det_kind = DET_SSD, det_in = 300, det_in_w = 300, n_anchors = 0, n_classes = 0, enc_batch = 0, enc_h = 64, enc_w = 32;   // enc_h x enc_w: the encoder's crop size (its engine's input)
    int label_offset = 1;                      // class id c is line c + label_offset of the label file (SSD 1, YOLOv5 0)
    float *d_anchors = nullptr;
    double det_conf = 0.5;
    int max_det = MAX_DET_DEFAULT; float ssd_score_thr = SSD_SCORE_THR, ssd_iou_thr = SSD_IOU_THR;   // TFLite_Detection_PostProcess options (dd_pipeline_ssd_options)
    std::vector<std::string> labels;           // label file lines (index = class id + 1, ssd_mobilenet.py:142-147)
    std::vector<std::string> wanted;
    // What the reference takes per process, per stream (dd_pipeline_stream_*; dd_pipeline_create's one value for every stream until then):
    std::vector<double> lines;                 // [S][4] --line
    std::vector<uint8_t> wanted_of;            // [S][n_wanted] --wanted-labels as a mask over `wanted`
    std::vector<double> nms_of;                // [S] --nms-max-overlap; nms_differ: not all equal
    std::vector<double> ratio_of;              // [S] --background-subtraction-ratio (while mog2 is set)
    bool nms_differ = false;
    long long nms_streams_launches = 0, reset_calls = 0, streams_reset = 0;      // dd_pipeline_stream_param_stats
    std::vector<StreamState> st;
    std::vector<dd_tracker *> trks;
    DevBuf d_resized, d_tmp, d_post, d_det, d_fin, d_pack, d_nms, d_crop, d_patches, d_feats;
    DevBuf d_tfl_boxes;                        // generic TFLite adaptor: one whole-frame CropBox per stream (bilinear stretch, BGR -> RGB)
    std::vector<std::string> tfl_labels;       // its label list: the label file's lines after the first, empty lines dropped (tflite.py:22, tflite_object_detector.py)
    bool det_late = true;                      // where the look-ahead detector run is queued (dd_pipeline_step2)
    bool ssd_dec = false;                      // SSD: the head layers decode in their epilogue (dd_net_ssd_decode)
    int ssd_per_class = 0;                     // > 0: the model file states use_regular_nms -- per-class NMS with this detections_per_class (dd_pipeline_ssd_regular_nms)
    struct { const uint8_t *box = nullptr, *cls = nullptr, *lut = nullptr; int stride = 0, n_classes = 0; float quant[4] = {0, 0, 0, 0}; } q8;   // uint8 engine: its head tensors
    bool yolo_dec = false;                     // YOLOv5: the Detect layers reduce their rows in their epilogue (dd_net_yolo_decode)
    size_t yolo_host_rows = 0;                 // YOLOv5: packed rows the first copy of a step brings to the host
    int letterbox_pad = -1;                    // YOLOv5: >= 0 = the detector sees the frame letterboxed on this pad value (dd_pipeline_detector_letterbox)
    std::vector<size_t> ybase;
    PinBuf h_fin, h_nms, h_crop;
    int crop_cap = 0;
    double t_det = 0, t_nms = 0, t_enc = 0, t_trk = 0;    // host wall seconds per stage, accumulated
    // GPU time per stage (dd_pipeline_stage_gpu_ms): HIP events on the streams the kernels run on -- the detector chain on its own stream
    // (Lanczos .. host copy; read when the step consumes it), and on the main stream the pairs 0 predict, 1 NMS, 2 crops + encoder,
    // 3 association, 4 Kalman update / gallery, 5 track management -- read lazily (at the next step or by the getter) so that no step
    // waits for anything it did not wait for before.  host = the step's wall time outside its waits for the GPU.
    hipEvent_t ev_det[2] = {nullptr, nullptr}, ev_main[12] = {};
    bool ev_pair[6] = {false, false, false, false, false, false}, ev_pending = false;
    double g_det = 0, g_nms = 0, g_enc = 0, g_trk = 0, g_host = 0, g_wall = 0;     // milliseconds, accumulated
    double step_wait = 0;                                                          // seconds of this step spent in stream / event waits
    long long steps = 0;
    // The detector has its own stream: like the reference, which keeps one detector call and one encoder call
    // in flight on different frames (deepdish.py:935,985,1008), the detector of frame t+1 can be queued while
    // frame t goes through NMS / encoder / tracker on the main stream.
    hipStream_t det_stream = nullptr;
    hipEvent_t det_done = nullptr, main_mark = nullptr;
    const uint8_t *det_pending = nullptr;      // frames the queued detector run belongs to
    // Background subtraction (deepdish.py:889,920-924,957; the reference's default, off in its benchmarks):
    // MOG2 over every frame on the main stream, then only boxes with enough moving pixels reach NMS.
    dd_mog2 *mog2 = nullptr;
    double motion_ratio = -1.0;                // --background-subtraction-ratio; < 0 = disabled
    bool bg_masking = false;                   // --enable-background-masking
    DevBuf d_mask, d_masked, d_mbox;
    PinBuf h_mbox;
    long long motion_rejected = 0;
    // The motion gate (dd_pipeline_motion_gate): after MOG2 a step counts the foreground pixels of its detector streams (csrc/gate.hip)
    // and takes those with count <= gate_thr[z] out of the detector run.  gate_thr empty = no gate: nothing of it runs.
    std::vector<int> gate_thr;
    ddhost::GateStats gate;
    DevBuf d_gate;
    PinBuf h_gate;
    std::vector<int> off, doff, eoff;          // per-step prefix sums over the positions of act: candidates, tracker input rows, encoder rows
    std::vector<double> tlwh;
    // --object-detector-skip-frames (deepdish.py:892-893,929-938,1003-1014): one set of counters (host_phases.h) drives both forms.  On
    // a skip step a stream keeps the adaptor output of its last detector step (StreamState::boxes0/scores0/cls0) and pairs its boxes with
    // the feature rows of its last encoder run.  Where those rows are kept is what differs:
    //  * dd_pipeline_detector_skip_frames (skip_lockstep; also a pipeline without the option): all streams step together, so the rows
    //    simply stay in d_feats, per-stream offsets foff, and a skip step gathers them with skip_gather_rows_k.  No store.
    //  * dd_pipeline_detector_skip_streams (skip_streams): d_feats is overwritten by the next encoder run of ANY stream, so every stream's
    //    rows are kept in a store of their own (csrc/featrows.hip), compact in stream order and double-buffered: a step that ran the
    //    encoder writes the other buffer (fresh rows replace, everything else is carried) in the launch that assembles the tracker's input.
    ddhost::SkipCounters sk;
    bool skip_lockstep = false, skip_streams = false;
    std::vector<int> foff;                     // row offsets of the last encoder run's features in d_feats, [S + 1]
    DevBuf d_feats_skip, d_gather;             // a skip step's tracker input rows; their per-stream offsets on the device
    PinBuf h_gather;
    hipEvent_t skip_mark = nullptr;            // a step without a detector run: its main stream waits here for what the detector stream holds at step entry
    std::vector<int> ret_off, ret_n, ret_off_new, ret_n_new;   // rows [ret_off[z], + ret_n[z]) of the current store are stream z's; the next store's
    DevBuf d_store[2];
    int store_cur = 0;
    long long det_stream_steps = 0, skip_stream_steps = 0, carry_launches = 0, rows_retained = 0;      // dd_pipeline_skip_stats
    // Presence masks (dd_pipeline_step3): a step advances the streams of plan.act only -- all S of them without a mask.
    ddhost::StepPlan plan;
    std::vector<int> det_pending_act;          // the streams of the queued detector run
    std::vector<dd_tracker *> atrks;           // trks of plan.act
    DevBuf d_gframes;                          // the detector's input frames compacted (frames_gather_k): S * H * W * 3 bytes, allocated by the
                                               // first masked step that needs them
    // index lists for kernels on the detector stream (frames_gather_k's list, the generic adaptor's box table): a ring of pinned / device
    // slots, each guarded by the event of its last copy -- a queued run that is discarded may still be reading the slot before
    static constexpr int LIST_SLOTS = 4;
    PinBuf h_lists;
    DevBuf d_lists;
    hipEvent_t list_copied[LIST_SLOTS] = {};
    int list_next = 0;
    std::vector<int> list_build;
    long long masked_steps = 0, gather_launches = 0, streams_stepped = 0;      // dd_pipeline_present_stats
};

namespace {
// Stage events of the previous step -> the accumulated GPU milliseconds (they completed long ago unless the caller asks right after a step).
int flush_stage_events(dd_pipeline *p) {
    if (!p->ev_pending) return DD_OK;
    p->ev_pending = false;
    double *into[6] = {&p->g_trk, &p->g_nms, &p->g_enc, &p->g_trk, &p->g_trk, &p->g_trk};
    for (int k = 0; k < 6; ++k) {
        if (!p->ev_pair[k]) continue;
        p->ev_pair[k] = false;
        float ms = 0.f;
        DD_HIP(hipEventSynchronize(p->ev_main[2 * k + 1]));
        DD_HIP(hipEventElapsedTime(&ms, p->ev_main[2 * k], p->ev_main[2 * k + 1]));
        *into[k] += (double)ms;
    }
    return DD_OK;
}

// n_ints <= 8 S ints from the host to the device in the order of stream s -> where they will be.  `host` is free when this returns.
int stage_list(dd_pipeline *p, hipStream_t s, const int *host, size_t n_ints, const int **dev) {
    const size_t slot_ints = (size_t)p->S * 8;
    int rc;
    if ((rc = p->h_lists.reserve(slot_ints * dd_pipeline::LIST_SLOTS * sizeof(int))) != DD_OK) return rc;
    if ((rc = p->d_lists.reserve(slot_ints * dd_pipeline::LIST_SLOTS * sizeof(int))) != DD_OK) return rc;
    DD_REQUIRE(n_ints <= slot_ints, DD_E_CAPACITY, "dd_pipeline_step3: a list of %zu ints, room for %zu", n_ints, slot_ints);
    const int k = p->list_next;
    p->list_next = (k + 1) % dd_pipeline::LIST_SLOTS;
    if (!p->list_copied[k]) DD_HIP(hipEventCreateWithFlags(&p->list_copied[k], hipEventDisableTiming));
    else DD_HIP(hipEventSynchronize(p->list_copied[k]));      // four lists ago: complete unless the detector stream is that far behind
    int *h = p->h_lists.as<int>() + k * slot_ints, *d = p->d_lists.as<int>() + k * slot_ints;
    memcpy(h, host, n_ints * sizeof(int));
    DD_HIP(hipMemcpyAsync(d, h, n_ints * sizeof(int), hipMemcpyHostToDevice, s));
    DD_HIP(hipEventRecord(p->list_copied[k], s));
    *dev = d;
    return DD_OK;
}

// present_host (u8 [S], 0 / 1, or NULL = every stream) -> the ascending list of present streams
int present_list(const dd_pipeline *p, const uint8_t *present_host, const char *what, std::vector<int> &act) {
    for (int z = 0; present_host && z < p->S; ++z)
        DD_REQUIRE(present_host[z] <= 1, DD_E_ARG, "dd_pipeline_step3: %s[%d] = %d (0 or 1)", what, z, (int)present_host[z]);
    act.clear();
    for (int z = 0; z < p->S; ++z) if (!present_host || present_host[z]) act.push_back(z);
    return DD_OK;
}

// One whole-frame CropBox per listed stream (the generic adaptor's bilinear stretch, BGR -> RGB): streams == NULL = 0 .. n - 1
void whole_frame_boxes(const dd_pipeline *p, const int *streams, int n, std::vector<int> &hb) {
    hb.assign((size_t)n * 8, 0);
    for (int i = 0; i < n; ++i) { int *b = hb.data() + (size_t)i * 8; b[2] = p->W; b[3] = p->H; b[4] = streams ? streams[i] : i; b[6] = 1; }   // whole frame, swap_rb
}

// index of `name` in the wanted list if stream z wants it, else -1
int wanted_index(const dd_pipeline *p, int z, const std::string &name) {
    const uint8_t *m = p->wanted_of.data() + (size_t)z * p->wanted.size();
    for (size_t i = 0; i < p->wanted.size(); ++i) if (m[i] && p->wanted[i] == name) return (int)i;
    return -1;
}

std::string class_name(const dd_pipeline *p, int c) {
    if (c >= 0 && c + p->label_offset < (int)p->labels.size()) return p->labels[c + p->label_offset];
    return std::string();
}

// track.py:154-188 get_label (Dirichlet-multinomial expectation + the motorbike/bicycle rule)
std::string vote_label(const dd_pipeline *p, const Votes &v) {
    if (v.cls.empty()) return std::string();
    double csum = 0, asum = 0;
    std::vector<double> avg(v.cls.size());
    for (size_t i = 0; i < v.cls.size(); ++i) { avg[i] = v.sum[i] / v.cnt[i]; csum += v.cnt[i]; asum += avg[i]; }
    std::vector<std::pair<double, std::string>> e;
    for (size_t i = 0; i < v.cls.size(); ++i) e.emplace_back((avg[i] + v.cnt[i]) / (csum + asum), class_name(p, v.cls[i]));
    std::sort(e.begin(), e.end());
    std::reverse(e.begin(), e.end());
    if (e.size() > 1 && e[0].second == "motorbike" && e[1].second == "bicycle")
        return e[0].first > e[1].first * 4 ? "motorbike" : "bicycle";
    return e[0].second;
}

double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

}  // namespace

#define DD_BEFORE_FIRST_STEP(name) DD_REQUIRE(p->steps == 0 && !p->det_pending, DD_E_STATE, name ": call before the first step")

extern "C" {

int dd_pipeline_create(dd_ctx *ctx, int n_streams, int frame_h, int frame_w, dd_net *detector,
                       const float *anchors_host, int n_anchors, int n_classes, dd_net *encoder,
                       const char *labels_nl, const char *wanted_nl, double max_cosine_distance, double nms_max_overlap,
                       double max_iou_distance, int max_age, int n_init, const double *line_host, int track_capacity,
                       int gallery_capacity, dd_pipeline **out) {
    DD_REQUIRE(ctx && encoder && out && n_streams > 0 && frame_h > 0 && frame_w > 0 && labels_nl && wanted_nl && line_host,
               DD_E_ARG, "dd_pipeline_create: bad argument");
    DD_REQUIRE(!detector || (n_anchors > 64 && n_classes > 1), DD_E_ARG, "dd_pipeline_create: detector needs its head shape");
    dd_pipeline *p = new dd_pipeline();
    p->ctx = ctx; p->S = n_streams; p->H = frame_h; p->W = frame_w;
    p->det = detector; p->enc = encoder; p->n_anchors = n_anchors; p->n_classes = n_classes;
    p->lines.resize((size_t)n_streams * 4);
    for (size_t i = 0; i < p->lines.size(); ++i) p->lines[i] = line_host[i % 4];
    p->nms_of.assign(n_streams, nms_max_overlap);
    auto split = [](const char *s, std::vector<std::string> &out) {
        std::string cur;
        for (const char *c = s; *c; ++c) { if (*c == '\n') { out.push_back(cur); cur.clear(); } else cur.push_back(*c); }
        if (!cur.empty()) out.push_back(cur);
    };
    split(labels_nl, p->labels);
    split(wanted_nl, p->wanted);
    p->wanted_of.assign((size_t)n_streams * p->wanted.size(), 1);
    DD_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = dd_net_max_batch(encoder, &p->enc_batch)) != DD_OK) return rc;
    if ((rc = dd_net_input_size(encoder, &p->enc_h, &p->enc_w)) != DD_OK) return rc;
    if (detector) {
        int db = 0;
        if ((rc = dd_net_max_batch(detector, &db)) != DD_OK) return rc;
        DD_REQUIRE(db >= n_streams, DD_E_CAPACITY, "dd_pipeline_create: detector max_batch %d < %d streams", db, n_streams);
        if ((rc = dd_net_input_size(detector, &p->det_in, &p->det_in_w)) != DD_OK) return rc;
        p->det_kind = anchors_host ? DET_SSD : DET_YOLOV5;
        if (p->det_kind == DET_YOLOV5) { p->label_offset = 0; p->det_conf = 0.25; }          // yolov5.py:38,134
        DD_HIP(hipStreamCreateWithFlags(&p->det_stream, hipStreamNonBlocking));
        DD_HIP(hipEventCreateWithFlags(&p->det_done, hipEventDisableTiming));
        DD_HIP(hipEventCreateWithFlags(&p->main_mark, hipEventDisableTiming));
        DD_HIP(hipEventCreateWithFlags(&p->skip_mark, hipEventDisableTiming));
        for (hipEvent_t &e : p->ev_det) DD_HIP(hipEventCreate(&e));
        const size_t S = n_streams;
        if ((rc = p->d_resized.reserve(S * p->det_in * p->det_in_w * 3)) != DD_OK) return rc;
        if ((rc = p->d_tmp.reserve(S * frame_h * p->det_in_w * 3 + 64)) != DD_OK) return rc;
        if (p->det_kind == DET_SSD) {
            DD_HIP(hipMalloc(&p->d_anchors, (size_t)n_anchors * 4 * sizeof(float)));
            DD_HIP(hipMemcpy(p->d_anchors, anchors_host, (size_t)n_anchors * 4 * sizeof(float), hipMemcpyHostToDevice));
            if ((rc = p->d_post.reserve(ddk::ssd_post_scratch_bytes(n_anchors, n_streams))) != DD_OK) return rc;
            // the op's first stage (best class, anchor decode, sigmoid, threshold) runs in the head layers' epilogues: the head
            // matrix is never written (DD_SSD_DEC=0 keeps the separate ssd_decode_k pass: same bits, for A/B runs)
            const char *e = getenv("DD_SSD_DEC");
            p->ssd_dec = !(e && atoi(e) == 0);
            if (p->ssd_dec && (rc = dd_net_ssd_decode(detector, anchors_host, n_anchors, SSD_SCORE_THR, 1)) != DD_OK) return rc;
            // sized for the largest max_detections the post-process kernels take: dd_pipeline_ssd_options may raise it before the first step
            if ((rc = p->d_det.reserve(TfliteBlock::bytes(S, MAX_DET_CAP) + 256)) != DD_OK) return rc;
            if ((rc = p->d_fin.reserve(SsdBlock::bytes(S, MAX_DET_CAP) + 256)) != DD_OK) return rc;
            if ((rc = p->h_fin.reserve(SsdBlock::bytes(S, MAX_DET_CAP) + 256)) != DD_OK) return rc;
        } else {
            if ((rc = p->d_post.reserve(S * n_anchors * 8 + 256)) != DD_OK) return rc;              // per-row confidence + class
            // yolov5.py:126-128 (cls *= obj, argmax, confidence) runs in the Detect layers' epilogues when the program carries their
            // per-anchor weight copy: the [rows][85] matrix is never written (DD_YOLO_DEC=0: the separate yolo_conf_k pass, same bits)
            if (p->det_kind == DET_YOLOV5) {
                const char *e = getenv("DD_YOLO_DEC");
                p->yolo_dec = !(e && atoi(e) == 0) && dd_net_yolo_decode(detector, 1) == DD_OK;
            }
            // every row of the head may pass the threshold: then the same rows packed over the images
            if ((rc = p->d_fin.reserve(YoloBlock::bytes(S, n_anchors) + 256)) != DD_OK) return rc;
            if ((rc = p->d_pack.reserve(S * (size_t)n_anchors * YoloHostBlock::ROW + 256)) != DD_OK) return rc;
            p->yolo_host_rows = (size_t)S * YOLO_HOST_ROWS;
            if ((rc = p->h_fin.reserve(YoloHostBlock::bytes(S, p->yolo_host_rows) + 64)) != DD_OK) return rc;
        }
    }
    // late look-ahead (dd_pipeline_step2) when a step's kernels fill the GPU; with a handful of streams they do not, and the detector of
    // the next frame runs beside the encoder from the consume point on (one stream: 0.46 ms per frame early, 0.66 ms late)
    { const char *e = getenv("DD_DET_LATE"); p->det_late = e ? atoi(e) != 0 : n_streams >= 64; }
    p->st.resize(n_streams);
    p->trks.resize(n_streams);
    p->foff.assign(n_streams + 1, 0);
    p->sk.start(n_streams, 0);
    if ((rc = ddk::tracker_group_create(ctx, n_streams, max_cosine_distance, max_iou_distance, max_age, n_init, 0,
                                        track_capacity, gallery_capacity, p->trks.data())) != DD_OK) return rc;
    for (int z = 0; z < n_streams; ++z) {
        p->st[z].trk = p->trks[z];
        p->st[z].counts.assign(p->wanted.size() * 4, 0);
    }
    for (hipEvent_t &e : p->ev_main) DD_HIP(hipEventCreate(&e));
    *out = p;
    return DD_OK;
}

int dd_pipeline_destroy(dd_pipeline *p) {
    if (!p) return DD_OK;
    for (hipEvent_t e : p->ev_det) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->ev_main) if (e) (void)hipEventDestroy(e);
    if (p->det_stream) { (void)hipStreamSynchronize(p->det_stream); (void)hipStreamDestroy(p->det_stream); }
    if (p->det_done) (void)hipEventDestroy(p->det_done);
    if (p->main_mark) (void)hipEventDestroy(p->main_mark);
    if (p->skip_mark) (void)hipEventDestroy(p->skip_mark);
    for (hipEvent_t e : p->list_copied) if (e) (void)hipEventDestroy(e);
    for (auto &s : p->st) dd_tracker_destroy(s.trk);
    (void)hipFree(p->d_anchors);
    dd_mog2_destroy(p->mog2);
    for (DevBuf *b : {&p->d_resized, &p->d_tmp, &p->d_post, &p->d_det, &p->d_fin, &p->d_pack, &p->d_tfl_boxes, &p->d_nms, &p->d_crop, &p->d_patches, &p->d_feats,
                      &p->d_mask, &p->d_masked, &p->d_mbox, &p->d_feats_skip, &p->d_gather, &p->d_gframes, &p->d_lists, &p->d_store[0], &p->d_store[1], &p->d_gate}) b->release();
    for (PinBuf *b : {&p->h_fin, &p->h_nms, &p->h_crop, &p->h_mbox, &p->h_gather, &p->h_lists, &p->h_gate}) b->release();
    delete p;
    return DD_OK;
}

// Which adaptor consumes an SSD-type detector (deepdish.py:482-502 picks the plugin by the model's file name): 0 =
// tools/ssd_mobilenet.py (the default of a pipeline created with anchors: Pillow Lanczos stretch, predict tail with per-class
// nms_boxes), 2 = the generic TFLite-Task adaptor (tools/tflite.py + tools/tflite_object_detector.py: cv2 bilinear stretch of
// the RGB frame, the post-process op's rows with score >= 0.5, int() corners, sorted by score).  Call before the first step.
// TFLite_Detection_PostProcess runs with the options the model file states (the interpreter at tools/ssd_mobilenet.py:100-109 upstream does):
// max_detections rows per frame, nms_score_threshold, nms_iou_threshold -- the stock export's 10 / 1e-8 / 0.6 until this is called.
int dd_pipeline_ssd_options(dd_pipeline *p, int max_detections, float nms_score_threshold, float nms_iou_threshold) {
    DD_REQUIRE(p && p->det && p->det_kind != DET_YOLOV5, DD_E_ARG, "dd_pipeline_ssd_options: needs a pipeline with an SSD-type detector");
    DD_REQUIRE(max_detections >= 1 && max_detections <= MAX_DET_CAP && nms_iou_threshold > 0.f && nms_iou_threshold <= 1.f, DD_E_ARG,
               "dd_pipeline_ssd_options: max_detections %d (1 .. %d), nms_iou_threshold %g (0 < t <= 1)", max_detections, MAX_DET_CAP, (double)nms_iou_threshold);
    DD_BEFORE_FIRST_STEP("dd_pipeline_ssd_options");
    DD_DEVICE(p->ctx);
    if (p->ssd_dec && nms_score_threshold != p->ssd_score_thr) {   // the head layers' decode epilogue carries the score threshold
        std::vector<float> anchors((size_t)p->n_anchors * 4);
        DD_HIP(hipMemcpy(anchors.data(), p->d_anchors, anchors.size() * sizeof(float), hipMemcpyDeviceToHost));
        const int rc = dd_net_ssd_decode(p->det, anchors.data(), p->n_anchors, nms_score_threshold, 1);
        if (rc != DD_OK) return rc;
    }
    p->max_det = max_detections; p->ssd_score_thr = nms_score_threshold; p->ssd_iou_thr = nms_iou_threshold;
    return DD_OK;
}

int dd_pipeline_ssd_regular_nms(dd_pipeline *p, int detections_per_class) {
    DD_REQUIRE(p && p->det && p->det_kind != DET_YOLOV5, DD_E_ARG, "dd_pipeline_ssd_regular_nms: needs a pipeline with an SSD-type detector");
    DD_REQUIRE(detections_per_class >= 1, DD_E_ARG, "dd_pipeline_ssd_regular_nms: detections_per_class %d (>= 1)", detections_per_class);
    DD_BEFORE_FIRST_STEP("dd_pipeline_ssd_regular_nms");
    DD_DEVICE(p->ctx);
    int rc, dtype = 0;
    if ((rc = dd_net_output(p->det, -1, nullptr, nullptr, nullptr, nullptr, nullptr, &dtype)) != DD_OK) return rc;
    if (dtype == 2) {                          // uint8 engine: the op reads the quantised head tensors where the forward leaves them
        int na = 0;
        if ((rc = dd_net_ssd_heads_u8(p->det, &p->q8.box, &p->q8.cls, &p->q8.stride, &p->q8.lut, p->q8.quant, &na, &p->q8.n_classes)) != DD_OK) return rc;
        DD_REQUIRE(na == p->n_anchors && p->q8.n_classes == p->n_classes, DD_E_ARG, "dd_pipeline_ssd_regular_nms: the engine's head has %d anchors x %d columns, the pipeline %d x %d",
                   na, p->q8.n_classes, p->n_anchors, p->n_classes);
    }
    // the decode epilogue keeps the best class of an anchor only: off (the f32 engine then writes its head matrix, as under DD_SSD_DEC=0).
    // The op needs no scratch: d_post stays as it is.
    if ((rc = dd_net_ssd_decode(p->det, nullptr, 0, 0.f, 0)) != DD_OK) return rc;
    p->ssd_dec = false;
    p->ssd_per_class = detections_per_class;
    return DD_OK;
}

int dd_pipeline_detector_adaptor(dd_pipeline *p, int adaptor) {
    DD_REQUIRE(p && p->det && p->det_kind != DET_YOLOV5 && (adaptor == DET_SSD || adaptor == DET_TFLITE), DD_E_ARG,
               "dd_pipeline_detector_adaptor: needs a pipeline with an SSD-type detector; adaptor 0 (ssd_mobilenet) or 2 (tflite)");
    DD_BEFORE_FIRST_STEP("dd_pipeline_detector_adaptor");
    DD_DEVICE(p->ctx);
    p->det_kind = adaptor;
    if (adaptor == DET_TFLITE) {
        p->tfl_labels.clear();
        for (size_t i = 1; i < p->labels.size(); ++i) if (!p->labels[i].empty()) p->tfl_labels.push_back(p->labels[i]);
        std::vector<int> hb;
        whole_frame_boxes(p, nullptr, p->S, hb);
        int rc;
        if ((rc = p->d_tfl_boxes.reserve(hb.size() * sizeof(int))) != DD_OK) return rc;
        DD_HIP(hipMemcpy(p->d_tfl_boxes.p, hb.data(), hb.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return DD_OK;
}

// --object-detector-skip-frames N (deepdish.py:892-893,929-938,1003-1014): the detector and the encoder run on one step in N + 1 --
// steps 0, N + 1, 2 (N + 1), ... counted from the first step; n <= 0 = every step (the default).  All streams step together, so a step
// is either a detector step or a skip step.  A skip step runs no detector chain (resize, forward, post-process, adaptor tail, host copy)
// and no crops / encoder: every stream keeps the adaptor output of the last detector step (what dd_pipeline_detections returns; injected
// detections passed on a skip step are ignored), and its boxes -- through this step's box hygiene, motion test and NMS -- pair with
// that step's feature rows as zip() does: the first min(kept boxes now, feature rows then) of each.  Call before the first step.
int dd_pipeline_detector_skip_frames(dd_pipeline *p, int n) {
    DD_REQUIRE(p, DD_E_ARG, "dd_pipeline_detector_skip_frames: NULL pipeline");
    DD_BEFORE_FIRST_STEP("dd_pipeline_detector_skip_frames");
    DD_REQUIRE(!p->skip_streams || n <= 0, DD_E_STATE,
               "dd_pipeline_detector_skip_frames: the pipeline has per-stream counters (dd_pipeline_detector_skip_streams); one form per pipeline");
    DD_REQUIRE(p->gate_thr.empty() || n <= 0, DD_E_STATE, "dd_pipeline_detector_skip_frames: n = %d on a pipeline with a motion gate "
               "(dd_pipeline_motion_gate): not built -- a gated step leaves no detector output for the skip steps after it to reuse", n);
    if (p->skip_streams) return DD_OK;         // n <= 0 beside per-stream counters: nothing to turn off
    p->skip_lockstep = n > 0;
    p->sk.start(p->S, std::max(n, 0));          // the same N for every stream, no phase
    return DD_OK;
}

// The same option with one counter per stream -- what the reference, one process per camera, has (its counter is per camera).  n_host[z]
// >= 0 is stream z's N; on a step in which z is present: rem[z] > 0 and z has a detector result -> a skip step for z, rem[z] -= 1;
// otherwise a detector step for z, then rem[z] = N[z].  A step without z moves nothing of z, its counter included.  phase_host (NULL:
// none; this build's addition, the reference has no such option) shortens the FIRST cycle only: after z's first detector step rem[z] =
// phase_host[z] in 0 .. N[z] instead of N[z], so that streams with equal N detect on different steps (phase z mod (N + 1): S / (N + 1)
// detector runs on every step after the first).  A mixed step runs predict, MOG2, box hygiene, the motion test, NMS, the tracker update
// and the count line for every present stream, the detector chain and crops + encoder for the streams on a detector step only; a stream
// on a skip step pairs its boxes with the rows of its own last encoder run, kept in a store of retained rows (csrc/featrows.hip).
// Presence masks are allowed in this form.  Call before the first step; not together with dd_pipeline_detector_skip_frames(n > 0).
int dd_pipeline_detector_skip_streams(dd_pipeline *p, const int *n_host, const int *phase_host) {
    DD_REQUIRE(p && n_host, DD_E_ARG, "dd_pipeline_detector_skip_streams: NULL argument");
    DD_BEFORE_FIRST_STEP("dd_pipeline_detector_skip_streams");
    DD_REQUIRE(!p->skip_lockstep, DD_E_STATE,
               "dd_pipeline_detector_skip_streams: the pipeline has the pipeline-wide counter (dd_pipeline_detector_skip_frames); one form per pipeline");
    for (int z = 0; z < p->S; ++z) {
        DD_REQUIRE(n_host[z] >= 0, DD_E_ARG, "dd_pipeline_detector_skip_streams: n[%d] = %d (>= 0)", z, n_host[z]);
        DD_REQUIRE(p->gate_thr.empty() || n_host[z] == 0, DD_E_STATE, "dd_pipeline_detector_skip_streams: n[%d] = %d on a pipeline with a motion gate "
                   "(dd_pipeline_motion_gate): not built -- a gated step leaves no detector output for the skip steps after it to reuse", z, n_host[z]);
        DD_REQUIRE(!phase_host || (phase_host[z] >= 0 && phase_host[z] <= n_host[z]), DD_E_ARG,
                   "dd_pipeline_detector_skip_streams: phase[%d] = %d (0 .. n[%d] = %d)", z, phase_host[z], z, n_host[z]);
    }
    const size_t S = p->S;
    p->skip_streams = true;
    p->sk.start(S, 0);
    p->sk.n.assign(n_host, n_host + S);
    if (phase_host) p->sk.phase.assign(phase_host, phase_host + S);
    p->ret_off.assign(S, 0); p->ret_n.assign(S, 0);
    return DD_OK;
}

// out5_host: detector stream-steps and skip stream-steps summed over the steps, feature_rows_carry_k launches, feature rows retained now,
// bytes allocated for the store (both halves) -- the last three are 0 without dd_pipeline_detector_skip_streams.  skipped_host (u8 [S],
// may be NULL): 1 where the stream's last step was a skip step (counted in both forms of the option).
int dd_pipeline_skip_stats(dd_pipeline *p, long long *out5_host, uint8_t *skipped_host) {
    DD_REQUIRE(p && out5_host, DD_E_ARG, "dd_pipeline_skip_stats: NULL argument");
    out5_host[0] = p->det_stream_steps; out5_host[1] = p->skip_stream_steps; out5_host[2] = p->carry_launches;
    out5_host[3] = p->rows_retained; out5_host[4] = (long long)(p->d_store[0].cap + p->d_store[1].cap);
    for (int z = 0; skipped_host && z < p->S; ++z) skipped_host[z] = p->sk.last[z];
    return DD_OK;
}

// YOLOv5 on aspect-preserving, padded input (csrc/letterbox.hip) instead of the reference adaptor's stretch (tools/yolov5.py:99): the
// step's resize becomes the letterbox launch and both decode forms un-map their boxes from the canvas.  Call before the first step.
int dd_pipeline_detector_letterbox(dd_pipeline *p, int pad) {
    DD_REQUIRE(p && p->det && p->det_kind == DET_YOLOV5, DD_E_ARG, "dd_pipeline_detector_letterbox: needs a pipeline with a YOLOv5 detector");
    DD_REQUIRE(pad >= 0 && pad <= 255, DD_E_ARG, "dd_pipeline_detector_letterbox: pad %d (0 .. 255)", pad);
    DD_BEFORE_FIRST_STEP("dd_pipeline_detector_letterbox");
    int rc;
    if ((rc = dd_letterbox_geometry(p->W, p->H, p->det_in_w, p->det_in, nullptr, nullptr, nullptr, nullptr)) != DD_OK) return rc;
    p->letterbox_pad = pad;
    return DD_OK;
}

// NearestNeighborDistanceMetric("euclidean", ...) for the pipeline's tracker group (nn_matching.py:5-28,57-75,126-132): metric 0 =
// cosine (the default, deepdish.py:515-516), 1 = euclidean -- the encoder's rows are then associated and stored as they come, and the
// max_cosine_distance given to dd_pipeline_create is the matching_threshold on the squared distance, as the reference passes
// --max-cosine-distance for either metric.  Call before the first step.
int dd_pipeline_metric(dd_pipeline *p, int metric) {
    DD_REQUIRE(p, DD_E_ARG, "dd_pipeline_metric: NULL pipeline");
    DD_REQUIRE(metric == 0 || metric == 1, DD_E_ARG, "dd_pipeline_metric: metric must be 0 (cosine) or 1 (euclidean), got %d", metric);
    DD_BEFORE_FIRST_STEP("dd_pipeline_metric");
    return ddk::tracker_group_set_metric(p->trks[0], metric);
}

// Where the pipeline's tracker group decides its association (dd_tracker_set_association for every stream's tracker at once): 0 = on the
// host from the cost matrices (the default), 1 = on the device (csrc/assoc.hip), the decisions being the same.  Between steps only.
int dd_pipeline_association(dd_pipeline *p, int where) {
    DD_REQUIRE(p, DD_E_ARG, "dd_pipeline_association: NULL pipeline");
    DD_REQUIRE(where == 0 || where == 1, DD_E_ARG, "dd_pipeline_association: where must be 0 (host) or 1 (device), got %d", where);
    return ddk::tracker_group_set_association(p->trks[0], where);
}

// ---------------- per-stream parameters (the reference's flags are per process, i.e. per camera; deepdish.py:1394-1460)

// --line (deepdish.py:739-744) per stream
int dd_pipeline_stream_lines(dd_pipeline *p, const double *lines_host) {
    DD_REQUIRE(p && lines_host, DD_E_ARG, "dd_pipeline_stream_lines: NULL argument");
    DD_BEFORE_FIRST_STEP("dd_pipeline_stream_lines");
    for (int i = 0; i < p->S * 4; ++i)
        DD_REQUIRE(std::isfinite(lines_host[i]), DD_E_ARG, "dd_pipeline_stream_lines: lines[%d][%d] is not finite", i / 4, i % 4);
    p->lines.assign(lines_host, lines_host + (size_t)p->S * 4);
    return DD_OK;
}

int dd_pipeline_lines(dd_pipeline *p, const int *streams_host, int n, double *out_host) {
    DD_REQUIRE(p && n >= 0 && (n == 0 || (streams_host && out_host)), DD_E_ARG, "dd_pipeline_lines: bad argument");
    for (int i = 0; i < n; ++i)
        DD_REQUIRE(streams_host[i] >= 0 && streams_host[i] < p->S, DD_E_ARG, "dd_pipeline_lines: stream %d of %d", streams_host[i], p->S);
    for (int i = 0; i < n; ++i) memcpy(out_host + (size_t)i * 4, p->lines.data() + (size_t)streams_host[i] * 4, 4 * sizeof(double));
    return DD_OK;
}

// --wanted-labels (deepdish.py:460-461) per stream, as a 0 / 1 mask over the pipeline's wanted list
int dd_pipeline_stream_wanted(dd_pipeline *p, const uint8_t *mask_host) {
    DD_REQUIRE(p && mask_host, DD_E_ARG, "dd_pipeline_stream_wanted: NULL argument");
    DD_BEFORE_FIRST_STEP("dd_pipeline_stream_wanted");
    const size_t nw = p->wanted.size();
    for (size_t i = 0; i < (size_t)p->S * nw; ++i)
        DD_REQUIRE(mask_host[i] <= 1, DD_E_ARG, "dd_pipeline_stream_wanted: mask[%zu][%zu] = %d (0 or 1)", i / nw, i % nw, (int)mask_host[i]);
    p->wanted_of.assign(mask_host, mask_host + (size_t)p->S * nw);
    return DD_OK;
}

// --max-cosine-distance, --max-iou-distance, --max-age (deepdish.py:516-517), n_init (tracker.py:40-49) per stream's tracker
int dd_pipeline_stream_tracker_params(dd_pipeline *p, const double *max_cos_host, const double *max_iou_host, const int *max_age_host,
                                      const int *n_init_host) {
    DD_REQUIRE(p, DD_E_ARG, "dd_pipeline_stream_tracker_params: NULL pipeline");
    DD_BEFORE_FIRST_STEP("dd_pipeline_stream_tracker_params");
    for (int z = 0; z < p->S; ++z) {
        DD_REQUIRE(!max_cos_host || (std::isfinite(max_cos_host[z]) && max_cos_host[z] >= 0), DD_E_ARG,
                   "dd_pipeline_stream_tracker_params: max_cos[%d] = %g (finite, >= 0)", z, max_cos_host[z]);
        DD_REQUIRE(!max_iou_host || (std::isfinite(max_iou_host[z]) && max_iou_host[z] >= 0), DD_E_ARG,
                   "dd_pipeline_stream_tracker_params: max_iou[%d] = %g (finite, >= 0)", z, max_iou_host[z]);
        DD_REQUIRE(!max_age_host || max_age_host[z] >= 0, DD_E_ARG, "dd_pipeline_stream_tracker_params: max_age[%d] = %d (>= 0)", z, max_age_host[z]);
        DD_REQUIRE(!n_init_host || n_init_host[z] >= 0, DD_E_ARG, "dd_pipeline_stream_tracker_params: n_init[%d] = %d (>= 0)", z, n_init_host[z]);
    }
    for (int z = 0; z < p->S; ++z) {
        const int rc = ddk::tracker_set_params(p->trks[z], max_cos_host ? max_cos_host + z : nullptr, max_iou_host ? max_iou_host + z : nullptr,
                                               max_age_host ? max_age_host + z : nullptr, n_init_host ? n_init_host + z : nullptr);
        if (rc != DD_OK) return rc;
    }
    return DD_OK;
}

// --nms-max-overlap (deepdish.py:995) per stream
int dd_pipeline_stream_nms_overlap(dd_pipeline *p, const double *overlap_host) {
    DD_REQUIRE(p && overlap_host, DD_E_ARG, "dd_pipeline_stream_nms_overlap: NULL argument");
    DD_BEFORE_FIRST_STEP("dd_pipeline_stream_nms_overlap");
    for (int z = 0; z < p->S; ++z)
        DD_REQUIRE(std::isfinite(overlap_host[z]), DD_E_ARG, "dd_pipeline_stream_nms_overlap: overlap[%d] is not finite", z);
    p->nms_of.assign(overlap_host, overlap_host + p->S);
    p->nms_differ = false;
    for (int z = 1; z < p->S; ++z) p->nms_differ = p->nms_differ || p->nms_of[z] != p->nms_of[0];
    return DD_OK;
}

// --background-subtraction-ratio (deepdish.py:957) per stream; subtraction itself is on or off for the whole pipeline
int dd_pipeline_stream_motion_ratio(dd_pipeline *p, const double *ratio_host) {
    DD_REQUIRE(p && ratio_host, DD_E_ARG, "dd_pipeline_stream_motion_ratio: NULL argument");
    DD_REQUIRE(p->mog2, DD_E_STATE, "dd_pipeline_stream_motion_ratio: background subtraction is off (dd_pipeline_background_subtraction first)");
    DD_BEFORE_FIRST_STEP("dd_pipeline_stream_motion_ratio");
    for (int z = 0; z < p->S; ++z)
        DD_REQUIRE(ratio_host[z] >= 0.0 && ratio_host[z] <= 1.0, DD_E_ARG,
                   "dd_pipeline_stream_motion_ratio: ratio[%d] = %g (0 .. 1; subtraction cannot be off for some streams only)", z, ratio_host[z]);
    for (int z = 0; z < p->S; ++z)
        DD_REQUIRE(p->gate_thr.empty() || ratio_host[z] > 0.0, DD_E_STATE, "dd_pipeline_stream_motion_ratio: ratio[%d] = 0 on a pipeline with a motion "
                   "gate (dd_pipeline_motion_gate): every box passes count >= 0, so an empty mask decides nothing", z);
    p->ratio_of.assign(ratio_host, ratio_host + p->S);
    return DD_OK;
}

// The motion gate.  threshold_host int32 [S], T[z] >= 0.  On every step, after MOG2 and before the detector is consumed, the foreground
// pixels (non-zero mask bytes, shadows included) of every stream on a detector step are counted by one launch of mask_stream_count_k
// and one wait; a stream with count <= T[z] is GATED for this step: no detector chain, no crops, no encoder rows, an empty adaptor
// output (injected rows for it are ignored: they stand for a detector output that was not made), and otherwise the step of a present
// stream with zero candidates.  With T = 0 that is the ungated result: an empty mask fails every box of positive area at any ratio > 0
// (deepdish.py:957).  Needs subtraction on with every ratio > 0 and no object_detector_skip_frames N > 0 (not built: a gated step
// leaves nothing for the following skip steps to reuse, and the reference would test the retained boxes against the next mask).  No
// frames_next run is queued ahead by a gated pipeline: the next step's detector list is not known before its mask is.
int dd_pipeline_motion_gate(dd_pipeline *p, const int *threshold_host) {
    DD_REQUIRE(p && threshold_host, DD_E_ARG, "dd_pipeline_motion_gate: NULL argument");
    DD_BEFORE_FIRST_STEP("dd_pipeline_motion_gate");
    DD_REQUIRE(p->mog2, DD_E_STATE, "dd_pipeline_motion_gate: background subtraction is off (dd_pipeline_background_subtraction first)");
    for (int z = 0; z < p->S; ++z) {
        DD_REQUIRE(threshold_host[z] >= 0, DD_E_ARG, "dd_pipeline_motion_gate: threshold[%d] = %d (>= 0)", z, threshold_host[z]);
        DD_REQUIRE(p->ratio_of[z] > 0.0, DD_E_STATE, "dd_pipeline_motion_gate: background_subtraction_ratio[%d] = 0 -- every box passes "
                   "count >= 0, so an empty mask decides nothing", z);
        DD_REQUIRE(p->sk.n[z] == 0, DD_E_STATE, "dd_pipeline_motion_gate: object_detector_skip_frames N[%d] = %d -- gating together with skip "
                   "frames is not built: a gated step leaves no detector output for the skip steps after it to reuse", z, p->sk.n[z]);
    }
    p->gate_thr.assign(threshold_host, threshold_host + p->S);
    p->gate.start(p->S);
    return DD_OK;
}

// out2_host = {steps on which the gate ran (some stream was on a detector step), gated stream-steps}; count_host int32 [S] (may be
// NULL): the foreground pixels measured on each stream's last detector-eligible step, -1 before its first (and after its reset);
// gated_host u8 [S] (may be NULL): whether that step was gated.  All zero / -1 for a pipeline without the gate.
int dd_pipeline_gate_stats(dd_pipeline *p, long long *out2_host, int *count_host, uint8_t *gated_host) {
    DD_REQUIRE(p && out2_host, DD_E_ARG, "dd_pipeline_gate_stats: NULL argument");
    out2_host[0] = p->gate.steps; out2_host[1] = p->gate.gated;
    for (int z = 0; z < p->S; ++z) {
        if (count_host) count_host[z] = p->gate_thr.empty() ? -1 : p->gate.last_count[z];
        if (gated_host) gated_host[z] = p->gate_thr.empty() ? 0 : p->gate.last_gated[z];
    }
    return DD_OK;
}

// The listed streams start over (the reference restarts the camera's process): every piece of per-stream state back to what
// dd_pipeline_create, dd_pipeline_background_subtraction and dd_pipeline_detector_skip_streams left.  Host state, plus the memsets of the
// MOG2 mode-count plane and the motion-mask plane on the main stream, which the next step's launches follow.
int dd_pipeline_reset_streams(dd_pipeline *p, const int *streams_host, int n) {
    DD_REQUIRE(p && n >= 0 && (n == 0 || streams_host), DD_E_ARG, "dd_pipeline_reset_streams: bad argument");
    std::vector<uint8_t> listed(p->S, 0);
    for (int i = 0; i < n; ++i) {
        const int z = streams_host[i];
        DD_REQUIRE(z >= 0 && z < p->S, DD_E_ARG, "dd_pipeline_reset_streams: stream %d of %d", z, p->S);
        DD_REQUIRE(!listed[z], DD_E_ARG, "dd_pipeline_reset_streams: stream %d is listed twice", z);
        listed[z] = 1;
    }
    // one counter for all streams cannot give one stream a fresh first detector step
    DD_REQUIRE(!p->skip_lockstep, DD_E_STATE, "dd_pipeline_reset_streams: the pipeline has the pipeline-wide object_detector_skip_frames counter "
               "(dd_pipeline_detector_skip_frames); dd_pipeline_detector_skip_streams has one per stream and takes a reset");
    if (n == 0) return DD_OK;
    DD_DEVICE(p->ctx);
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = ddk::tracker_reset(p->trks[streams_host[i]])) != DD_OK) return rc;
    if (p->mog2) {
        hipStream_t s = p->ctx->stream;
        if ((rc = ddk::mog2_reset_streams(p->mog2, s, streams_host, n)) != DD_OK) return rc;
        const size_t hw = (size_t)p->H * p->W;
        for (int i = 0; i < n; ++i) DD_HIP(hipMemsetAsync(p->d_mask.as<uint8_t>() + (size_t)streams_host[i] * hw, 0, hw, s));
    }
    for (int i = 0; i < n; ++i) {
        const int z = streams_host[i];
        p->st[z].restart(p->wanted.size());
        p->sk.restart(z);                          // counter and phase as at construction
        if (!p->gate_thr.empty()) p->gate.restart(z);
        if (p->skip_streams) {                     // the retained rows leave the store at its next refresh
            p->rows_retained -= p->ret_n[z];
            p->ret_n[z] = 0;
        }
    }
    p->det_pending = nullptr;                      // a queued look-ahead run is discarded: the next step runs the detector itself
    p->reset_calls += 1; p->streams_reset += n;
    return DD_OK;
}

int dd_pipeline_stream_param_stats(dd_pipeline *p, long long *out4_host) {
    DD_REQUIRE(p && out4_host, DD_E_ARG, "dd_pipeline_stream_param_stats: NULL argument");
    out4_host[0] = p->nms_streams_launches; out4_host[1] = ddk::tracker_group_stream_param_launches(p->trks[0]);
    out4_host[2] = p->reset_calls; out4_host[3] = p->streams_reset;
    return DD_OK;
}

int dd_pipeline_mog2(dd_pipeline *p, dd_mog2 **out) {
    DD_REQUIRE(p && out, DD_E_ARG, "dd_pipeline_mog2: NULL argument");
    *out = p->mog2;
    return DD_OK;
}

// deepdish.py:512,889: background subtraction on (ratio = --background-subtraction-ratio, default 0.25) or off
// (ratio < 0 = --disable-background-subtraction).  Turning it on starts a fresh model; masking =
// --enable-background-masking (the detector and the encoder then see cv2.bitwise_and(frame, frame, mask=fgMask)).
int dd_pipeline_background_subtraction(dd_pipeline *p, double ratio, int masking) {
    DD_REQUIRE(p && !(ratio > 1.0), DD_E_ARG, "dd_pipeline_background_subtraction: ratio must be <= 1 (negative = off)");
    DD_REQUIRE(p->gate_thr.empty() || ratio > 0.0, DD_E_STATE, "dd_pipeline_background_subtraction: ratio %g on a pipeline with a motion gate "
               "(dd_pipeline_motion_gate), which needs subtraction on and a ratio above 0", ratio);
    DD_DEVICE(p->ctx);
    DD_HIP(hipStreamSynchronize(p->ctx->stream));
    if (p->det_stream) DD_HIP(hipStreamSynchronize(p->det_stream));
    p->det_pending = nullptr;                    // a detector run queued ahead is dropped: it may not match the new setting
    dd_mog2_destroy(p->mog2);
    p->mog2 = nullptr; p->motion_ratio = -1.0; p->bg_masking = false;
    if (ratio < 0) return DD_OK;
    int rc;
    if ((rc = dd_mog2_create(p->ctx, p->S, p->H, p->W, 500, 16.0, 1, &p->mog2)) != DD_OK) return rc;
    if ((rc = p->d_mask.reserve((size_t)p->S * p->H * p->W)) != DD_OK) return rc;
    if (masking && (rc = p->d_masked.reserve((size_t)p->S * p->H * p->W * 3)) != DD_OK) return rc;
    p->motion_ratio = ratio; p->bg_masking = masking != 0;
    p->ratio_of.assign(p->S, ratio);
    return DD_OK;
}

// Foreground mask of the last step, u8 [S][H][W], copied to dst (host or device memory); dst may be NULL to read
// only the number of boxes the motion test has rejected so far.
int dd_pipeline_motion_mask(dd_pipeline *p, uint8_t *dst, int dst_on_device, long long *rejected_host) {
    DD_REQUIRE(p, DD_E_ARG, "dd_pipeline_motion_mask: NULL argument");
    DD_DEVICE(p->ctx);
    if (rejected_host) *rejected_host = p->motion_rejected;
    if (!dst) return DD_OK;
    DD_REQUIRE(p->mog2, DD_E_ARG, "dd_pipeline_motion_mask: background subtraction is off");
    DD_HIP(hipMemcpyAsync(dst, p->d_mask.p, (size_t)p->S * p->H * p->W, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          p->ctx->stream));
    DD_HIP(hipStreamSynchronize(p->ctx->stream));
    return DD_OK;
}

int dd_pipeline_tracker(dd_pipeline *p, int stream, dd_tracker **out) {
    DD_REQUIRE(p && out && stream >= 0 && stream < p->S, DD_E_ARG, "dd_pipeline_tracker: bad argument");
    *out = p->st[stream].trk;
    return DD_OK;
}

int dd_pipeline_counts(dd_pipeline *p, int64_t *counts_host) {
    DD_REQUIRE(p && counts_host, DD_E_ARG, "dd_pipeline_counts: NULL argument");
    const size_t n = p->wanted.size() * 4;
    for (int s = 0; s < p->S; ++s) memcpy(counts_host + (size_t)s * n, p->st[s].counts.data(), n * sizeof(int64_t));
    return DD_OK;
}

int dd_pipeline_detector_stream(dd_pipeline *p, void **stream_out) {
    DD_REQUIRE(p && stream_out, DD_E_ARG, "dd_pipeline_detector_stream: NULL argument");
    *stream_out = p->det ? reinterpret_cast<void *>(p->det_stream) : nullptr;
    return DD_OK;
}

int dd_pipeline_stage_gpu_ms(dd_pipeline *p, double *out6_host, long long *steps_host) {
    DD_REQUIRE(p && out6_host, DD_E_ARG, "dd_pipeline_stage_gpu_ms: NULL argument");
    DD_DEVICE(p->ctx);
    const int rc = flush_stage_events(p);
    if (rc != DD_OK) return rc;
    out6_host[0] = p->g_det; out6_host[1] = p->g_nms; out6_host[2] = p->g_enc; out6_host[3] = p->g_trk; out6_host[4] = p->g_host; out6_host[5] = p->g_wall;
    if (steps_host) *steps_host = p->steps;
    return DD_OK;
}

int dd_pipeline_detections(dd_pipeline *p, int stream, double *boxes_host, double *scores_host, int *classes_host, int cap, int *n_host) {
    DD_REQUIRE(p && n_host && stream >= 0 && stream < p->S && cap >= 0, DD_E_ARG, "dd_pipeline_detections: bad argument");
    const StreamState &q = p->st[stream];
    const int n = (int)q.scores0.size();
    *n_host = n;
    DD_REQUIRE(n <= cap || (!boxes_host && !scores_host && !classes_host), DD_E_CAPACITY, "dd_pipeline_detections: %d rows, room for %d", n, cap);
    if (boxes_host) memcpy(boxes_host, q.boxes0.data(), (size_t)n * 4 * sizeof(double));
    if (scores_host) memcpy(scores_host, q.scores0.data(), (size_t)n * sizeof(double));
    if (classes_host) memcpy(classes_host, q.cls0.data(), (size_t)n * sizeof(int));
    return DD_OK;
}

int dd_pipeline_frames_seen(dd_pipeline *p, int64_t *seen_host) {
    DD_REQUIRE(p && seen_host, DD_E_ARG, "dd_pipeline_frames_seen: NULL argument");
    for (int z = 0; z < p->S; ++z) seen_host[z] = p->st[z].seen;
    return DD_OK;
}

int dd_pipeline_present_stats(dd_pipeline *p, long long *out3_host) {
    DD_REQUIRE(p && out3_host, DD_E_ARG, "dd_pipeline_present_stats: NULL argument");
    out3_host[0] = p->masked_steps; out3_host[1] = p->gather_launches; out3_host[2] = p->streams_stepped;
    return DD_OK;
}

// The overlay elements of the last step, read off the state the step left: the tracker's host mirror, StreamState::db and votes, the
// tracker input rows (StreamState::det_tlwh) and the counters.  A stream absent from the last step shows its own last step.
int dd_pipeline_overlay(dd_pipeline *p, const int *streams_host, int n, int *sizes_host, const int *caps_host, int64_t *track_ints_host,
                        double *track_tlbr_host, double *points_host, double *cross_host, double *det_tlbr_host, int64_t *counts_host,
                        double *line_host) {
    DD_REQUIRE(p && streams_host && sizes_host && n > 0, DD_E_ARG, "dd_pipeline_overlay: bad argument");
    for (int i = 0; i < n; ++i)
        DD_REQUIRE(streams_host[i] >= 0 && streams_host[i] < p->S, DD_E_ARG, "dd_pipeline_overlay: stream %d of %d", streams_host[i], p->S);
    const bool fill = track_ints_host && track_tlbr_host && points_host && cross_host && det_tlbr_host && counts_host && line_host;
    DD_REQUIRE(!fill || caps_host, DD_E_ARG, "dd_pipeline_overlay: arrays without their capacities");
    size_t nt = 0, np = 0, nc = 0, nd = 0;
    std::vector<int64_t> ints;
    std::vector<double> means;
    for (int i = 0; i < n; ++i) {
        const int z = streams_host[i];
        StreamState &st = p->st[z];
        const bool stepped = st.seen > 0;
        const double *line = p->lines.data() + (size_t)z * 4;
        int nl = 0, rc;
        if ((rc = dd_tracker_count(st.trk, 0, &nl)) != DD_OK) return rc;
        ints.resize((size_t)nl * 6); means.resize((size_t)nl * 8);
        if (nl && stepped && (rc = ddk::tracker_read_host(st.trk, 0, ints.data(), means.data())) != DD_OK) return rc;
        int *sz = sizes_host + (size_t)i * 4;
        sz[0] = sz[1] = sz[2] = 0;
        sz[3] = (int)(st.det_tlwh.size() / 4);
        for (int k = 0; stepped && k < nl; ++k) {
            const int64_t *r = ints.data() + (size_t)k * 6;
            if (r[1] != CONFIRMED || r[2] > 1) continue;                // deepdish.py:1053
            const auto it = st.db.find(r[0]);
            const size_t npts = it == st.db.end() ? 0 : it->second.size();
            bool crossed = false;
            if (npts > 1) {                                               // :1071-1078
                const double a[2] = {it->second[npts - 1].first, it->second[npts - 1].second};
                const double b[2] = {it->second[npts - 2].first, it->second[npts - 2].second};
                crossed = seg_intersect(line, line + 2, a, b);
            }
            if (fill) {
                DD_REQUIRE(nt < (size_t)caps_host[0] && np + npts <= (size_t)caps_host[1] && nc + crossed <= (size_t)caps_host[2], DD_E_CAPACITY,
                           "dd_pipeline_overlay: more rows than the arrays have room for");
                const auto vt = st.votes.find(r[0]);
                const std::string lbl = vt == st.votes.end() ? std::string() : vote_label(p, vt->second);
                int64_t line_no = -1;
                for (size_t li = 0; li < p->labels.size() && line_no < 0 && !lbl.empty(); ++li) if (p->labels[li] == lbl) line_no = (int64_t)li;
                int64_t *ti = track_ints_host + nt * 3;
                ti[0] = r[0]; ti[1] = line_no; ti[2] = (int64_t)npts;
                const double *m = means.data() + (size_t)k * 8;
                const double w = m[2] * m[3];                            // track.py:84-111 to_tlbr
                double *tb = track_tlbr_host + nt * 4;
                tb[0] = m[0] - w / 2; tb[1] = m[1] - m[3] / 2; tb[2] = tb[0] + w; tb[3] = tb[1] + m[3];
                for (size_t q = 0; q < npts; ++q) { points_host[(np + q) * 2] = it->second[q].first; points_host[(np + q) * 2 + 1] = it->second[q].second; }
                if (crossed) {
                    double *c = cross_host + nc * 4;
                    c[0] = it->second[npts - 2].first; c[1] = it->second[npts - 2].second; c[2] = it->second[npts - 1].first; c[3] = it->second[npts - 1].second;
                }
            }
            ++nt; ++sz[0]; np += npts; sz[1] += (int)npts; nc += crossed; sz[2] += crossed;
        }
        if (fill) {
            DD_REQUIRE(nd + sz[3] <= (size_t)caps_host[3], DD_E_CAPACITY, "dd_pipeline_overlay: more detections than the array has room for");
            for (int j = 0; j < sz[3]; ++j) {                            // detection.py to_tlbr
                const double *b = st.det_tlwh.data() + (size_t)j * 4;
                double *o = det_tlbr_host + (nd + j) * 4;
                o[0] = b[0]; o[1] = b[1]; o[2] = b[0] + b[2]; o[3] = b[1] + b[3];
            }
            const size_t nw = p->wanted.size() * 4;
            memcpy(counts_host + (size_t)i * nw, st.counts.data(), nw * sizeof(int64_t));
        }
        nd += sz[3];
    }
    if (fill) for (int i = 0; i < 4; ++i) line_host[i] = p->lines[(size_t)streams_host[0] * 4 + i];
    return DD_OK;
}

int dd_pipeline_stage_seconds(dd_pipeline *p, double *out4_host, long long *steps_host) {
    DD_REQUIRE(p && out4_host, DD_E_ARG, "dd_pipeline_stage_seconds: NULL argument");
    out4_host[0] = p->t_det; out4_host[1] = p->t_nms; out4_host[2] = p->t_enc; out4_host[3] = p->t_trk;
    if (steps_host) *steps_host = p->steps;
    return DD_OK;
}

}  // extern "C"

namespace {

// resize -> forward -> post-process -> adaptor tail -> pinned host block, all streams at once, on the
// detector stream; det_done fires when the host block is complete.
// DD_STAGE_EVENTS=0: no stage events (dd_pipeline_stage_gpu_ms then reports zeros for the GPU stages); fourteen event records and seven
// reads per step are ~10 us of host time -- noise against a multi-millisecond batched step, a few % of a single stream's 0.45 ms frame
static const bool g_stage_events = !(getenv("DD_STAGE_EVENTS") && atoi(getenv("DD_STAGE_EVENTS")) == 0);
#define DD_STAGE_BEGIN(k) do { if (g_stage_events) DD_HIP(hipEventRecord(p->ev_main[2 * (k)], s)); } while (0)
#define DD_STAGE_END(k) do { if (g_stage_events) { DD_HIP(hipEventRecord(p->ev_main[2 * (k) + 1], s)); p->ev_pair[k] = true; } } while (0)
#define DD_TIMED_WAIT(expr) do { const double w0_ = now_s(); DD_HIP(expr); p->step_wait += now_s() - w0_; } while (0)

// `act`: the streams whose frames the run takes, ascending (dd_pipeline_step3's present streams; all S of them without a mask).  The
// batch is n = act.size(): every block of the run's output is indexed by POSITION in act.  With n < S the resize launches, which take a
// dense batch, read the n frames compacted into d_gframes by one frames_gather_k launch; the generic adaptor's crop_resize carries a
// stream index per box, so its box table is built over act instead.
int enqueue_detector(dd_pipeline *p, const uint8_t *frames, const std::vector<int> &act) {
    hipStream_t s = p->det_stream;
    const int n = (int)act.size(), MAX_DET = p->max_det;
    int rc;
    const uint8_t *src = frames;               // what the resize reads: n dense frames
    const int *d_tfl = p->d_tfl_boxes.as<int>(), *d_idx_gather = nullptr;
    if (n < p->S && p->det_kind == DET_TFLITE) {
        whole_frame_boxes(p, act.data(), n, p->list_build);
        if ((rc = stage_list(p, s, p->list_build.data(), p->list_build.size(), &d_tfl)) != DD_OK) return rc;
    } else if (n < p->S) {
        const size_t frame_bytes = (size_t)p->H * p->W * 3;
        if (!p->d_gframes.p) {                 // the first masked step that needs it: S frames, exactly (DevBuf::reserve would add a quarter)
            DD_HIP(hipMalloc(&p->d_gframes.p, (size_t)p->S * frame_bytes));
            p->d_gframes.cap = (size_t)p->S * frame_bytes;
        }
        if ((rc = stage_list(p, s, act.data(), act.size(), &d_idx_gather)) != DD_OK) return rc;
        src = p->d_gframes.as<uint8_t>();
    }
    // order after whatever the caller has queued on the main stream so far (e.g. the ingest ring's wait for the
    // upload of these frames)
    DD_HIP(hipEventRecord(p->main_mark, p->ctx->stream));
    DD_HIP(hipStreamWaitEvent(s, p->main_mark, 0));
    if (g_stage_events) DD_HIP(hipEventRecord(p->ev_det[0], s));
    if (src != frames) {
        if ((rc = ddk::gather_frames(s, frames, (long long)p->H * p->W * 3, d_idx_gather, n, p->d_gframes.as<uint8_t>())) != DD_OK) return rc;
        p->gather_launches += 1;
    }
    if (p->det_kind == DET_TFLITE) {                           // tflite_object_detector.py:207-211: cv2.resize (INTER_LINEAR) of the RGB frame
        if ((rc = ddk::crop_resize(s, frames, p->H, p->W, d_tfl, n, p->det_in, p->det_in_w, p->d_resized.as<uint8_t>())) != DD_OK) return rc;
    } else if (p->letterbox_pad >= 0) {                        // dd_pipeline_detector_letterbox: d_tmp holds n * H * det_in_w * 3 >= n * H * new_w * 3 bytes
        if ((rc = ddk::resize_lanczos_letterbox(s, p->ctx->device, src, n, p->H, p->W, 3, 1, p->d_resized.as<uint8_t>(), p->det_in, p->det_in_w,
                                                p->letterbox_pad, p->d_tmp.as<uint8_t>())) != DD_OK) return rc;
    } else if ((rc = ddk::resize_lanczos(s, p->ctx->device, src, p->H, p->W, 3, 1, p->d_resized.as<uint8_t>(), p->det_in,
                                         p->det_in_w, p->d_tmp.as<uint8_t>(), n)) != DD_OK) return rc;    // ssd_mobilenet.py:54-57, yolov5.py:99
    if ((rc = dd_net_forward(p->det, p->d_resized.as<uint8_t>(), n, s)) != DD_OK) return rc;       // :102-103 / yolov5.py:107-109
    void *raw = nullptr;
    if ((rc = dd_net_output(p->det, -1, &raw, nullptr, nullptr, nullptr, nullptr, nullptr)) != DD_OK) return rc;
    // every adaptor ends the same way: its block to the pinned host copy, then the run is the pending one
    auto finish = [&](const void *d_block, size_t bytes, size_t h_offset) -> int {
        DD_HIP(hipMemcpyAsync(p->h_fin.as<char>() + h_offset, d_block, bytes, hipMemcpyDeviceToHost, s));
        if (g_stage_events) DD_HIP(hipEventRecord(p->ev_det[1], s));
        DD_HIP(hipEventRecord(p->det_done, s));
        p->det_pending = frames; p->det_pending_act = act;
        return DD_OK;
    };
    if (p->det_kind == DET_YOLOV5) {                                                               // yolov5.py:120-131
        const YoloBlock y = YoloBlock::at(p->d_fin.p, n, p->n_anchors);
        if (p->yolo_dec) {                                       // :126-128 ran in the Detect layers' epilogues
            float *b4 = nullptr, *cf = nullptr; int *cl = nullptr;
            if ((rc = dd_net_yolo_decoded(p->det, &b4, &cf, &cl, nullptr)) != DD_OK) return rc;
            if (p->letterbox_pad >= 0) {
                if ((rc = ddk::yolov5_select_letterbox(s, b4, cf, cl, p->n_anchors, (float)p->det_conf, p->W, p->H, p->det_in_w, p->det_in, y.boxes, y.scores, y.cls,
                                                       p->n_anchors, y.count, n)) != DD_OK) return rc;
            } else
            if ((rc = ddk::yolov5_select(s, b4, cf, cl, p->n_anchors, (float)p->det_conf, (float)p->W, (float)p->H, y.boxes, y.scores, y.cls,
                                         p->n_anchors, y.count, n)) != DD_OK) return rc;
        } else if (p->letterbox_pad >= 0) {
            if ((rc = ddk::yolov5_decode_letterbox(s, static_cast<const float *>(raw), p->n_anchors, p->n_classes, (float)p->det_conf, p->W, p->H,
                                                   p->det_in_w, p->det_in, y.boxes, y.scores, y.cls, p->n_anchors, y.count, n, p->d_post.p)) != DD_OK) return rc;
        } else
        if ((rc = ddk::yolov5_decode(s, static_cast<const float *>(raw), p->n_anchors, p->n_classes, (float)p->det_conf, (float)p->W,
                                     (float)p->H, y.boxes, y.scores, y.cls, p->n_anchors, y.count, n, p->d_post.p)) != DD_OK) return rc;
        // the passing rows of all streams packed behind one another; of the host block the counts and the first yolo_host_rows rows
        // now, whatever lies beyond them when the step consumes the block
        if ((rc = ddk::yolov5_pack(s, y.boxes, y.scores, y.cls, y.count, p->n_anchors, n, p->d_pack.as<float>())) != DD_OK) return rc;
        DD_HIP(hipMemcpyAsync(p->h_fin.p, y.count, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        return finish(p->d_pack.p, p->yolo_host_rows * YoloHostBlock::ROW, YoloHostBlock::head(n));
    }
    const TfliteBlock d = TfliteBlock::at(p->d_det.p, n, MAX_DET);
    if (p->ssd_per_class > 0) {                                 // use_regular_nms = true: per-class NMS, straight from the head
        if (p->q8.cls) rc = ddk::ssd_regular_nms_u8(s, p->q8.box, p->q8.cls, p->q8.stride, p->q8.lut, p->q8.quant, p->d_anchors, p->n_anchors, p->n_classes,
                                                    MAX_DET, p->ssd_per_class, p->ssd_score_thr, p->ssd_iou_thr, d.boxes, d.classes, d.scores, d.count, n);
        else rc = ddk::ssd_regular_nms_raw(s, static_cast<const float *>(raw), p->d_anchors, p->n_anchors, p->n_classes, MAX_DET, p->ssd_per_class,
                                           p->ssd_score_thr, p->ssd_iou_thr, d.boxes, d.classes, d.scores, d.count, n);
        if (rc != DD_OK) return rc;
    } else if (p->ssd_dec) {
        float *eb = nullptr, *es = nullptr, *ek = nullptr;
        int *ec = nullptr;
        if ((rc = dd_net_ssd_decoded(p->det, &eb, &es, &ec, &ek)) != DD_OK) return rc;
        if ((rc = ddk::ssd_postprocess_decoded(s, eb, es, ec, ek, p->n_anchors, MAX_DET, p->ssd_score_thr, p->ssd_iou_thr, d.boxes, d.classes, d.scores, d.count, n,
                                               p->d_post.p, p->d_post.cap)) != DD_OK) return rc;
    } else if ((rc = ddk::ssd_postprocess(s, static_cast<const float *>(raw), p->d_anchors, p->n_anchors, p->n_classes, MAX_DET,
                                          p->ssd_score_thr, p->ssd_iou_thr, d.boxes, d.classes, d.scores, d.count, n, p->d_post.p, p->d_post.cap)) != DD_OK) return rc;
    if (p->det_kind == DET_TFLITE)                             // the generic adaptor's tail is a few integer truncations: on the host (consume_tflite)
        return finish(p->d_det.p, TfliteBlock::bytes(n, MAX_DET), 0);
    const SsdBlock f = SsdBlock::at(p->d_fin.p, n, MAX_DET);
    if ((rc = ddk::ssd_finish(s, d.boxes, d.classes, d.scores, n, MAX_DET, p->det_conf, 0.5, (double)p->W, (double)p->H, f.boxes, f.cls, f.scores, f.count)) != DD_OK)
        return rc;                                                                                    // :111-150
    return finish(p->d_fin.p, SsdBlock::bytes(n, MAX_DET), 0);
}

// A skip step's tracker input (deepdish.py:1003-1014: zip(boxes, labels, scores, features) with the last encoder run's features):
// row j < n_z = dst_off[z + 1] - dst_off[z] of stream z is feature row src_off[z] + j of that run; the host has truncated n_z to the
// rows stream z had then, so every read stays inside them.  One block per stream; a 128-f32 row moves as 32 float4.
__global__ void __launch_bounds__(256) skip_gather_rows_k(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                          const int *__restrict__ dst_off, const int *__restrict__ src_off) {
    const int z = blockIdx.x;
    const int a = dst_off[z], n = dst_off[z + 1] - a;
    const float4 *sp = src + (size_t)src_off[z] * 32;
    float4 *dp = dst + (size_t)a * 32;
    for (int i = threadIdx.x; i < n * 32; i += blockDim.x) dp[i] = sp[i];
}

// Count-line logic of one stream after its tracker update (deepdish.py:1035-1114, 1303-1312); host only.
void count_line_one_stream(dd_pipeline *p, int z) {
    StreamState &st = p->st[z];
    const double *line = p->lines.data() + (size_t)z * 4;
    int nd = 0, nl = 0;
    dd_tracker_count(st.trk, 1, &nd);
    dd_tracker_count(st.trk, 0, &nl);
    std::vector<int64_t> &ints = st.ints;
    std::vector<double> &means = st.means;
    std::map<std::string, int> delcounts;
    if (nd) {
        ints.resize((size_t)nd * 6);
        ddk::tracker_read_host(st.trk, 1, ints.data(), nullptr);
        for (int i = 0; i < nd; ++i) {
            const int64_t id = ints[(size_t)i * 6];
            delcounts.clear();                                  // overwritten per deleted track (:1040-1044)
            auto it = st.db.find(id);
            if (it != st.db.end() && it->second.size() > 1) {
                bool hit = false;
                for (size_t q = 0; q + 1 < it->second.size() && !hit; ++q) {
                    const double a[2] = {it->second[q].first, it->second[q].second};
                    const double b[2] = {it->second[q + 1].first, it->second[q + 1].second};
                    hit = seg_intersect(line, line + 2, a, b);
                }
                if (hit) delcounts[vote_label(p, st.votes[id])] += 1;
                it->second.clear();
            }
            st.votes.erase(id);
        }
    }
    if (nl) {
        ints.resize((size_t)nl * 6);
        means.resize((size_t)nl * 8);
        ddk::tracker_read_host(st.trk, 0, ints.data(), means.data());
    }
    std::vector<std::pair<std::string, double>> events;
    for (int i = 0; i < nl; ++i) {
        const int64_t *r = ints.data() + (size_t)i * 6;
        const int64_t id = r[0];
        if (r[5] >= 0) st.votes[id].add(st.det_cls[r[5]], st.det_conf[r[5]]);
        if (r[1] != CONFIRMED || r[2] > 1) continue;
        const double *m = means.data() + (size_t)i * 8;
        const double w = m[2] * m[3];                            // track.py:84-111 to_tlbr
        const double x1 = m[0] - w / 2, y1 = m[1] - m[3] / 2;
        const double x2 = x1 + w, y2 = y1 + m[3];
        auto &pts = st.db[id];
        pts.emplace_back((x1 + x2) / 2.0, y2);
        if (pts.size() > 1) {
            const double p2[2] = {pts.back().first, pts.back().second};
            const double q2[2] = {pts[pts.size() - 2].first, pts[pts.size() - 2].second};
            const double cp = cross2(line[2] - line[0], line[3] - line[1], q2[0] - p2[0], q2[1] - p2[1]);
            if (seg_intersect(line, line + 2, p2, q2)) events.emplace_back(vote_label(p, st.votes[id]), cp);
        }
    }
    for (auto &e : events) {
        const int wi = wanted_index(p, z, e.first);
        if (wi < 0) continue;
        st.counts[wi * 4 + (e.second >= 0 ? 0 : 1)] += 1;
        st.counts[wi * 4 + 2] += 1;
    }
    for (auto &d : delcounts) {
        const int wi = wanted_index(p, z, d.first);
        if (wi >= 0) st.counts[wi * 4 + 3] += d.second;
    }
}

}  // namespace

// ---------------- the phases of one step, in the order dd_pipeline_step3 calls them.  i is a position in pl.act and z = pl.act[i] the
// stream, except in the adaptor tails, where i is a position in pl.dl (the detector run's blocks hold dl.size() images).

// 1. Which streams step, which of them run the detector, what the counters will be, which frames are read, whether a look-ahead run is
// queued: everything the step decides, before it launches anything.
static int phase_plan(dd_pipeline *p, StepPlan &pl, const uint8_t *frames_in, const uint8_t *present_host, const uint8_t *frames_next,
                      const uint8_t *present_next_host, const double *inj_boxes_host, const double *inj_scores_host, const int *inj_cls_host,
                      const int *inj_offsets_host) {
    int rc;
    if ((rc = present_list(p, present_host, "present", pl.act)) != DD_OK) return rc;
    if ((rc = present_list(p, present_next_host, "present_next", pl.act_next)) != DD_OK) return rc;
    ddhost::plan_skip(p->sk, pl);              // deepdish.py:929-938: a stream's first step detects; then N skip steps follow every detector step
    const bool masking = p->mog2 && p->bg_masking;          // the detector and the encoder then read the masked copy, which a look-ahead run cannot
    pl.frames_in = frames_in; pl.present = present_host;
    pl.frames = masking ? p->d_masked.as<uint8_t>() : frames_in;
    // no stream of the next step on a detector step: nothing to queue; under the motion gate the next step's list is not known before
    // its mask is
    pl.frames_next = pl.dl_next.empty() || masking || !p->gate_thr.empty() ? nullptr : frames_next;
    pl.inj_boxes = inj_boxes_host; pl.inj_scores = inj_scores_host; pl.inj_cls = inj_cls_host; pl.inj_offsets = inj_offsets_host;
    return DD_OK;
}

// 2. tracker predict for the step's streams; MOG2 over their frames
static int phase_predict_mog2(dd_pipeline *p, const StepPlan &pl) {
    hipStream_t s = p->ctx->stream;
    int rc;
    if ((pl.dl.empty() || !p->gate_thr.empty()) && p->det) {
        // no detector run reads these frames (or, under the motion gate, none was queued ahead and none may follow): the main stream takes over what the detector stream holds for them (the wait an ingest
        // ring queued there for their upload, dd_pipeline_detector_stream) before MOG2 reads them
        DD_HIP(hipEventRecord(p->skip_mark, p->det_stream));
        DD_HIP(hipStreamWaitEvent(s, p->skip_mark, 0));
    }
    DD_STAGE_BEGIN(0);
    if ((rc = ddk::trackers_predict(p->atrks.data(), (int)pl.act.size())) != DD_OK) return rc;      // deepdish.py:1028
    DD_STAGE_END(0);
    if (p->mog2) {                                                                      // :920-924
        if ((rc = ddk::mog2_apply_streams(p->mog2, s, pl.frames_in, pl.present, -1.0, p->d_mask.as<uint8_t>(),
                                          p->bg_masking ? p->d_masked.as<uint8_t>() : nullptr)) != DD_OK) return rc;
        if (p->bg_masking) p->det_pending = nullptr;           // a run queued on the unmasked frames: dropped
    }
    return DD_OK;
}

// 2b. The motion gate: the foreground pixels of every stream of dl, one launch and one wait; the streams with nothing (at most T[z]
// pixels) moving leave dl -- the third state of a position: not on a skip step, no block in the detector run -- with an empty adaptor
// output.  The index arithmetic is ddhost::gate_streams.
static int phase_motion_gate(dd_pipeline *p, StepPlan &pl) {
    if (p->gate_thr.empty() || pl.dl.empty()) return DD_OK;
    hipStream_t s = p->ctx->stream;
    const int nd = (int)pl.dl.size();
    int rc;
    if ((rc = p->d_gate.reserve((size_t)p->S * sizeof(int))) != DD_OK) return rc;
    if ((rc = p->h_gate.reserve((size_t)p->S * sizeof(int))) != DD_OK) return rc;
    const int *d_list = nullptr;               // every stream: the planes in order, no list
    if (nd < p->S && (rc = stage_list(p, s, pl.dl.data(), pl.dl.size(), &d_list)) != DD_OK) return rc;
    if ((rc = ddk::mask_stream_count(s, p->d_mask.as<uint8_t>(), p->H, p->W, d_list, nd, p->d_gate.as<int>())) != DD_OK) return rc;
    DD_HIP(hipMemcpyAsync(p->h_gate.p, p->d_gate.p, (size_t)nd * sizeof(int), hipMemcpyDeviceToHost, s));
    DD_TIMED_WAIT(hipStreamSynchronize(s));                                                        // the gate's round trip
    ddhost::gate_streams(p->gate_thr, p->h_gate.as<int>(), pl);
    for (size_t i = 0; i < pl.act.size(); ++i)
        if (pl.gat[i]) { StreamState &q = p->st[pl.act[i]]; q.boxes0.clear(); q.scores0.clear(); q.cls0.clear(); }
    return DD_OK;
}

// 3a. YOLOv5's tail (yolov5.py:137-145) over the packed host block; a busy step fetches the rows its first copy had no room for
static int consume_yolov5(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &dl = pl.dl;
    const int nd = (int)dl.size();
    int rc;
    const size_t head = YoloHostBlock::head(nd), ROW = YoloHostBlock::ROW;
    const int *yn = YoloHostBlock::at(p->h_fin.p, nd, p->yolo_host_rows).count;
    std::vector<size_t> &ybase = p->ybase;
    ybase.assign(nd + 1, 0);
    for (int i = 0; i < nd; ++i) ybase[i + 1] = ybase[i] + (size_t)std::min(yn[i], p->n_anchors);
    if (ybase[nd] > p->yolo_host_rows) {                    // a busy step: fetch the rest (the detector stream is idle here) and
        const size_t have = p->yolo_host_rows, total = ybase[nd];      // make room for twice as many from now on
        // ... but never more than the packed block holds (S * n_anchors rows): the first copy of every later step reads that many
        const size_t grown = std::min(2 * total, (size_t)p->S * (size_t)p->n_anchors);
        PinBuf bigger;
        if ((rc = bigger.reserve(head + grown * ROW)) != DD_OK) return rc;
        memcpy(bigger.p, p->h_fin.p, head + have * ROW);
        hipError_t he = hipMemcpyAsync(bigger.as<char>() + head + have * ROW, p->d_pack.as<char>() + have * ROW, (total - have) * ROW,
                                       hipMemcpyDeviceToHost, p->det_stream);
        if (he == hipSuccess) he = hipStreamSynchronize(p->det_stream);
        if (he != hipSuccess) { bigger.release(); DD_HIP(he); }
        p->h_fin.release();
        p->h_fin = bigger;
        p->yolo_host_rows = grown;
    }
    const float *rows = YoloHostBlock::at(p->h_fin.p, nd, p->yolo_host_rows).rows;
    ddk::parallel_for(nd, GRAIN, [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) {
            StreamState &q = p->st[dl[i]];
            q.boxes0.clear(); q.scores0.clear(); q.cls0.clear();
            const int nr = (int)(ybase[i + 1] - ybase[i]);
            for (int r = 0; r < nr; ++r) {
                const float *b = rows + (ybase[i] + r) * 6;
                int c;
                memcpy(&c, b + 5, 4);
                const float sc = b[4];
                if (wanted_index(p, dl[i], class_name(p, c)) < 0 || !(sc >= (float)p->det_conf)) continue;
                q.boxes0.insert(q.boxes0.end(), {(double)b[0], (double)b[1], (double)(b[2] - b[0]), (double)(b[3] - b[1])});   // f32 arithmetic, :140-142
                q.scores0.push_back((double)sc);
                q.cls0.push_back(c);
            }
        }
    });
    return DD_OK;
}

// 3b. The generic TFLite adaptor's tail: tflite_object_detector.py:234-295 (_postprocess) + tools/tflite.py:26-41 -- score >= threshold,
// int() of the scaled corners (f32 arithmetic, truncation), label = label_list[class], stable sort by descending score, wanted labels only
static int consume_tflite(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &dl = pl.dl;
    const int nd = (int)dl.size(), MAX_DET = p->max_det;
    const TfliteBlock h = TfliteBlock::at(p->h_fin.p, nd, MAX_DET);
    const float *hb = h.boxes, *hc = h.classes, *hs = h.scores;
    const int *hn = h.count;
    ddk::parallel_for(nd, GRAIN, [&](int z0, int z1) {
        for (int z = z0; z < z1; ++z) {
            StreamState &q = p->st[dl[z]];
            q.boxes0.clear(); q.scores0.clear(); q.cls0.clear();
            int order[MAX_DET_CAP], no = 0;
            for (int i = 0; i < hn[z] && i < MAX_DET; ++i)
                if ((double)hs[z * MAX_DET + i] >= p->det_conf) order[no++] = i;     // np.float32 >= python float: compared in float64
            std::stable_sort(order, order + no, [&](int a, int b) { return hs[z * MAX_DET + a] > hs[z * MAX_DET + b]; });
            for (int k = 0; k < no; ++k) {
                const int i = order[k], c = (int)hc[z * MAX_DET + i];
                if (c < 0 || c >= (int)p->tfl_labels.size() || wanted_index(p, dl[z], p->tfl_labels[c]) < 0) continue;
                // the class stored for the vote is resolved through class_name() = labels[c + label_offset]: the same line of the
                // label file only while no blank line precedes it -- store the index class_name() maps back to this very label
                int cs = -1;
                for (int li = p->label_offset; li < (int)p->labels.size() && cs < 0; ++li) if (p->labels[li] == p->tfl_labels[c]) cs = li - p->label_offset;
                if (cs < 0) continue;
                const float *b = hb + ((size_t)z * MAX_DET + i) * 4;                          // ymin, xmin, ymax, xmax (normalised)
                // int(np.float32 * python int): the reference's pinned NumPy promotes the product to float64 (exact), then truncates
                const int top = (int)((double)b[0] * (double)p->H), left = (int)((double)b[1] * (double)p->W);
                const int bottom = (int)((double)b[2] * (double)p->H), right = (int)((double)b[3] * (double)p->W);
                q.boxes0.insert(q.boxes0.end(), {(double)left, (double)top, (double)(right - left), (double)(bottom - top)});
                q.scores0.push_back((double)hs[z * MAX_DET + i]);
                q.cls0.push_back(cs);
            }
        }
    });
    return DD_OK;
}

// 3c. The SSD adaptor's tail (ssd_mobilenet.py:204-212) over what ssd_finish left
static int consume_ssd(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &dl = pl.dl;
    const int nd = (int)dl.size(), MAX_DET = p->max_det;
    const SsdBlock h = SsdBlock::at(p->h_fin.p, nd, MAX_DET);
    const double *hb = h.boxes, *hs = h.scores;
    const int *hc = h.cls, *hn = h.count;
    ddk::parallel_for(nd, GRAIN, [&](int z0, int z1) {
        for (int z = z0; z < z1; ++z) {
            StreamState &q = p->st[dl[z]];
            q.boxes0.clear(); q.scores0.clear(); q.cls0.clear();
            for (int i = 0; i < hn[z]; ++i) {
                const double sc = hs[z * MAX_DET + i];
                if (!(sc >= p->det_conf) || wanted_index(p, dl[z], class_name(p, hc[z * MAX_DET + i])) < 0) continue;
                const double *b = hb + ((size_t)z * MAX_DET + i) * 4;
                q.boxes0.insert(q.boxes0.end(), {b[0], b[1], b[2] - b[0], b[3] - b[1]});
                q.scores0.push_back(sc);
                q.cls0.push_back(hc[z * MAX_DET + i]);
            }
        }
    });
    return DD_OK;
}

// 3. The detector's block for the streams of dl -> their adaptor output (StreamState::boxes0 / scores0 / cls0); the streams on a skip
// step keep theirs.  The early look-ahead form queues the next frames here.
static int phase_consume_detector(dd_pipeline *p, const StepPlan &pl) {
    int rc;
    if (pl.dl.empty()) {
        p->det_pending = nullptr;                  // (a run queued for a step that turns out to have no detector stream: dropped)
        if (p->det && pl.frames_next && !p->det_late && (rc = enqueue_detector(p, pl.frames_next, pl.dl_next)) != DD_OK) return rc;
        return DD_OK;
    }
    if (!p->det) {                                 // injected detections only
        for (int z : pl.dl) { StreamState &q = p->st[z]; q.boxes0.clear(); q.scores0.clear(); q.cls0.clear(); }
        return DD_OK;
    }
    if ((p->det_pending != pl.frames || p->det_pending_act != pl.dl) && (rc = enqueue_detector(p, pl.frames, pl.dl)) != DD_OK) return rc;   // not queued ahead (or for other streams): run it now
    DD_TIMED_WAIT(hipEventSynchronize(p->det_done));                                               // round trip 1
    p->det_pending = nullptr;
    if (g_stage_events) {   // the detector chain of these frames on its stream: resize, forward, post-process, adaptor tail, host copy
        float ms = 0.f;
        DD_HIP(hipEventElapsedTime(&ms, p->ev_det[0], p->ev_det[1]));
        p->g_det += (double)ms;
    }
    rc = p->det_kind == DET_YOLOV5 ? consume_yolov5(p, pl) : p->det_kind == DET_TFLITE ? consume_tflite(p, pl) : consume_ssd(p, pl);
    if (rc != DD_OK) return rc;
    // the host block has been consumed: the detector buffers are free for the next frames
    if (pl.frames_next && !p->det_late && (rc = enqueue_detector(p, pl.frames_next, pl.dl_next)) != DD_OK) return rc;
    return DD_OK;
}

// 4. Injected detections replace the adaptor output of the streams on a detector step (not of a gated one: there was no such output); box hygiene (deepdish.py:940-960) for every
// stream; off = the candidates per position
static void phase_inject_hygiene(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &act = pl.act;
    const int n = (int)act.size();
    std::vector<int> &off = p->off;
    off.assign(n + 1, 0);
    ddk::parallel_for(n, GRAIN, [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) {
            const int z = act[i];
            StreamState &q = p->st[z];
            if (pl.inj_offsets && !pl.skp[i] && !pl.gat[i]) {
                const int a = pl.inj_offsets[z], b = pl.inj_offsets[z + 1];
                q.boxes0.assign(pl.inj_boxes + (size_t)a * 4, pl.inj_boxes + (size_t)b * 4);
                q.scores0.assign(pl.inj_scores + a, pl.inj_scores + b);
                q.cls0.assign(pl.inj_cls + a, pl.inj_cls + b);
            }
            q.ib.clear(); q.is.clear(); q.ic.clear();
            ddhost::clean_boxes(q.boxes0, q.scores0, q.cls0, p->W, p->H, q.ib, q.is, q.ic);
        }
    });
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int)p->st[act[i]].is.size();
}

// 5. deepdish.py:957: the motion test on every candidate, against its stream's own mask plane (the extra round trip)
static int phase_motion_test(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &act = pl.act;
    const int n = (int)act.size();
    std::vector<int> &off = p->off;
    if (!p->mog2 || off[n] == 0) return DD_OK;
    hipStream_t s = p->ctx->stream;
    int rc;
    const int K0 = off[n];
    const size_t in_bytes = (size_t)K0 * 5 * sizeof(int), all_bytes = in_bytes + (size_t)K0 * sizeof(int);
    if ((rc = p->h_mbox.reserve(all_bytes)) != DD_OK) return rc;
    if ((rc = p->d_mbox.reserve(all_bytes)) != DD_OK) return rc;
    int *hm = p->h_mbox.as<int>(), *dm = p->d_mbox.as<int>();
    for (int i = 0; i < n; ++i) {
        const StreamState &q = p->st[act[i]];
        for (size_t k = 0; k < q.is.size(); ++k) {
            for (int c = 0; c < 4; ++c) hm[(size_t)(off[i] + k) * 4 + c] = (int)q.ib[k * 4 + c];
            hm[(size_t)K0 * 4 + off[i] + k] = act[i];                 // the mask plane is the stream's own
        }
    }
    DD_HIP(hipMemcpyAsync(dm, hm, in_bytes, hipMemcpyHostToDevice, s));
    if ((rc = ddk::mask_box_count(s, p->d_mask.as<uint8_t>(), p->H, p->W, dm, dm + (size_t)K0 * 4, K0, dm + (size_t)K0 * 5)) != DD_OK) return rc;
    DD_HIP(hipMemcpyAsync(hm + (size_t)K0 * 5, dm + (size_t)K0 * 5, (size_t)K0 * sizeof(int), hipMemcpyDeviceToHost, s));
    DD_TIMED_WAIT(hipStreamSynchronize(s));                                                        // extra round trip
    const int *cnt = hm + (size_t)K0 * 5;
    std::vector<int> off0 = off;
    for (int i = 0; i < n; ++i) {
        StreamState &q = p->st[act[i]];
        size_t nk = 0;
        for (size_t k = 0; k < q.is.size(); ++k) {
            const int64_t w = q.ib[k * 4 + 2], h = q.ib[k * 4 + 3];
            if (!((double)cnt[off0[i] + k] >= p->ratio_of[act[i]] * (double)w * (double)h)) { p->motion_rejected++; continue; }
            for (int c = 0; c < 4; ++c) q.ib[nk * 4 + c] = q.ib[k * 4 + c];
            q.is[nk] = q.is[k]; q.ic[nk] = q.ic[k];
            ++nk;
        }
        q.ib.resize(nk * 4); q.is.resize(nk); q.ic.resize(nk);
        off[i + 1] = off[i] + (int)nk;
    }
    return DD_OK;
}

// 6. batched NMS (deepdish.py:995), one problem per position -> StreamState::keep
static int phase_nms(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &act = pl.act, &off = p->off;
    const int n = (int)act.size(), K = off[n];
    std::vector<StreamState> &st = p->st;
    if (K == 0) {
        for (int z : act) st[z].keep.clear();
        return DD_OK;
    }
    hipStream_t s = p->ctx->stream;
    int rc;
    bool small = true;
    for (int i = 0; i < n; ++i) if (off[i + 1] - off[i] > 64) small = false;
    // one --nms-max-overlap per stream: when this step's streams do not agree, their thresholds ride in the same upload, in front
    // of the offsets, for the per-problem launch
    bool thr_differ = false;
    for (int i = 1; i < n && p->nms_differ && !thr_differ; ++i) thr_differ = p->nms_of[act[i]] != p->nms_of[act[0]];
    const size_t n_thr = small && thr_differ ? (size_t)n : 0;
    const size_t in_bytes = ((size_t)K * 5 + n_thr) * sizeof(double) + (size_t)(n + 1) * sizeof(int);
    const size_t out_bytes = (size_t)(K + n) * sizeof(int);
    if ((rc = p->h_nms.reserve(in_bytes + out_bytes + 256)) != DD_OK) return rc;
    if ((rc = p->d_nms.reserve(in_bytes + out_bytes + 256 + (small ? 0 : ddk::nms_scratch_bytes(4096)))) != DD_OK) return rc;
    double *hb = p->h_nms.as<double>(), *hk = hb + (size_t)K * 4;
    for (size_t i = 0; i < n_thr; ++i) hk[K + i] = p->nms_of[act[i]];
    int *ho = reinterpret_cast<int *>(hk + K + n_thr);
    ddk::parallel_for(n, GRAIN, [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) {
            const StreamState &q = st[act[i]];
            for (size_t k = 0; k < q.ib.size(); ++k) hb[(size_t)off[i] * 4 + k] = (double)q.ib[k];   // astype(np.float)
            for (size_t k = 0; k < q.is.size(); ++k) hk[off[i] + k] = q.is[k];
        }
    });
    memcpy(ho, off.data(), (size_t)(n + 1) * sizeof(int));
    char *d = p->d_nms.as<char>();
    DD_STAGE_BEGIN(1);
    DD_HIP(hipMemcpyAsync(d, hb, in_bytes, hipMemcpyHostToDevice, s));
    const double *dbx = reinterpret_cast<const double *>(d), *dk = dbx + (size_t)K * 4;
    const int *doff = reinterpret_cast<const int *>(dk + K + n_thr);
    int *didx = reinterpret_cast<int *>(d + ((in_bytes + 63) / 64) * 64), *dnk = didx + K;
    if (n_thr) {
        if ((rc = ddk::nms_batched_small_streams(s, dbx, dk, doff, n, dk + K, 0, didx, dnk)) != DD_OK) return rc;
        p->nms_streams_launches += 1;
    } else if (small) {
        if ((rc = ddk::nms_batched_small(s, dbx, dk, doff, n, p->nms_of[act[0]], 0, didx, dnk)) != DD_OK) return rc;
    } else {
        void *scr = d + ((in_bytes + 63) / 64) * 64 + ((out_bytes + 63) / 64) * 64;
        for (int i = 0; i < n; ++i) {
            const int k = off[i + 1] - off[i];
            if ((rc = ddk::nms_ex(s, dbx + (size_t)off[i] * 4, dk + off[i], k, p->nms_of[act[i]], 0, 0, didx + off[i], dnk + i,
                                  scr, ddk::nms_scratch_bytes(4096))) != DD_OK) return rc;
        }
    }
    int *hidx = reinterpret_cast<int *>(p->h_nms.as<char>() + ((in_bytes + 63) / 64) * 64);
    DD_HIP(hipMemcpyAsync(hidx, didx, out_bytes, hipMemcpyDeviceToHost, s));
    DD_STAGE_END(1);
    DD_TIMED_WAIT(hipStreamSynchronize(s));                                                        // round trip 2
    const int *hnk = hidx + K;
    for (int i = 0; i < n; ++i) st[act[i]].keep.assign(hidx + off[i], hidx + off[i] + hnk[i]);
    return DD_OK;
}

// 7. Pair every stream's kept boxes with feature rows (doff; eoff = the rows made now), then crops + MARS for the boxes of the streams
// on a detector step (deepdish.py:1008).  A stream on a skip step runs neither (:1003-1014): it pairs with the rows of its last run.
static int phase_pair_crops_encoder(dd_pipeline *p, const StepPlan &pl) {
    const std::vector<int> &act = pl.act;
    const std::vector<uint8_t> &skp = pl.skp;
    const int n = (int)act.size();
    hipStream_t s = p->ctx->stream;
    int rc;
    std::vector<StreamState> &st = p->st;
    std::vector<int> &doff = p->doff, &eoff = p->eoff;
    // (the rows of a stream's last run: retained in the store, or -- all streams stepping together, i is the stream -- still in d_feats)
    ddhost::pair_counts(skp, [&](int i) { return (int)st[act[i]].keep.size(); },
                        [&](int i) { return p->skip_streams ? p->ret_n[act[i]] : p->foff[i + 1] - p->foff[i]; }, doff, eoff);
    const int D = doff[n], E = eoff[n];             // tracker input rows; rows the encoder makes in this step (E == D unless streams skip)
    std::vector<double> &tlwh = p->tlwh;
    tlwh.resize((size_t)D * 4);
    if (D > 0) {
        if (E > 0) {
            if ((rc = p->h_crop.reserve((size_t)E * 32)) != DD_OK) return rc;
            if ((rc = p->d_crop.reserve((size_t)E * 32)) != DD_OK) return rc;
            if ((rc = p->d_patches.reserve((size_t)E * p->enc_h * p->enc_w * 3)) != DD_OK) return rc;
            if ((rc = p->d_feats.reserve((size_t)E * 128 * sizeof(float))) != DD_OK) return rc;
        }
        int *hc0 = E > 0 ? p->h_crop.as<int>() : nullptr;
        ddk::parallel_for(n, GRAIN, [&](int i0, int i1) {
            for (int i = i0; i < i1; ++i) {
                const int z = act[i];
                StreamState &q = st[z];
                q.det_cls.clear(); q.det_conf.clear();
                int *hc = skp[i] ? nullptr : hc0;
                for (int j = 0; j < doff[i + 1] - doff[i]; ++j) {
                    const int k = q.keep[j];
                    const int64_t *b = q.ib.data() + (size_t)k * 4;
                    if (hc) {
                        int *c = hc + (size_t)(eoff[i] + j) * 8;
                        ddk::crop_box_host(b, p->enc_h, p->enc_w, p->H, p->W, c, c + 1, c + 2, c + 3);     // generate_detections.py:63-80
                        c[4] = z; c[5] = c[6] = c[7] = 0;             // the crop reads the stream's own frame slot
                    }
                    for (int c4 = 0; c4 < 4; ++c4) tlwh[(size_t)(doff[i] + j) * 4 + c4] = (double)b[c4];
                    q.det_cls.push_back(q.ic[k]);
                    q.det_conf.push_back(q.is[k]);
                }
                q.det_tlwh.assign(tlwh.begin() + (size_t)doff[i] * 4, tlwh.begin() + (size_t)doff[i + 1] * 4);
            }
        });
        if (E > 0) {
            DD_STAGE_BEGIN(2);
            DD_HIP(hipMemcpyAsync(p->d_crop.p, hc0, (size_t)E * 32, hipMemcpyHostToDevice, s));
            if ((rc = ddk::crop_resize(s, pl.frames, p->H, p->W, p->d_crop.p, E, p->enc_h, p->enc_w, p->d_patches.as<uint8_t>())) != DD_OK) return rc;
            for (int a = 0; a < E; a += p->enc_batch) {
                const int nb = std::min(p->enc_batch, E - a);
                if ((rc = dd_net_forward(p->enc, p->d_patches.as<uint8_t>() + (size_t)a * p->enc_h * p->enc_w * 3, nb, s)) != DD_OK) return rc;
                if ((rc = dd_net_read(p->enc, -1, nb, p->d_feats.as<float>() + (size_t)a * 128, 1, s)) != DD_OK) return rc;
            }
            DD_STAGE_END(2);
        }
    } else {
        for (int z : act) { StreamState &q = st[z]; q.det_cls.clear(); q.det_conf.clear(); q.det_tlwh.clear(); }
    }
    if (!p->skip_streams && !pl.dl.empty()) p->foff = doff;   // the rows d_feats now holds: what the skip steps up to the next detector step pair with
    return DD_OK;
}

// 8. The tracker's feature rows, in act order (opens stage pair 3, which phase 9 closes).  d_feats already is that input unless a stream
// on a skip step has rows to pair; then they are assembled in d_feats_skip --
//  * all streams stepping together: skip_gather_rows_k out of d_feats (n == S: such a pipeline takes no mask);
//  * per-stream counters: one feature_rows_carry launch (csrc/featrows.hip) -- fresh encoder rows for the streams of dl, retained rows
//    for the others -- which also writes the next store when an encoder run changed what is retained.
static int phase_feature_rows(dd_pipeline *p, const StepPlan &pl, const float **feats_out) {
    hipStream_t s = p->ctx->stream;
    const int S = p->S, n = (int)pl.act.size(), D = p->doff[n];
    int rc;
    bool gathered = false;
    DD_STAGE_BEGIN(3);
    if (!p->skip_streams) {
        if (pl.dl.empty() && D > 0) {
            if ((rc = p->h_gather.reserve((size_t)(2 * S + 1) * sizeof(int))) != DD_OK) return rc;
            if ((rc = p->d_gather.reserve((size_t)(2 * S + 1) * sizeof(int))) != DD_OK) return rc;
            if ((rc = p->d_feats_skip.reserve((size_t)D * 128 * sizeof(float))) != DD_OK) return rc;
            int *hg = p->h_gather.as<int>();           // the previous step's copy out of it completed at that step's last stream wait
            memcpy(hg, p->doff.data(), (size_t)(S + 1) * sizeof(int));
            memcpy(hg + S + 1, p->foff.data(), (size_t)S * sizeof(int));
            DD_HIP(hipMemcpyAsync(p->d_gather.p, hg, (size_t)(2 * S + 1) * sizeof(int), hipMemcpyHostToDevice, s));
            const int *dg = p->d_gather.as<int>();
            hipLaunchKernelGGL(skip_gather_rows_k, dim3(S), dim3(256), 0, s, p->d_feats.as<float4>(), p->d_feats_skip.as<float4>(), dg, dg + S + 1);
            DD_LAUNCH_CHECK();
            gathered = true;
        }
    } else {
        const bool refresh = !pl.dl.empty();
        std::vector<int> &tb = p->list_build;
        const ddhost::RowTable rt = ddhost::feature_row_table(S, pl.act, pl.skp, p->doff, p->eoff, p->ret_off, p->ret_n, refresh, tb,
                                                              p->ret_off_new, p->ret_n_new);
        if (!tb.empty()) {
            DevBuf &next = p->d_store[1 - p->store_cur];
            if (rt.gather && (rc = p->d_feats_skip.reserve((size_t)D * 128 * sizeof(float))) != DD_OK) return rc;
            if (refresh && (rc = next.reserve((size_t)rt.total * 128 * sizeof(float))) != DD_OK) return rc;
            const int *d_table = nullptr;
            if ((rc = stage_list(p, s, tb.data(), tb.size(), &d_table)) != DD_OK) return rc;
            if ((rc = ddk::feature_rows_carry(s, p->d_feats.as<float>(), p->d_store[p->store_cur].as<float>(), p->d_feats_skip.as<float>(),
                                              next.as<float>(), d_table, (int)(tb.size() / 8))) != DD_OK) return rc;
            p->carry_launches += 1;
        }
        if (refresh) {
            p->ret_off.swap(p->ret_off_new); p->ret_n.swap(p->ret_n_new);
            p->store_cur = 1 - p->store_cur;
            p->rows_retained = rt.total;
        }
        gathered = rt.gather;
    }
    *feats_out = D == 0 ? nullptr : gathered ? p->d_feats_skip.as<float>() : p->d_feats.as<float>();
    return DD_OK;
}

// 9. deep_sort update, phase-split so all streams share two round trips (deepdish.py:1029), with the late look-ahead between its
// first launches and its first wait
static int phase_tracker_update(dd_pipeline *p, const StepPlan &pl, const float *feats) {
    hipStream_t s = p->ctx->stream;
    const int n = (int)pl.act.size();
    dd_tracker **atrks = p->atrks.data();
    int rc;
    if ((rc = ddk::trackers_update_begin(atrks, n, p->tlwh.data(), feats, 1, p->doff.data())) != DD_OK) return rc;
    DD_STAGE_END(3);
    // Look-ahead, late form (default): the detector run of the next frames is queued HERE, behind this step's NMS / crops / encoder /
    // association kernels (enqueue_detector orders the detector stream after what the main stream holds so far).  Queued at the
    // consume point instead (DD_DET_LATE=0) it shares the GPU with the encoder from the start, the chain the host waits for takes
    // twice as long, and then the GPU idles through the host's matching / count-line tail: one worker group ran 6.3 ms per
    // 384-frame step for 5.0 ms of kernels.  Here the chain runs alone, and the detector fills the tail.
    if (p->det && pl.frames_next && p->det_late && (rc = enqueue_detector(p, pl.frames_next, pl.dl_next)) != DD_OK) return rc;
    DD_TIMED_WAIT(hipStreamSynchronize(s));                                                            // round trip 3
    DD_STAGE_BEGIN(4);
    if ((rc = ddk::trackers_update_match(atrks, n)) != DD_OK) return rc;
    DD_STAGE_END(4);
    DD_TIMED_WAIT(hipStreamSynchronize(s));                                                            // round trip 4
    DD_STAGE_BEGIN(5);
    if ((rc = ddk::trackers_update_end(atrks, n)) != DD_OK) return rc;
    DD_STAGE_END(5);
    return DD_OK;
}

// 10. the count line of every stream of the step; its frame number moves on
static void phase_count_line(dd_pipeline *p, const StepPlan &pl) {
    ddk::parallel_for((int)pl.act.size(), GRAIN, [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) { count_line_one_stream(p, pl.act[i]); p->st[pl.act[i]].seen += 1; }
    });
}

// 11. the step has succeeded: the plan's counters become the pipeline's
static void phase_commit(dd_pipeline *p, const StepPlan &pl) {
    const int n = (int)pl.act.size(), nd = (int)pl.dl.size();
    p->ev_pending = true;
    p->steps += 1;
    p->sk.rem = pl.rem_next; p->sk.has = pl.has_next;
    for (int i = 0; i < n; ++i) p->sk.last[pl.act[i]] = pl.skp[i];
    int n_skp = 0;
    for (int i = 0; i < n; ++i) n_skp += pl.skp[i];
    p->det_stream_steps += nd; p->skip_stream_steps += n_skp;      // (a gated stream-step is neither)
    if (!p->gate_thr.empty()) p->gate.commit(p->gate_thr, pl);
}

extern "C" {

// frames: device u8 [S][H][W][3] BGR.  inj_*: optional injected detections that REPLACE the detector's
// output (the detector still runs): boxes tlwh as the detector adaptor would return them (f64),
// scores, class ids, stream s owns rows [inj_offsets[s], inj_offsets[s+1]).
// frames_next (optional): the frames of the following step; their detector run is queued on the detector
// stream as soon as this step has read its own detections, and overlaps this step's NMS / encoder / tracker.
// With dd_pipeline_detector_skip_frames a skip step ignores inj_* (they stand for the detector's output, and it does not run), and
// frames_next is queued only when the next step is a detector step.
int dd_pipeline_step(dd_pipeline *p, const uint8_t *frames, const double *inj_boxes_host, const double *inj_scores_host,
                     const int *inj_cls_host, const int *inj_offsets_host) {
    return dd_pipeline_step2(p, frames, nullptr, inj_boxes_host, inj_scores_host, inj_cls_host, inj_offsets_host);
}

int dd_pipeline_step2(dd_pipeline *p, const uint8_t *frames, const uint8_t *frames_next, const double *inj_boxes_host,
                      const double *inj_scores_host, const int *inj_cls_host, const int *inj_offsets_host) {
    return dd_pipeline_step3(p, frames, nullptr, frames_next, nullptr, inj_boxes_host, inj_scores_host, inj_cls_host, inj_offsets_host);
}

// The same step for the streams with present_host[z] != 0 only (u8 [S]; NULL = every stream): for the others this step does not exist --
// no predict, no update, no count-line pass, no vote, no MOG2 update, nothing of their frame slot or injected rows read, nothing of
// their state written.  present_next_host belongs to frames_next.  The queued look-ahead run remembers its stream list: a next step
// that arrives with other frames or another list discards it and runs the detector itself, with the same result.
int dd_pipeline_step3(dd_pipeline *p, const uint8_t *frames_in, const uint8_t *present_host, const uint8_t *frames_next,
                      const uint8_t *present_next_host, const double *inj_boxes_host, const double *inj_scores_host,
                      const int *inj_cls_host, const int *inj_offsets_host) {
    DD_REQUIRE(p && frames_in, DD_E_ARG, "dd_pipeline_step: NULL argument");
    DD_REQUIRE(frames_next != frames_in, DD_E_ARG,
               "dd_pipeline_step2: frames_next must be a different buffer from frames (its detector run is queued while "
               "this step still reads frames, and the next step consumes it by address)");
    DD_REQUIRE(!present_next_host || frames_next, DD_E_ARG, "dd_pipeline_step3: present_next without frames_next");
    // all streams of that form step together: it keeps their rows in d_feats by stream, not in a store
    DD_REQUIRE(!(present_host || present_next_host) || !p->skip_lockstep, DD_E_STATE,
               "dd_pipeline_step3: a presence mask on a pipeline with object_detector_skip_frames set (dd_pipeline_detector_skip_frames)");
    int rc;
    if ((rc = phase_plan(p, p->plan, frames_in, present_host, frames_next, present_next_host, inj_boxes_host, inj_scores_host, inj_cls_host,
                         inj_offsets_host)) != DD_OK) return rc;
    StepPlan &pl = p->plan;
    DD_DEVICE(p->ctx);
    const int n = (int)pl.act.size();
    p->masked_steps += present_host != nullptr;
    p->streams_stepped += n;
    if (n == 0) {                                  // a legal step: nothing is launched and no state changes (a queued look-ahead run was
        p->det_pending = nullptr;                  // announced for other streams than arrived: dropped)
        p->steps += 1;
        return DD_OK;
    }
    p->atrks.resize(n);
    for (int i = 0; i < n; ++i) p->atrks[i] = p->trks[pl.act[i]];
    if ((rc = flush_stage_events(p)) != DD_OK) return rc;
    const double t0 = now_s();
    p->step_wait = 0;
    if ((rc = phase_predict_mog2(p, pl)) != DD_OK) return rc;
    if ((rc = phase_motion_gate(p, pl)) != DD_OK) return rc;
    if ((rc = phase_consume_detector(p, pl)) != DD_OK) return rc;
    if (inj_offsets_host)
        DD_REQUIRE(inj_boxes_host && inj_scores_host && inj_cls_host, DD_E_ARG, "dd_pipeline_step: injected arrays missing");
    const double t1 = now_s();
    phase_inject_hygiene(p, pl);
    if ((rc = phase_motion_test(p, pl)) != DD_OK) return rc;
    if ((rc = phase_nms(p, pl)) != DD_OK) return rc;
    const double t2 = now_s();
    if ((rc = phase_pair_crops_encoder(p, pl)) != DD_OK) return rc;
    const double t3 = now_s();
    const float *feats = nullptr;
    if ((rc = phase_feature_rows(p, pl, &feats)) != DD_OK) return rc;
    if ((rc = phase_tracker_update(p, pl, feats)) != DD_OK) return rc;
    phase_count_line(p, pl);
    const double t4 = now_s();
    p->t_det += t1 - t0; p->t_nms += t2 - t1; p->t_enc += t3 - t2; p->t_trk += t4 - t3;
    p->g_wall += 1e3 * (t4 - t0); p->g_host += 1e3 * ((t4 - t0) - p->step_wait);
    phase_commit(p, pl);
    return DD_OK;
}

}  // extern "C"

// ---------------- stream snapshots (include/deepdish_hip.h; the blob: csrc/snapshot_fmt.h; the gallery kernels: csrc/snapshot.hip)
namespace {

// What a stream's entry records of its parameters, and what restore compares the destination's with
ddsnap::Params stream_params(const dd_pipeline *p, int z) {
    ddsnap::Params q;
    ddk::TrackerPoolView tv;
    ddk::tracker_pool_view(p->trks[z], &tv);
    q.H = p->H; q.W = p->W; q.feat_len = 128; q.metric = tv.metric; q.nn_budget = tv.budget;
    q.det_kind = p->det_kind; q.max_det = p->max_det; q.n_labels = (int32_t)p->labels.size(); q.label_offset = p->label_offset;
    uint64_t h = ddsnap::fnv1a(nullptr, 0);
    for (const std::string &l : p->labels) { h = ddsnap::fnv1a(l.data(), l.size(), h); h = ddsnap::fnv1a("\n", 1, h); }
    q.labels_hash = h;
    memcpy(q.line, p->lines.data() + (size_t)z * 4, sizeof q.line);
    q.max_age = tv.max_age; q.n_init = tv.n_init; q.max_cos = tv.max_cos; q.max_iou = tv.max_iou; q.nms = p->nms_of[z];
    if (p->mog2) {
        q.mog_on = 1; q.ratio = p->ratio_of[z]; q.masking = p->bg_masking;
        ddk::mog2_stream_planes(p->mog2, z, nullptr, nullptr, nullptr, nullptr, &q.mog_history, &q.mog_var_thr, &q.mog_shadows);
    }
    q.skip_form = p->skip_streams; q.skip_n = p->sk.n[z]; q.skip_phase = p->sk.phase[z];
    for (size_t i = 0; i < p->wanted.size(); ++i) if (p->wanted_of[(size_t)z * p->wanted.size() + i]) q.wanted.push_back(p->wanted[i]);
    return q;
}

// the first parameter of the source stream (a) that differs from the destination's (b); NULL: none.  Floats by bit pattern.
const char *params_differ(const ddsnap::Params &a, const ddsnap::Params &b) {
    const auto bits = [](const void *x, const void *y, size_t n) { return memcmp(x, y, n) != 0; };
    if (a.H != b.H) return "H";
    if (a.W != b.W) return "W";
    if (a.feat_len != b.feat_len) return "feature length";
    if (a.metric != b.metric) return "metric";
    if (a.nn_budget != b.nn_budget) return "nn_budget";
    if (a.det_kind != b.det_kind) return "detector kind";
    if (a.max_det != b.max_det) return "max_det";
    if (a.labels_hash != b.labels_hash || a.n_labels != b.n_labels || a.label_offset != b.label_offset) return "labels";
    {
        std::vector<std::string> x = a.wanted, y = b.wanted;
        std::sort(x.begin(), x.end()); std::sort(y.begin(), y.end());
        if (x != y) return "wanted labels";
    }
    if (bits(a.line, b.line, sizeof a.line)) return "line";
    if (a.max_age != b.max_age) return "max_age";
    if (a.n_init != b.n_init) return "n_init";
    if (bits(&a.max_cos, &b.max_cos, 8)) return "max_cosine_distance";
    if (bits(&a.max_iou, &b.max_iou, 8)) return "max_iou_distance";
    if (bits(&a.nms, &b.nms, 8)) return "nms_max_overlap";
    if (a.mog_on != b.mog_on || bits(&a.ratio, &b.ratio, 8)) return "background_subtraction_ratio";
    if (a.masking != b.masking) return "background_masking";
    if (a.mog_history != b.mog_history) return "MOG2 history";
    if (bits(&a.mog_var_thr, &b.mog_var_thr, 4)) return "MOG2 varThreshold";
    if (a.mog_shadows != b.mog_shadows) return "MOG2 detect_shadows";
    if (a.skip_form != b.skip_form || a.skip_n != b.skip_n) return "object_detector_skip_frames";
    if (a.skip_phase != b.skip_phase) return "object_detector_skip_phase";
    return nullptr;
}

int snapshot_streams(const dd_pipeline *p, const char *name, const int *streams_host, int n, std::vector<int> &zs) {
    DD_REQUIRE(p && n >= 0 && n <= p->S, DD_E_ARG, "%s: bad argument (n = %d)", name, n);
    zs.resize(n);
    std::vector<uint8_t> listed(p->S, 0);
    for (int i = 0; i < n; ++i) {
        const int z = streams_host ? streams_host[i] : i;
        DD_REQUIRE(z >= 0 && z < p->S, DD_E_ARG, "%s: stream %d of %d", name, z, p->S);
        DD_REQUIRE(!listed[z], DD_E_ARG, "%s: stream %d is listed twice", name, z);
        listed[z] = 1;
        zs[i] = z;
    }
    DD_REQUIRE(!p->skip_lockstep, DD_E_STATE, "%s: the pipeline has the pipeline-wide object_detector_skip_frames counter (dd_pipeline_detector_skip_frames): "
               "one counter for all streams cannot continue one stream's cycle; dd_pipeline_detector_skip_streams (a sequence of N) has one per stream", name);
    ddk::TrackerPoolView tv;
    ddk::tracker_pool_view(p->trks[0], &tv);
    DD_REQUIRE(!tv.upd_inflight, DD_E_STATE, "%s: an update of the tracker group is in flight", name);
    return DD_OK;
}

// The host half of a snapshot: every listed stream's entry but for means, covariances and the bulk sections, and the track views
// (slots and chunk lists) the gather table is built from.
int snapshot_collect(dd_pipeline *p, const std::vector<int> &zs, int background, std::vector<ddsnap::Entry> &es, std::vector<std::vector<ddk::TrackView>> &views) {
    es.assign(zs.size(), ddsnap::Entry());
    views.assign(zs.size(), std::vector<ddk::TrackView>());
    std::vector<ddk::TrackView> dead;
    for (size_t i = 0; i < zs.size(); ++i) {
        const int z = zs[i];
        const StreamState &st = p->st[z];
        ddsnap::Entry &e = es[i];
        e.par = stream_params(p, z);
        for (const std::string &w : e.par.wanted) {
            const int wi = wanted_index(p, z, w);
            e.counts.insert(e.counts.end(), st.counts.begin() + (size_t)wi * 4, st.counts.begin() + (size_t)wi * 4 + 4);
        }
        e.seen = st.seen; e.rem = p->sk.rem[z]; e.has = p->sk.has[z]; e.last = p->sk.last[z];
        e.det_cls.assign(st.det_cls.begin(), st.det_cls.end()); e.det_conf = st.det_conf; e.det_tlwh = st.det_tlwh;
        e.boxes0 = st.boxes0; e.scores0 = st.scores0; e.cls0.assign(st.cls0.begin(), st.cls0.end());
        int rc;
        if ((rc = ddk::tracker_export(st.trk, &e.next_id, views[i], dead)) != DD_OK) return rc;
        e.n_live = (int32_t)views[i].size(); e.n_dead = (int32_t)dead.size();
        views[i].insert(views[i].end(), dead.begin(), dead.end());
        e.tracks.resize(views[i].size());
        for (size_t k = 0; k < views[i].size(); ++k) {
            const ddk::TrackView &v = views[i][k];
            ddsnap::Track &t = e.tracks[k];
            t.id = v.id; t.state = v.state; t.tsu = v.tsu; t.hits = v.hits; t.age = v.age; t.last_det = v.last_det; t.slot_total = v.slot_total; t.n_rows = v.n_rows;
            e.gallery_rows += (uint64_t)v.n_rows;
        }
        for (const auto &kv : st.db) {
            if (kv.second.empty()) continue;
            ddsnap::Path q;
            q.id = kv.first;
            for (const auto &pt : kv.second) { q.xy.push_back(pt.first); q.xy.push_back(pt.second); }
            e.paths.push_back(std::move(q));
        }
        for (const auto &kv : st.votes) {
            if (kv.second.cls.empty()) continue;
            ddsnap::Vote v;
            v.id = kv.first; v.cls.assign(kv.second.cls.begin(), kv.second.cls.end()); v.cnt.assign(kv.second.cnt.begin(), kv.second.cnt.end()); v.sum = kv.second.sum;
            e.votes.push_back(std::move(v));
        }
        e.n_ret = p->skip_streams ? p->ret_n[z] : 0;
        e.has_bg = background && p->mog2;
        if (e.has_bg) {
            long long *nf = nullptr;
            ddk::mog2_stream_planes(p->mog2, z, nullptr, nullptr, nullptr, &nf, nullptr, nullptr, nullptr);
            e.nframes = *nf;
        }
    }
    return DD_OK;
}

}  // namespace

extern "C" {

int dd_pipeline_snapshot_bytes(dd_pipeline *p, const int *streams_host, int n, int background, int64_t *bytes_host) {
    DD_REQUIRE(p && bytes_host, DD_E_ARG, "dd_pipeline_snapshot_bytes: NULL argument");
    std::vector<int> zs;
    int rc;
    if ((rc = snapshot_streams(p, "dd_pipeline_snapshot_bytes", streams_host, n, zs)) != DD_OK) return rc;
    std::vector<ddsnap::Entry> es;
    std::vector<std::vector<ddk::TrackView>> views;
    if ((rc = snapshot_collect(p, zs, background, es, views)) != DD_OK) return rc;
    uint64_t total = ddsnap::header_bytes((uint32_t)n);
    for (const ddsnap::Entry &e : es) total += ddsnap::write_entry(e, nullptr);
    *bytes_host = (int64_t)total;
    return DD_OK;
}

int dd_pipeline_snapshot(dd_pipeline *p, const int *streams_host, int n, int background, uint8_t *blob_host, int64_t cap, int64_t *bytes_host) {
    DD_REQUIRE(p && blob_host && bytes_host, DD_E_ARG, "dd_pipeline_snapshot: NULL argument");
    std::vector<int> zs;
    int rc;
    if ((rc = snapshot_streams(p, "dd_pipeline_snapshot", streams_host, n, zs)) != DD_OK) return rc;
    std::vector<ddsnap::Entry> es;
    std::vector<std::vector<ddk::TrackView>> views;
    if ((rc = snapshot_collect(p, zs, background, es, views)) != DD_OK) return rc;
    std::vector<uint64_t> sizes(n);
    uint64_t total = ddsnap::header_bytes((uint32_t)n);
    for (int i = 0; i < n; ++i) { sizes[i] = ddsnap::write_entry(es[i], nullptr); total += sizes[i]; }
    DD_REQUIRE((uint64_t)cap >= total, DD_E_CAPACITY, "dd_pipeline_snapshot: %llu bytes, room for %lld", (unsigned long long)total, (long long)cap);
    DD_DEVICE(p->ctx);
    hipStream_t s = p->ctx->stream;
    DD_HIP(hipStreamSynchronize(s));                              // between steps: the main stream is idle from here on, the detector stream is not touched
    // ---- the gather table: one entry per track {offset of its chunk list, rows, first dense row, slot}; dense = [rows][36 units per track]
    std::vector<int> table, chunks;
    uint64_t rows = 0;
    for (int i = 0; i < n; ++i)
        for (const ddk::TrackView &v : views[i]) {
            const int e[4] = {(int)chunks.size(), v.n_rows, (int)rows, v.slot};
            table.insert(table.end(), e, e + 4);
            chunks.insert(chunks.end(), v.chunks, v.chunks + v.n_chunks);
            rows += (uint64_t)v.n_rows;
        }
    DD_REQUIRE(rows < (1ull << 31), DD_E_CAPACITY, "dd_pipeline_snapshot: %llu gallery rows in one snapshot; list fewer streams", (unsigned long long)rows);
    const size_t nt = table.size() / 4;
    DevBuf d_dense, d_tab;
    PinBuf h_tab;
    const auto done = [&](int r) { d_dense.release(); d_tab.release(); h_tab.release(); return r; };
    if (nt > 0) {
        ddk::TrackerPoolView tv;
        ddk::tracker_pool_view(p->trks[0], &tv);
        const size_t b_tab = table.size() * sizeof(int), b_ch = chunks.size() * sizeof(int), b_rows = (size_t)rows * 512, b_state = nt * 576;
        if ((rc = d_dense.reserve(b_rows + b_state)) != DD_OK || (rc = d_tab.reserve(b_tab + b_ch)) != DD_OK ||
            (rc = h_tab.reserve(std::max(b_tab + b_ch, b_state))) != DD_OK) return done(rc);
        memcpy(h_tab.p, table.data(), b_tab);
        if (b_ch) memcpy(h_tab.as<char>() + b_tab, chunks.data(), b_ch);
        hipError_t he = hipMemcpyAsync(d_tab.p, h_tab.p, b_tab + b_ch, hipMemcpyHostToDevice, s);
        if (he != hipSuccess) { dd_set_error("dd_pipeline_snapshot: table upload -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
        double *d_state = reinterpret_cast<double *>(d_dense.as<char>() + b_rows);
        if ((rc = ddk::chunk_rows_gather(s, tv.d_arenas, tv.arena_shift, reinterpret_cast<const int *>(d_tab.as<char>() + b_tab), d_tab.as<int>(), (int)nt,
                                         d_dense.as<float>(), tv.d_means, tv.d_covs, d_state)) != DD_OK) return done(rc);
        he = hipStreamSynchronize(s);                             // (the table has been read: h_tab now takes the state block)
        if (he == hipSuccess) he = hipMemcpyAsync(h_tab.p, d_state, b_state, hipMemcpyDeviceToHost, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        if (he != hipSuccess) { dd_set_error("dd_pipeline_snapshot: gather -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
        const double *hs = h_tab.as<double>();
        size_t k = 0;
        for (int i = 0; i < n; ++i)
            for (ddsnap::Track &t : es[i].tracks) { memcpy(t.mean, hs + k * 72, sizeof t.mean); memcpy(t.cov, hs + k * 72 + 8, sizeof t.cov); ++k; }
    }
    // ---- the blob: header, then per entry its host part; the bulk sections come straight from the device
    ddsnap::write_header(blob_host, sizes);
    uint64_t at = ddsnap::header_bytes((uint32_t)n), row0 = 0;
    const size_t hw = (size_t)p->H * p->W;
    hipError_t he = hipSuccess;
    for (int i = 0; i < n && he == hipSuccess; ++i) {
        uint64_t off[3] = {0, 0, 0};
        ddsnap::write_entry(es[i], blob_host + at, off);
        const ddsnap::Entry &e = es[i];
        const int z = zs[i];
        if (e.gallery_rows) he = hipMemcpyAsync(blob_host + at + off[0], d_dense.as<char>() + row0 * 512, e.gallery_rows * 512, hipMemcpyDeviceToHost, s);
        row0 += e.gallery_rows;
        if (e.n_ret && he == hipSuccess)
            he = hipMemcpyAsync(blob_host + at + off[1], p->d_store[p->store_cur].as<char>() + (size_t)p->ret_off[z] * 512, (size_t)e.n_ret * 512, hipMemcpyDeviceToHost, s);
        if (e.has_bg) {
            void *rec = nullptr, *m2 = nullptr, *nm = nullptr;
            ddk::mog2_stream_planes(p->mog2, z, &rec, &m2, &nm, nullptr, nullptr, nullptr, nullptr);
            uint8_t *o = blob_host + at + off[2];
            const void *src[4] = {rec, m2, nm, p->d_mask.as<uint8_t>() + (size_t)z * hw};
            const size_t len[4] = {hw * 80, hw * 20, hw, hw};
            for (int k = 0; k < 4 && he == hipSuccess; ++k) { he = hipMemcpyAsync(o, src[k], len[k], hipMemcpyDeviceToHost, s); o += len[k]; }
        }
        at += sizes[i];
    }
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) { dd_set_error("dd_pipeline_snapshot: copy to the host -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
    *bytes_host = (int64_t)total;
    return done(DD_OK);
}

int dd_snapshot_info(const uint8_t *blob_host, int64_t n_bytes, int *n_entries_host, int64_t *info_host, int cap_entries) {
    DD_REQUIRE(blob_host && n_bytes >= 0 && n_entries_host, DD_E_ARG, "dd_snapshot_info: bad argument");
    std::vector<ddsnap::Entry> es;
    std::vector<std::pair<uint64_t, uint64_t>> table;
    std::string err;
    DD_REQUIRE(ddsnap::parse_blob(blob_host, (uint64_t)n_bytes, es, table, err), DD_E_ARG, "dd_snapshot_info: the blob is refused: %s", err.c_str());
    *n_entries_host = (int)es.size();
    if (!info_host) return DD_OK;
    DD_REQUIRE(cap_entries >= (int)es.size(), DD_E_ARG, "dd_snapshot_info: %zu entries, room for %d", es.size(), cap_entries);
    for (size_t i = 0; i < es.size(); ++i) {
        int64_t *o = info_host + i * 8;
        o[0] = es[i].seen; o[1] = es[i].n_live + es[i].n_dead; o[2] = es[i].next_id; o[3] = (int64_t)es[i].gallery_rows; o[4] = es[i].has_bg;
        o[5] = (int64_t)table[i].second; o[6] = (int64_t)table[i].first; o[7] = 0;
    }
    return DD_OK;
}

int dd_pipeline_restore(dd_pipeline *p, const uint8_t *blob_host, int64_t n_bytes, const int *streams_host, int n) {
    DD_REQUIRE(p && blob_host && n_bytes >= 0, DD_E_ARG, "dd_pipeline_restore: bad argument");
    // ---- everything that can be refused, before anything changes
    std::vector<ddsnap::Entry> es;
    std::vector<std::pair<uint64_t, uint64_t>> table;
    std::string err;
    DD_REQUIRE(ddsnap::parse_blob(blob_host, (uint64_t)n_bytes, es, table, err), DD_E_ARG, "dd_pipeline_restore: the blob is refused: %s", err.c_str());
    DD_REQUIRE(n == (int)es.size(), DD_E_ARG, "dd_pipeline_restore: %d streams for a snapshot of %zu entries", n, es.size());
    std::vector<int> zs;
    int rc;
    if ((rc = snapshot_streams(p, "dd_pipeline_restore", streams_host, n, zs)) != DD_OK) return rc;
    size_t need_chunks = 0, nt = 0, ret_add = 0;
    uint64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        const ddsnap::Entry &e = es[i];
        const ddsnap::Params dst = stream_params(p, zs[i]);
        const char *what = params_differ(e.par, dst);
        DD_REQUIRE(!what, DD_E_ARG, "dd_pipeline_restore: entry %d -> stream %d: %s differs between the snapshot's stream and the destination "
                   "(parameters are checked, not carried)", i, zs[i], what);
        DD_REQUIRE(!e.has_bg || p->mog2, DD_E_ARG, "dd_pipeline_restore: entry %d carries a background model and subtraction is off", i);
        ddk::TrackerPoolView tv;
        ddk::tracker_pool_view(p->trks[zs[i]], &tv);
        DD_REQUIRE(e.n_live + e.n_dead <= tv.tcap, DD_E_CAPACITY, "dd_pipeline_restore: entry %d has %d tracks, track_capacity of stream %d is %d", i,
                   e.n_live + e.n_dead, zs[i], tv.tcap);
        for (const ddsnap::Track &t : e.tracks) need_chunks += (size_t)((t.n_rows + 31) / 32);
        nt += e.tracks.size();
        rows += e.gallery_rows;
        ret_add += (size_t)e.n_ret;
    }
    DD_REQUIRE(rows < (1ull << 31), DD_E_CAPACITY, "dd_pipeline_restore: %llu gallery rows in one call; restore fewer entries at a time", (unsigned long long)rows);
    if (n == 0) return DD_OK;
    DD_DEVICE(p->ctx);
    hipStream_t s = p->ctx->stream;
    // ---- reserve: gallery chunks, staging, the retained-rows store -- a failure here gives back what it took
    if ((rc = ddk::tracker_pool_reserve_chunks(p->trks[0], need_chunks)) != DD_OK) return rc;
    DevBuf d_dense, d_tab, d_store_new;
    PinBuf h_tab;
    const auto done = [&](int r) { d_dense.release(); d_tab.release(); h_tab.release(); d_store_new.release(); return r; };
    const size_t b_tab = nt * 4 * sizeof(int), b_ch = need_chunks * sizeof(int), b_rows = (size_t)rows * 512, b_state = nt * 576;
    const size_t o_state = (b_tab + b_ch + 15) / 16 * 16;
    if (nt > 0 && ((rc = d_dense.reserve(b_rows + b_state)) != DD_OK || (rc = d_tab.reserve(b_tab + b_ch)) != DD_OK ||
                   (rc = h_tab.reserve(o_state + b_state)) != DD_OK)) return done(rc);
    std::vector<uint8_t> listed(p->S, 0);
    for (int z : zs) listed[z] = 1;
    int ret_end = 0;                                             // rows of the current store the other streams use
    if (p->skip_streams) for (int z = 0; z < p->S; ++z) if (!listed[z] && p->ret_n[z] > 0) ret_end = std::max(ret_end, p->ret_off[z] + p->ret_n[z]);
    const bool store_grows = ret_add > 0 && ((size_t)ret_end + ret_add) * 512 > p->d_store[p->store_cur].cap;
    if (store_grows && (rc = d_store_new.reserve(((size_t)ret_end + ret_add) * 512)) != DD_OK) return done(rc);
    DD_HIP(hipStreamSynchronize(s));
    // ---- commit: as dd_pipeline_reset_streams, then the state
    hipError_t he = hipSuccess;
    if (store_grows) {
        if (ret_end) he = hipMemcpyAsync(d_store_new.p, p->d_store[p->store_cur].p, (size_t)ret_end * 512, hipMemcpyDeviceToDevice, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        if (he != hipSuccess) { dd_set_error("dd_pipeline_restore: store copy -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
        std::swap(p->d_store[p->store_cur], d_store_new);         // (the old buffer is released with d_store_new)
    }
    if (p->mog2) {
        if ((rc = ddk::mog2_reset_streams(p->mog2, s, zs.data(), n)) != DD_OK) return done(rc);
        const size_t hw = (size_t)p->H * p->W;
        for (int z : zs) if (hipMemsetAsync(p->d_mask.as<uint8_t>() + (size_t)z * hw, 0, hw, s) != hipSuccess) { dd_set_error("dd_pipeline_restore: memset failed"); return done(DD_E_HIP); }
    }
    std::vector<int> slots, chunks;
    std::vector<ddk::TrackLoad> loads;
    for (int i = 0; i < n; ++i) {
        const ddsnap::Entry &e = es[i];
        loads.clear();
        for (const ddsnap::Track &t : e.tracks) loads.push_back({t.id, t.state, t.tsu, t.hits, t.age, t.last_det, t.slot_total, t.n_rows, t.mean});
        if ((rc = ddk::tracker_import(p->trks[zs[i]], e.next_id, loads.data(), e.n_live, e.n_dead, slots, chunks)) != DD_OK) return done(rc);
    }
    if (nt > 0) {
        int *ht = h_tab.as<int>(), *hc = ht + nt * 4;
        double *hs = reinterpret_cast<double *>(h_tab.as<char>() + o_state);
        size_t k = 0, c0 = 0, r0 = 0;
        for (int i = 0; i < n; ++i)
            for (const ddsnap::Track &t : es[i].tracks) {
                int *e4 = ht + k * 4;
                e4[0] = (int)c0; e4[1] = t.n_rows; e4[2] = (int)r0; e4[3] = slots[k];
                memcpy(hs + k * 72, t.mean, sizeof t.mean); memcpy(hs + k * 72 + 8, t.cov, sizeof t.cov);
                c0 += (size_t)((t.n_rows + 31) / 32); r0 += (size_t)t.n_rows; ++k;
            }
        if (b_ch) memcpy(hc, chunks.data(), b_ch);
        double *d_state = reinterpret_cast<double *>(d_dense.as<char>() + b_rows);
        he = hipMemcpyAsync(d_tab.p, ht, b_tab + b_ch, hipMemcpyHostToDevice, s);
        if (he == hipSuccess) he = hipMemcpyAsync(d_state, hs, b_state, hipMemcpyHostToDevice, s);
        size_t at_row = 0;
        for (int i = 0; i < n && he == hipSuccess; ++i) {
            if (es[i].gallery_rows) he = hipMemcpyAsync(d_dense.as<char>() + at_row * 512, es[i].gallery, es[i].gallery_rows * 512, hipMemcpyHostToDevice, s);
            at_row += es[i].gallery_rows;
        }
        if (he != hipSuccess) { dd_set_error("dd_pipeline_restore: upload -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
        ddk::TrackerPoolView tv;
        ddk::tracker_pool_view(p->trks[0], &tv);
        if ((rc = ddk::chunk_rows_scatter(s, tv.d_arenas, tv.arena_shift, reinterpret_cast<const int *>(d_tab.as<char>() + b_tab), d_tab.as<int>(), (int)nt,
                                          d_dense.as<float>(), tv.d_means, tv.d_covs, d_state)) != DD_OK) return done(rc);
    }
    if ((rc = ddk::tracker_gallery_flush(p->trks[0], s)) != DD_OK) return done(rc);
    const size_t hw = (size_t)p->H * p->W;
    int ret_at = ret_end;
    for (int i = 0; i < n; ++i) {
        const ddsnap::Entry &e = es[i];
        const int z = zs[i];
        StreamState &st = p->st[z];
        st.restart(p->wanted.size());
        for (size_t k = 0; k < e.par.wanted.size(); ++k) {
            const int wi = wanted_index(p, z, e.par.wanted[k]);
            for (int c = 0; c < 4; ++c) st.counts[(size_t)wi * 4 + c] = e.counts[k * 4 + c];
        }
        st.seen = e.seen;
        st.det_cls.assign(e.det_cls.begin(), e.det_cls.end()); st.det_conf = e.det_conf; st.det_tlwh = e.det_tlwh;
        st.boxes0 = e.boxes0; st.scores0 = e.scores0; st.cls0.assign(e.cls0.begin(), e.cls0.end());
        for (const ddsnap::Path &q : e.paths) {
            auto &pts = st.db[q.id];
            for (size_t k = 0; k + 1 < q.xy.size(); k += 2) pts.emplace_back(q.xy[k], q.xy[k + 1]);
        }
        for (const ddsnap::Vote &v : e.votes) {
            Votes &w = st.votes[v.id];
            w.cls.assign(v.cls.begin(), v.cls.end()); w.cnt.assign(v.cnt.begin(), v.cnt.end()); w.sum = v.sum;
        }
        p->sk.rem[z] = e.rem; p->sk.has[z] = e.has; p->sk.last[z] = e.last;
        if (p->skip_streams) {
            p->rows_retained += e.n_ret - p->ret_n[z];
            p->ret_off[z] = e.n_ret ? ret_at : 0; p->ret_n[z] = e.n_ret;
            if (e.n_ret && he == hipSuccess)
                he = hipMemcpyAsync(p->d_store[p->store_cur].as<char>() + (size_t)ret_at * 512, e.ret_rows, (size_t)e.n_ret * 512, hipMemcpyHostToDevice, s);
            ret_at += e.n_ret;
        }
        if (e.has_bg) {
            void *rec = nullptr, *m2 = nullptr, *nm = nullptr;
            long long *nf = nullptr;
            ddk::mog2_stream_planes(p->mog2, z, &rec, &m2, &nm, &nf, nullptr, nullptr, nullptr);
            *nf = e.nframes;
            const uint8_t *o = e.bg;
            void *dst[4] = {rec, m2, nm, p->d_mask.as<uint8_t>() + (size_t)z * hw};
            const size_t len[4] = {hw * 80, hw * 20, hw, hw};
            for (int k = 0; k < 4 && he == hipSuccess; ++k) { he = hipMemcpyAsync(dst[k], o, len[k], hipMemcpyHostToDevice, s); o += len[k]; }
        }
    }
    p->det_pending = nullptr;                                     // as after a reset: the next step runs the detector itself
    if (he == hipSuccess) he = hipStreamSynchronize(s);           // the blob and the staging buffers are the caller's / released below
    if (he != hipSuccess) { dd_set_error("dd_pipeline_restore: copy to the device -> %s", hipGetErrorString(he)); return done(DD_E_HIP); }
    return done(DD_OK);
}

}  // extern "C"
