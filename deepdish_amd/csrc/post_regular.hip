// TFLite_Detection_PostProcess with use_regular_nms = true (the custom op inside the reference's SSD .tflite graph, invoked at
// tools/ssd_mobilenet.py:103, outputs read at :107-109; kernels/detection_postprocess.cc NonMaxSuppressionMultiClassRegularHelper
// over NonMaxSuppressionSingleClassHelper): per-class greedy NMS (candidates score >= nms_score_threshold, at most
// detections_per_class survivors per class, IoU > nms_iou_threshold suppresses inside the class only), the classes' survivors
// merged by score (stable: earlier class first, inside a class the keep order), the first max_detections rows.  TensorFlow Lite
// is a third-party dependency absent from this image; the op is restated from its published behaviour -- parity unpinned.
//
// The class-by-class form equals ONE greedy selection over all (anchor, class) pairs ordered by (score descending, class
// ascending, anchor ascending): take the best live pair as the next row, kill the live pairs of ITS class that it suppresses,
// kill the class once it has detections_per_class rows, stop at max_detections rows (tests/regular_nms_ref.py checks the two
// forms against each other).  So a round selects one row and touches one class column:
//   first pass  the A x C scores are read once (a wave per row, a lane per column: coalesced); every class gets a head = its
//               best candidate as a composite key (order-preserving score bits << 32 | ~anchor: the maximum is the highest
//               score, the LOWER anchor on ties).  Decoded boxes are staged in LDS.
//   a round     every wave finds the best head (lower class on ties) on its own; thread 0 writes the row; the threads sweep
//               that class's column -- one score and one IoU against the pivot (an LDS broadcast) per live anchor --, record
//               the kills in the class's bit row (a class gets a bit row when it is first visited: at most max_detections
//               rows of ceil(A / 64) words; a wave owns the words of its own anchors, so the rows need no synchronisation)
//               and reduce the column's next head.  One barrier per round: the waves' partial heads alternate between two
//               LDS rows and every thread folds them itself at the top of the next round.
// Three front ends feed the one kernel body through a loader type: decoded boxes + a ready score matrix, the f32 head matrix
// (box decode and sigmoid are csrc/ssd_dev.h's expressions: a row's box has the bits dd_ssd_decode gives that anchor; the
// sigmoid is applied to EVERY class logit before comparing -- the op sees scores, and distinct logits can round to one
// score), the uint8 head tensors (class bytes through the model's 256-entry logistic table, then scale * (q - zero point):
// what q_ssd_decode_k in csrc/netsq.hip reads).  Same f32 IoU expressions as `suppresses` mode 2 in csrc/nms.hip.
#include "common.h"
#include "ssd_dev.h"

namespace {

typedef unsigned long long u64;

constexpr int RN_THREADS = 1024, RN_WAVES = RN_THREADS / 64;
constexpr int RN_MAX_ANCHORS = 4096, RN_MAX_DET = 64;
constexpr int RN_MAX_COLS = 256;              // score columns a lane quartet covers (background column included where the loader has one)
constexpr int RN_ROWS = 4;                    // rows of the first pass in flight per wave

__device__ __forceinline__ unsigned score_bits(float s) {                   // order-preserving; never 0 for a non-NaN score
    const unsigned b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float bits_score(unsigned m) { return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m); }

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// ---- loaders.  FIRST = leading columns that are no class (the background column); column `col` is class col - FIRST.
// load_row / row_score: the first pass's view of row a -- lane l gets the four columns col4(k, l), all loads of a row in one go.

struct DecodedLoad {                          // boxes [batch][A][4], scores [batch][A][ld] (the pointer already stands on class 0's column)
    const float *boxes, *scores;
    int ld;
    static constexpr int FIRST = 0;
    struct Row { float v[4]; };
    __device__ __forceinline__ static int col4(int k, int lane) { return k * 64 + lane; }
    __device__ __forceinline__ void image(size_t z, int A) { boxes += z * A * 4; scores += z * A * ld; }
    __device__ __forceinline__ void table(float *, int) const {}
    __device__ __forceinline__ float4 box(int a) const { return *reinterpret_cast<const float4 *>(boxes + (size_t)a * 4); }
    __device__ __forceinline__ float score(int a, int col, const float *) const { return scores[(size_t)a * ld + col]; }
    __device__ __forceinline__ Row load_row(int a, int lane, int ncols) const {
        Row r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = col4(k, lane) < ncols ? scores[(size_t)a * ld + col4(k, lane)] : 0.f;
        return r;
    }
    __device__ __forceinline__ float row_score(const Row &r, int k, const float *) const { return r.v[k]; }
};

struct RawLoad {                              // f32 head matrix [batch][A][4 + n_classes]: four box encodings, background logit, class logits
    const float *raw, *anchors;
    int ld;
    static constexpr int FIRST = 1;
    struct Row { float v[4]; };
    __device__ __forceinline__ static int col4(int k, int lane) { return k * 64 + lane; }
    __device__ __forceinline__ void image(size_t z, int A) { raw += z * A * ld; }
    __device__ __forceinline__ void table(float *, int) const {}
    __device__ __forceinline__ float4 box(int a) const {
        const float *r = raw + (size_t)a * ld;
        const float rr[4] = {r[0], r[1], r[2], r[3]};
        const float an[4] = {anchors[a * 4 + 0], anchors[a * 4 + 1], anchors[a * 4 + 2], anchors[a * 4 + 3]};
        float bx[4];
        (void)ssddev::decode_anchor(rr, an, 0.f, bx);
        return float4{bx[0], bx[1], bx[2], bx[3]};
    }
    __device__ __forceinline__ float score(int a, int col, const float *) const { return ssddev::sigmoid(raw[(size_t)a * ld + 4 + col]); }
    __device__ __forceinline__ Row load_row(int a, int lane, int ncols) const {
        Row r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = col4(k, lane) < ncols ? raw[(size_t)a * ld + 4 + col4(k, lane)] : 0.f;
        return r;
    }
    __device__ __forceinline__ float row_score(const Row &r, int k, const float *) const { return ssddev::sigmoid(r.v[k]); }
};

struct Q8Load {                               // uint8 head tensors: box [batch][A][4], cls [batch][A][stride] (class bytes first, background at 0)
    const uint8_t *boxq, *cls, *lut;          // lut: the graph's uint8 LOGISTIC as a 256-byte table
    const float *anchors;
    int stride;                               // a multiple of 4: a lane's four class bytes are one aligned load inside the row
    float box_scale, box_zp, sc_scale, sc_zp;
    static constexpr int FIRST = 1;
    typedef unsigned Row;
    __device__ __forceinline__ static int col4(int k, int lane) { return lane * 4 + k; }
    __device__ __forceinline__ void image(size_t z, int A) { boxq += z * A * 4; cls += z * A * stride; }
    __device__ __forceinline__ void table(float *lutf, int tid) const {     // byte -> score, once: DequantizeClassPredictions behind the LOGISTIC table
#pragma clang fp contract(off)
        if (tid < 256) lutf[tid] = sc_scale * ((float)lut[tid] - sc_zp);
    }
    __device__ __forceinline__ float4 box(int a) const {
#pragma clang fp contract(off)
        const uint8_t *b = boxq + (size_t)a * 4;
        float r[4], an[4], bx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { r[q] = box_scale * ((float)b[q] - box_zp); an[q] = anchors[a * 4 + q]; }
        (void)ssddev::decode_anchor(r, an, 0.f, bx);
        return float4{bx[0], bx[1], bx[2], bx[3]};
    }
    __device__ __forceinline__ float score(int a, int col, const float *lutf) const { return lutf[cls[(size_t)a * stride + col]]; }
    __device__ __forceinline__ Row load_row(int a, int lane, int) const {
        return lane * 4 < stride ? *reinterpret_cast<const unsigned *>(cls + (size_t)a * stride + lane * 4) : 0u;
    }
    __device__ __forceinline__ float row_score(const Row &r, int k, const float *lutf) const { return lutf[(r >> (8 * k)) & 0xffu]; }
};

// One workgroup per image.  ncols = L::FIRST + classes <= RN_MAX_COLS.  Dynamic LDS: float4 [A] boxes, then u64 [max_det][ceil(A / 64)].
template <class L>
__global__ __launch_bounds__(RN_THREADS) void ssd_regular_nms_k(L ld, int A, int ncols, int max_det, int per_class, float score_thr,
                                                                float iou_thr, float *__restrict__ out_boxes, float *__restrict__ out_cls,
                                                                float *__restrict__ out_scores, int *__restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ u64 heads[RN_MAX_COLS];          // per column: the best live pair, 0 = none
    __shared__ u64 part[2][RN_WAVES];           // the waves' parts of the swept column's next head (alternating rows: one barrier per round)
    __shared__ float lutf[256];
    float4 *sbox = reinterpret_cast<float4 *>(smem);
    const int kw = (A + 63) >> 6;
    u64 *kill = reinterpret_cast<u64 *>(smem + (size_t)A * sizeof(float4));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const size_t z = blockIdx.x;
        ld.image(z, A);
        out_boxes += z * max_det * 4; out_cls += z * max_det; out_scores += z * max_det; out_count += z;
    }
    if (tid < RN_MAX_COLS) heads[tid] = 0ull;
    ld.table(lutf, tid);
    for (int i = tid; i < max_det * kw; i += RN_THREADS) kill[i] = 0ull;
    for (int a = tid; a < A; a += RN_THREADS) sbox[a] = ld.box(a);
    __syncthreads();

    // ---- first pass: the head of every class
    {
        u64 best[4] = {0ull, 0ull, 0ull, 0ull};
        for (int a0 = wave; a0 < A; a0 += RN_WAVES * RN_ROWS) {
            typename L::Row r[RN_ROWS];
#pragma unroll
            for (int u = 0; u < RN_ROWS; ++u) { const int a = a0 + RN_WAVES * u; r[u] = ld.load_row(a < A ? a : a0, lane, ncols); }   // all loads first
#pragma unroll
            for (int u = 0; u < RN_ROWS; ++u) {
                const int a = a0 + RN_WAVES * u;
                if (a >= A) break;                                                 // wave-uniform
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int col = L::col4(k, lane);
                    if (col < L::FIRST || col >= ncols) continue;
                    const float s = ld.row_score(r[u], k, lutf);
                    if (s >= score_thr) {                                          // a NaN is no candidate
                        const u64 key = ((u64)score_bits(s) << 32) | (unsigned)~a;
                        best[k] = key > best[k] ? key : best[k];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = L::col4(k, lane);
            if (col >= L::FIRST && col < ncols && best[k]) atomicMax(&heads[col], best[k]);
        }
    }
    __syncthreads();

    // ---- rounds
    int n = 0, n_slots = 0;
    int v_col = -1, v_cnt = 0;                  // lane l (of every wave alike): the column that owns bit row l, and its rows so far
    int prev_col = -1;
    u64 prev_head = 0ull;
    for (int it = 0; n < max_det; ++it) {
        if (prev_col >= 0) {                    // the column swept in the last round: fold the waves' parts
            u64 h = part[(it - 1) & 1][0];
#pragma unroll
            for (int w = 1; w < RN_WAVES; ++w) { const u64 o = part[(it - 1) & 1][w]; h = o > h ? o : h; }
            prev_head = h;
            if (tid == 0) heads[prev_col] = h;  // read from the next round on (nobody reads this entry in this one)
        }
        u64 sel = 0ull;                         // score bits << 32 | ~column: the maximum is the best score, the lower class on ties
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = k * 64 + lane;
            if (col < L::FIRST || col >= ncols) continue;
            const u64 h = col == prev_col ? prev_head : heads[col];
            const u64 sk = (h & 0xffffffff00000000ull) | (unsigned)~col;
            if (h != 0ull && sk > sel) sel = sk;
        }
        sel = wave_max(sel);
        if (sel == 0ull) break;                 // nothing live (uniform over the workgroup: every wave read the same heads)
        const int col = (int)~(unsigned)sel;
        const u64 hk = col == prev_col ? prev_head : heads[col];
        const int ap = (int)~(unsigned)hk;
        const u64 owner = __ballot(v_col == col);
        const int slot = owner ? __ffsll((long long)owner) - 1 : n_slots;
        if (!owner) { ++n_slots; if (lane == slot) { v_col = col; v_cnt = 0; } }
        if (lane == slot) ++v_cnt;
        const int cnt = __shfl(v_cnt, slot, 64);
        const float4 pv = sbox[ap];
        if (tid == 0) {
            out_boxes[n * 4 + 0] = pv.x; out_boxes[n * 4 + 1] = pv.y; out_boxes[n * 4 + 2] = pv.z; out_boxes[n * 4 + 3] = pv.w;
            out_cls[n] = (float)(col - L::FIRST);
            out_scores[n] = bits_score((unsigned)(hk >> 32));
        }
        if (++n == max_det) break;
        u64 wbest = 0ull;
        if (cnt < per_class) {                  // else the class is full: no head any more
            const float ia = pv.x, ib = pv.y, ic = pv.z, id = pv.w;
            const float iarea = (ic - ia) * (id - ib);
            u64 *krow = kill + (size_t)slot * kw;
            float s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int a = tid + RN_THREADS * j; s[j] = ld.score(a < A ? a : ap, col, lutf); }     // all loads first
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = tid + RN_THREADS * j, w = RN_WAVES * j + wave;       // w: the word of this wave's 64 anchors
                if (w >= kw) break;                                                // wave-uniform
                const u64 dead = krow[w];
                const bool cand = a < A && !((dead >> lane) & 1ull) && s[j] >= score_thr;
                bool gone = false;
                if (cand) {
                    const float4 b = sbox[a];
                    const float area = (b.z - b.x) * (b.w - b.y);
                    gone = a == ap;
                    if (iarea > 0.f && area > 0.f) {
                        const float y0 = fmaxf(ia, b.x), x0 = fmaxf(ib, b.y), y1 = fminf(ic, b.z), x1 = fminf(id, b.w);
                        const float inter = fmaxf(y1 - y0, 0.f) * fmaxf(x1 - x0, 0.f);
                        gone = gone || inter / (iarea + area - inter) > iou_thr;
                    }
                }
                const u64 kb = __ballot(gone);
                if (kb && lane == 0) krow[w] = dead | kb;
                if (cand && !gone) {
                    const u64 key = ((u64)score_bits(s[j]) << 32) | (unsigned)~a;
                    wbest = key > wbest ? key : wbest;
                }
            }
            wbest = wave_max(wbest);
        }
        if (lane == 0) part[it & 1][wave] = wbest;
        prev_col = col;
        __syncthreads();
    }
    if (tid >= n && tid < max_det) {            // rows past the count are zero
        out_boxes[tid * 4 + 0] = 0.f; out_boxes[tid * 4 + 1] = 0.f; out_boxes[tid * 4 + 2] = 0.f; out_boxes[tid * 4 + 3] = 0.f;
        out_cls[tid] = 0.f; out_scores[tid] = 0.f;
    }
    if (tid == 0) *out_count = n;
}

int check_shape(const char *who, int A, int classes, int max_det, int per_class, int batch, int first) {
    DD_REQUIRE(A > 64 && A <= RN_MAX_ANCHORS && max_det >= 1 && max_det <= RN_MAX_DET && batch > 0 && per_class >= 1 && classes >= 1 &&
               classes + first <= RN_MAX_COLS, DD_E_ARG,
               "%s: bad shape (anchors %d: 65 .. %d, classes %d: 1 .. %d, max_detections %d: 1 .. %d, detections_per_class %d: >= 1, batch %d)", who, A,
               RN_MAX_ANCHORS, classes, RN_MAX_COLS - first, max_det, RN_MAX_DET, per_class, batch);
    return DD_OK;
}

template <class L>
int launch(hipStream_t s, const L &ld, int A, int ncols, int max_det, int per_class, float score_thr, float iou_thr, float *boxes,
           float *classes, float *scores, int *count, int batch) {
    static DevOnce once;                        // a per-device attribute of this instantiation: once per device, not on every launch
    int dev = 0;
    DD_HIP(hipGetDevice(&dev));
    constexpr size_t lds_max = (size_t)RN_MAX_ANCHORS * sizeof(float4) + (size_t)RN_MAX_DET * (RN_MAX_ANCHORS / 64) * sizeof(u64);
    const int rc = once.run(dev, [&]() -> int {
        DD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ssd_regular_nms_k<L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        return DD_OK;
    });
    if (rc != DD_OK) return rc;
    const size_t lds = (size_t)A * sizeof(float4) + (size_t)max_det * ((A + 63) / 64) * sizeof(u64);
    hipLaunchKernelGGL(ssd_regular_nms_k<L>, dim3(batch), dim3(RN_THREADS), lds, s, ld, A, ncols, max_det, per_class, score_thr, iou_thr, boxes,
                       classes, scores, count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace

namespace ddk {

// raw f32 [batch][n_anchors][4 + n_classes] (n_classes counts the background column, as in ssd_postprocess) -> rows [batch][max_det]
int ssd_regular_nms_raw(hipStream_t s, const float *raw, const float *anchors, int n_anchors, int n_classes, int max_det, int per_class,
                        float score_thr, float iou_thr, float *boxes, float *classes, float *scores, int *count, int batch) {
    int rc;
    if ((rc = check_shape("ssd_regular_nms", n_anchors, n_classes - 1, max_det, per_class, batch, 1)) != DD_OK) return rc;
    RawLoad L;
    L.raw = raw; L.anchors = anchors; L.ld = 4 + n_classes;
    return launch(s, L, n_anchors, n_classes, max_det, per_class, score_thr, iou_thr, boxes, classes, scores, count, batch);
}

// uint8 head tensors of `batch` images; quant4 = box scale, box zero point, score scale, score zero point (the LOGISTIC output's)
int ssd_regular_nms_u8(hipStream_t s, const uint8_t *box_q, const uint8_t *cls_q, int cls_stride, const uint8_t *lut, const float *quant4,
                       const float *anchors, int n_anchors, int n_classes, int max_det, int per_class, float score_thr, float iou_thr,
                       float *boxes, float *classes, float *scores, int *count, int batch) {
    int rc;
    if ((rc = check_shape("ssd_regular_nms_u8", n_anchors, n_classes - 1, max_det, per_class, batch, 1)) != DD_OK) return rc;
    DD_REQUIRE(cls_stride >= n_classes && cls_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(cls_q) & 3u) == 0, DD_E_ARG,
               "ssd_regular_nms_u8: class rows of %d bytes for %d columns (a multiple of 4, 4-byte aligned)", cls_stride, n_classes);
    Q8Load L;
    L.boxq = box_q; L.cls = cls_q; L.lut = lut; L.anchors = anchors; L.stride = cls_stride;
    L.box_scale = quant4[0]; L.box_zp = quant4[1]; L.sc_scale = quant4[2]; L.sc_zp = quant4[3];
    return launch(s, L, n_anchors, n_classes, max_det, per_class, score_thr, iou_thr, boxes, classes, scores, count, batch);
}

}  // namespace ddk

extern "C" {

int dd_ssd_regular_nms_decoded(dd_ctx *ctx, const float *dec_boxes, const float *scores_in, int score_ld, int first_class_col, int n_anchors,
                               int n_classes, int max_det, int detections_per_class, float score_thr, float iou_thr, float *boxes,
                               float *classes, float *scores, int *count, int batch, void *stream) {
    DD_REQUIRE(ctx && dec_boxes && scores_in && boxes && classes && scores && count, DD_E_ARG, "dd_ssd_regular_nms_decoded: NULL argument");
    int rc;
    if ((rc = check_shape("dd_ssd_regular_nms_decoded", n_anchors, n_classes, max_det, detections_per_class, batch, 0)) != DD_OK) return rc;
    DD_REQUIRE(first_class_col >= 0 && score_ld >= first_class_col + n_classes && (reinterpret_cast<uintptr_t>(dec_boxes) & 15u) == 0, DD_E_ARG,
               "dd_ssd_regular_nms_decoded: score rows of %d floats for classes at columns %d .. %d; boxes 16-byte aligned", score_ld,
               first_class_col, first_class_col + n_classes - 1);
    DD_DEVICE(ctx);
    DecodedLoad L;
    L.boxes = dec_boxes; L.scores = scores_in + first_class_col; L.ld = score_ld;
    return launch(dd_pick_stream(ctx, stream), L, n_anchors, n_classes, max_det, detections_per_class, score_thr, iou_thr, boxes, classes,
                  scores, count, batch);
}

int dd_ssd_postprocess_regular(dd_ctx *ctx, const float *raw, const float *anchors, int n_anchors, int n_classes, int max_det,
                               int detections_per_class, float score_thr, float iou_thr, float *boxes, float *classes, float *scores,
                               int *count, int batch, void *stream) {
    DD_REQUIRE(ctx && raw && anchors && boxes && classes && scores && count, DD_E_ARG, "dd_ssd_postprocess_regular: NULL argument");
    DD_DEVICE(ctx);
    return ddk::ssd_regular_nms_raw(dd_pick_stream(ctx, stream), raw, anchors, n_anchors, n_classes, max_det, detections_per_class, score_thr,
                                    iou_thr, boxes, classes, scores, count, batch);
}

int dd_ssd_postprocess_regular_u8(dd_ctx *ctx, const uint8_t *box_q, const uint8_t *cls_q, int cls_stride, const uint8_t *logistic_table,
                                  const float *quant4_host, const float *anchors, int n_anchors, int n_classes, int max_det,
                                  int detections_per_class, float score_thr, float iou_thr, float *boxes, float *classes, float *scores,
                                  int *count, int batch, void *stream) {
    DD_REQUIRE(ctx && box_q && cls_q && logistic_table && quant4_host && anchors && boxes && classes && scores && count, DD_E_ARG,
               "dd_ssd_postprocess_regular_u8: NULL argument");
    DD_DEVICE(ctx);
    return ddk::ssd_regular_nms_u8(dd_pick_stream(ctx, stream), box_q, cls_q, cls_stride, logistic_table, quant4_host, anchors, n_anchors,
                                   n_classes, max_det, detections_per_class, score_thr, iou_thr, boxes, classes, scores, count, batch);
}

}  // extern "C"
