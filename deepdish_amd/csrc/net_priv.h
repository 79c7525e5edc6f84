// Engine state shared by the two executor translation units: csrc/nets.hip (f16 programs) and csrc/netsq.hip (uint8 programs).
#pragma once
#include <map>
#include <utility>
#include <vector>
#include "common.h"

struct TensorDesc { int buf, h, w, c, cs, coff, dtype, pad; };

struct dd_net {
    dd_ctx *ctx = nullptr;
    int max_batch = 0;
    std::vector<int32_t> prog;
    std::vector<TensorDesc> tensors;
    std::vector<int64_t> buf_elems;          // per image
    std::vector<void *> bufs;
    std::vector<int> buf_dtype;
    int n_ops = 0, ops_off = 0;
    void *arena = nullptr;                   // dd_net_create_shared: one allocation, the buffers are offsets into it
    int64_t arena_bytes = 0;
    char *d_weights = nullptr;
    int64_t weight_bytes = 0;
    int in_h = 0, in_w = 0, out_tensor = -1;
    bool profile = false;
    int last_batch = 0;
    DevBuf slab;                             // split-K partial sums (sized for max_batch: see launch_conv)
    // dd_net_ssd_decode: the SSD head ops decode in their epilogue into these per-anchor arrays ([max_batch][n_anchors] each)
    bool ssd_dec = false, yolo_dec = false;                      // dd_net_yolo_decode: the Detect heads reduce their rows to (box, confidence, class); dec_anchors = rows per image
    int dec_anchors = 0; float dec_thr = 0.f;
    float *d_anchors = nullptr, *dec_boxes = nullptr, *dec_score = nullptr, *dec_keys = nullptr; int *dec_cls = nullptr;
    bool slab_moved = false;                 // the slab was reallocated during the last eager forward: captured graphs hold a dead pointer
    _Float16 *d_zero = nullptr;              // 256 bytes of zeros (padding taps of the direct-to-LDS fills)
    std::vector<hipEvent_t> events;           // n_ops + 1 when profiling
    std::vector<int32_t> op_launch;           // per op of the last forward: DD_OPK_* (which launch ran it)
    std::vector<int32_t> op_variant;          // per op of the last forward: tile / fill mode / K split of the generic conv launcher, 0 = another kernel
    // Latency mode (dd_net_use_graph): the launch train of one forward -- 20 to 75 short kernels at batch 1 -- captured
    // once per (input pointer, batch) and replayed as one hipGraph launch; the first call of a key runs eagerly (it may
    // still allocate split-K slabs and set function attributes), the second captures.
    struct GraphEntry { int calls = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
    bool use_graph = false;
    std::map<std::pair<const void *, int>, GraphEntry> graphs;
};

// ---- the op record: OP_WORDS int32 words per op, written by deepdish_amd/nets.py (Program._op; OP_FIELDS there is this enum, name for name --
// tests/test_op_fields.py) and read through OpView.  One enumerator per line, each with its index.
constexpr int OP_WORDS = 48;
constexpr int TENSOR_WORDS = 8;    // buf, h, w, c, cs, coff, dtype, bordered (TensorDesc)

enum { OP_INPUT = 1, OP_CONV = 2, OP_DWCONV = 3, OP_MAXPOOL = 4, OP_UPSAMPLE = 5, OP_FC = 6, OP_L2NORM = 7, OP_STEM = 8, OP_DWPW = 9 };
enum { OP_QCONV0 = 16, OP_QCONV = 17, OP_QDW = 18, OP_QDWPW = 19, OP_QSSD_DECODE = 20, OP_QADD = 21 };      // the uint8 programs' ops (csrc/netsq*.hip)
enum { ACT_NONE = 0, ACT_RELU6 = 1, ACT_ELU = 2, ACT_SILU = 3, ACT_RELU = 4, ACT_SIGMOID = 5 };
enum { EPI_F16 = 0, EPI_F32 = 1, EPI_SSD_HEAD = 2, EPI_YOLO = 3 };
enum { DT_F16 = 0, DT_F32 = 1, DT_U8 = 2 };
// W_HINT: what the compiler knows about the ops behind this one (the executor still checks shapes, batch and balance before it folds anything)
enum { HINT_NONE = 0,
       HINT_NEXT_ONLY = 1,      // only the next op reads my output
       HINT_HOLD_UNIT = 2,      // hold this residual unit for the next one (res_pair_rows_k)
       HINT_NEXT_IS_PROJ = 3,   // the next op is this block's 1x1 stride-2 projection
       HINT_PAIR_MEMBER = 4 };  // member of a conv3_x block launch (csrc/mars_pair.hip)

enum OpWord {
    // every op
    W_KIND = 0,
    W_SRC = 1,
    W_DST = 2,
    W_RES = 3,
    W_DST2 = 4,
    W_KH = 5,
    W_KW = 6,
    W_STRIDE = 7,
    W_PAD_T = 8,
    W_PAD_L = 9,
    W_CIN = 10,
    W_COUT = 11,
    W_COUT_PAD = 12,
    W_KPAD = 13,
    W_ACT = 14,
    W_EPI = 15,
    W_W_OFF = 16,
    W_B_OFF = 17,
    W_AFF_OFF = 18,           // second-output affine / per-anchor weight copy of a decoding head / lo part of a split uint8 filter
    W_HAS_AFF = 19,
    W_P0 = 20,                // p(0..5): W_P0 + i
    W_P1 = 21,
    W_P2 = 22,
    W_P3 = 23,
    W_P4 = 24,
    W_P5 = 25,
    W_HO = 26,
    W_WO = 27,
    W_BK = 28,
    W_POOL = 29,
    W_HINT = 30,
    W_AUX_OFF = 31,           // per-anchor bias copy of a decoding head
    // words 5 and 6 of the input op and of a pool
    W_S2D = 5,
    W_SWAP_RB = 6,
    W_POOL_K = 5,
    W_POOL_CASCADE = 6,
    // f16 ops: float words f(0..7)
    W_F0 = 32,
    W_F1 = 33,
    W_F2 = 34,
    W_F3 = 35,
    W_F4 = 36,
    W_F5 = 37,
    W_F6 = 38,
    W_F7 = 39,
    // ---- the uint8 ops' own (deepdish_amd/netsq.py): the requantisation of the op's (pointwise) layer ...
    W_Q_MULT = 32,
    W_Q_SHIFT = 33,
    W_Q_LO = 36,
    W_Q_HI = 37,
    W_Q_ZWC = 38,             // 128 - the weight zero point (0: folded into the filter)
    W_Q_IN_ZP = 39,
    W_Q_OUT_ZP = 40,
    W_Q_LINEAR = 41,
    W_Q_ROW_BYTES = 42,       // QEPI_ROWS: geometry of the rows written
    W_Q_BASE_OFF = 43,
    W_Q_COUT_STORE = 44,
    W_Q_DW_CQ_OFF = 45,       // folded 64-bit requantisation addends: depthwise half of a block, the op's layer
    W_Q_CQ_OFF = 46,
    W_Q_DUP = 47,
    // ... OP_QDW / OP_QDWPW: the depthwise half (operand table, its constants, its requantisation)
    W_Q_DW_A_OFF = 20,
    W_Q_DW_CB_OFF = 21,
    W_Q_DW_MULT = 22,
    W_Q_DW_SHIFT = 23,
    W_Q_DW_LO = 24,
    W_Q_DW_HI = 25,
    W_Q_DW_OUT_ZP = 28,
    // ... OP_QCONV with two predictors (netsq.py conv_heads): the box layer behind the class layer's fragments (W_ACT = their count)
    W_Q_BOX_MULT = 20,
    W_Q_BOX_SHIFT = 21,
    W_Q_BOX_OUT_ZP = 22,
    W_Q_BOX_ROW_BYTES = 23,
    W_Q_BOX_BASE_OFF = 24,
    W_Q_BOX_COUT_STORE = 25,
    W_Q_BOX_ZWC = 28,
    // ... OP_QADD, and OP_QCONV with a residual operand (netsq.py add_words)
    W_Q_ADD_M1 = 20,
    W_Q_ADD_E1 = 21,
    W_Q_ADD_M2 = 22,
    W_Q_ADD_E2 = 23,
    W_Q_ADD_MO = 24,
    W_Q_ADD_EO = 25,
    W_Q_ADD_Z1 = 28,
    W_Q_ADD_Z2 = 29,
    W_Q_ADD_ZO = 31,
    W_Q_ADD_LO = 34,
    W_Q_ADD_HI = 35,
    // ... OP_QSSD_DECODE (floats)
    W_Q_DEC_CLASSES = 20,
    W_Q_DEC_ANCHORS = 21,
    W_Q_DEC_BOX_SCALE = 32,
    W_Q_DEC_BOX_ZP = 33,
    W_Q_DEC_SCORE_SCALE = 34,
    W_Q_DEC_SCORE_ZP = 35,
};

// Read-only view of one op record.
struct OpView {
    const int32_t *w;
    int operator[](OpWord i) const { return w[i]; }
    float fw(OpWord i) const { return reinterpret_cast<const float *>(w)[i]; }
    int kind() const { return w[W_KIND]; }
    int src() const { return w[W_SRC]; }
    int dst() const { return w[W_DST]; }
    int res() const { return w[W_RES]; }
    int dst2() const { return w[W_DST2]; }
    int kh() const { return w[W_KH]; }
    int kw() const { return w[W_KW]; }
    int stride() const { return w[W_STRIDE]; }
    int pad_t() const { return w[W_PAD_T]; }
    int pad_l() const { return w[W_PAD_L]; }
    int cin() const { return w[W_CIN]; }
    int cout() const { return w[W_COUT]; }
    int cout_pad() const { return w[W_COUT_PAD]; }
    int kpad() const { return w[W_KPAD]; }
    int act() const { return w[W_ACT]; }
    int epi() const { return w[W_EPI]; }
    uint32_t w_off() const { return (uint32_t)w[W_W_OFF]; }
    uint32_t bias_off() const { return (uint32_t)w[W_B_OFF]; }
    uint32_t aff_off() const { return (uint32_t)w[W_AFF_OFF]; }
    bool has_aff() const { return w[W_HAS_AFF] != 0; }
    int ho() const { return w[W_HO]; }
    int wo() const { return w[W_WO]; }
    int bk() const { return w[W_BK]; }
    bool pool() const { return w[W_POOL] != 0; }
    int hint() const { return w[W_HINT]; }
    uint32_t aux_off() const { return (uint32_t)w[W_AUX_OFF]; }
    int p(int i) const { return w[W_P0 + i]; }
    float f(int i) const { return reinterpret_cast<const float *>(w)[W_F0 + i]; }
    // the input op / a pool
    int s2d() const { return w[W_S2D]; }
    int swap_rb() const { return w[W_SWAP_RB]; }
    int pool_k() const { return w[W_POOL_K]; }
    int pool_cascade() const { return w[W_POOL_CASCADE]; }
};

inline OpView op(const dd_net *net, int k) { return OpView{net->prog.data() + net->ops_off + (size_t)k * OP_WORDS}; }

// csrc/netsq.hip: ops of the uint8 programs (kinds >= 16).  `handled` = 0 when the kind is not one of them.
int netq_run_op(dd_net *net, int op_index, const int32_t *o, const uint8_t *input, int nimg, hipStream_t s, int *handled);
// csrc/netsq_front.hip: the first three ops of a uint8 SSD-MobileNet-v1 program (first layer, blocks 1 and 2) as one launch; *ran = 0: not this
// program / geometry / quantisation -- run the ops one by one
int netq_run_front(dd_net *net, const int32_t *o0, const int32_t *o1, const int32_t *o2, const uint8_t *input, int nimg, hipStream_t s, int *ran);
// csrc/netsq_mid.hip: two consecutive block ops (MobileNet blocks 3 and 4 of a uint8 SSD-MobileNet-v1 program) as one launch; *ran = 0: not those
int netq_run_mid(dd_net *net, const int32_t *o3, const int32_t *o4, int nimg, hipStream_t s, int *ran);
int netq_prepare(dd_net *net);           // after dd_net_create allocated the buffers: borders of the uint8 tensors
