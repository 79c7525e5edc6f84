// Host arithmetic of the batched pipeline that needs no device: per stream, tools/intersection.py:4-24 and the box hygiene of
// deepdish.py:940-960; per step, the skip counters and stream lists (StepPlan), the pairing counts and the feature-row table.  A header
// of its own so that csrc/pipeline.hip and the sanitizer harness (tests/sanitize/host_harness.cpp, built with -fsanitize=thread /
// address,undefined by tests/test_sanitizers.py) compile the same statements.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ddhost {

inline double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// tools/intersection.py:4-24
inline bool seg_intersect(const double p[2], const double pr[2], const double q[2], const double qs[2]) {
    const double eps = 2.220446049250313e-16;
    const double rx = pr[0] - p[0], ry = pr[1] - p[1], sx = qs[0] - q[0], sy = qs[1] - q[1];
    const double rxs = cross2(rx, ry, sx, sy);
    const double mx = q[0] - p[0], my = q[1] - p[1];
    const double qpxr = cross2(mx, my, rx, ry);
    if (fabs(rxs) < eps) {
        if (fabs(qpxr) >= eps) return false;
        const double rr = rx * rx + ry * ry;
        const double ex = rx / rr, ey = ry / rr;
        double t0 = mx * ex + my * ey;
        double t1 = t0 + sx * ex + sy * ey;
        if (t0 > t1) std::swap(t0, t1);
        return !(t1 < 0 || t0 > 1);
    }
    const double t = cross2(mx, my, sx, sy) / rxs, u = qpxr / rxs;
    return 0.0 <= t && t <= 1.0 && 0.0 <= u && u <= 1.0;
}

// deepdish.py:947-953 for one stream: nothing survives a NaN anywhere; x, y clipped to the frame and truncated, w, h clipped to what is
// left of it; boxes over 90 % of the frame dropped.  boxes tlwh f64 rows; appends to the three output vectors.
inline void clean_boxes(const std::vector<double> &boxes, const std::vector<double> &scores, const std::vector<int> &cls, int W, int H,
                        std::vector<int64_t> &ib, std::vector<double> &is, std::vector<int> &ic) {
    const int k0 = (int)scores.size();
    for (double v : boxes) if (v != v) return;
    for (int i = 0; i < k0; ++i) {
        const double *b = boxes.data() + (size_t)i * 4;
        auto clipi = [](double v, double lo, double hi) { return (int64_t)(v < lo ? lo : (v > hi ? hi : v)); };
        const int64_t x = clipi(b[0], 0, W), y = clipi(b[1], 0, H);
        const int64_t w = clipi(b[2], 0, (double)(W - x)), h = clipi(b[3], 0, (double)(H - y));
        if ((double)(w * h) > 0.9 * W * H) continue;
        ib.insert(ib.end(), {x, y, w, h});
        is.push_back(scores[i]);
        ic.push_back(cls[i]);
    }
}

// ---------------- the batched step's index arithmetic (csrc/pipeline.hip): plain vectors, no device, no pipeline handle

// --object-detector-skip-frames (deepdish.py:892-893,929-938), one counter per stream.  dd_pipeline_detector_skip_frames is the same
// N for every stream and no phase; a pipeline without the option has N = 0 everywhere.
struct SkipCounters {
    std::vector<int> n, phase, rem;            // N[z]; phase[z] (-1: none); skip steps left before z's next detector step
    std::vector<uint8_t> has, last;            // z has a detector result; z's last step was a skip step
    void start(size_t S, int n_all) { n.assign(S, n_all); phase.assign(S, -1); rem.assign(S, 0); has.assign(S, 0); last.assign(S, 0); }
    void restart(int z) { rem[z] = 0; has[z] = 0; last[z] = 0; }
};

// What one step does, decided before it launches anything.  Four index spaces, each named once: a stream z; a POSITION i in act (every
// per-step array -- off, doff, eoff, tlwh, skp, the tracker pointer list -- is per position); a position in dl (the detector run's
// blocks); and skp[i], whether position i is on a skip step.
struct StepPlan {
    std::vector<int> act, act_next;            // the streams this step advances, ascending (all S without a mask); those frames_next is for
    std::vector<int> dl, dl_next;              // the streams of act on a detector step; the streams of act_next that will be on one
    std::vector<uint8_t> skp;                  // per position in act: a skip step for that stream (all ones = a lock-step skip step: dl empty)
    std::vector<int> rem_next;                 // the counters after this step (committed when it has succeeded)
    std::vector<uint8_t> has_next;
    // the motion gate (gate_streams, below): empty / zero in a pipeline without it.  A gated stream is a third state of a position:
    // not on a skip step (skp 0), yet without a block in the detector run (not in dl).
    std::vector<uint8_t> gat;                  // per position in act: gated in this step
    std::vector<int> dl_elig, cnt_elig;        // dl as plan_skip left it (the streams the gate counted), and their foreground pixels
    // the step's arguments.  frames: what the detector and the crops read (the masked copy under --enable-background-masking).
    // frames_next: NULL = no look-ahead run is queued (none given, no stream of it on a detector step, or masking).
    const uint8_t *frames_in = nullptr, *frames = nullptr, *frames_next = nullptr, *present = nullptr;
    const double *inj_boxes = nullptr, *inj_scores = nullptr;
    const int *inj_cls = nullptr, *inj_offsets = nullptr;
};

// pl.act / pl.act_next -> skp, dl, dl_next and the counters after the step.  On a step with z: rem[z] > 0 and z has a detector result
// -> a skip step for z, rem[z] -= 1; else a detector step, then rem[z] = N[z] (phase[z] after z's first).  A step without z moves
// nothing of z.  The counters after the step follow from those at its entry, so what the look-ahead queues is known here.
inline void plan_skip(const SkipCounters &c, StepPlan &pl) {
    const int n = (int)pl.act.size();
    pl.skp.assign(n, 0);
    pl.gat.assign(n, 0);
    pl.dl.clear(); pl.dl_next.clear(); pl.dl_elig.clear(); pl.cnt_elig.clear();
    pl.rem_next = c.rem; pl.has_next = c.has;
    for (int i = 0; i < n; ++i) {
        const int z = pl.act[i];
        if (c.rem[z] > 0 && c.has[z]) { pl.skp[i] = 1; pl.rem_next[z] = c.rem[z] - 1; }
        else {
            pl.dl.push_back(z);
            pl.rem_next[z] = !c.has[z] && c.phase[z] >= 0 ? c.phase[z] : c.n[z];
            pl.has_next[z] = 1;
        }
    }
    for (int z : pl.act_next) if (!(pl.rem_next[z] > 0 && pl.has_next[z])) pl.dl_next.push_back(z);
}

// The motion gate (dd_pipeline_motion_gate): "nothing moved on this stream, so whatever the detector finds fails the motion test".
// thr[z] = T[z] >= 0.  After MOG2 the step counts the foreground pixels of every stream of dl; counts[j] belongs to pl.dl[j].  A
// stream with counts <= T leaves dl and is marked in gat: this step runs no detector chain, crops or encoder rows for it, its adaptor
// output is empty, and the rest of the step sees a present stream with zero candidates.  dl stays ascending.  Returns the number gated.
inline int gate_streams(const std::vector<int> &thr, const int *counts, StepPlan &pl) {
    pl.dl_elig = pl.dl;
    pl.cnt_elig.assign(counts, counts + pl.dl.size());
    pl.dl.clear();
    int gated = 0;
    for (size_t i = 0, j = 0; i < pl.act.size() && j < pl.dl_elig.size(); ++i) {
        if (pl.act[i] != pl.dl_elig[j]) continue;
        const int z = pl.dl_elig[j];
        if (pl.cnt_elig[j] <= thr[z]) { pl.gat[i] = 1; ++gated; }
        else pl.dl.push_back(z);
        ++j;
    }
    return gated;
}

// What dd_pipeline_gate_stats reports: steps on which the gate ran, gated stream-steps, and per stream the count of its last
// detector-eligible step (-1: none yet) and whether that step was gated.  A step's plan enters when the step has succeeded.
struct GateStats {
    long long steps = 0, gated = 0;
    std::vector<int> last_count;
    std::vector<uint8_t> last_gated;
    void start(size_t S) { steps = gated = 0; last_count.assign(S, -1); last_gated.assign(S, 0); }
    void restart(int z) { last_count[z] = -1; last_gated[z] = 0; }
    void commit(const std::vector<int> &thr, const StepPlan &pl) {
        if (pl.dl_elig.empty()) return;
        steps += 1;
        for (size_t j = 0; j < pl.dl_elig.size(); ++j) {
            const int z = pl.dl_elig[j];
            last_count[z] = pl.cnt_elig[j];
            last_gated[z] = pl.cnt_elig[j] <= thr[z];
            gated += last_gated[z];
        }
    }
};

// Prefix sums per position in act.  doff: the tracker's input rows -- a stream on a detector step brings its kept boxes, one on a skip
// step the first min(kept boxes now, feature rows of its last encoder run) of them, as zip() truncates (deepdish.py:1003-1014); a gated
// stream has no candidates, so kept(i) is 0 and it takes no row of either kind.
// eoff: the rows the encoder makes in this step, the detector streams' only.  kept(i), retained(i): per position.
template <class Kept, class Retained>
inline void pair_counts(const std::vector<uint8_t> &skp, Kept kept, Retained retained, std::vector<int> &doff, std::vector<int> &eoff) {
    const int n = (int)skp.size();
    doff.assign(n + 1, 0);
    eoff.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int k = kept(i);
        doff[i + 1] = doff[i] + (skp[i] ? std::min(k, (int)retained(i)) : k);
        eoff[i + 1] = eoff[i] + (skp[i] ? 0 : k);
    }
}

// The table of one feature_rows_carry launch (csrc/featrows.hip; 8 ints per entry: {sel 0 fresh / 1 store, src row, n_out, dst row in
// out} {n_store, dst row in the next store, 0, 0}) and the store it leaves, over ALL S streams in stream order.  A stream of the step
// reads its fresh encoder rows (eoff) or its retained rows [ret_off[z], + ret_n[z]) of the current store.  Rows go to the tracker's input
// at doff only when some stream on a skip step has rows to pair (`gather`; otherwise the encoder's output already is that input), and to
// the next store only when an encoder run changed what is retained (`refresh`: fresh rows replace, the rest is carried, absent streams
// included).  A stream with nothing to move has no entry.  ret_off_new / ret_n_new / total describe the next store; they are the
// current one's when !refresh is all the caller may rely on (then total is 0 and nothing is written).
struct RowTable { bool gather; int total; };
inline RowTable feature_row_table(int S, const std::vector<int> &act, const std::vector<uint8_t> &skp, const std::vector<int> &doff,
                                  const std::vector<int> &eoff, const std::vector<int> &ret_off, const std::vector<int> &ret_n, bool refresh,
                                  std::vector<int> &table, std::vector<int> &ret_off_new, std::vector<int> &ret_n_new) {
    const int n = (int)act.size();
    bool gather = false;
    for (int i = 0; i < n; ++i) gather = gather || (skp[i] && doff[i + 1] > doff[i]);
    table.clear();
    ret_off_new.assign(S, 0); ret_n_new.assign(S, 0);
    int total = 0;
    for (int z = 0, i = 0; z < S; ++z) {
        const bool here = i < n && act[i] == z;
        const bool fresh = here && !skp[i];
        const int kept = here ? (fresh ? eoff[i + 1] - eoff[i] : doff[i + 1] - doff[i]) : 0;
        const int n_out = here && gather ? kept : 0, n_store = !refresh ? 0 : fresh ? kept : ret_n[z];
        if (n_out > 0 || n_store > 0) {
            const int e[8] = {fresh ? 0 : 1, fresh ? eoff[i] : ret_off[z], n_out, here ? doff[i] : 0, n_store, total, 0, 0};
            table.insert(table.end(), e, e + 8);
        }
        ret_off_new[z] = total;
        ret_n_new[z] = n_store;
        total += n_store;
        i += here;
    }
    return {gather, total};
}

}  // namespace ddhost
