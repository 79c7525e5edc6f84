// The association DECISION of the tracker update on the device: the matching cascade, the thresholded assignment and the
// assignment solver, one wave64 per stream, working on the cost matrices tracker_assoc_k left in HBM.
//
// Reference (upstream paths): deep_sort/linear_assignment.py:11-141 (min_cost_matching, matching_cascade), deep_sort/tracker.py:95-133
// (_match), scipy.optimize.linear_sum_assignment as called at linear_assignment.py:58.  The host code this restates choice for choice:
// csrc/lsap.cpp (solver), csrc/pyset.cpp (CPython's set iteration order), ddk::match_decide_host in csrc/tracker.hip (cascade).
// The three lists a stream's decision consists of -- matches, unmatched tracks, unmatched detections -- come out element for element in
// the order the host code builds them: the order of the unmatched detections hands out new track ids, the order of the matches drives
// gallery placement.
//
// Every loop here has a bound computable from the problem's shape or a table size; a bound that is hit, or a NaN / -inf cost, sets the
// stream's status word and ends that stream's work (the host then decides that stream itself).
#include <algorithm>
#include <limits>
#include "common.h"

namespace {

constexpr int CAP = DD_ASSOC_DEVICE_MAX;                  // rows and columns of one problem
constexpr int SET_TABLE = 1024;                           // entries of one set table
enum { ST_OK = 0, ST_BADCOST = 1, ST_INFEASIBLE = 2, ST_BOUND = 3 };
enum { CONFIRMED = 2 };                                   // track.py:15-17

// ---- the set tables never outgrow SET_TABLE: CPython's growth rule (pyset.cpp: resize when fill * 5 >= mask * 3, to the first size > the
// request) replayed at compile time for CAP distinct keys, for a set filled by add() and for set_merge into an empty set.
constexpr int table_after_adds(int keys) {
    int mask = 7, fill = 0, top = 8;
    for (int used = 1; used <= keys; ++used) {
        ++fill;
        if (fill * 5 >= mask * 3) {
            int size = 8;
            while (size <= used * 4) size <<= 1;
            mask = size - 1; fill = used;
            if (size > top) top = size;
        }
    }
    return top;
}
constexpr int table_after_merge(int keys) {
    int top = 8;
    for (int used = 1; used <= keys; ++used) {
        if (used * 5 >= 7 * 3) {
            int size = 8;
            while (size <= used * 2) size <<= 1;
            if (size > top) top = size;
        }
    }
    return top;
}
static_assert(table_after_adds(CAP) <= SET_TABLE && table_after_merge(CAP) <= SET_TABLE, "set tables sized below what CAP keys need");

struct LsapLds {
    double u[CAP], v[CAP], dist[CAP];
    int pred[CAP], col_of_row[CAP], row_of_col[CAP], cand[CAP], row_seen[CAP], col_seen[CAP];
    int flag;
};

// lsap.cpp's Solver for nr <= nc, one wave.  acc(i, j): cost of solver row i, solver column j.  On ST_OK L.col_of_row[0..nr) /
// L.row_of_col[0..nc) hold the assignment.  Wave-uniform control flow throughout (the block is this one wave).
template <class Acc>
__device__ int lsap_wave(LsapLds &L, const Acc &acc, int nr, int nc, int lane) {
    const double INF = std::numeric_limits<double>::infinity();
    int bad = 0;
    for (int e = lane; e < nr * nc; e += 64) {
        const double c = acc(e / nc, e % nc);
        bad |= (c != c) || c == -INF;
    }
    if (__any(bad)) return ST_BADCOST;
    for (int i = lane; i < nr; i += 64) { L.u[i] = 0.0; L.col_of_row[i] = -1; }
    for (int j = lane; j < nc; j += 64) { L.v[j] = 0.0; L.row_of_col[j] = -1; L.pred[j] = -1; }
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {
        for (int t = lane; t < nc; t += 64) { L.cand[t] = nc - 1 - t; L.col_seen[t] = 0; L.dist[t] = INF; }
        for (int i = lane; i < nr; i += 64) L.row_seen[i] = 0;
        __syncthreads();
        double base = 0.0;
        int live = nc, row = cur, sink = -1;
        for (int it = 0; it < nc && sink < 0; ++it) {         // Dijkstra over the reduced costs: one column leaves per iteration
            if (lane == 0) L.row_seen[row] = 1;
            const double ur = L.u[row];
            double low = INF;
            int pick = -1;
            bool pick_free = false;
            for (int t = lane; t < live; t += 64) {
                const int j = L.cand[t];
                const double r = base + acc(row, j) - ur - L.v[j];
                double d = L.dist[j];
                if (r < d) { d = r; L.dist[j] = r; L.pred[j] = row; }
                const bool fr = L.row_of_col[j] < 0;
                if (d < low || (d == low && fr)) { low = d; pick = t; pick_free = fr; }
            }
            // the sequential scan's pick ("first strictly smaller, on an exact tie prefer a free column") among the candidates at the
            // minimum: the LARGEST t that is a free column if there is one, else the SMALLEST t
            double m = low;
            for (int o = 32; o; o >>= 1) m = fmin(m, __shfl_xor(m, o));
            if (!(m < INF)) return ST_INFEASIBLE;
            int score = (pick >= 0 && low == m) ? (pick_free ? 0x10000 + pick : 0xFFFF - pick) : -1;
            for (int o = 32; o; o >>= 1) score = max(score, __shfl_xor(score, o));
            if (score < 0) return ST_BOUND;
            const int tp = score >= 0x10000 ? score - 0x10000 : 0xFFFF - score;
            if (tp >= live) return ST_BOUND;
            base = m;
            const int j = L.cand[tp], jl = L.cand[live - 1], rc = L.row_of_col[j];
            __syncthreads();
            if (lane == 0) { L.col_seen[j] = 1; L.cand[tp] = jl; }
            --live;
            if (rc < 0) sink = j; else row = rc;
            __syncthreads();
        }
        if (sink < 0) return ST_BOUND;
        const double reach = base;
        for (int i = lane; i < nr; i += 64) {
            if (i == cur) L.u[i] += reach;
            else if (L.row_seen[i]) {
                const int c = L.col_of_row[i];
                if (c >= 0) L.u[i] += reach - L.dist[c];
            }
        }
        for (int j = lane; j < nc; j += 64)
            if (L.col_seen[j]) L.v[j] -= reach - L.dist[j];
        __syncthreads();
        if (lane == 0) {                                      // flip the alternating path: at most nr rows lie on it
            int j = sink, ok = 0;
            for (int k = 0; k < nr; ++k) {
                const int i = L.pred[j];
                if (i < 0 || i >= nr) break;
                L.row_of_col[j] = i;
                const int prev = L.col_of_row[i];
                L.col_of_row[i] = j;
                j = prev;
                if (i == cur) { ok = 1; break; }
                if (j < 0 || j >= nc) break;
            }
            L.flag = ok;
        }
        __syncthreads();
        if (!L.flag) return ST_BOUND;
    }
    return ST_OK;
}

// A raw row-major [nr][nc] matrix, solved as it is or transposed (lsap.cpp:101-104).
struct RawAcc {
    const double *c;
    int ld;
    bool tr;
    __device__ double operator()(int i, int j) const { return tr ? c[(size_t)j * ld + i] : c[(size_t)i * ld + j]; }
};

// The clamped, index-gathered sub-matrix of min_cost_matching (linear_assignment.py:56-57).
struct SubAcc {
    const double *full;
    const int *rows, *dets;
    int n_det;
    double maxd;
    bool tr;
    __device__ double at(int r, int q) const {
        const double v = full[(size_t)rows[r] * n_det + dets[q]];
        return v > maxd ? maxd + 1e-5 : v;
    }
    __device__ double operator()(int i, int j) const { return tr ? at(j, i) : at(i, j); }
};

// One wave per problem.  desc[4 p ..]: nr, nc, output offset (pairs), unused; off[p]: element offset of the matrix.
__global__ __launch_bounds__(64) void lsap_batch_k(const double *__restrict__ cost, const long long *__restrict__ off,
                                                   const int *__restrict__ desc, int *__restrict__ rows, int *__restrict__ cols,
                                                   int *__restrict__ status) {
    __shared__ LsapLds L;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int nr = desc[4 * p], nc = desc[4 * p + 1], o = desc[4 * p + 2];
    if (nr <= 0 || nc <= 0 || nr > CAP || nc > CAP) {         // (the launcher refuses these before launching)
        if (lane == 0) status[p] = ST_BOUND;
        return;
    }
    const bool tr = nr > nc;
    const RawAcc acc{cost + off[p], nc, tr};
    const int st = tr ? lsap_wave(L, acc, nc, nr, lane) : lsap_wave(L, acc, nr, nc, lane);
    if (lane == 0) status[p] = st;
    if (st != ST_OK) return;
    if (!tr) {
        for (int i = lane; i < nr; i += 64) { rows[o + i] = i; cols[o + i] = L.col_of_row[i]; }
        return;
    }
    // tall: pairs sorted by row (lsap.cpp:106-109); the solver's columns are the rows here
    int cnt = 0;
    for (int b = 0; b < nr; b += 64) {
        const int r = b + lane;
        const int c = r < nr ? L.row_of_col[r] : -1;
        const unsigned long long mk = __ballot(c >= 0);
        if (c >= 0) {
            const int k = cnt + __popcll(mk & ((1ull << lane) - 1));
            rows[o + k] = r; cols[o + k] = c;
        }
        cnt += __popcll(mk);
    }
}

// ---- pyset.cpp's set model on tables in LDS (run by one lane).  Keys are row indices < CAP; -1 empty, -2 dummy.
constexpr int LINEAR_PROBES = 9, PERTURB_SHIFT = 5, EMPTY = -1, DUMMY = -2;
struct DSet {
    int *tab;
    int mask, fill, used;
};
struct SetLds {
    int t[6][SET_TABLE];
};

__device__ void dset_init(DSet &s, int *tab) {
    s.tab = tab; s.mask = 7; s.fill = 0; s.used = 0;
    for (int i = 0; i < 8; ++i) tab[i] = EMPTY;
}

__device__ bool dset_insert_clean(int *t, int mask, int key) {
    unsigned perturb = (unsigned)key, i = (unsigned)key & mask;
    for (int guard = 0; guard < 4 * SET_TABLE; ++guard) {
        if (t[i] == EMPTY) { t[i] = key; return true; }
        if ((int)i + LINEAR_PROBES <= mask)
            for (int j = 1; j <= LINEAR_PROBES; ++j)
                if (t[i + j] == EMPTY) { t[i + j] = key; return true; }
        perturb >>= PERTURB_SHIFT;
        i = (i * 5 + 1 + perturb) & mask;
    }
    return false;
}

// into `spare`, which then becomes the set's table (and the old table the spare)
__device__ bool dset_resize(DSet &s, int minused, int *&spare) {
    int newsize = 8;
    while (newsize <= minused && newsize <= SET_TABLE) newsize <<= 1;
    if (newsize > SET_TABLE) return false;
    for (int i = 0; i < newsize; ++i) spare[i] = EMPTY;
    for (int i = 0; i <= s.mask; ++i)
        if (s.tab[i] >= 0 && !dset_insert_clean(spare, newsize - 1, s.tab[i])) return false;
    int *old = s.tab;
    s.tab = spare; spare = old;
    s.mask = newsize - 1;
    s.fill = s.used;
    return true;
}

// 1 / 0; -1 when the probe bound is hit
__device__ int dset_contains(const DSet &s, int key) {
    unsigned perturb = (unsigned)key, i = (unsigned)key & s.mask;
    for (int guard = 0; guard < 4 * SET_TABLE; ++guard) {
        int probes = ((int)i + LINEAR_PROBES <= s.mask) ? LINEAR_PROBES : 0;
        unsigned e = i;
        do {
            if (s.tab[e] == EMPTY) return 0;
            if (s.tab[e] == key) return 1;
            ++e;
        } while (probes--);
        perturb >>= PERTURB_SHIFT;
        i = (i * 5 + 1 + perturb) & s.mask;
    }
    return -1;
}

__device__ bool dset_add(DSet &s, int key, int *&spare) {    // set_add_entry
    unsigned perturb = (unsigned)key, i = (unsigned)key & s.mask;
    int freeslot = -1;
    for (int guard = 0; guard < 4 * SET_TABLE; ++guard) {
        int probes = ((int)i + LINEAR_PROBES <= s.mask) ? LINEAR_PROBES : 0;
        unsigned e = i;
        do {
            if (s.tab[e] == EMPTY) {
                if (freeslot >= 0) { s.tab[freeslot] = key; ++s.used; return true; }
                s.tab[e] = key;
                ++s.fill; ++s.used;
                if (s.fill * 5 >= s.mask * 3) return dset_resize(s, s.used * 4, spare);
                return true;
            }
            if (s.tab[e] == key) return true;
            if (s.tab[e] == DUMMY) freeslot = (int)e;
            ++e;
        } while (probes--);
        perturb >>= PERTURB_SHIFT;
        i = (i * 5 + 1 + perturb) & s.mask;
    }
    return false;
}

__device__ bool dset_discard(DSet &s, int key) {              // set_discard_entry: leaves a dummy
    unsigned perturb = (unsigned)key, i = (unsigned)key & s.mask;
    for (int guard = 0; guard < 4 * SET_TABLE; ++guard) {
        int probes = ((int)i + LINEAR_PROBES <= s.mask) ? LINEAR_PROBES : 0;
        unsigned e = i;
        do {
            if (s.tab[e] == EMPTY) return true;
            if (s.tab[e] == key) { s.tab[e] = DUMMY; --s.used; return true; }
            ++e;
        } while (probes--);
        perturb >>= PERTURB_SHIFT;
        i = (i * 5 + 1 + perturb) & s.mask;
    }
    return false;
}

// set_merge into an EMPTY set (what set_copy does)
__device__ bool dset_merge_from(DSet &r, const DSet &o, int *&spare) {
    if (o.used == 0) return true;
    if ((r.fill + o.used) * 5 >= r.mask * 3 && !dset_resize(r, (r.used + o.used) * 2, spare)) return false;
    if (r.fill == 0 && r.mask == o.mask && o.fill == o.used) {
        for (int i = 0; i <= o.mask; ++i) r.tab[i] = o.tab[i];
        r.fill = o.fill; r.used = o.used;
        return true;
    }
    r.fill = o.used; r.used = o.used;
    for (int i = 0; i <= o.mask; ++i)
        if (o.tab[i] >= 0 && !dset_insert_clean(r.tab, r.mask, o.tab[i])) return false;
    return true;
}

// out = list(set(a) - set(b)) in CPython 3.10 iteration order (ddk::pyset_difference_order); returns the length or -1.
// Each of the three sets owns a table and the spare its resizes move into.
__device__ int dset_difference_order(SetLds &S, const int *a, int na, const int *b, int nb, int *out) {
    int *spare_a = S.t[1], *spare_b = S.t[3], *spare_r = S.t[5];
    DSet sa, sb, r;
    dset_init(sa, S.t[0]);
    dset_init(sb, S.t[2]);
    dset_init(r, S.t[4]);
    for (int i = 0; i < na; ++i) if (!dset_add(sa, a[i], spare_a)) return -1;
    for (int i = 0; i < nb; ++i) if (!dset_add(sb, b[i], spare_b)) return -1;
    if ((sa.used >> 2) > sb.used) {                           // set_copy_and_difference
        if (!dset_merge_from(r, sa, spare_r)) return -1;
        for (int i = 0; i <= sb.mask; ++i)
            if (sb.tab[i] >= 0 && !dset_discard(r, sb.tab[i])) return -1;
    } else {
        for (int i = 0; i <= sa.mask; ++i)
            if (sa.tab[i] >= 0) {
                const int c = dset_contains(sb, sa.tab[i]);
                if (c < 0) return -1;
                if (!c && !dset_add(r, sa.tab[i], spare_r)) return -1;
            }
    }
    int n = 0;
    for (int i = 0; i <= r.mask; ++i)
        if (r.tab[i] >= 0 && n < CAP) out[n++] = r.tab[i];
    return n;
}

struct MatchLds {
    int confirmed[CAP], unconfirmed[CAP], rows[CAP], dets[CAP], dets_next[CAP], matched_rows[CAP], un_a[CAP];
    int n_next, n_matches, n_un_rows, flag;
};

// position of this lane's element among the flagged ones of the wave's 64, and the wave's count
__device__ __forceinline__ int wave_rank(bool f, int lane, int &total) {
    const unsigned long long mk = __ballot(f);
    const int k = total + __popcll(mk & ((1ull << lane) - 1));
    total += __popcll(mk);
    return k;
}

// linear_assignment.py:11-75 on M.rows[0..nr) x M.dets[0..nc) of `full` ([.][n_det]).  Appends to the matches (global, pairs) and, when
// un_rows is given, to the unmatched rows (global); writes the unmatched detections to M.dets_next / M.n_next.  nr, nc > 0.
__device__ int min_cost_matching_wave(LsapLds &L, MatchLds &M, const double *full, int n_det, double maxd, int nr, int nc,
                                      int *matches, int *un_rows, int lane) {
    const bool tr = nr > nc;
    const SubAcc acc{full, M.rows, M.dets, n_det, maxd, tr};
    const int st = tr ? lsap_wave(L, acc, nc, nr, lane) : lsap_wave(L, acc, nr, nc, lane);
    if (st != ST_OK) return st;
    const int *mrow = tr ? L.row_of_col : L.col_of_row;       // matched column of row r / matched row of column q, else -1
    const int *mcol = tr ? L.col_of_row : L.row_of_col;
    int nd = 0, nu = M.n_un_rows, nm = M.n_matches;
    for (int b = 0; b < nc; b += 64) {                        // :62-64
        const int q = b + lane;
        const bool f = q < nc && mcol[q] < 0;
        const int k = wave_rank(f, lane, nd);
        if (f) M.dets_next[k] = M.dets[q];
    }
    for (int b = 0; b < nr; b += 64) {                        // :65-67
        const int r = b + lane;
        const bool f = r < nr && mrow[r] < 0;
        const int k = wave_rank(f, lane, nu);
        if (f && un_rows) un_rows[k] = M.rows[r];
    }
    for (int b = 0; b < nr; b += 64) {                        // :68-74, pairs in row order
        const int r = b + lane;
        const int q = r < nr ? mrow[r] : -1;
        const bool over = q >= 0 && acc.at(r, q) > maxd;
        const bool under = q >= 0 && !over;
        const int ku = wave_rank(over, lane, nu);
        const int kd = wave_rank(over, lane, nd);
        const int km = wave_rank(under, lane, nm);
        if (over) {
            if (un_rows) un_rows[ku] = M.rows[r];
            M.dets_next[kd] = M.dets[q];
        }
        if (under) {
            matches[2 * km] = M.rows[r]; matches[2 * km + 1] = M.dets[q];
            M.matched_rows[km] = M.rows[r];
        }
    }
    __syncthreads();
    if (lane == 0) { M.n_next = nd; M.n_matches = nm; if (un_rows) M.n_un_rows = nu; }
    __syncthreads();
    return ST_OK;
}

// One wave per stream with T > 0 and n > 0.  desc[5 b ..]: row base (into state / tsu), T, n, cost base (appearance [T][n], then IoU
// [T][n]), output base.  out + output base: status, #matches, #unmatched rows, #unmatched detections, then the matches ((row, det) pairs,
// room for min(T, n)), the unmatched rows (room for T) and the unmatched detections (room for n).
__device__ __forceinline__ void assoc_match_body(const double *__restrict__ cost, const int *__restrict__ row_state,
                                                 const int *__restrict__ row_tsu, const int *__restrict__ desc, double max_cos,
                                                 double max_iou, int max_age, int *__restrict__ out) {
    __shared__ LsapLds L;
    __shared__ MatchLds M;
    __shared__ SetLds S;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = desc[5 * b + 1], n = desc[5 * b + 2];
    int *o = out + desc[5 * b + 4];
    if (T <= 0 || n <= 0 || T > CAP || n > CAP) {             // (decided on the host before launching)
        if (lane == 0) o[0] = ST_BOUND;
        return;
    }
    const int *state = row_state + desc[5 * b], *tsu = row_tsu + desc[5 * b];
    const double *app = cost + desc[5 * b + 3], *iou = app + (size_t)T * n;
    int *matches = o + 4, *un_rows = matches + 2 * min(T, n), *un_dets = un_rows + T;
    // ---- tracker.py:95-133 _match
    int n_conf = 0, n_unconf = 0;
    for (int base = 0; base < T; base += 64) {
        const int i = base + lane;
        const bool c = i < T && state[i] == CONFIRMED, u = i < T && !c;
        const int kc = wave_rank(c, lane, n_conf), ku = wave_rank(u, lane, n_unconf);
        if (c) M.confirmed[kc] = i;
        if (u) M.unconfirmed[ku] = i;
    }
    for (int q = lane; q < n; q += 64) M.dets[q] = q;
    if (lane == 0) { M.n_matches = 0; M.n_un_rows = 0; M.n_next = n; }
    __syncthreads();
    int nd = n, status = ST_OK;
    for (int level = 0; level < max_age && nd > 0; ++level) {    // linear_assignment.py:78-141
        int nl = 0;
        for (int base = 0; base < n_conf; base += 64) {
            const int i = base + lane;
            const int k = i < n_conf ? M.confirmed[i] : 0;
            const bool f = i < n_conf && tsu[k] == 1 + level;
            const int pos = wave_rank(f, lane, nl);
            if (f) M.rows[pos] = k;
        }
        if (nl == 0) continue;
        __syncthreads();
        status = min_cost_matching_wave(L, M, app, n, max_cos, nl, nd, matches, nullptr, lane);
        if (status != ST_OK) break;
        nd = M.n_next;
        for (int q = lane; q < nd; q += 64) M.dets[q] = M.dets_next[q];
        __syncthreads();
    }
    if (status == ST_OK) {
        // unmatched_tracks_a = list(set(track_indices) - set(k for k, _ in matches)) (linear_assignment.py:140) in CPython's order
        if (lane == 0) M.flag = dset_difference_order(S, M.confirmed, n_conf, M.matched_rows, M.n_matches, M.un_a);
        __syncthreads();
        const int n_a = M.flag;
        if (n_a < 0) status = ST_BOUND;
        else {
            // IoU stage on unconfirmed + [k in unmatched_tracks_a : tsu == 1]; the others are unmatched as they stand (tracker.py:117-123)
            for (int i = lane; i < n_unconf; i += 64) M.rows[i] = M.unconfirmed[i];
            int ni = n_unconf, nu = 0;
            for (int base = 0; base < n_a; base += 64) {
                const int i = base + lane;
                const int k = i < n_a ? M.un_a[i] : 0;
                const bool recent = i < n_a && tsu[k] == 1, old = i < n_a && !recent;
                const int pr = wave_rank(recent, lane, ni), po = wave_rank(old, lane, nu);
                if (recent) M.rows[pr] = k;
                if (old) un_rows[po] = k;
            }
            if (lane == 0) M.n_un_rows = nu;
            __syncthreads();
            if (ni > 0 && nd > 0) {
                status = min_cost_matching_wave(L, M, iou, n, max_iou, ni, nd, matches, un_rows, lane);
                if (status == ST_OK) {
                    nd = M.n_next;
                    for (int q = lane; q < nd; q += 64) un_dets[q] = M.dets_next[q];
                }
            } else {                                            // linear_assignment.py:49-50: nothing to assign
                for (int i = lane; i < ni; i += 64) un_rows[nu + i] = M.rows[i];
                for (int q = lane; q < nd; q += 64) un_dets[q] = M.dets[q];
                __syncthreads();
                if (lane == 0) M.n_un_rows = nu + ni;
                __syncthreads();
            }
        }
    }
    if (lane == 0) {
        o[0] = status;
        o[1] = M.n_matches; o[2] = M.n_un_rows; o[3] = nd;
    }
}

__global__ __launch_bounds__(64) void assoc_match_k(const double *__restrict__ cost, const int *__restrict__ row_state,
                                                    const int *__restrict__ row_tsu, const int *__restrict__ desc, double max_cos,
                                                    double max_iou, int max_age, int *__restrict__ out) {
    assoc_match_body(cost, row_state, row_tsu, desc, max_cos, max_iou, max_age, out);
}

// The same with --max-cosine-distance, --max-iou-distance and --max-age of each decided stream's own tracker: par_d[2 b], par_d[2 b + 1]
// and par_age[b] lie beside desc in the block the update uploads.
__global__ __launch_bounds__(64) void assoc_match_streams_k(const double *__restrict__ cost, const int *__restrict__ row_state,
                                                            const int *__restrict__ row_tsu, const int *__restrict__ desc,
                                                            const double *__restrict__ par_d, const int *__restrict__ par_age,
                                                            int *__restrict__ out) {
    const int b = blockIdx.x;
    assoc_match_body(cost, row_state, row_tsu, desc, par_d[2 * b], par_d[2 * b + 1], par_age[b], out);
}

}  // namespace

namespace ddk {

size_t assoc_out_ints(int T, int n) { return (size_t)4 + 2 * (size_t)std::min(T, n) + T + n; }

// Enqueue only.  cost / row_state / row_tsu / desc / out: device; layouts as assoc_match_k documents them.
int assoc_match(hipStream_t s, const double *cost, const int *row_state, const int *row_tsu, const int *desc, int n_streams,
                double max_cos, double max_iou, int max_age, int *out) {
    if (n_streams <= 0) return DD_OK;
    hipLaunchKernelGGL(assoc_match_k, dim3(n_streams), dim3(64), 0, s, cost, row_state, row_tsu, desc, max_cos, max_iou, max_age, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

int assoc_match_streams(hipStream_t s, const double *cost, const int *row_state, const int *row_tsu, const int *desc, int n_streams,
                        const double *par_d, const int *par_age, int *out) {
    if (n_streams <= 0) return DD_OK;
    hipLaunchKernelGGL(assoc_match_streams_k, dim3(n_streams), dim3(64), 0, s, cost, row_state, row_tsu, desc, par_d, par_age, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

extern "C" {

int dd_lsap_batch(dd_ctx *ctx, const double *cost_dev, const int *nr_host, const int *nc_host, const int64_t *offset_host,
                  int n_problems, int *rows_host, int *cols_host) {
    DD_REQUIRE(ctx && n_problems >= 0, DD_E_ARG, "dd_lsap_batch: bad argument");
    if (n_problems == 0) return DD_OK;
    DD_REQUIRE(cost_dev && nr_host && nc_host && offset_host && rows_host && cols_host, DD_E_ARG, "dd_lsap_batch: NULL argument");
    DD_DEVICE(ctx);
    std::vector<int> desc((size_t)4 * n_problems, 0);
    std::vector<long long> off(n_problems);
    int total = 0;
    for (int p = 0; p < n_problems; ++p) {
        const int nr = nr_host[p], nc = nc_host[p];
        DD_REQUIRE(nr > 0 && nc > 0 && offset_host[p] >= 0, DD_E_ARG, "dd_lsap_batch: problem %d has shape %d x %d, offset %lld", p, nr, nc,
                   (long long)offset_host[p]);
        DD_REQUIRE(nr <= CAP && nc <= CAP, DD_E_ARG, "dd_lsap_batch: problem %d is %d x %d, above the device solver's %d x %d", p, nr, nc, CAP,
                   CAP);
        desc[4 * p] = nr; desc[4 * p + 1] = nc; desc[4 * p + 2] = total;
        off[p] = offset_host[p];
        total += std::min(nr, nc);
    }
    hipStream_t s = ctx->stream;
    int rc;
    const size_t b_desc = desc.size() * sizeof(int), b_off = off.size() * sizeof(long long);
    const size_t b_out = ((size_t)2 * total + n_problems) * sizeof(int);
    if ((rc = ctx->scratch[0].reserve(b_off + b_desc)) != DD_OK) return rc;
    if ((rc = ctx->scratch[1].reserve(b_out)) != DD_OK) return rc;
    char *d_in = ctx->scratch[0].as<char>();
    int *d_out = ctx->scratch[1].as<int>();
    DD_HIP(hipMemcpyAsync(d_in, off.data(), b_off, hipMemcpyHostToDevice, s));
    DD_HIP(hipMemcpyAsync(d_in + b_off, desc.data(), b_desc, hipMemcpyHostToDevice, s));
    DD_HIP(hipStreamSynchronize(s));                              // the staging vectors are pageable
    hipLaunchKernelGGL(lsap_batch_k, dim3(n_problems), dim3(64), 0, s, cost_dev, reinterpret_cast<const long long *>(d_in),
                       reinterpret_cast<const int *>(d_in + b_off), d_out, d_out + total, d_out + 2 * total);
    DD_LAUNCH_CHECK();
    std::vector<int> h((size_t)2 * total + n_problems);
    DD_HIP(hipMemcpyAsync(h.data(), d_out, b_out, hipMemcpyDeviceToHost, s));
    DD_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < n_problems; ++p)
        DD_REQUIRE(h[(size_t)2 * total + p] == ST_OK, DD_E_ARG,
                   "dd_lsap_batch: problem %d stopped with status %d: %s", p, h[(size_t)2 * total + p],
                   h[(size_t)2 * total + p] == ST_BADCOST ? "its cost matrix contains NaN/-inf" :
                   h[(size_t)2 * total + p] == ST_INFEASIBLE ? "its cost matrix is infeasible" : "a loop bound of the solver was hit");
    memcpy(rows_host, h.data(), (size_t)total * sizeof(int));
    memcpy(cols_host, h.data() + total, (size_t)total * sizeof(int));
    return DD_OK;
}

int dd_match_cascade(dd_ctx *ctx, int where, const double *app, const double *iou, int T, int n, const int *state_host,
                     const int *tsu_host, double max_cos, double max_iou, int max_age, int *matches_host, int *n_matches_host,
                     int *un_rows_host, int *n_un_rows_host, int *un_dets_host, int *n_un_dets_host) {
    DD_REQUIRE(where == 0 || where == 1, DD_E_ARG, "dd_match_cascade: where must be 0 (host) or 1 (device), got %d", where);
    DD_REQUIRE(T >= 0 && n >= 0 && n_matches_host && n_un_rows_host && n_un_dets_host, DD_E_ARG, "dd_match_cascade: bad argument");
    DD_REQUIRE((T == 0 || (state_host && tsu_host && un_rows_host)) && (n == 0 || un_dets_host) &&
               (T == 0 || n == 0 || (app && iou && matches_host)), DD_E_ARG, "dd_match_cascade: NULL argument");
    std::vector<int> m, ur, ud;
    if (where == 0 || T == 0 || n == 0) {
        ddk::match_decide_host(app, iou, T, n, state_host, tsu_host, max_cos, max_iou, max_age, m, ur, ud);
    } else {
        DD_REQUIRE(ctx, DD_E_ARG, "dd_match_cascade: the device path needs a context");
        DD_REQUIRE(T <= CAP && n <= CAP, DD_E_ARG, "dd_match_cascade: %d x %d is above the device path's %d x %d", T, n, CAP, CAP);
        DD_DEVICE(ctx);
        hipStream_t s = ctx->stream;
        int rc;
        const size_t tn = (size_t)T * n, n_out = ddk::assoc_out_ints(T, n);
        const size_t b_int = ((size_t)2 * T + 5) * sizeof(int);
        if ((rc = ctx->scratch[0].reserve(2 * tn * sizeof(double))) != DD_OK) return rc;
        if ((rc = ctx->scratch[1].reserve(b_int)) != DD_OK) return rc;
        if ((rc = ctx->scratch[2].reserve(n_out * sizeof(int))) != DD_OK) return rc;
        double *d_cost = ctx->scratch[0].as<double>();
        int *d_int = ctx->scratch[1].as<int>(), *d_out = ctx->scratch[2].as<int>();
        std::vector<int> hi((size_t)2 * T + 5), ho(n_out);
        memcpy(hi.data(), state_host, (size_t)T * sizeof(int));
        memcpy(hi.data() + T, tsu_host, (size_t)T * sizeof(int));
        int *d = hi.data() + 2 * T;
        d[0] = 0; d[1] = T; d[2] = n; d[3] = 0; d[4] = 0;
        DD_HIP(hipMemcpyAsync(d_cost, app, tn * sizeof(double), hipMemcpyDeviceToDevice, s));
        DD_HIP(hipMemcpyAsync(d_cost + tn, iou, tn * sizeof(double), hipMemcpyDeviceToDevice, s));
        DD_HIP(hipMemcpyAsync(d_int, hi.data(), b_int, hipMemcpyHostToDevice, s));
        DD_HIP(hipStreamSynchronize(s));
        if ((rc = ddk::assoc_match(s, d_cost, d_int, d_int + T, d_int + 2 * T, 1, max_cos, max_iou, max_age, d_out)) != DD_OK) return rc;
        DD_HIP(hipMemcpyAsync(ho.data(), d_out, n_out * sizeof(int), hipMemcpyDeviceToHost, s));
        DD_HIP(hipStreamSynchronize(s));
        DD_REQUIRE(ho[0] == ST_OK, DD_E_ARG, "dd_match_cascade: the device decision stopped with status %d (1 NaN/-inf cost, 2 infeasible, 3 bound)",
                   ho[0]);
        const int *pm = ho.data() + 4, *pr = pm + 2 * std::min(T, n), *pd = pr + T;
        m.assign(pm, pm + 2 * ho[1]);
        ur.assign(pr, pr + ho[2]);
        ud.assign(pd, pd + ho[3]);
    }
    *n_matches_host = (int)m.size() / 2;
    *n_un_rows_host = (int)ur.size();
    *n_un_dets_host = (int)ud.size();
    if (!m.empty()) memcpy(matches_host, m.data(), m.size() * sizeof(int));
    if (!ur.empty()) memcpy(un_rows_host, ur.data(), ur.size() * sizeof(int));
    if (!ud.empty()) memcpy(un_dets_host, ud.data(), ud.size() * sizeof(int));
    return DD_OK;
}

}  // extern "C"
