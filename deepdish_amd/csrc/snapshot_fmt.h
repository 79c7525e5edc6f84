// The stream-snapshot blob (dd_pipeline_snapshot / dd_pipeline_restore): writer, parser and validator.  Host only, no HIP: the pipeline
// (csrc/pipeline.hip) and the stand-alone check (scripts/snapshot_check.cpp, built with -fsanitize=address,undefined by
// tests/test_snapshot_host.py) compile the same statements.
//
// Little-endian.  Blob = {magic u32, version u32, n_entries u32, 0 u32} {offset u64, bytes u64} x n_entries, then the entries behind one
// another in table order without gaps, the last one ending the blob.  An entry is self-contained (select = copy its bytes):
//   parameters of the source stream (checked by restore, never applied) | counts by wanted label name | frame number, next id, skip counter |
//   the last step's detections | the retained adaptor output | tracks (live, then deleted) with mean and covariance | paths | votes |
//   gallery rows of every track in track order, each gallery in STORAGE order | retained encoder rows | background (optional).
// There is no checksum: the validator is the defence.  Every read is bounds-checked against the length; parse_entry accepts an entry only
// when every count, id, state, class id and index in it is in range, so that what restore then does with it stays inside its buffers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ddsnap {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the blob is little-endian and written with memcpy");

constexpr uint32_t MAGIC = 0x4E534444u;        // "DDSN"
constexpr uint32_t VERSION = 1;
constexpr int FEAT = 128, ROW_BYTES = FEAT * 4, NMIX = 5;
constexpr int64_t BG_BYTES_PER_PIXEL = NMIX * 16 + NMIX * 4 + 1 + 1;      // rec float4 x5, m2 f32 x5, nm u8, motion mask u8
constexpr int32_t MAX_COUNT = 1 << 24;         // no table of a stream is longer (a bound on what a damaged count may make us allocate)

inline uint64_t fnv1a(const void *data, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const uint8_t *p = static_cast<const uint8_t *>(data);
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

struct Params {
    int32_t H = 0, W = 0, feat_len = FEAT, metric = 0, nn_budget = 0, det_kind = 0, max_det = 0, n_labels = 0, label_offset = 0;
    uint64_t labels_hash = 0;                  // FNV-1a of the label lines, each followed by '\n'
    double line[4] = {0, 0, 0, 0};
    int32_t max_age = 0, n_init = 0;
    double max_cos = 0, max_iou = 0, nms = 0, ratio = -1.0;
    int32_t masking = 0, mog_on = 0, mog_history = 0, mog_shadows = 0;
    float mog_var_thr = 0.f;
    int32_t skip_form = 0, skip_n = 0, skip_phase = -1;      // form 0: no per-stream counter (N = 0), 1: one per stream
    std::vector<std::string> wanted;           // the stream's own wanted labels
};

struct Track {
    int64_t id = 0;
    int32_t state = 0, tsu = 0, hits = 0, age = 0, last_det = -1, slot_total = 0, n_rows = 0;
    double mean[8] = {}, cov[64] = {};
};
struct Path { int64_t id = 0; std::vector<double> xy; };
struct Vote { int64_t id = 0; std::vector<int32_t> cls, cnt; std::vector<double> sum; };

struct Entry {
    Params par;
    std::vector<int64_t> counts;               // [par.wanted.size()][4]
    int64_t seen = 0, next_id = 1;
    int32_t rem = 0;
    uint8_t has = 0, last = 0;
    std::vector<int32_t> det_cls;
    std::vector<double> det_conf, det_tlwh;
    std::vector<double> boxes0, scores0;
    std::vector<int32_t> cls0;
    int32_t n_live = 0, n_dead = 0;
    std::vector<Track> tracks;                 // n_live live tracks, then n_dead deleted ones
    std::vector<Path> paths;                   // ascending id
    std::vector<Vote> votes;                   // ascending id
    // bulk sections: views into the blob (parse) or into the caller's memory (write)
    const uint8_t *gallery = nullptr;          // gallery_rows x 128 f32
    uint64_t gallery_rows = 0;
    const uint8_t *ret_rows = nullptr;         // n_ret x 128 f32
    int32_t n_ret = 0;
    uint8_t has_bg = 0;
    int64_t nframes = 0;
    const uint8_t *bg = nullptr;               // H W x BG_BYTES_PER_PIXEL: rec, m2, nm, motion mask planes
    uint64_t bg_bytes() const { return has_bg ? (uint64_t)par.H * (uint64_t)par.W * (uint64_t)BG_BYTES_PER_PIXEL : 0; }
};

// ---------------------------------------------------------------- writer (out == nullptr: count only)
struct Wr {
    uint8_t *out;
    uint64_t o = 0;
    void put(const void *src, uint64_t n) { if (out && n) memcpy(out + o, src, n); o += n; }
    template <class T> void val(T v) { put(&v, sizeof v); }
    template <class T> void vec(const std::vector<T> &v) { put(v.data(), v.size() * sizeof(T)); }
};

// -> the entry's bytes.  bulk_off (may be NULL): where its gallery, retained-row and background sections begin, from the entry's start.
inline uint64_t write_entry(const Entry &e, uint8_t *out, uint64_t *bulk_off = nullptr) {
    Wr w{out};
    const Params &p = e.par;
    for (int32_t v : {p.H, p.W, p.feat_len, p.metric, p.nn_budget, p.det_kind, p.max_det, p.n_labels, p.label_offset}) w.val(v);
    w.val(p.labels_hash);
    w.put(p.line, sizeof p.line);
    w.val(p.max_age); w.val(p.n_init);
    w.val(p.max_cos); w.val(p.max_iou); w.val(p.nms); w.val(p.ratio);
    w.val(p.masking); w.val(p.mog_on); w.val(p.mog_history); w.val(p.mog_shadows); w.val(p.mog_var_thr);
    w.val(p.skip_form); w.val(p.skip_n); w.val(p.skip_phase);
    w.val((int32_t)p.wanted.size());
    for (const std::string &s : p.wanted) { w.val((uint16_t)s.size()); w.put(s.data(), s.size()); }
    w.vec(e.counts);
    w.val(e.seen); w.val(e.next_id); w.val(e.rem); w.val(e.has); w.val(e.last);
    w.val((int32_t)e.det_cls.size()); w.vec(e.det_cls); w.vec(e.det_conf); w.vec(e.det_tlwh);
    w.val((int32_t)e.cls0.size()); w.vec(e.boxes0); w.vec(e.scores0); w.vec(e.cls0);
    w.val(e.n_live); w.val(e.n_dead);
    for (const Track &t : e.tracks) {
        w.val(t.id);
        for (int32_t v : {t.state, t.tsu, t.hits, t.age, t.last_det, t.slot_total, t.n_rows}) w.val(v);
        w.put(t.mean, sizeof t.mean); w.put(t.cov, sizeof t.cov);
    }
    w.val((int32_t)e.paths.size());
    for (const Path &q : e.paths) { w.val(q.id); w.val((int32_t)(q.xy.size() / 2)); w.vec(q.xy); }
    w.val((int32_t)e.votes.size());
    for (const Vote &v : e.votes) { w.val(v.id); w.val((int32_t)v.cls.size()); w.vec(v.cls); w.vec(v.cnt); w.vec(v.sum); }
    // a bulk section whose pointer is NULL is left for the caller to fill (the pipeline copies it there straight from the device)
    const auto bulk = [&](const uint8_t *src, uint64_t n, int which) {
        if (bulk_off) bulk_off[which] = w.o;
        if (out && src) w.put(src, n); else w.o += n;
    };
    w.val((uint64_t)e.gallery_rows);
    bulk(e.gallery, e.gallery_rows * ROW_BYTES, 0);
    w.val(e.n_ret);
    bulk(e.ret_rows, (uint64_t)e.n_ret * ROW_BYTES, 1);
    w.val(e.has_bg);
    if (e.has_bg) {
        w.val(e.nframes);
        bulk(e.bg, e.bg_bytes(), 2);
    }
    return w.o;
}

inline uint64_t header_bytes(uint32_t n_entries) { return 16 + (uint64_t)n_entries * 16; }

// sizes[i] = bytes of entry i; the entries follow the table without gaps
inline void write_header(uint8_t *out, const std::vector<uint64_t> &sizes) {
    Wr w{out};
    w.val(MAGIC); w.val(VERSION); w.val((uint32_t)sizes.size()); w.val((uint32_t)0);
    uint64_t at = header_bytes((uint32_t)sizes.size());
    for (uint64_t s : sizes) { w.val(at); w.val(s); at += s; }
}

// ---------------------------------------------------------------- parser + validator
struct Rd {
    const uint8_t *p;
    uint64_t n, o = 0;
    bool ok = true;
    bool take(void *dst, uint64_t k) {
        if (!ok || k > n - o) { ok = false; return false; }
        if (k) memcpy(dst, p + o, k);
        o += k;
        return true;
    }
    template <class T> T val() { T v{}; take(&v, sizeof v); return v; }
    const uint8_t *span(uint64_t k) {
        if (!ok || k > n - o) { ok = false; return nullptr; }
        const uint8_t *q = p + o;
        o += k;
        return q;
    }
    // count elements of `each` bytes: refused unless 0 <= count <= MAX_COUNT and they fit into what is left
    template <class T> bool vec(std::vector<T> &v, int64_t count, int per = 1) {
        if (!ok || count < 0 || count > MAX_COUNT || (uint64_t)count * per * sizeof(T) > n - o) { ok = false; return false; }
        v.resize((size_t)count * per);
        return take(v.data(), v.size() * sizeof(T));
    }
};

#define DDSNAP_NEED(cond, what) do { if (!(cond)) { err = (what); return false; } } while (0)

inline bool all_finite(const double *v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// One entry occupying exactly [data, data + n).  On success every index the pipeline will follow is in range.
inline bool parse_entry(const uint8_t *data, uint64_t n, Entry &e, std::string &err) {
    Rd r{data, n};
    e = Entry();
    Params &p = e.par;
    for (int32_t *v : {&p.H, &p.W, &p.feat_len, &p.metric, &p.nn_budget, &p.det_kind, &p.max_det, &p.n_labels, &p.label_offset}) *v = r.val<int32_t>();
    p.labels_hash = r.val<uint64_t>();
    r.take(p.line, sizeof p.line);
    p.max_age = r.val<int32_t>(); p.n_init = r.val<int32_t>();
    p.max_cos = r.val<double>(); p.max_iou = r.val<double>(); p.nms = r.val<double>(); p.ratio = r.val<double>();
    p.masking = r.val<int32_t>(); p.mog_on = r.val<int32_t>(); p.mog_history = r.val<int32_t>(); p.mog_shadows = r.val<int32_t>();
    p.mog_var_thr = r.val<float>();
    p.skip_form = r.val<int32_t>(); p.skip_n = r.val<int32_t>(); p.skip_phase = r.val<int32_t>();
    DDSNAP_NEED(r.ok, "truncated parameters");
    DDSNAP_NEED(p.H >= 1 && p.H <= 16384 && p.W >= 1 && p.W <= 16384, "frame size out of range");
    DDSNAP_NEED(p.feat_len == FEAT, "feature length is not 128");
    DDSNAP_NEED(p.metric == 0 || p.metric == 1, "metric out of range");
    DDSNAP_NEED(p.nn_budget >= 0, "negative nn_budget");
    DDSNAP_NEED(p.det_kind >= 0 && p.det_kind <= 2, "detector kind out of range");
    DDSNAP_NEED(p.max_det >= 1 && p.max_det <= 64, "max_det out of range");
    DDSNAP_NEED(p.n_labels >= 0 && p.n_labels <= MAX_COUNT && (p.label_offset == 0 || p.label_offset == 1), "label list out of range");
    DDSNAP_NEED(all_finite(p.line, 4), "line is not finite");
    DDSNAP_NEED(p.max_age >= 0 && p.n_init >= 0, "negative max_age or n_init");
    DDSNAP_NEED(std::isfinite(p.max_cos) && p.max_cos >= 0 && std::isfinite(p.max_iou) && p.max_iou >= 0 && std::isfinite(p.nms), "tracker distances are not finite");
    DDSNAP_NEED((p.masking | 1) == 1 && (p.mog_on | 1) == 1 && (p.mog_shadows | 1) == 1, "a flag is not 0 or 1");
    DDSNAP_NEED(p.mog_on ? (p.ratio >= 0 && p.ratio <= 1 && p.mog_history >= 1 && std::isfinite(p.mog_var_thr))
                         : (p.ratio == -1.0 && p.masking == 0 && p.mog_history == 0 && p.mog_shadows == 0 && p.mog_var_thr == 0.f), "background settings out of range");
    DDSNAP_NEED((p.skip_form == 0 && p.skip_n == 0 && p.skip_phase == -1) || (p.skip_form == 1 && p.skip_n >= 0 && p.skip_phase >= -1 && p.skip_phase <= p.skip_n),
                "skip N or phase out of range");
    const int32_t nw = r.val<int32_t>();
    DDSNAP_NEED(r.ok && nw >= 0 && nw <= 4096, "wanted label count out of range");
    for (int32_t i = 0; i < nw; ++i) {
        const uint16_t len = r.val<uint16_t>();
        const uint8_t *s = r.span(len);
        DDSNAP_NEED(r.ok && len <= 255, "wanted label out of range");
        p.wanted.emplace_back(reinterpret_cast<const char *>(s), len);
        DDSNAP_NEED(p.wanted.back().find('\n') == std::string::npos && p.wanted.back().find('\0') == std::string::npos, "wanted label holds a separator");
        for (int32_t k = 0; k < i; ++k) DDSNAP_NEED(p.wanted[k] != p.wanted[i], "wanted label listed twice");
    }
    DDSNAP_NEED(r.vec(e.counts, nw, 4), "truncated counts");
    for (int64_t c : e.counts) DDSNAP_NEED(c >= 0, "negative count");
    e.seen = r.val<int64_t>(); e.next_id = r.val<int64_t>(); e.rem = r.val<int32_t>(); e.has = r.val<uint8_t>(); e.last = r.val<uint8_t>();
    DDSNAP_NEED(r.ok && e.seen >= 0 && e.next_id >= 1, "frame number or next id out of range");
    DDSNAP_NEED(e.rem >= 0 && e.rem <= p.skip_n && e.has <= 1 && e.last <= 1, "skip counter out of range");
    const auto cls_ok = [&](int32_t c) { return c >= 0 && (int64_t)c + p.label_offset < (int64_t)p.n_labels; };
    const int32_t nd = r.val<int32_t>();
    DDSNAP_NEED(r.vec(e.det_cls, nd) && r.vec(e.det_conf, nd) && r.vec(e.det_tlwh, nd, 4), "truncated detections");
    for (int32_t c : e.det_cls) DDSNAP_NEED(cls_ok(c), "detection class outside the label list");
    const int32_t n0 = r.val<int32_t>();
    DDSNAP_NEED(r.vec(e.boxes0, n0, 4) && r.vec(e.scores0, n0) && r.vec(e.cls0, n0), "truncated adaptor output");
    for (int32_t c : e.cls0) DDSNAP_NEED(cls_ok(c), "adaptor class outside the label list");
    e.n_live = r.val<int32_t>(); e.n_dead = r.val<int32_t>();
    DDSNAP_NEED(r.ok && e.n_live >= 0 && e.n_dead >= 0 && e.n_live <= MAX_COUNT && e.n_dead <= MAX_COUNT, "track counts out of range");
    const uint64_t nt = (uint64_t)e.n_live + (uint64_t)e.n_dead, track_bytes = 8 + 7 * 4 + 72 * 8;
    DDSNAP_NEED(nt * track_bytes <= r.n - r.o, "truncated tracks");
    e.tracks.resize((size_t)nt);
    uint64_t rows = 0;
    for (uint64_t i = 0; i < nt; ++i) {
        Track &t = e.tracks[(size_t)i];
        t.id = r.val<int64_t>();
        for (int32_t *v : {&t.state, &t.tsu, &t.hits, &t.age, &t.last_det, &t.slot_total, &t.n_rows}) *v = r.val<int32_t>();
        r.take(t.mean, sizeof t.mean); r.take(t.cov, sizeof t.cov);
        DDSNAP_NEED(r.ok, "truncated tracks");
        DDSNAP_NEED(t.id >= 1 && t.id < e.next_id, "track id outside 1 .. next id - 1");
        DDSNAP_NEED(i < (uint64_t)e.n_live ? (t.state == 1 || t.state == 2) : t.state == 3, "track state out of range");
        DDSNAP_NEED(t.tsu >= 0 && t.hits >= 0 && t.age >= 0, "negative track counter");
        DDSNAP_NEED(t.last_det >= -1 && t.last_det < nd, "track's detection outside the detections");
        DDSNAP_NEED(t.slot_total >= 0 && t.n_rows == (p.nn_budget > 0 ? std::min(t.slot_total, p.nn_budget) : t.slot_total),
                    "gallery rows do not match the sample count and the budget");
        DDSNAP_NEED(all_finite(t.mean, 8) && all_finite(t.cov, 64), "track mean or covariance is not finite");
        rows += (uint64_t)t.n_rows;
    }
    {
        std::vector<int64_t> ids(e.tracks.size());
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = e.tracks[i].id;
        std::sort(ids.begin(), ids.end());
        DDSNAP_NEED(std::adjacent_find(ids.begin(), ids.end()) == ids.end(), "track id listed twice");
    }
    const int32_t np = r.val<int32_t>();
    DDSNAP_NEED(r.ok && np >= 0 && (uint64_t)np * 12 <= r.n - r.o, "path count out of range");
    e.paths.resize((size_t)np);
    for (int32_t i = 0; i < np; ++i) {
        Path &q = e.paths[(size_t)i];
        q.id = r.val<int64_t>();
        const int32_t k = r.val<int32_t>();
        DDSNAP_NEED(r.vec(q.xy, k, 2), "truncated path");
        DDSNAP_NEED(q.id >= 1 && q.id < e.next_id && (i == 0 || q.id > e.paths[(size_t)i - 1].id), "path ids out of range or out of order");
        DDSNAP_NEED(k >= 1 && all_finite(q.xy.data(), q.xy.size()), "path is empty or not finite");
    }
    const int32_t nv = r.val<int32_t>();
    DDSNAP_NEED(r.ok && nv >= 0 && (uint64_t)nv * 12 <= r.n - r.o, "vote count out of range");
    e.votes.resize((size_t)nv);
    for (int32_t i = 0; i < nv; ++i) {
        Vote &v = e.votes[(size_t)i];
        v.id = r.val<int64_t>();
        const int32_t k = r.val<int32_t>();
        DDSNAP_NEED(r.vec(v.cls, k) && r.vec(v.cnt, k) && r.vec(v.sum, k), "truncated votes");
        DDSNAP_NEED(v.id >= 1 && v.id < e.next_id && (i == 0 || v.id > e.votes[(size_t)i - 1].id), "vote ids out of range or out of order");
        DDSNAP_NEED(k >= 1 && all_finite(v.sum.data(), v.sum.size()), "votes are empty or not finite");
        for (int32_t j = 0; j < k; ++j) {
            DDSNAP_NEED(cls_ok(v.cls[(size_t)j]) && v.cnt[(size_t)j] >= 1, "vote class or count out of range");
            for (int32_t j2 = 0; j2 < j; ++j2) DDSNAP_NEED(v.cls[(size_t)j2] != v.cls[(size_t)j], "vote class listed twice");
        }
    }
    e.gallery_rows = r.val<uint64_t>();
    DDSNAP_NEED(r.ok && e.gallery_rows == rows, "gallery section does not match the tracks' row counts");
    DDSNAP_NEED(e.gallery_rows <= (r.n - r.o) / ROW_BYTES, "truncated gallery");
    e.gallery = r.span(e.gallery_rows * ROW_BYTES);
    e.n_ret = r.val<int32_t>();
    DDSNAP_NEED(r.ok && e.n_ret >= 0 && (uint64_t)e.n_ret <= (r.n - r.o) / ROW_BYTES, "retained rows out of range");
    DDSNAP_NEED(p.skip_form == 1 || e.n_ret == 0, "retained rows without a per-stream skip counter");
    e.ret_rows = r.span((uint64_t)e.n_ret * ROW_BYTES);
    e.has_bg = r.val<uint8_t>();
    DDSNAP_NEED(r.ok && e.has_bg <= 1 && (!e.has_bg || p.mog_on), "background flag out of range");
    if (e.has_bg) {
        e.nframes = r.val<int64_t>();
        DDSNAP_NEED(r.ok && e.nframes >= 0, "negative background frame count");
        e.bg = r.span(e.bg_bytes());
        DDSNAP_NEED(r.ok, "truncated background");
        const uint64_t hw = (uint64_t)p.H * p.W;
        const uint8_t *nm = e.bg + hw * (NMIX * 20);
        for (uint64_t i = 0; i < hw; ++i) DDSNAP_NEED(nm[i] <= NMIX, "background mode count above 5");
    }
    DDSNAP_NEED(r.ok && r.o == r.n, "entry length does not match its contents");
    return true;
}

// The blob's entry table -> (offset, bytes) per entry; every entry lies inside the blob, in order, without gaps.
inline bool parse_table(const uint8_t *data, uint64_t n, std::vector<std::pair<uint64_t, uint64_t>> &table, std::string &err) {
    Rd r{data, n};
    table.clear();
    const uint32_t magic = r.val<uint32_t>(), version = r.val<uint32_t>(), ne = r.val<uint32_t>(), zero = r.val<uint32_t>();
    DDSNAP_NEED(r.ok && magic == MAGIC, "not a stream snapshot (magic)");
    DDSNAP_NEED(version == VERSION && zero == 0, "unknown snapshot version");
    DDSNAP_NEED((uint64_t)ne * 16 <= n - r.o, "entry table longer than the blob");
    uint64_t at = header_bytes(ne);
    for (uint32_t i = 0; i < ne; ++i) {
        const uint64_t off = r.val<uint64_t>(), len = r.val<uint64_t>();
        DDSNAP_NEED(r.ok && off == at && len <= n - at, "entry table does not match the blob");
        table.emplace_back(off, len);
        at += len;
    }
    DDSNAP_NEED(at == n, "blob length does not match its entry table");
    return true;
}

inline bool parse_blob(const uint8_t *data, uint64_t n, std::vector<Entry> &entries, std::vector<std::pair<uint64_t, uint64_t>> &table, std::string &err) {
    entries.clear();
    if (!parse_table(data, n, table, err)) return false;
    entries.resize(table.size());
    for (size_t i = 0; i < table.size(); ++i)
        if (!parse_entry(data + table[i].first, table[i].second, entries[i], err)) { err = "entry " + std::to_string(i) + ": " + err; return false; }
    return true;
}

}  // namespace ddsnap
