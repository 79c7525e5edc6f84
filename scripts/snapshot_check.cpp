// Stand-alone check of the stream-snapshot blob (deepdish_amd/csrc/snapshot_fmt.h: writer, parser, validator -- no HIP), built with
// -fsanitize=address,undefined by tests/test_snapshot_host.py.  Blobs are written from plain structs: 0 tracks; galleries of 0, 1, 31, 32,
// 33, 64 and 65 rows; a budget ring that has wrapped; deleted tracks with paths; with and without a background section; several entries.
// Every blob must parse and write back to the same bytes.  Then two blobs are cut at every byte length and 3 000 seeded single-byte
// replacements are applied: every damaged blob, held in an allocation of exactly its length, must be refused or validate to a state
// whose every index is in range (re-checked here, touching every byte of the bulk sections), and never be read out of bounds.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/snapshot_check.cpp -o snapshot_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include "../deepdish_amd/csrc/snapshot_fmt.h"

using namespace ddsnap;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "ERROR %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_fail; } } while (0)

// the memory the bulk pointers of a hand-made entry point into
struct Backing { std::vector<float> gallery, ret; std::vector<uint8_t> bg; };

static Track make_track(std::mt19937 &rng, int64_t id, int state, int budget, int total, int n_det) {
    Track t;
    t.id = id; t.state = state; t.tsu = (int)(rng() % 4); t.hits = 1 + (int)(rng() % 50); t.age = t.hits + (int)(rng() % 9);
    t.last_det = n_det > 0 && state != 3 && rng() % 2 ? (int)(rng() % n_det) : -1;
    t.slot_total = total; t.n_rows = budget > 0 ? std::min(total, budget) : total;
    for (double &v : t.mean) v = (double)(rng() % 10000) / 7.0;
    for (double &v : t.cov) v = (double)(rng() % 1000) / 13.0;
    return t;
}

static Entry make_entry(std::mt19937 &rng, Backing &mem, const std::vector<int> &live_rows, int n_dead, int budget, bool paths, bool bg, bool skip, int n_ret) {
    Entry e;
    Params &p = e.par;
    p.H = 4; p.W = 6; p.metric = 0; p.nn_budget = budget; p.det_kind = 0; p.max_det = 10; p.n_labels = 91; p.label_offset = 1;
    p.labels_hash = 0x1234567890abcdefull;
    p.line[0] = 3; p.line[1] = 0; p.line[2] = 3; p.line[3] = 4;
    p.max_age = 5; p.n_init = 3; p.max_cos = 0.2; p.max_iou = 0.7; p.nms = 0.6;
    if (bg) { p.mog_on = 1; p.ratio = 0.25; p.masking = 0; p.mog_history = 500; p.mog_shadows = 1; p.mog_var_thr = 16.f; }
    if (skip) { p.skip_form = 1; p.skip_n = 2; p.skip_phase = 1; }
    p.wanted = {"person", "bicycle"};
    e.counts = {3, 1, 4, 0, 0, 2, 2, 1};
    e.seen = 37; e.rem = skip ? 1 : 0; e.has = 1; e.last = skip;
    const int n_det = 3;
    e.det_cls = {0, 1, 0}; e.det_conf = {0.9, 0.8, 0.7}; e.det_tlwh.assign(12, 5.0);
    e.boxes0.assign(8, 2.0); e.scores0 = {0.5, 0.6}; e.cls0 = {0, 3};
    int64_t id = 1;
    for (int rows : live_rows) e.tracks.push_back(make_track(rng, id++, 1 + (int)(rng() % 2), budget, budget > 0 ? rows + 2 * budget : rows, n_det));
    for (int k = 0; k < n_dead; ++k) e.tracks.push_back(make_track(rng, id++, 3, budget, 7, n_det));
    e.n_live = (int)live_rows.size(); e.n_dead = n_dead;
    e.next_id = id + 2;
    if (paths)
        for (const Track &t : e.tracks) {
            Path q;
            q.id = t.id;
            for (int k = 0; k < 1 + (int)(t.id % 4); ++k) { q.xy.push_back(10.0 * k); q.xy.push_back(3.5 + k); }
            e.paths.push_back(q);
            if (t.state != 3) {
                Vote v;
                v.id = t.id; v.cls = {0, 1}; v.cnt = {4, 1}; v.sum = {3.2, 0.6};
                e.votes.push_back(v);
            }
        }
    for (const Track &t : e.tracks) e.gallery_rows += (uint64_t)t.n_rows;
    mem.gallery.resize((size_t)e.gallery_rows * FEAT);
    for (float &v : mem.gallery) v = (float)(rng() % 2000) / 1000.f - 1.f;
    e.gallery = reinterpret_cast<const uint8_t *>(mem.gallery.data());
    e.n_ret = skip ? n_ret : 0;
    mem.ret.assign((size_t)e.n_ret * FEAT, 0.25f);
    e.ret_rows = reinterpret_cast<const uint8_t *>(mem.ret.data());
    if (bg) {
        e.has_bg = 1; e.nframes = 36;
        mem.bg.resize((size_t)e.bg_bytes());
        for (uint8_t &v : mem.bg) v = (uint8_t)(rng() % 256);
        const size_t hw = (size_t)p.H * p.W;
        for (size_t i = 0; i < hw; ++i) mem.bg[hw * NMIX * 20 + i] = (uint8_t)(rng() % (NMIX + 1));
        e.bg = mem.bg.data();
    }
    return e;
}

static std::vector<uint8_t> make_blob(const std::vector<Entry> &es) {
    std::vector<uint64_t> sizes;
    uint64_t total = header_bytes((uint32_t)es.size());
    for (const Entry &e : es) { sizes.push_back(write_entry(e, nullptr)); total += sizes.back(); }
    std::vector<uint8_t> b((size_t)total);
    write_header(b.data(), sizes);
    uint64_t at = header_bytes((uint32_t)es.size());
    for (size_t i = 0; i < es.size(); ++i) { write_entry(es[i], b.data() + at); at += sizes[i]; }
    return b;
}

// what restore relies on, asserted independently of parse_entry; touches every byte of the bulk sections
static uint64_t in_range(const Entry &e) {
    const Params &p = e.par;
    const auto cls_ok = [&](int c) { return c >= 0 && c + p.label_offset < p.n_labels; };
    CHECK(e.counts.size() == p.wanted.size() * 4, "counts");
    const int nd = (int)e.det_cls.size();
    CHECK(e.det_conf.size() == (size_t)nd && e.det_tlwh.size() == (size_t)nd * 4, "detections");
    CHECK(e.boxes0.size() == e.cls0.size() * 4 && e.scores0.size() == e.cls0.size(), "adaptor output");
    for (int c : e.det_cls) CHECK(cls_ok(c), "det class");
    for (int c : e.cls0) CHECK(cls_ok(c), "adaptor class");
    CHECK(e.tracks.size() == (size_t)e.n_live + (size_t)e.n_dead, "track count");
    uint64_t rows = 0;
    for (size_t i = 0; i < e.tracks.size(); ++i) {
        const Track &t = e.tracks[i];
        CHECK(t.id >= 1 && t.id < e.next_id, "track id");
        CHECK(i < (size_t)e.n_live ? (t.state == 1 || t.state == 2) : t.state == 3, "state");
        CHECK(t.tsu >= 0 && t.hits >= 0 && t.age >= 0 && t.last_det >= -1 && t.last_det < nd, "track counters");
        CHECK(t.n_rows >= 0 && t.n_rows <= t.slot_total && (p.nn_budget == 0 || t.n_rows <= p.nn_budget), "gallery rows");
        for (size_t k = 0; k < i; ++k) CHECK(e.tracks[k].id != t.id, "duplicate id");
        for (double v : t.mean) CHECK(std::isfinite(v), "mean");
        for (double v : t.cov) CHECK(std::isfinite(v), "cov");
        rows += (uint64_t)t.n_rows;
    }
    CHECK(rows == e.gallery_rows, "gallery section");
    for (const Vote &v : e.votes) for (int c : v.cls) CHECK(cls_ok(c), "vote class");
    CHECK(e.rem >= 0 && e.rem <= p.skip_n && e.has <= 1 && e.last <= 1, "skip counter");
    uint64_t sum = 0;
    for (uint64_t i = 0; i < e.gallery_rows * ROW_BYTES; ++i) sum += e.gallery[i];
    for (uint64_t i = 0; i < (uint64_t)e.n_ret * ROW_BYTES; ++i) sum += e.ret_rows[i];
    if (e.has_bg) {
        for (uint64_t i = 0; i < e.bg_bytes(); ++i) sum += e.bg[i];
        const uint64_t hw = (uint64_t)p.H * p.W;
        for (uint64_t i = 0; i < hw; ++i) CHECK(e.bg[hw * NMIX * 20 + i] <= NMIX, "mode count");
    }
    return sum;
}

// parse a blob held in an allocation of exactly n bytes -> accepted?
static bool try_blob(const uint8_t *src, size_t n, uint64_t *sink) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) memcpy(exact.get(), src, n);
    std::vector<Entry> es;
    std::vector<std::pair<uint64_t, uint64_t>> table;
    std::string err;
    if (!parse_blob(exact.get(), n, es, table, err)) return false;
    for (const Entry &e : es) *sink += in_range(e);
    return true;
}

int main() {
    std::mt19937 rng(20240611);
    std::vector<Backing> mem(8);
    std::vector<std::vector<Entry>> cases;
    cases.push_back({make_entry(rng, mem[0], {}, 0, 0, false, false, false, 0)});                              // 0 tracks
    cases.push_back({make_entry(rng, mem[1], {0, 1, 31, 32, 33, 64, 65}, 0, 0, true, false, false, 0)});       // gallery sizes around the chunk
    cases.push_back({make_entry(rng, mem[2], {5, 9}, 0, 40, true, false, true, 3)});                           // a budget ring that has wrapped
    cases.push_back({make_entry(rng, mem[3], {33, 2}, 2, 0, true, false, false, 0)});                          // deleted tracks with paths
    cases.push_back({make_entry(rng, mem[4], {33, 2}, 1, 0, true, true, true, 2)});                            // with a background section
    cases.push_back({cases[0][0], cases[3][0], cases[4][0]});                                                  // three entries
    std::vector<std::vector<uint8_t>> blobs;
    uint64_t sink = 0;
    for (const auto &c : cases) {
        blobs.push_back(make_blob(c));
        const std::vector<uint8_t> &b = blobs.back();
        std::vector<Entry> es;
        std::vector<std::pair<uint64_t, uint64_t>> table;
        std::string err;
        const bool ok = parse_blob(b.data(), b.size(), es, table, err);
        CHECK(ok, "a valid blob is refused: %s", err.c_str());
        if (!ok) continue;
        CHECK(es.size() == c.size(), "entry count");
        for (const Entry &e : es) sink += in_range(e);
        const std::vector<uint8_t> again = make_blob(es);
        CHECK(again == b, "parse -> write does not give the same bytes (%zu vs %zu)", again.size(), b.size());
        CHECK(es[0].tracks.size() == c[0].tracks.size() && es[0].gallery_rows == c[0].gallery_rows, "tracks lost");
    }
    // cut two blobs at every byte length: only the whole blob may be accepted
    long cut_accepted = 0, cut_refused = 0;
    for (int k : {3, 4}) {
        const std::vector<uint8_t> &b = blobs[(size_t)k];
        for (size_t n = 0; n < b.size(); ++n) (try_blob(b.data(), n, &sink) ? cut_accepted : cut_refused) += 1;
    }
    CHECK(cut_accepted == 0, "%ld cut blobs were accepted", cut_accepted);
    // 3 000 seeded single-byte replacements in the one-entry blobs with galleries, a third each: in the blob's header and entry table,
    // where every byte is checked (magic, version, count, the entry's offset and length: all must be refused); in the gallery rows,
    // which are data the pipeline may hold any value of (no checksum: all must be accepted); anywhere
    long rep_accepted = 0, rep_refused = 0, head_refused = 0, gallery_accepted = 0;
    for (int i = 0; i < 3000; ++i) {
        const size_t k = (size_t)(1 + i % 4);
        std::vector<uint8_t> b = blobs[k];
        uint64_t off[3] = {0, 0, 0};
        write_entry(cases[k][0], nullptr, off);
        const size_t head = (size_t)header_bytes(1), gal = head + (size_t)off[0], gal_bytes = (size_t)cases[k][0].gallery_rows * ROW_BYTES;
        const int cls = i / 4 % 3;
        const size_t at = cls == 0 ? rng() % head : cls == 1 ? gal + rng() % gal_bytes : rng() % b.size();
        uint8_t v = (uint8_t)(rng() % 256);
        if (v == b[at]) v ^= 0x80;
        b[at] = v;
        const bool ok = try_blob(b.data(), b.size(), &sink);
        (ok ? rep_accepted : rep_refused) += 1;
        head_refused += cls == 0 && !ok;
        gallery_accepted += cls == 1 && ok;
    }
    printf("%zu blobs round-trip; %ld cut blobs refused, %ld accepted; %ld replacements refused, %ld accepted; %ld of 1000 in the header refused, "
           "%ld of 1000 in the galleries accepted (checksum %llu)\n", blobs.size(), cut_refused, cut_accepted, rep_refused, rep_accepted, head_refused,
           gallery_accepted, (unsigned long long)sink);
    if (g_fail) { fprintf(stderr, "ERROR: %d checks failed\n", g_fail); return 1; }
    return 0;
}
