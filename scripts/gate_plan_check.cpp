// Host check of the motion gate's index arithmetic (csrc/host_phases.h: plan_skip, gate_streams, GateStats, pair_counts,
// feature_row_table), as a stand-alone program: tests/test_motion_gate_host.py builds it with -fsanitize=address,undefined and runs it on
// the CPU.  A few thousand seeded sequences of steps, driven as dd_pipeline_step3 drives them -- plan, gate, pairing counts, feature-row
// table, commit -- over presence lists (empty ones and full ones among them), foreground counts (at, below and above the threshold; steps
// with every stream gated and with none) and thresholds, S = 1 .. 9.  After every step dl, the gated flags, the row offsets, the store of
// retained rows and the statistics are held to a direct restatement per stream: a stream is gated iff it is present and its count is at
// most its threshold; a gated stream brings no tracker row, no encoder row and retains none.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../deepdish_amd/csrc/host_phases.h"

struct Rng { unsigned long long s; unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); } };

static long long g_checks = 0, g_bad = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_bad <= 20) { printf("MISMATCH %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static long long g_steps = 0, g_gated = 0, g_all_gated = 0, g_none_gated = 0, g_empty = 0;

static void one_sequence(unsigned seed) {
    Rng r{seed * 2654435761ull + 17};
    const int S = 1 + (int)(seed % 9), F = 4 + (int)(r.next() % 9);
    const bool per_stream_store = r.next() % 2;             // the store of retained rows (dd_pipeline_detector_skip_streams with every N = 0)
    std::vector<int> thr(S);
    for (int &t : thr) { const unsigned k = r.next() % 4; t = k == 0 ? 0 : k == 1 ? (int)(r.next() % 8) : k == 2 ? (int)(r.next() % 3000) : 1000000; }
    ddhost::SkipCounters sk;
    sk.start(S, 0);                                         // the gate goes with N = 0 only
    ddhost::GateStats gs;
    gs.start(S);
    ddhost::StepPlan pl;
    std::vector<int> doff, eoff, table, ret_off(S, 0), ret_n(S, 0), ret_off_new, ret_n_new;
    // the restatement's state
    long long want_steps = 0, want_gated = 0;
    std::vector<int> want_last(S, -1), want_flag(S, 0), held(S, 0);
    for (int f = 0; f < F; ++f) {
        const unsigned pm = r.next() % 6, cm = r.next() % 6;   // presence: 0 none, 1 all, else random; counts: 0 all gated, 1 none gated, else mixed
        std::vector<uint8_t> present(S), present_next(S);
        for (int z = 0; z < S; ++z) { present[z] = pm == 0 ? 0 : pm == 1 ? 1 : r.next() % 3 != 0; present_next[z] = r.next() % 2; }
        pl.act.clear(); pl.act_next.clear();
        for (int z = 0; z < S; ++z) { if (present[z]) pl.act.push_back(z); if (present_next[z]) pl.act_next.push_back(z); }
        ddhost::plan_skip(sk, pl);
        CHECK(pl.dl == pl.act, "seed %u step %d: N = 0, every present stream is on a detector step", seed, f);
        CHECK(pl.gat.size() == pl.act.size() && pl.dl_elig.empty(), "seed %u step %d: the plan starts ungated", seed, f);
        std::vector<int> count_of(S, -1), counts;
        for (int z : pl.dl) {
            const unsigned k = r.next() % 5;
            int c = cm == 0 ? (thr[z] ? (int)(r.next() % (unsigned)(thr[z] + 1)) : 0) : cm == 1 ? thr[z] + 1 + (int)(r.next() % 50)
                    : k == 0 ? 0 : k == 1 ? thr[z] : k == 2 ? thr[z] + 1 : (int)(r.next() % 4000);
            count_of[z] = c;
            counts.push_back(c);
        }
        const std::vector<int> elig = pl.dl;
        int n_gated = 0;
        if (!pl.dl.empty()) n_gated = ddhost::gate_streams(thr, counts.data(), pl);      // phase_motion_gate runs only if some stream of dl exists
        // ---- the restatement
        std::vector<int> want_dl, want_gat;
        int want_n = 0;
        for (int z = 0; z < S; ++z) {
            if (!present[z]) continue;
            const bool g = count_of[z] <= thr[z];
            want_gat.push_back(g);
            want_n += g;
            if (!g) want_dl.push_back(z);
        }
        CHECK(pl.dl == want_dl, "seed %u step %d: dl", seed, f);
        CHECK(n_gated == want_n, "seed %u step %d: %d gated, want %d", seed, f, n_gated, want_n);
        for (size_t i = 0; i < pl.act.size(); ++i) CHECK(pl.gat[i] == want_gat[i], "seed %u step %d position %zu: gated flag", seed, f, i);
        for (size_t i = 0; i < pl.act.size(); ++i) CHECK(pl.skp[i] == 0, "seed %u step %d: no skip step", seed, f);
        if (!elig.empty()) { CHECK(pl.dl_elig == elig && pl.cnt_elig == counts, "seed %u step %d: the eligible list and its counts are kept", seed, f); }
        // kept boxes per position: a gated stream has no candidates
        std::vector<int> kept(pl.act.size());
        for (size_t i = 0; i < kept.size(); ++i) kept[i] = pl.gat[i] ? 0 : (int)(r.next() % 6);
        ddhost::pair_counts(pl.skp, [&](int i) { return kept[i]; }, [&](int i) { return per_stream_store ? ret_n[pl.act[i]] : 0; }, doff, eoff);
        CHECK(doff.size() == pl.act.size() + 1 && eoff == doff, "seed %u step %d: without skip steps the tracker's rows are the encoder's", seed, f);
        int run = 0;
        for (size_t i = 0; i < pl.act.size(); ++i) {
            CHECK(doff[i] == run, "seed %u step %d position %zu: row offset %d, want %d", seed, f, i, doff[i], run);
            CHECK(!pl.gat[i] || doff[i + 1] == doff[i], "seed %u step %d position %zu: a gated stream brings rows", seed, f, i);
            run += kept[i];
        }
        CHECK(doff[pl.act.size()] == run, "seed %u step %d: row total", seed, f);
        if (per_stream_store) {
            const bool refresh = !pl.dl.empty();
            const ddhost::RowTable rt = ddhost::feature_row_table(S, pl.act, pl.skp, doff, eoff, ret_off, ret_n, refresh, table, ret_off_new, ret_n_new);
            CHECK(!rt.gather, "seed %u step %d: nothing to gather without a skip step", seed, f);
            if (refresh) {
                size_t e = 0;
                int total = 0;
                for (int z = 0, i = 0; z < S; ++z) {
                    const int now = present[z] ? kept[i] : held[z];
                    if (now > 0) {
                        const int want_e[8] = {present[z] ? 0 : 1, present[z] ? eoff[i] : ret_off[z], 0, present[z] ? doff[i] : 0, now, total, 0, 0};
                        const bool have = (e + 1) * 8 <= table.size();
                        CHECK(have, "seed %u step %d stream %d: table entry missing", seed, f, z);
                        for (int q = 0; have && q < 8; ++q) CHECK(table[e * 8 + q] == want_e[q], "seed %u step %d stream %d: table word %d = %d, want %d", seed, f, z, q, table[e * 8 + q], want_e[q]);
                        ++e;
                    }
                    CHECK(ret_off_new[z] == total && ret_n_new[z] == now, "seed %u step %d stream %d: store (%d, %d), want (%d, %d)", seed, f, z,
                          ret_off_new[z], ret_n_new[z], total, now);
                    held[z] = now;
                    total += now;
                    i += present[z];
                }
                CHECK(e * 8 == table.size() && rt.total == total, "seed %u step %d: %zu table words, total %d, want %zu, %d", seed, f, table.size(), rt.total, e * 8, total);
                ret_off.swap(ret_off_new); ret_n.swap(ret_n_new);
            } else {
                CHECK(table.empty() && rt.total == 0, "seed %u step %d: no encoder run, nothing moves", seed, f);
            }
        }
        // ---- commit, as phase_commit does
        sk.rem = pl.rem_next; sk.has = pl.has_next;
        gs.commit(thr, pl);
        bool any = false;
        for (int z = 0; z < S; ++z) {
            if (!present[z]) continue;
            any = true;
            want_last[z] = count_of[z];
            want_flag[z] = count_of[z] <= thr[z];
            want_gated += want_flag[z];
        }
        want_steps += any;
        CHECK(gs.steps == want_steps && gs.gated == want_gated, "seed %u step %d: stats (%lld, %lld), want (%lld, %lld)", seed, f, gs.steps, gs.gated,
              want_steps, want_gated);
        for (int z = 0; z < S; ++z)
            CHECK(gs.last_count[z] == want_last[z] && gs.last_gated[z] == want_flag[z], "seed %u step %d stream %d: last (%d, %d), want (%d, %d)", seed, f, z,
                  gs.last_count[z], (int)gs.last_gated[z], want_last[z], want_flag[z]);
        for (int z = 0; z < S; ++z) CHECK(sk.rem[z] == 0, "seed %u step %d: counters stay at 0", seed, f);
        if (f == F / 2 && S > 1) {                            // a reset between steps: the stream's entry starts over, the others keep theirs
            const int z = (int)(r.next() % (unsigned)S);
            sk.restart(z); gs.restart(z);
            want_last[z] = -1; want_flag[z] = 0;
            if (per_stream_store) { ret_n[z] = 0; held[z] = 0; }
        }
        g_steps += 1; g_gated += want_n;
        g_empty += pl.act.empty();
        g_all_gated += !pl.act.empty() && want_n == (int)pl.act.size();
        g_none_gated += !pl.act.empty() && want_n == 0;
    }
}

int main() {
    const unsigned N = 4000;
    for (unsigned seed = 1; seed <= N; ++seed) one_sequence(seed);
    printf("%u sequences, %lld steps (%lld without a stream, %lld with every stream gated, %lld with none), %lld gated stream-steps, %lld checks, %lld differ\n",
           N, g_steps, g_empty, g_all_gated, g_none_gated, g_gated, g_checks, g_bad);
    return g_bad == 0 && g_empty > 0 && g_all_gated > 0 && g_none_gated > 0 && g_gated > 0 ? 0 : 1;
}
