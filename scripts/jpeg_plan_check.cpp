// Stand-alone check of the JPEG decoder's call plan (csrc/jpeg_dec_plan.h jd_plan_call and its helpers): the statements jpegdec_launch runs
// over the records before it queues anything, here over records forged in memory, under the address and undefined-behaviour sanitizers.
// Plain C++, no GPU, not loaded into Python:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_plan_check.cpp -o jpeg_plan_check
//     ./jpeg_plan_check            every case's outcome against the table below; exit status 0 when all agree
//     ./jpeg_plan_check --print    the outcomes in the table's form, for a new case
//
// A case is a decoder's planning config and one call: records, scan scripts, scales, byte count.  Its outcome is the error code and the
// message, and after DD_OK every field the plan fills -- per record interval_base, reserved, path (as the kernels take it apart),
// n_intervals, restart_interval, scan_offset, scan_length; per scan script n_scans, n_levels, level_base and every scan's interval_base --
// and the whole JdCall with the three launch predicates and the lanes per wave that follow from it.
//
// The expected outcomes were printed by the planning loop as it stood inside jpegdec_launch before it became jd_plan_call (the commit
// "JPEG decoder and ring: files of any size, per-file scale, default DHT"), compiled against these same cases; they were not taken from
// the code under test.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../deepdish_amd/csrc/jpeg_dec_plan.h"
#include "../deepdish_amd/csrc/jpeg_parse.h"

namespace {

struct Case {
    std::string name;
    JdConfig cfg{};
    std::vector<dd_jpeg_info> recs;
    std::vector<dd_jpeg_scans> scans;          // empty: no scan scripts are given
    std::vector<int> scales;                   // empty: no scales are given
    size_t n_bytes = 4096;
    int n = -1;                                // -1: as many as there are records
};

JdConfig config(int h, int w, int scale, int flags, int split_log2 = 6, bool split_auto = true) {
    JdConfig c{};
    char msg[320];
    if (jd_geometry(h, w, "jpeg_plan_check", &c.g, msg, sizeof(msg)) != DD_OK) std::fprintf(stderr, "ERROR %s\n", msg);
    c.scale = scale, c.flags = flags, c.split_log2 = split_log2, c.split_auto = split_auto;
    c.max_frames = 8, c.max_bytes = 1 << 20, c.lanes = 0;
    return c;
}

// A baseline record as the parser leaves it (csrc/jpeg_parse.h), status OK, with the scan at [scan_offset, scan_offset + scan_length).
dd_jpeg_info file(int h, int w, int ncomp, int hs, int vs, int dri, int scan_length, int64_t file_offset = 0, int scan_offset = 100) {
    dd_jpeg_info r;
    std::memset(&r, 0, sizeof(r));
    r.height = h, r.width = w, r.ncomp = ncomp, r.sof = 0xC0;
    r.hmax = hs, r.vmax = vs;
    r.mcus_x = (w + 8 * hs - 1) / (8 * hs), r.mcus_y = (h + 8 * vs - 1) / (8 * vs);
    r.blocks_per_mcu = ncomp == 1 ? 1 : hs * vs + 2;
    r.restart_interval = dri;
    const int mcus = r.mcus_x * r.mcus_y, ri = dri ? dri : mcus;
    r.n_intervals = (mcus + ri - 1) / ri;
    r.scan_offset = scan_offset, r.scan_length = scan_length;
    r.status = DD_JPEG_ST_OK, r.file_offset = file_offset;
    r.path = 77, r.interval_base = 77, r.reserved = 77;                     // what the plan must overwrite
    return r;
}

dd_jpeg_info dead(int status) {
    dd_jpeg_info r;
    std::memset(&r, 0, sizeof(r));
    r.status = status, r.n_intervals = 9, r.interval_base = 77, r.reserved = 77;
    return r;
}

// A progressive record: the frame alone; the scan fields hold what the plan must zero for jpeg_entropy_k.
dd_jpeg_info prog_file(int h, int w, int64_t file_offset = 0) {
    dd_jpeg_info r = file(h, w, 3, 2, 2, 0, 5, file_offset);
    r.sof = 0xC2, r.n_intervals = 7, r.restart_interval = 3;
    return r;
}

struct ScanSpec {
    int level, n_intervals, offset, length;
};

dd_jpeg_scans script(int n_levels, const std::vector<ScanSpec> &specs) {
    dd_jpeg_scans S;
    std::memset(&S, 0, sizeof(S));
    S.n_scans = (int)specs.size(), S.n_levels = n_levels;
    for (int l = 0; l < DD_JPEG_MAX_LEVELS; ++l) S.level_base[l] = 77;
    for (size_t k = 0; k < specs.size(); ++k) {
        dd_jpeg_scan &sc = S.scan[k];
        sc.level = specs[k].level, sc.n_intervals = specs[k].n_intervals, sc.offset = specs[k].offset, sc.length = specs[k].length;
        sc.interval_base = 77;
    }
    return S;
}

dd_jpeg_scans no_script() { return script(0, {}); }

std::vector<Case> cases() {
    std::vector<Case> all;
    auto add = [&](const std::string &name, const JdConfig &cfg) -> Case & {
        all.emplace_back();
        all.back().name = name, all.back().cfg = cfg;
        return all.back();
    };
    const int P = DD_JPEGDEC_PROGRESSIVE, S = DD_JPEGDEC_SPLIT, A = DD_JPEGDEC_ANY_SIZE;

    // ---- the LDS path at every scale, one 16 x 16 4:2:0 file without DRI
    for (int s : {1, 2, 4, 8}) add("lds, fixed scale " + std::to_string(s), config(16, 16, s, 0)).recs = {file(16, 16, 3, 2, 2, 0, 40)};
    {
        Case &c = add("lds, per-file scales 1 2 4 8", config(16, 16, 1, A));
        for (int i = 0; i < 4; ++i) c.recs.push_back(file(16, 16, 3, 2, 2, 0, 40, 200 * i));
        c.scales = {1, 2, 4, 8};
    }
    // ---- DRI = 1: one MCU, one interval; the bases run over two such files
    add("dri 1, two files", config(16, 16, 1, 0)).recs = {file(16, 16, 3, 2, 2, 1, 40), file(16, 16, 3, 2, 2, 1, 40, 200)};
    // ---- 26 bytes of LDS per column of a 4:2:0 band: 2513 .. 2528 columns are the narrowest beyond 64 KiB
    {
        Case &c = add("planes at scale 1, lds at scale 2, 2512 wide still lds", config(16, 2528, 1, A));
        c.recs = {file(16, 2528, 3, 2, 2, 0, 40), file(16, 2528, 3, 2, 2, 0, 40, 200), file(16, 2512, 3, 2, 2, 0, 40, 400)};
        c.scales = {1, 2, 1};
    }
    add("planes, fixed scale 1", config(16, 2528, 1, 0)).recs = {file(16, 2528, 3, 2, 2, 0, 40), file(16, 2528, 1, 1, 1, 0, 40, 200)};
    // ---- dead records between live ones; two progressive files with different scan counts
    {
        Case &c = add("mixed: header, empty, size, progressive, baseline, progressive, baseline", config(32, 32, 1, P));
        c.recs = {dead(DD_JPEG_ST_HEADER), dead(DD_JPEG_ST_NO_FRAME), dead(DD_JPEG_ST_SIZE), prog_file(32, 32, 300), file(32, 32, 3, 2, 2, 2, 50, 600),
                  prog_file(32, 32, 900),  file(32, 32, 3, 1, 1, 0, 60, 1500)};
        c.scans = {script(2, {{0, 1, 0, 1}, {1, 1, 0, 1}}), script(1, {{0, 4, 0, 1}}), no_script(),
                   script(2, {{0, 1, 20, 10}, {0, 4, 40, 10}, {1, 2, 60, 10}}), script(3, {{0, 5, 0, 1}}),
                   script(3, {{0, 2, 20, 10}, {1, 4, 40, 10}, {1, 1, 60, 10}, {2, 16, 80, 10}, {0, 1, 100, 10}}), no_script()};
    }
    // ---- DD_JPEGDEC_SPLIT routing
    {
        Case &c = add("split: 64 bytes stay, 65 go, 16385 double once, DRI >= MCUs is one interval, two intervals stay", config(16, 32, 1, S));
        c.n_bytes = 40000;
        c.recs = {file(16, 32, 3, 2, 2, 0, 64), file(16, 32, 3, 2, 2, 0, 65, 200), file(16, 32, 3, 2, 2, 0, 16385, 400), file(16, 32, 3, 2, 2, 5, 200, 17000),
                  file(16, 32, 3, 2, 2, 1, 200, 17400)};
    }
    {
        Case &c = add("split, size fixed at 16: 4097 bytes keep it, 32769 double once", config(16, 32, 1, S, 4, false));
        c.n_bytes = 40000;
        c.recs = {file(16, 32, 3, 2, 2, 0, 4097), file(16, 32, 3, 2, 2, 0, 32769, 5000)};
    }
    {
        Case &c = add("split decoder, a progressive file is not routed", config(32, 32, 1, S | P));
        c.recs = {prog_file(32, 32), file(32, 32, 3, 2, 2, 0, 300, 1000)};
        c.recs[0].n_intervals = 1, c.recs[0].scan_length = 500;
        c.scans = {script(1, {{0, 1, 20, 300}}), no_script()};
    }
    add("split files only: nothing for the baseline kernel", config(16, 16, 1, S)).recs = {file(16, 16, 3, 2, 2, 0, 300), file(16, 16, 1, 1, 1, 0, 100, 500)};
    {
        Case &c = add("progressive files only: nothing for the baseline kernel", config(32, 32, 1, P));
        c.recs = {prog_file(32, 32), prog_file(32, 32, 500)};
        c.scans = {script(1, {{0, 1, 20, 30}}), script(2, {{0, 1, 20, 30}, {1, 4, 60, 30}})};
    }
    // ---- DD_JPEGDEC_ANY_SIZE: each buffer check failing alone
    add("any size: a side too large", config(64, 64, 1, A)).recs = {file(64, 64, 3, 2, 2, 0, 40), file(64, 80, 3, 2, 2, 0, 40, 200)};
    {
        Case &c = add("any size: MCU counts that are not the size's", config(64, 64, 1, A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.recs[0].mcus_x = 5;
    }
    {
        Case &c = add("any size: more bands than the decoder's", config(64, 64, 1, A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.recs[0].mcus_y = 9;
    }
    {
        Case &c = add("any size: blocks beyond coef_stride", config(64, 64, 1, A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.recs[0].blocks_per_mcu = 60;
    }
    {
        Case &c = add("any size: planes beyond plane_stride", config(32, 512, 1, A));
        c.recs = {file(32, 512, 3, 2, 2, 0, 40)};
        c.recs[0].vmax = 16, c.recs[0].mcus_y = 1;                          // a band of 128 rows
    }
    {
        Case &c = add("any size: a scale below the decoder's", config(64, 64, 2, A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40), file(64, 64, 3, 2, 2, 0, 40, 200)};
        c.scales = {4, 1};
    }
    {
        Case &c = add("any size: a scale that is none", config(64, 64, 1, A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.scales = {3};
    }
    {
        Case &c = add("scales for a decoder without DD_JPEGDEC_ANY_SIZE", config(64, 64, 1, P | S));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.scales = {1};
    }
    {
        Case &c = add("scan scripts for a decoder without DD_JPEGDEC_PROGRESSIVE", config(64, 64, 1, S | A));
        c.recs = {file(64, 64, 3, 2, 2, 0, 40)};
        c.scans = {no_script()};
    }
    // ---- capacity and byte ranges
    {
        Case &c = add("no file", config(16, 16, 1, 0));
        c.recs = {file(16, 16, 3, 2, 2, 0, 40)};
        c.n = 0;
    }
    {
        Case &c = add("more files than max_frames", config(16, 16, 1, 0));
        c.cfg.max_frames = 2;
        for (int i = 0; i < 3; ++i) c.recs.push_back(file(16, 16, 3, 2, 2, 0, 40, 200 * i));
    }
    {
        Case &c = add("more bytes than max_bytes", config(16, 16, 1, 0));
        c.cfg.max_bytes = 4095;
        c.recs = {file(16, 16, 3, 2, 2, 0, 40)};
    }
    add("a file that ends at the last byte", config(16, 16, 1, 0)).recs = {file(16, 16, 3, 2, 2, 0, 40, 3956)};
    add("a file that ends one byte past the bytes given", config(16, 16, 1, 0)).recs = {file(16, 16, 3, 2, 2, 0, 40), file(16, 16, 3, 2, 2, 0, 40, 3957)};
    add("a file at a negative offset", config(16, 16, 1, 0)).recs = {file(16, 16, 3, 2, 2, 0, 40, -1)};
    {
        Case &c = add("a scan that ends one byte past the bytes given", config(32, 32, 1, P));
        c.recs = {prog_file(32, 32, 1000)};
        c.scans = {script(1, {{0, 1, 20, 3076}, {0, 1, 96, 3001}})};
    }
    {
        Case &c = add("a scan at a level the file does not have", config(32, 32, 1, P));
        c.recs = {prog_file(32, 32)};
        c.scans = {script(2, {{0, 1, 20, 30}, {2, 1, 60, 30}})};
    }
    {
        Case &c = add("a scan without intervals", config(32, 32, 1, P));
        c.recs = {prog_file(32, 32)};
        c.scans = {script(1, {{0, 0, 20, 30}})};
    }
    {
        Case &c = add("more scans than a script holds", config(32, 32, 1, P));
        c.recs = {prog_file(32, 32)};
        c.scans = {script(1, {{0, 1, 20, 30}})};
        c.scans[0].n_scans = DD_JPEG_MAX_SCANS + 1;
    }
    {
        Case &c = add("more than 2^31 intervals", config(16, 16, 1, 0));
        c.recs = {file(16, 16, 3, 2, 2, 0, 40), file(16, 16, 3, 2, 2, 0, 40, 200)};
        c.recs[0].n_intervals = c.recs[1].n_intervals = 0x40000000;
    }
    // ---- the lanes override reaches both entropy kernels
    {
        Case &c = add("DD_JPEGDEC_LANES 8", config(32, 32, 1, P));
        c.cfg.lanes = 8;
        c.recs = {prog_file(32, 32), file(32, 32, 3, 2, 2, 1, 50, 600)};
        c.scans = {script(1, {{0, 4, 20, 30}}), no_script()};
    }
    return all;
}

void put(std::string &o, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void put(std::string &o, const char *fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    o += line;
}

std::string outcome(Case c) {
    std::string o;
    JdCall call{};
    char msg[320] = "";
    const int n = c.n >= 0 ? c.n : (int)c.recs.size();
    const int rc = jd_plan_call(c.cfg, c.recs.data(), c.scans.empty() ? nullptr : c.scans.data(), c.n_bytes, n, c.scales.empty() ? nullptr : c.scales.data(), &call, msg, sizeof(msg));
    put(o, "rc %d: %s\n", rc, msg);
    if (rc != DD_OK) return o;
    put(o, "call: total %lld ptotal %lld max_scans %d n_levels %d n_split %d max_sub %d lds %zu any_planes %d any %d\n", call.total, call.ptotal, call.max_scans, call.n_levels,
        call.n_split, call.max_sub, call.lds, (int)call.any_planes, (int)call.any);
    o += "  level_total";
    for (int l = 0; l < DD_JPEG_MAX_LEVELS; ++l) put(o, " %lld", call.level_total[l]);
    o += "\n  per scale:";
    for (int k = 0; k < 4; ++k) put(o, " [any %d lds %zu planes %d]", (int)call.per_scale.any_at[k], call.per_scale.lds_at[k], (int)call.per_scale.planes_at[k]);
    put(o, "\n  launch: split %d baseline %d progressive %d; lanes per wave %d, per level", (int)jd_call_has_split(call), (int)jd_call_has_baseline_lanes(call),
        (int)jd_call_has_progressive(call), jd_lanes_per_wave(call.total, c.cfg.lanes));
    for (int l = 0; l < call.n_levels; ++l) put(o, " %d", jd_lanes_per_wave(call.level_total[l], c.cfg.lanes));
    o += "\n";
    for (int i = 0; i < n; ++i) {
        const dd_jpeg_info &r = c.recs[i];
        put(o, "file %d: interval_base %d reserved %d (split log2 %d) path 0x%x (path %d scale log2 %d) n_intervals %d restart_interval %d scan %d + %d\n", i, r.interval_base,
            r.reserved, jd_split_log2_of(r), r.path, jd_path_of(r.path), jd_path_scale_log2(r.path), r.n_intervals, r.restart_interval, r.scan_offset, r.scan_length);
        if (c.scans.empty()) continue;
        const dd_jpeg_scans &S = c.scans[i];
        put(o, "  scans %d levels %d level_base", S.n_scans, S.n_levels);
        for (int l = 0; l < DD_JPEG_MAX_LEVELS; ++l) put(o, " %d", S.level_base[l]);
        o += "; interval_base";
        for (int k = 0; k < S.n_scans; ++k) put(o, " %d", S.scan[k].interval_base);
        o += "\n";
    }
    return o;
}

// The lanes-per-wave rule at its steps: 64 lanes from 2048 intervals each, halved below, never under one.
std::string lanes_outcome() {
    std::string o;
    for (long long t : {0ll, 1ll, 2047ll, 2048ll, 4095ll, 4096ll, 65535ll, 65536ll, 131071ll, 131072ll, 0x7fffffffll}) put(o, "%lld -> %d, with 3 lanes -> %d\n", t, jd_lanes_per_wave(t, 0), jd_lanes_per_wave(t, 3));
    return o;
}

struct Expected {
    const char *name, *outcome;
};

// clang-format off
const Expected EXPECTED[] = {
    {"lds, fixed scale 1",
     "rc 0: \n"
     "call: total 1 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 416 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"lds, fixed scale 2",
     "rc 0: \n"
     "call: total 1 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 192 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"lds, fixed scale 4",
     "rc 0: \n"
     "call: total 1 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 48 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"lds, fixed scale 8",
     "rc 0: \n"
     "call: total 1 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 12 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"lds, per-file scales 1 2 4 8",
     "rc 0: \n"
     "call: total 4 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 416 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 1 lds 416 planes 0] [any 1 lds 192 planes 0] [any 1 lds 48 planes 0] [any 1 lds 12 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 1: interval_base 1 reserved 0 (split log2 0) path 0x100 (path 0 scale log2 1) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 2: interval_base 2 reserved 0 (split log2 0) path 0x200 (path 0 scale log2 2) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 3: interval_base 3 reserved 0 (split log2 0) path 0x300 (path 0 scale log2 3) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"dri 1, two files",
     "rc 0: \n"
     "call: total 2 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 416 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 1 scan 100 + 40\n"
     "file 1: interval_base 1 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 1 scan 100 + 40\n"
    },
    {"planes at scale 1, lds at scale 2, 2512 wide still lds",
     "rc 0: \n"
     "call: total 3 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 65312 any_planes 1 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 1 lds 65312 planes 1] [any 1 lds 30336 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x1 (path 1 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 1: interval_base 1 reserved 0 (split log2 0) path 0x100 (path 0 scale log2 1) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 2: interval_base 2 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"planes, fixed scale 1",
     "rc 0: \n"
     "call: total 2 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 20224 any_planes 1 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x1 (path 1 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
     "file 1: interval_base 1 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"mixed: header, empty, size, progressive, baseline, progressive, baseline",
     "rc 0: \n"
     "call: total 3 ptotal 31 max_scans 5 n_levels 3 n_split 0 max_sub 0 lds 832 any_planes 0 any 1\n"
     "  level_total 8 7 16 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 1; lanes per wave 1, per level 1 1 1\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 0 levels 0 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
     "file 1: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 0 levels 0 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
     "file 2: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 0 levels 0 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
     "file 3: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 3 levels 2 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 0 1 5\n"
     "file 4: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 2 restart_interval 2 scan 100 + 50\n"
     "  scans 0 levels 0 level_base 5 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
     "file 5: interval_base 2 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 5 levels 3 level_base 5 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 7 9 13 14 30\n"
     "file 6: interval_base 2 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 60\n"
     "  scans 0 levels 0 level_base 8 7 16 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
    },
    {"split: 64 bytes stay, 65 go, 16385 double once, DRI >= MCUs is one interval, two intervals stay",
     "rc 0: \n"
     "call: total 6 ptotal 0 max_scans 0 n_levels 0 n_split 3 max_sub 129 lds 832 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 1 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 64\n"
     "file 1: interval_base 1 reserved 6 (split log2 6) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 65\n"
     "file 2: interval_base 2 reserved 7 (split log2 7) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 16385\n"
     "file 3: interval_base 3 reserved 6 (split log2 6) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 5 scan 100 + 200\n"
     "file 4: interval_base 4 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 2 restart_interval 1 scan 100 + 200\n"
    },
    {"split, size fixed at 16: 4097 bytes keep it, 32769 double once",
     "rc 0: \n"
     "call: total 2 ptotal 0 max_scans 0 n_levels 0 n_split 2 max_sub 1025 lds 832 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 1 baseline 0 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 4 (split log2 4) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 4097\n"
     "file 1: interval_base 1 reserved 5 (split log2 5) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 32769\n"
    },
    {"split decoder, a progressive file is not routed",
     "rc 0: \n"
     "call: total 1 ptotal 1 max_scans 1 n_levels 1 n_split 1 max_sub 5 lds 832 any_planes 0 any 1\n"
     "  level_total 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 1 baseline 0 progressive 1; lanes per wave 1, per level 1\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 1 levels 1 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 0\n"
     "file 1: interval_base 0 reserved 6 (split log2 6) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 300\n"
     "  scans 0 levels 0 level_base 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
    },
    {"split files only: nothing for the baseline kernel",
     "rc 0: \n"
     "call: total 2 ptotal 0 max_scans 0 n_levels 0 n_split 2 max_sub 5 lds 416 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 1 baseline 0 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 6 (split log2 6) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 300\n"
     "file 1: interval_base 1 reserved 6 (split log2 6) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 100\n"
    },
    {"progressive files only: nothing for the baseline kernel",
     "rc 0: \n"
     "call: total 0 ptotal 6 max_scans 2 n_levels 2 n_split 0 max_sub 0 lds 832 any_planes 0 any 1\n"
     "  level_total 2 4 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 0 progressive 1; lanes per wave 1, per level 1 1\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 1 levels 1 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 0\n"
     "file 1: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 2 levels 2 level_base 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 1 2\n"
    },
    {"any size: a side too large",
     "rc -1: jpeg decoder: file 1 is 80 x 64, the decoder holds at most 64 x 64\n"
    },
    {"any size: MCU counts that are not the size's",
     "rc -1: jpeg decoder: file 0: 5 x 4 MCUs for 64 x 64 pixels\n"
    },
    {"any size: more bands than the decoder's",
     "rc -1: jpeg decoder: file 0: 4 x 9 MCUs for 64 x 64 pixels\n"
    },
    {"any size: blocks beyond coef_stride",
     "rc -1: jpeg decoder: file 0 has 960 blocks, a frame's coefficients hold 192\n"
    },
    {"any size: planes beyond plane_stride",
     "rc -1: jpeg decoder: file 0 needs 69632 bytes of planes, a frame holds 49152\n"
    },
    {"any size: a scale below the decoder's",
     "rc -1: jpeg decoder: file 1 at scale 1 (1, 2, 4 or 8, and at least the decoder's 2)\n"
    },
    {"any size: a scale that is none",
     "rc -1: jpeg decoder: file 0 at scale 3 (1, 2, 4 or 8, and at least the decoder's 1)\n"
    },
    {"scales for a decoder without DD_JPEGDEC_ANY_SIZE",
     "rc -3: jpeg decoder: a scale per file for a decoder that was not made with DD_JPEGDEC_ANY_SIZE\n"
    },
    {"scan scripts for a decoder without DD_JPEGDEC_PROGRESSIVE",
     "rc -3: jpeg decoder: scan scripts for a decoder that was not made to take progressive files\n"
    },
    {"no file",
     "rc -4: jpeg decoder: 0 frames in a call (1 .. 8)\n"
    },
    {"more files than max_frames",
     "rc -4: jpeg decoder: 3 frames in a call (1 .. 2)\n"
    },
    {"more bytes than max_bytes",
     "rc -4: jpeg decoder: 4096 bytes of files in a call (at most 4095)\n"
    },
    {"a file that ends at the last byte",
     "rc 0: \n"
     "call: total 1 ptotal 0 max_scans 0 n_levels 0 n_split 0 max_sub 0 lds 416 any_planes 0 any 1\n"
     "  level_total 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 0; lanes per wave 1, per level\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 1 restart_interval 0 scan 100 + 40\n"
    },
    {"a file that ends one byte past the bytes given",
     "rc -1: jpeg decoder: file 1 lies outside the 4096 bytes given\n"
    },
    {"a file at a negative offset",
     "rc -1: jpeg decoder: file 0 lies outside the 4096 bytes given\n"
    },
    {"a scan that ends one byte past the bytes given",
     "rc -1: jpeg decoder: scan 1 of file 0 lies outside the 4096 bytes given\n"
    },
    {"a scan at a level the file does not have",
     "rc -1: jpeg decoder: scan 1 of file 0: level 2, 1 intervals\n"
    },
    {"a scan without intervals",
     "rc -1: jpeg decoder: scan 0 of file 0: level 0, 0 intervals\n"
    },
    {"more scans than a script holds",
     "rc -1: jpeg decoder: file 0: 65 scans at 1 levels\n"
    },
    {"more than 2^31 intervals",
     "rc -4: jpeg decoder: more than 2^31 restart intervals in a call\n"
    },
    {"DD_JPEGDEC_LANES 8",
     "rc 0: \n"
     "call: total 4 ptotal 4 max_scans 1 n_levels 1 n_split 0 max_sub 0 lds 832 any_planes 0 any 1\n"
     "  level_total 4 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n"
     "  per scale: [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0] [any 0 lds 0 planes 0]\n"
     "  launch: split 0 baseline 1 progressive 1; lanes per wave 8, per level 8\n"
     "file 0: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 0 restart_interval 0 scan 0 + 0\n"
     "  scans 1 levels 1 level_base 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base 0\n"
     "file 1: interval_base 0 reserved 0 (split log2 0) path 0x0 (path 0 scale log2 0) n_intervals 4 restart_interval 1 scan 100 + 50\n"
     "  scans 0 levels 0 level_base 4 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0; interval_base\n"
    },
    {"lanes per wave",
     "0 -> 1, with 3 lanes -> 3\n"
     "1 -> 1, with 3 lanes -> 3\n"
     "2047 -> 1, with 3 lanes -> 3\n"
     "2048 -> 1, with 3 lanes -> 3\n"
     "4095 -> 1, with 3 lanes -> 3\n"
     "4096 -> 2, with 3 lanes -> 3\n"
     "65535 -> 16, with 3 lanes -> 3\n"
     "65536 -> 32, with 3 lanes -> 3\n"
     "131071 -> 32, with 3 lanes -> 3\n"
     "131072 -> 64, with 3 lanes -> 3\n"
     "2147483647 -> 64, with 3 lanes -> 3\n"
    },
};
// clang-format on

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::pair<std::string, std::string>> got;
    for (const Case &c : cases()) got.emplace_back(c.name, outcome(c));
    got.emplace_back("lanes per wave", lanes_outcome());
    if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {
        for (const auto &g : got) {
            std::printf("    {\"%s\",\n", g.first.c_str());
            size_t at = 0;
            while (at < g.second.size()) {
                const size_t nl = g.second.find('\n', at);
                std::printf("     \"%s\\n\"\n", g.second.substr(at, nl - at).c_str());
                at = nl + 1;
            }
            std::printf("    },\n");
        }
        return 0;
    }
    int bad = 0;
    const size_t n_expected = sizeof(EXPECTED) / sizeof(EXPECTED[0]);
    if (n_expected != got.size()) std::fprintf(stderr, "ERROR %zu cases, %zu expected outcomes\n", got.size(), n_expected), ++bad;
    for (size_t i = 0; i < got.size() && i < n_expected; ++i) {
        if (got[i].first == EXPECTED[i].name && got[i].second == EXPECTED[i].outcome) continue;
        std::fprintf(stderr, "ERROR case %zu \"%s\":\n--- expected (\"%s\")\n%s--- got\n%s", i, got[i].first.c_str(), EXPECTED[i].name, EXPECTED[i].outcome, got[i].second.c_str());
        ++bad;
    }
    std::printf("%zu plans, %d differ from the recorded outcomes\n", got.size(), bad);
    return bad ? 1 : 0;
}
