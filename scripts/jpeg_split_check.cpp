// Stand-alone check of the statements jpeg_split_entropy_k runs (csrc/jpeg_dec_dev.h: jpd_span_fill, jpd_decode_span and what they call)
// under the address and undefined-behaviour sanitizers.  Plain C++, no GPU, not loaded into Python:
//
//     python scripts/make_jpeg_split_corpus.py DIR
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_split_check.cpp -o jpeg_split_check
//     ./jpeg_split_check DIR
//
// DIR/index.txt lists one file per line, "valid NAME" or "damaged NAME" (NAME.jpg).  Every file the header parser accepts as one restart
// interval is decoded by jpd_decode_interval, the sequential decoder, and then by the kernel's rounds emulated on the host, at subsequence
// sizes of 16, 32 and 128 bytes and under three schedules: the kernel's own (every lane reads its predecessor's end state, then all decode),
// and lanes that read and decode at once in ascending and in descending order.  For every file, size and schedule
//   - the status equals jpd_decode_interval's, and where both are DD_JPEG_ST_OK so do the coefficients (a valid file must be OK);
//   - the rounds never exceed the subsequences + 1;
//   - no sanitizer finding: the file and the coefficient buffer are exactly as large as the header implies.
// Hostile input is exercised here, exhaustively, and not on the card.  Exit status 0 when all is well.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "../deepdish_amd/csrc/jpeg_dec_dev.h"

static std::vector<uint8_t> slurp(const std::string &path, bool *ok) {
    std::ifstream f(path, std::ios::binary);
    *ok = (bool)f;
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

enum Schedule { KERNEL, ASCENDING, DESCENDING };

struct Sub {
    JpdState used, end;
    JpdSpanSums sums;
    bool due;
};

// What jpeg_split_entropy_k does for one file.  Returns the status; *rounds: how many rounds ran.
static int split_decode(const dd_jpeg_info &r, const uint8_t *scan, uint32_t len, int log2b, Schedule how, std::vector<int16_t> &coef, long long *rounds, long long *decodes) {
    uint32_t end = len;
    for (uint32_t p = 0; p < len; ++p)
        if (jpd_marker_at(scan, p, len)) {
            end = p;
            break;
        }
    const long long n_sub = ((long long)end + (1ll << log2b) - 1) >> log2b;
    const uint32_t n_blocks = (uint32_t)r.mcus_x * (uint32_t)r.mcus_y * (uint32_t)r.blocks_per_mcu;
    std::vector<Sub> sub((size_t)n_sub);
    auto lim = [&](long long i) { return (uint32_t)std::min<long long>(end, (i + 1) << log2b); };
    auto count = [&](long long i) {
        JpdState st = sub[i].used;
        jpd_decode_span(r, r.huff, scan, end, lim(i), st, JPD_SPAN_COUNT, sub[i].sums, nullptr, 0, 0, nullptr);
        sub[i].end = st;
        ++*decodes;
    };
    for (long long i = 0; i < n_sub; ++i) {
        sub[i].used = jpd_span_guess(scan, (uint32_t)i, log2b, end);
        count(i);
    }
    *rounds = 1;
    for (long long round = 1; round <= n_sub; ++round) {
        bool any = false;
        auto read = [&](long long i) {
            sub[i].due = false;
            if (i == 0) return;
            const JpdState p = sub[i - 1].end;
            if (p.kj == JPD_STATE_UNKNOWN || jpd_state_eq(p, sub[i].used)) return;
            sub[i].used = p;
            sub[i].due = any = true;
        };
        if (how == KERNEL) {
            for (long long i = 0; i < n_sub; ++i) read(i);
            for (long long i = 0; i < n_sub; ++i)
                if (sub[i].due) count(i);
        } else {
            for (long long q = 0; q < n_sub; ++q) {
                const long long i = how == ASCENDING ? q : n_sub - 1 - q;
                read(i);
                if (sub[i].due) count(i);
            }
        }
        ++*rounds;
        if (!any) break;
    }
    long long first_bad = n_sub;
    for (long long i = n_sub - 1; i >= 0; --i)
        if (sub[i].end.kj == JPD_STATE_UNKNOWN) first_bad = i;
    uint32_t blk = 0, pred[3] = {0, 0, 0};
    bool ok = false;
    for (long long i = 0; i < n_sub; ++i) {
        JpdState st = sub[i].used;
        JpdSpanSums unused;
        uint32_t p[3] = {pred[0] & 0xFFFFu, pred[1] & 0xFFFFu, pred[2] & 0xFFFFu};
        const bool done = jpd_decode_span(r, r.huff, scan, end, lim(i), st, JPD_SPAN_WRITE, unused, coef.data(), blk, n_blocks, p);
        if (done && i <= first_bad) ok = true;
        blk += sub[i].sums.blocks;
        for (int c = 0; c < 3; ++c) pred[c] += sub[i].sums.dc[c];
    }
    return ok ? DD_JPEG_ST_OK : DD_JPEG_ST_DATA;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_split_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream index(dir + "/index.txt");
    if (!index) {
        std::fprintf(stderr, "jpeg_split_check: no %s/index.txt\n", dir.c_str());
        return 2;
    }
    std::string kind, name;
    long long valid = 0, damaged = 0, refused = 0, other = 0, split_ok = 0, split_data = 0, runs = 0, most_rounds = 0, subs = 0, decodes = 0;
    while (index >> kind >> name) {
        bool got;
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpg", &got);
        if (!got) {
            std::fprintf(stderr, "jpeg_split_check: cannot read %s\n", name.c_str());
            return 1;
        }
        const bool is_valid = kind == "valid";
        ++(is_valid ? valid : damaged);
        dd_jpeg_info r;
        char msg[256];
        const std::vector<uint8_t> exact(file);                      // an exact-size copy: a read past the file's end is a finding
        if (jpd_parse(exact.data(), exact.size(), &r, msg, sizeof(msg)) != DD_JPEG_R_OK) {
            if (is_valid) {
                std::fprintf(stderr, "jpeg_split_check: %s: refused: %s\n", name.c_str(), msg);
                return 1;
            }
            ++refused;
            continue;
        }
        const uint8_t *scan = exact.data() + r.scan_offset;
        const uint32_t len = (uint32_t)r.scan_length;
        bool rst = false;                                            // jpeg_markers_k: an RSTn marker in a file of one interval is DD_JPEG_ST_DATA already
        for (uint32_t p = 0; p + 1 < len; ++p) rst = rst || jpd_rst_at(scan, p) >= 0;
        if (r.n_intervals != 1 || rst) {
            if (is_valid) {
                std::fprintf(stderr, "jpeg_split_check: %s: a valid file of %d intervals\n", name.c_str(), r.n_intervals);
                return 1;
            }
            ++other;
            continue;
        }
        const int mcus = r.mcus_x * r.mcus_y;
        const size_t n_coef = (size_t)mcus * r.blocks_per_mcu * 64;
        std::vector<int16_t> want(n_coef, 0);
        const int want_status = jpd_decode_interval(r, scan, 0, len, 0, mcus, want.data());
        if (is_valid && want_status != DD_JPEG_ST_OK) {
            std::fprintf(stderr, "jpeg_split_check: %s: the sequential decoder reports %d for a valid file\n", name.c_str(), want_status);
            return 1;
        }
        for (int log2b : {4, 5, 7}) {
            if ((long long)len <= (1ll << log2b)) continue;          // not routed
            for (Schedule how : {KERNEL, ASCENDING, DESCENDING}) {
                std::vector<int16_t> coef(n_coef, 0);
                long long rounds = 0;
                const int status = split_decode(r, scan, len, log2b, how, coef, &rounds, &decodes);
                const long long n_sub = ((long long)len + (1ll << log2b) - 1) >> log2b;
                if (status != want_status || (status == DD_JPEG_ST_OK && coef != want) || rounds > n_sub + 1) {
                    std::fprintf(stderr, "jpeg_split_check: %s at %d bytes, schedule %d: status %d against %d%s, %lld rounds for %lld subsequences\n", name.c_str(), 1 << log2b,
                                 (int)how, status, want_status, status == want_status && status == DD_JPEG_ST_OK ? ", and the coefficients differ" : "", rounds, n_sub);
                    return 1;
                }
                ++runs, ++(status == DD_JPEG_ST_OK ? split_ok : split_data);
                if (how == KERNEL) subs += n_sub;
                most_rounds = rounds > most_rounds ? rounds : most_rounds;
            }
        }
    }
    std::printf("jpeg_split_check: %lld valid and %lld damaged files (%lld refused by the parser, %lld not one marker-less interval); %lld split decodes agree with the "
                "sequential decoder: status 0 for %lld, data %lld; at most %lld rounds; %lld subsequences, %lld decodes of one (all schedules)\n",
                valid, damaged, refused, other, runs, split_ok, split_data, most_rounds, subs, decodes);
    return valid > 0 && damaged > 0 && split_ok > 0 && split_data > 0 ? 0 : 1;
}
