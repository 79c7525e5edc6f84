// Stand-alone check of the progressive JPEG decoder's shared statements (csrc/jpeg_parse.h: jpd_parse_scans; csrc/jpeg_dec_dev.h:
// jpd_prog_decode_interval and what it calls, the very code jpeg_prog_entropy_k of csrc/jpeg_dec.hip runs) under the address and
// undefined-behaviour sanitizers.  Plain C++, no GPU, not loaded into Python:
//
//     python scripts/make_jpeg_prog_corpus.py DIR
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_prog_check.cpp -o jpeg_prog_check
//     ./jpeg_prog_check DIR
//
// DIR/index.txt lists one file per line: "valid NAME" (NAME.jpg with NAME.coef, the int16 coefficients tests/jpeg_prog_ref.py gives; the
// program must decode exactly those), "damaged NAME" (cut or with a byte replaced: the program must come back with a status, whatever it
// is, and no sanitizer finding; the file and the coefficient buffer are exactly as large as they are, so a read or a store outside is a
// finding) or "refused NAME REASON" (a script the parser must refuse with that DD_JPEG_R_* and a message).  The scans are decoded level by
// level, as the kernel launches them, not in file order.  Exit status 0 when all is well.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>
#include "../deepdish_amd/csrc/jpeg_dec_dev.h"

static std::vector<uint8_t> slurp(const std::string &path, bool *ok) {
    std::ifstream f(path, std::ios::binary);
    *ok = (bool)f;
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// What jpeg_prog_markers_k does for one scan.  Returns false for a wrong marker count or sequence.
static bool markers(const uint8_t *scan, uint32_t len, int n_int, std::vector<uint32_t> &start, std::vector<uint32_t> &end) {
    start.assign((size_t)n_int + 1, 0), end.assign((size_t)n_int + 1, 0);
    int k = 0;
    for (uint32_t p = 0; p + 1 < len; ++p) {
        const int m = jpd_rst_at(scan, p);
        if (m < 0) continue;
        if (m != (k & 7) || k + 1 >= n_int) return false;
        end[k] = p;
        start[++k] = p + 2;
        ++p;
    }
    end[k] = len;
    return k + 1 == n_int;
}

// Returns the frame's status; *reason is the parser's.
static int decode(const std::vector<uint8_t> &file, std::vector<int16_t> &coef, int *reason, long long *checksum) {
    dd_jpeg_info r;
    std::unique_ptr<dd_jpeg_scans> S(new dd_jpeg_scans);
    char msg[320];
    msg[0] = 0;
    std::vector<uint8_t> exact(file);          // an exact-size copy: a read past the file's end is a finding
    *reason = jpd_parse_scans(exact.data(), exact.size(), &r, S.get(), msg, sizeof(msg));
    if (*reason != DD_JPEG_R_OK) {
        if (!msg[0] || S->n_scans != 0) {
            std::fprintf(stderr, "jpeg_prog_check: a refusal without a message, or with scans left in the record\n");
            std::exit(1);
        }
        return DD_JPEG_ST_HEADER;
    }
    const int mcus = r.mcus_x * r.mcus_y;
    coef.assign((size_t)mcus * r.blocks_per_mcu * 64, 0);
    int status = DD_JPEG_ST_OK;
    if (S->n_scans == 0) {                     // a baseline file: what scripts/jpeg_decode_check.cpp covers, here only decoded
        const uint8_t *scan = exact.data() + r.scan_offset;
        const int ri = r.restart_interval ? r.restart_interval : mcus;
        std::vector<uint32_t> start, end;
        if (!markers(scan, (uint32_t)r.scan_length, r.n_intervals, start, end)) return DD_JPEG_ST_DATA;
        for (int iv = 0; iv < r.n_intervals; ++iv)
            if (jpd_decode_interval(r, scan, start[iv], end[iv], iv * ri, mcus - iv * ri < ri ? mcus - iv * ri : ri, coef.data()) != DD_JPEG_ST_OK) status = DD_JPEG_ST_DATA;
    } else {
        std::vector<std::vector<uint32_t>> start((size_t)S->n_scans), end((size_t)S->n_scans);
        for (int i = 0; i < S->n_scans; ++i) {
            const dd_jpeg_scan &sc = S->scan[i];
            if ((size_t)sc.offset + (size_t)sc.length > exact.size() || sc.level < 0 || sc.level >= S->n_levels) {
                std::fprintf(stderr, "jpeg_prog_check: scan %d lies outside the file, or its level outside the file's levels\n", i);
                std::exit(1);
            }
            if (!markers(exact.data() + sc.offset, (uint32_t)sc.length, sc.n_intervals, start[i], end[i])) status = DD_JPEG_ST_DATA;
        }
        if (status != DD_JPEG_ST_OK) return status;
        for (int level = 0; level < S->n_levels; ++level)
            for (int i = S->n_scans - 1; i >= 0; --i) {          // within a level the order must not matter: take the reverse of the file's
                const dd_jpeg_scan &sc = S->scan[i];
                if (sc.level != level) continue;
                const int units = sc.blocks_x * sc.blocks_y, ri = sc.restart_interval ? sc.restart_interval : units;
                for (int iv = sc.n_intervals - 1; iv >= 0; --iv)
                    if (jpd_prog_decode_interval(r, sc, S->pool, exact.data() + sc.offset, start[i][iv], end[i][iv], iv * ri, units - iv * ri < ri ? units - iv * ri : ri,
                                                 coef.data()) != DD_JPEG_ST_OK)
                        status = DD_JPEG_ST_DATA;
            }
    }
    // the transform, on whatever was decoded: hostile coefficients must not trip the undefined-behaviour sanitizer
    const int ny = r.blocks_per_mcu == 1 ? 1 : r.blocks_per_mcu - 2;
    for (size_t b = 0; b < coef.size() / 64; ++b) {
        const int kk = (int)(b % r.blocks_per_mcu), c = kk < ny ? 0 : kk - ny + 1;
        int32_t d[64];
        for (int i = 0; i < 64; ++i) d[i] = coef[b * 64 + i] * (int32_t)r.quant[r.tq[c]][i];
        jpd_idct(d);
        for (int i = 0; i < 64; ++i) *checksum += d[i];
    }
    return status;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_prog_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream index(dir + "/index.txt");
    if (!index) {
        std::fprintf(stderr, "jpeg_prog_check: no %s/index.txt\n", dir.c_str());
        return 2;
    }
    std::string kind, name;
    long long checksum = 0;
    int valid = 0, damaged = 0, refused = 0, by_status[5] = {0, 0, 0, 0, 0};
    while (index >> kind >> name) {
        int want_reason = 0;
        if (kind == "refused") index >> want_reason;
        bool ok;
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpg", &ok);
        if (!ok) {
            std::fprintf(stderr, "jpeg_prog_check: cannot read %s\n", name.c_str());
            return 1;
        }
        std::vector<int16_t> coef;
        int reason = 0;
        const int status = decode(file, coef, &reason, &checksum);
        if (kind == "valid") {
            const std::vector<uint8_t> want = slurp(dir + "/" + name + ".coef", &ok);
            if (!ok || status != DD_JPEG_ST_OK || want.size() != coef.size() * 2 || std::memcmp(want.data(), coef.data(), want.size()) != 0) {
                std::fprintf(stderr, "jpeg_prog_check: %s: status %d (reason %d), %zu coefficients against %zu expected%s\n", name.c_str(), status, reason, coef.size(),
                             want.size() / 2, ok && want.size() == coef.size() * 2 ? ", and they differ" : "");
                return 1;
            }
            ++valid;
        } else if (kind == "refused") {
            if (status != DD_JPEG_ST_HEADER || reason != want_reason) {
                std::fprintf(stderr, "jpeg_prog_check: %s: status %d, reason %d where %d belongs\n", name.c_str(), status, reason, want_reason);
                return 1;
            }
            ++refused;
        } else {
            ++damaged;
            ++by_status[status];
        }
    }
    std::printf("jpeg_prog_check: %d valid files decoded to the expected coefficients; %d scripts refused by name; %d damaged files: status 0 for %d, header %d, data %d "
                "(checksum %lld)\n",
                valid, refused, damaged, by_status[0], by_status[1], by_status[3], checksum);
    return valid > 0 && damaged > 0 && refused > 0 ? 0 : 1;
}
