// Stand-alone check of the default Huffman tables (DD_JPEGDEC_STD_TABLES; csrc/jpeg_parse.h jpd_huffman_std) under the address and
// undefined-behaviour sanitizers: the flagged parser, then the very interval loop the kernels run (csrc/jpeg_dec_dev.h
// jpd_decode_interval) with the tables it filled in.  Plain C++, no GPU, not loaded into Python:
//
//     python scripts/make_jpeg_std_corpus.py DIR
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_std_tables_check.cpp -o jpeg_std_tables_check
//     ./jpeg_std_tables_check DIR
//
// DIR/index.txt lists one file per line: "valid NAME" (NAME.jpg, a file without some or all of its DHT tables, with NAME.coef, the int16
// coefficients tests/jpeg_dec_ref.py gives for the file it was stripped from: the program must decode exactly those, and the parser
// without the flag must refuse the file as undefined or take it as it is) or "damaged NAME" (such a file truncated or with a byte replaced:
// the program must come back with a status, whatever it is, and no sanitizer finding; the coefficient buffer is exactly as large as the
// header implies).  Exit status 0 when all is well.
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

// What the host and jpeg_markers_k, jpeg_entropy_k do for one file of a decoder made with the flag, serially.  Returns the frame's status.
static int decode(const std::vector<uint8_t> &file, std::vector<int16_t> &coef, int *plain_reason) {
    dd_jpeg_info r, plain;
    char msg[256];
    std::vector<uint8_t> exact(file);                           // an exact-size copy: a read past the file's end is a finding
    *plain_reason = jpd_parse(exact.data(), exact.size(), &plain, msg, sizeof(msg));
    if (jpd_parse(exact.data(), exact.size(), &r, msg, sizeof(msg), DD_JPEGDEC_STD_TABLES) != DD_JPEG_R_OK) {
        if (!msg[0]) {
            std::fprintf(stderr, "jpeg_std_tables_check: a refusal without a message\n");
            std::exit(1);
        }
        return DD_JPEG_ST_HEADER;
    }
    for (int c = 0; c < r.ncomp; ++c)
        if (!r.huff[r.td[c]].defined || !r.huff[2 + r.ta[c]].defined) {
            std::fprintf(stderr, "jpeg_std_tables_check: an accepted file with an undefined table\n");
            std::exit(1);
        }
    const uint8_t *scan = exact.data() + r.scan_offset;
    const uint32_t len = (uint32_t)r.scan_length;
    const int mcus = r.mcus_x * r.mcus_y, ri = r.restart_interval ? r.restart_interval : mcus;
    std::vector<uint32_t> start((size_t)r.n_intervals + 1, 0), end((size_t)r.n_intervals + 1, 0);
    int k = 0, status = DD_JPEG_ST_OK;
    for (uint32_t p = 0; p + 1 < len; ++p) {
        const int m = jpd_rst_at(scan, p);
        if (m < 0) continue;
        if (m != (k & 7) || k + 1 >= r.n_intervals) {
            status = DD_JPEG_ST_DATA;
            break;
        }
        end[k] = p;
        start[++k] = p + 2;
        ++p;
    }
    end[k] = len;
    if (k + 1 != r.n_intervals) status = DD_JPEG_ST_DATA;
    coef.assign((size_t)mcus * r.blocks_per_mcu * 64, 0);
    if (status != DD_JPEG_ST_OK) return status;
    for (int iv = 0; iv < r.n_intervals; ++iv) {
        const int m0 = iv * ri, nm = mcus - m0 < ri ? mcus - m0 : ri;
        if (jpd_decode_interval(r, scan, start[iv], end[iv], m0, nm, coef.data()) != DD_JPEG_ST_OK) status = DD_JPEG_ST_DATA;
    }
    return status;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_std_tables_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream index(dir + "/index.txt");
    if (!index) {
        std::fprintf(stderr, "jpeg_std_tables_check: no %s/index.txt\n", dir.c_str());
        return 2;
    }
    std::string kind, name;
    int valid = 0, filled = 0, damaged = 0, by_status[5] = {0, 0, 0, 0, 0};
    while (index >> kind >> name) {
        bool ok;
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpg", &ok);
        if (!ok) {
            std::fprintf(stderr, "jpeg_std_tables_check: cannot read %s\n", name.c_str());
            return 1;
        }
        std::vector<int16_t> coef;
        int plain = 0;
        const int status = decode(file, coef, &plain);
        if (kind == "valid") {
            const std::vector<uint8_t> want = slurp(dir + "/" + name + ".coef", &ok);
            if (!ok || status != DD_JPEG_ST_OK || want.size() != coef.size() * 2 || std::memcmp(want.data(), coef.data(), want.size()) != 0) {
                std::fprintf(stderr, "jpeg_std_tables_check: %s: status %d, %zu coefficients against %zu expected%s\n", name.c_str(), status, coef.size(), want.size() / 2,
                             ok && want.size() == coef.size() * 2 ? ", and they differ" : "");
                return 1;
            }
            if (plain != DD_JPEG_R_UNDEFINED && plain != DD_JPEG_R_OK) {
                std::fprintf(stderr, "jpeg_std_tables_check: %s: the parser without the flag gives reason %d\n", name.c_str(), plain);
                return 1;
            }
            filled += plain == DD_JPEG_R_UNDEFINED;
            ++valid;
        } else {
            ++damaged;
            ++by_status[status];
        }
    }
    std::printf("jpeg_std_tables_check: %d stripped files decoded to the expected coefficients (%d refused without the flag); %d damaged files: status 0 for %d, header %d, "
                "data %d\n", valid, filled, damaged, by_status[0], by_status[1], by_status[3]);
    return valid > 0 && filled > 0 && damaged > 0 ? 0 : 1;
}
