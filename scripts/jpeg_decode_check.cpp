// Stand-alone check of the JPEG decoder's shared statements (csrc/jpeg_parse.h: the header parser; csrc/jpeg_dec_dev.h: the bit reader,
// the Huffman decoder, the interval loop and the IDCT, the very code the kernels of csrc/jpeg_dec.hip run) under the address and
// undefined-behaviour sanitizers.  Plain C++, no GPU, not loaded into Python:
//
//     python scripts/make_jpeg_corpus.py DIR
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_decode_check.cpp -o jpeg_decode_check
//     ./jpeg_decode_check DIR
//
// DIR/index.txt lists one file per line: "valid NAME" (NAME.jpg with NAME.coef, the int16 coefficients tests/jpeg_dec_ref.py gives; the
// program must decode exactly those) or "damaged NAME" (truncated or with a byte replaced: the program must come back with a status,
// whatever it is, and no sanitizer finding; the coefficient buffer is exactly as large as the header implies, so a store outside a
// frame's own blocks is a finding).  Hostile input is exercised here, exhaustively, and not on the card.  Exit status 0 when all is well.
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

// What jpeg_markers_k, jpeg_entropy_k and the transform of jpeg_pixels_k do for one file, serially.  Returns the frame's status.
static int decode(const std::vector<uint8_t> &file, std::vector<int16_t> &coef, long long *checksum) {
    dd_jpeg_info r;
    char msg[256];
    // an exact-size copy: a read past the file's end is a finding
    std::vector<uint8_t> exact(file);
    if (jpd_parse(exact.data(), exact.size(), &r, msg, sizeof(msg)) != DD_JPEG_R_OK) {
        if (!msg[0]) {
            std::fprintf(stderr, "jpeg_decode_check: a refusal without a message\n");
            std::exit(1);
        }
        return DD_JPEG_ST_HEADER;
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
    // the transform, on whatever was decoded: hostile coefficients must not trip the undefined-behaviour sanitizer
    const int ny = r.blocks_per_mcu == 1 ? 1 : r.blocks_per_mcu - 2;
    for (size_t b = 0; b < coef.size() / 64; ++b) {
        const int kk = (int)(b % r.blocks_per_mcu), c = kk < ny ? 0 : kk - ny + 1;
        int32_t d[64];
        for (int i = 0; i < 64; ++i) d[i] = coef[b * 64 + i] * (int32_t)r.quant[r.tq[c]][i];
        jpd_idct(d);
        for (int i = 0; i < 64; ++i) {
            if (d[i] < 0 || d[i] > 255) {
                std::fprintf(stderr, "jpeg_decode_check: a sample of %d\n", d[i]);
                std::exit(1);
            }
            *checksum += d[i];
        }
        *checksum += jpd_bgr(d[0], d[1], d[2]);
    }
    return status;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_decode_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream index(dir + "/index.txt");
    if (!index) {
        std::fprintf(stderr, "jpeg_decode_check: no %s/index.txt\n", dir.c_str());
        return 2;
    }
    std::string kind, name;
    long long checksum = 0;
    int valid = 0, damaged = 0, by_status[5] = {0, 0, 0, 0, 0};
    while (index >> kind >> name) {
        bool ok;
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpg", &ok);
        if (!ok) {
            std::fprintf(stderr, "jpeg_decode_check: cannot read %s\n", name.c_str());
            return 1;
        }
        std::vector<int16_t> coef;
        const int status = decode(file, coef, &checksum);
        if (kind == "valid") {
            const std::vector<uint8_t> want = slurp(dir + "/" + name + ".coef", &ok);
            if (!ok || status != DD_JPEG_ST_OK || want.size() != coef.size() * 2 || std::memcmp(want.data(), coef.data(), want.size()) != 0) {
                std::fprintf(stderr, "jpeg_decode_check: %s: status %d, %zu coefficients against %zu expected%s\n", name.c_str(), status, coef.size(), want.size() / 2,
                             ok && want.size() == coef.size() * 2 ? ", and they differ" : "");
                return 1;
            }
            ++valid;
        } else {
            ++damaged;
            ++by_status[status];
        }
    }
    std::printf("jpeg_decode_check: %d valid files decoded to the expected coefficients; %d damaged files: status 0 for %d, header %d, data %d (checksum %lld)\n",
                valid, damaged, by_status[0], by_status[1], by_status[3], checksum);
    return valid > 0 && damaged > 0 ? 0 : 1;
}
