// Stand-alone check of the host side of csrc/jpeg.hip (csrc/jpeg_tables.h: quality scaling, canonical Huffman codes, the file header)
// under the address and undefined-behaviour sanitizers.  Plain C++, no GPU, not loaded into Python:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_header_check.cpp -o jpeg_header_check
//     ./jpeg_header_check
//
// Builds the header for every quality at several frame sizes and walks its segments; prints one line and exits 0 when all is well.
#include <cstdio>
#include <cstdlib>
#include "../deepdish_amd/csrc/jpeg_tables.h"

static void fail(const char *what, int h, int w, int q, int r) {
    std::fprintf(stderr, "jpeg_header_check: %s (h %d, w %d, quality %d, restart_rows %d)\n", what, h, w, q, r);
    std::exit(1);
}

int main() {
    const int sizes[][3] = {{1, 1, 1}, {480, 640, 1}, {720, 1280, 3}, {8192, 8192, 127}, {33, 47, 2}};
    const int want[10] = {0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA};
    size_t headers = 0;
    for (const auto &s : sizes)
        for (int q = 1; q <= 100; ++q) {
            std::vector<uint8_t> h;
            jp_build_header(s[0], s[1], q, s[2], h);
            if (h.size() < 4 || h[0] != 0xFF || h[1] != 0xD8) fail("no SOI", s[0], s[1], q, s[2]);
            size_t i = 2;
            int k = 0;
            while (i + 4 <= h.size()) {
                if (h[i] != 0xFF || k >= 10 || h[i + 1] != want[k]) fail("segment order", s[0], s[1], q, s[2]);
                const size_t len = ((size_t)h[i + 2] << 8) | h[i + 3];
                if (h[i + 1] == 0xDB)
                    for (size_t j = 1; j < 65; ++j)
                        if (h[i + 4 + j] < 1) fail("a zero quantiser", s[0], s[1], q, s[2]);
                if (h[i + 1] == 0xC0 && ((h[i + 5] << 8 | h[i + 6]) != s[0] || (h[i + 7] << 8 | h[i + 8]) != s[1])) fail("SOF0 size", s[0], s[1], q, s[2]);
                if (h[i + 1] == 0xDD && (h[i + 4] << 8 | h[i + 5]) != s[2] * ((s[1] + 15) / 16)) fail("DRI interval", s[0], s[1], q, s[2]);
                i += 2 + len;
                ++k;
            }
            if (i != h.size() || k != 10) fail("segment lengths", s[0], s[1], q, s[2]);
            ++headers;
        }
    // canonical codes: prefix-free by construction; every symbol of the four tables gets a length of 1 .. 16
    uint32_t ac[256] = {0}, dc[16] = {0};
    jp_huffman(JP_AC_LUMA_BITS, JP_AC_LUMA_VALS, ac);
    jp_huffman(JP_DC_CHROMA_BITS, JP_DC_VALS, dc);
    for (int i = 0; i < 162; ++i)
        if ((ac[JP_AC_LUMA_VALS[i]] & 31) < 1 || (ac[JP_AC_LUMA_VALS[i]] & 31) > 16) fail("AC code length", 0, 0, 0, 0);
    for (int i = 0; i < 12; ++i)
        if ((dc[i] & 31) < 2 || (dc[i] & 31) > 11) fail("DC code length", 0, 0, 0, 0);
    std::printf("jpeg_header_check: %zu headers ok\n", headers);
    return 0;
}
