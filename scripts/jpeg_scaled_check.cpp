// Stand-alone run of the scaled decoder's host-callable statements (csrc/jpeg_dec_dev.h: jpd_idct4, jpd_idct2, jpd_idct1, jpd_plane) under
// the address and undefined-behaviour sanitizers.  Plain C++, no GPU, not loaded into Python:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_scaled_check.cpp -o jpeg_scaled_check
//     ./jpeg_scaled_check IN OUT
//
// IN, little-endian: int32 K, then K blocks of { int32 n (4, 2 or 1); int16 coef[64]; uint16 quant[64] }, natural order; int32 M, then M
// queries of { int32 h, w, hs, vs, hmax, vmax, s }.  OUT: per block its n * n samples, row by row, one byte each; then per query int32 n,
// rows, cols.  tests/test_jpeg_scaled_host.py writes IN and compares OUT with tests/jpeg_scaled_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../deepdish_amd/csrc/jpeg_dec_dev.h"

static void fail(const char *what) {
    std::fprintf(stderr, "jpeg_scaled_check: %s\n", what);
    std::exit(1);
}

static int32_t take32(const std::vector<uint8_t> &in, size_t &at) {
    if (at + 4 > in.size()) fail("the input ends inside a record");
    int32_t v;
    std::memcpy(&v, in.data() + at, 4);
    at += 4;
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) fail("usage: jpeg_scaled_check IN OUT");
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) fail("cannot open IN");
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    std::vector<uint8_t> out;
    size_t at = 0;
    const int32_t K = take32(in, at);
    if (K < 0) fail("a negative block count");
    for (int32_t k = 0; k < K; ++k) {
        const int32_t n = take32(in, at);
        if (at + 256 > in.size()) fail("the input ends inside a block");
        int16_t c[64];
        uint16_t q[64];
        std::memcpy(c, in.data() + at, 128);
        std::memcpy(q, in.data() + at + 128, 128);
        at += 256;
        int32_t d[64];
        for (int i = 0; i < 64; ++i) d[i] = (int32_t)c[i] * (int32_t)q[i];
        if (n == 4) {
            int o[16];
            jpd_idct4(d, o);
            for (int v : o) out.push_back((uint8_t)v);
        } else if (n == 2) {
            int o[4];
            jpd_idct2(d, o);
            for (int v : o) out.push_back((uint8_t)v);
        } else if (n == 1) {
            out.push_back((uint8_t)jpd_idct1(d[0]));
        } else
            fail("a block size that is none of 4, 2, 1");
    }
    const int32_t M = take32(in, at);
    if (M < 0) fail("a negative query count");
    for (int32_t m = 0; m < M; ++m) {
        int32_t a[7];
        for (int32_t &v : a) v = take32(in, at);
        if (!jpd_scale_ok(a[6]) || a[0] < 1 || a[1] < 1 || a[0] > JPD_MAX_SIDE || a[1] > JPD_MAX_SIDE || a[2] < 1 || a[3] < 1 || a[2] > a[4] || a[3] > a[5] || a[4] > 2 || a[5] > 2)
            fail("a query outside what the decoder accepts");
        const JpdPlane p = jpd_plane(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
        const int32_t r[3] = {p.n, p.rows, p.cols};
        const uint8_t *b = reinterpret_cast<const uint8_t *>(r);
        out.insert(out.end(), b, b + 12);
    }
    if (at != in.size()) fail("bytes behind the last query");
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) fail("cannot write OUT");
    std::printf("jpeg_scaled_check: %d blocks, %d plane queries\n", (int)K, (int)M);
    return 0;
}
