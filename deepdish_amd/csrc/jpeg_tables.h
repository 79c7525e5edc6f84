// Host side of csrc/jpeg.hip, plain C++ (no HIP): ITU-T T.81 Annex K tables, libjpeg's quality rule, the canonical Huffman codes and the
// file header.  scripts/jpeg_header_check.cpp builds this alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>
#include <vector>

static constexpr int JP_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                                  62, 63};
// ITU-T T.81 Annex K.1 / K.2 (natural order) and K.3
static constexpr uint8_t JP_Q_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                                      95, 98, 112, 100, 103, 99};
static constexpr uint8_t JP_Q_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99};
static constexpr uint8_t JP_DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static constexpr uint8_t JP_DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static constexpr uint8_t JP_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr uint8_t JP_AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static constexpr uint8_t JP_AC_LUMA_VALS[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
    36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
    73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
    178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
    217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
static constexpr uint8_t JP_AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static constexpr uint8_t JP_AC_CHROMA_VALS[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
    21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
    71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
    122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
    168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
    214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};

inline void jp_huffman(const uint8_t *bits, const uint8_t *vals, uint32_t *out) {         // Annex C: canonical codes in order of length
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}

inline void jp_quant(int quality, uint8_t (*q)[64]) {              // libjpeg's jpeg_set_quality, force_baseline
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = ((t ? JP_Q_CHROMA : JP_Q_LUMA)[i] * s + 50) / 100;
            q[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

inline void jp_segment(std::vector<uint8_t> &out, int marker, const std::vector<uint8_t> &payload) {
    out.push_back(0xFF);
    out.push_back((uint8_t)marker);
    out.push_back((uint8_t)((payload.size() + 2) >> 8));
    out.push_back((uint8_t)((payload.size() + 2) & 255));
    out.insert(out.end(), payload.begin(), payload.end());
}

// SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI, SOS: what libjpeg writes in front of the scan.  Host only.
inline void jp_build_header(int h, int w, int quality, int restart_rows, std::vector<uint8_t> &out) {
    uint8_t q[2][64];
    jp_quant(quality, q);
    out.assign({0xFF, 0xD8});
    jp_segment(out, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        std::vector<uint8_t> p(1, (uint8_t)t);
        for (int k = 0; k < 64; ++k) p.push_back(q[t][JP_ZIGZAG[k]]);
        jp_segment(out, 0xDB, p);
    }
    jp_segment(out, 0xC0, {8, (uint8_t)(h >> 8), (uint8_t)(h & 255), (uint8_t)(w >> 8), (uint8_t)(w & 255), 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    const struct { int id; const uint8_t *bits, *vals; int n; } dht[4] = {{0x00, JP_DC_LUMA_BITS, JP_DC_VALS, 12}, {0x10, JP_AC_LUMA_BITS, JP_AC_LUMA_VALS, 162},
                                                                          {0x01, JP_DC_CHROMA_BITS, JP_DC_VALS, 12}, {0x11, JP_AC_CHROMA_BITS, JP_AC_CHROMA_VALS, 162}};
    for (const auto &t : dht) {
        std::vector<uint8_t> p(1, (uint8_t)t.id);
        p.insert(p.end(), t.bits, t.bits + 16);
        p.insert(p.end(), t.vals, t.vals + t.n);
        jp_segment(out, 0xC4, p);
    }
    const int interval = restart_rows * ((w + 15) / 16);
    jp_segment(out, 0xDD, {(uint8_t)(interval >> 8), (uint8_t)(interval & 255)});
    jp_segment(out, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

