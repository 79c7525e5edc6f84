// Pillow's Lanczos coefficient tables (precompute_coeffs + normalize_coeffs_8bpc), defined in image.hip and shared with letterbox.hip.
#pragma once
#include <vector>

namespace ddk {

struct LanczosTable {                     // host: bounds = (first source index, taps) per output, kk = ksize 22-bit coefficients per output
    int ksize = 0;
    std::vector<int> bounds, kk;
};
struct DevTable { int ksize; int *bounds; int *kk; };      // the same arrays, device-resident

int lanczos_ksize(int in_size, int out_size);              // taps per output
LanczosTable make_table(int in_size, int out_size);        // host only
int get_table(int device, int in_size, int out_size, DevTable *out);      // cached per (device, in, out); uploads on first use

}  // namespace ddk
