// Foreground pixels per stream: np.count_nonzero of whole mask planes, for the streams an index list names -- what the motion gate of
// the batched pipeline (dd_pipeline_motion_gate) asks after MOG2 and before the detector.  Any non-zero byte counts: MOG2 writes 0,
// 127 (shadow) and 255, and the reference's count_nonzero (deepdish.py:957) counts shadows.
//
// Pure read, one launch, grid (chunks, n): block (c, i) counts chunk c of plane streams[i].  Algorithmic bytes: H * W read per listed
// plane, one dword per wave that found something written.  A plane is H * W bytes behind the one before it, so with H * W no multiple
// of 16 it starts anywhere: up to 15 head bytes to the next 16-byte address and up to 15 tail bytes are counted byte by byte (block 0
// of the plane, one lane each), everything between as 16-byte loads, four per lane and all issued before the first is used.  A dword
// counts its non-zero bytes in five integer instructions; a wave sums its 64 lanes by shuffles and lane 0 adds the sum to the plane's
// counter -- an integer add, so the result is the same in every run whatever order the waves arrive in.  Waves that found nothing (most
// of them on a corridor at night) add nothing.  Offsets are 64-bit: plane 7 000 of 640 x 480 starts past 2^31 bytes.  No LDS.
#include <algorithm>
#include "common.h"

namespace {

constexpr int COUNT_UNITS = 256 * 4;       // 16-byte units one block counts: four per lane

// non-zero bytes of a dword: bit 7 of every byte <- (low seven bits != 0) | bit 7, then a population count
__device__ __forceinline__ int nonzero_bytes(uint32_t w) {
    return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u);
}
__device__ __forceinline__ int nonzero_bytes(const uint4 v) {
    return nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
}

__global__ __launch_bounds__(256) void mask_stream_count_k(const uint8_t *__restrict__ mask, const long long hw, const int *__restrict__ streams,
                                                           int *__restrict__ counts) {
    const int i = blockIdx.y;
    const uint8_t *m = mask + (size_t)(streams ? streams[i] : i) * (size_t)hw;
    const long long to16 = (long long)((16 - (reinterpret_cast<uintptr_t>(m) & 15)) & 15), head = to16 < hw ? to16 : hw;
    const long long units = (hw - head) >> 4, tail = hw - head - (units << 4);
    const uint4 *body = reinterpret_cast<const uint4 *>(m + head);
    int c = 0;
    const long long u0 = (long long)blockIdx.x * COUNT_UNITS + threadIdx.x, u1 = u0 + 256, u2 = u0 + 512, u3 = u0 + 768;
    uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (u0 < units) v0 = body[u0];
    if (u1 < units) v1 = body[u1];
    if (u2 < units) v2 = body[u2];
    if (u3 < units) v3 = body[u3];
    c = nonzero_bytes(v0) + nonzero_bytes(v1) + nonzero_bytes(v2) + nonzero_bytes(v3);
    if (blockIdx.x == 0 && threadIdx.x < 32) {                 // lanes 0 .. 15: head byte, lanes 16 .. 31: tail byte
        const int t = threadIdx.x & 15;
        if (threadIdx.x < 16) { if (t < head) c += m[t] != 0; }
        else if (t < tail) c += m[head + (units << 4) + t] != 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + i, c);
}

}  // namespace

namespace ddk {

// mask: device u8 planes of H * W bytes behind one another; d_streams: device int32 [n], every value a plane of mask (the caller has
// checked them), or NULL = planes 0 .. n - 1; d_counts: device int32 [n], cleared and then summed into on s.  n <= 65 535 (grid.y).
int mask_stream_count(hipStream_t s, const uint8_t *mask, int H, int W, const int *d_streams, int n, int *d_counts) {
    if (n <= 0) return DD_OK;
    DD_REQUIRE(n <= 65535, DD_E_ARG, "dd_mask_stream_count: %d planes in one launch (<= 65535)", n);
    const long long hw = (long long)H * W, chunks = std::max<long long>(1, ((hw >> 4) + COUNT_UNITS - 1) / COUNT_UNITS);
    DD_REQUIRE(hw > 0 && chunks <= 0x7fffffffll, DD_E_ARG, "dd_mask_stream_count: planes of %lld bytes", hw);
    DD_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(int), s));
    hipLaunchKernelGGL(mask_stream_count_k, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, mask, hw, d_streams, d_counts);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

extern "C" int dd_mask_stream_count(dd_ctx *ctx, const uint8_t *mask_dev, int n_streams, int height, int width, const int *streams_host, int n,
                                    int *counts_host) {
    DD_REQUIRE(ctx && mask_dev && n_streams > 0 && height > 0 && width > 0 && n >= 0 && n <= 65535 && (n == 0 || counts_host), DD_E_ARG,
               "dd_mask_stream_count: bad argument (n_streams %d, %d x %d, n %d)", n_streams, width, height, n);
    DD_REQUIRE(streams_host || n == n_streams, DD_E_ARG, "dd_mask_stream_count: no stream list means all %d streams, n = %d", n_streams, n);
    for (int i = 0; streams_host && i < n; ++i)               // checked here, never by a faulting kernel
        DD_REQUIRE(streams_host[i] >= 0 && streams_host[i] < n_streams, DD_E_ARG, "dd_mask_stream_count: streams[%d] = %d of %d", i,
                   streams_host[i], n_streams);
    DD_DEVICE(ctx);
    if (n == 0) return DD_OK;
    hipStream_t s = ctx->stream;
    int rc;
    const size_t bytes = (size_t)n * sizeof(int);
    if ((rc = ctx->scratch[0].reserve(2 * bytes)) != DD_OK) return rc;
    if ((rc = ctx->pin[0].reserve(2 * bytes)) != DD_OK) return rc;
    int *h = ctx->pin[0].as<int>(), *d = ctx->scratch[0].as<int>();
    if (streams_host) {
        memcpy(h, streams_host, bytes);
        DD_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = ddk::mask_stream_count(s, mask_dev, height, width, streams_host ? d : nullptr, n, d + n)) != DD_OK) return rc;
    DD_HIP(hipMemcpyAsync(h + n, d + n, bytes, hipMemcpyDeviceToHost, s));
    DD_HIP(hipStreamSynchronize(s));
    memcpy(counts_host, h + n, bytes);
    return DD_OK;
}
