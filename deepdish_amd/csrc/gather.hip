// Frame compaction: the n frames of a batch that an index list names, copied behind one another -- what a masked pipeline step
// (dd_pipeline_step3) does before the detector's resize, whose launches take a dense batch.
//
// Pure copy, one launch, grid (chunks, n): block (c, i) moves chunk c of frame idx[i] to chunk c of frame i.  Algorithmic bytes:
// frame_bytes read + frame_bytes written per listed frame, nothing else (the index is one dword per block).  A lane moves four units
// of 16 bytes (all loads issued before the first store) when both bases and frame_bytes are multiples of 16 -- 640x480x3 and 1280x720x3
// are -- of 4 bytes when they are multiples of 4, of 1 byte otherwise.  Offsets are 64-bit throughout: frame 2 400 of 640x480x3 starts
// past 2^31 bytes.  No LDS, no reuse to tile for.
#include "common.h"

namespace {

constexpr int GATHER_UNITS = 256 * 4;      // units of sizeof(T) one block moves: four per lane

template <class T>
__global__ __launch_bounds__(256) void frames_gather_k(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int *__restrict__ idx,
                                                       const long long frame_bytes, const long long units) {
    const size_t i = blockIdx.y;
    const T *sp = reinterpret_cast<const T *>(src + (size_t)idx[i] * (size_t)frame_bytes);
    T *dp = reinterpret_cast<T *>(dst + i * (size_t)frame_bytes);
    const long long u0 = (long long)blockIdx.x * GATHER_UNITS + threadIdx.x;
    // (four named registers, not an array: the compiler moved a guarded T v[4] into 16 KiB of LDS)
    const long long u1 = u0 + 256, u2 = u0 + 512, u3 = u0 + 768;
    T v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (u0 < units) v0 = sp[u0];
    if (u1 < units) v1 = sp[u1];
    if (u2 < units) v2 = sp[u2];
    if (u3 < units) v3 = sp[u3];
    if (u0 < units) dp[u0] = v0;
    if (u1 < units) dp[u1] = v1;
    if (u2 < units) dp[u2] = v2;
    if (u3 < units) dp[u3] = v3;
}

template <class T>
int launch(hipStream_t s, const uint8_t *src, long long frame_bytes, const int *d_idx, int n, uint8_t *dst) {
    const long long units = frame_bytes / (long long)sizeof(T), chunks = (units + GATHER_UNITS - 1) / GATHER_UNITS;
    DD_REQUIRE(chunks <= 0x7fffffffll, DD_E_ARG, "dd_gather_frames: frames of %lld bytes take too many blocks", frame_bytes);
    hipLaunchKernelGGL(frames_gather_k<T>, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, src, dst, d_idx, frame_bytes, units);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace

namespace ddk {

// d_idx: device int32 [n], every value a frame of src; the caller has checked them.  n <= 65 535 (grid.y).
int gather_frames(hipStream_t s, const uint8_t *src, long long frame_bytes, const int *d_idx, int n, uint8_t *dst) {
    if (n <= 0 || frame_bytes <= 0) return DD_OK;
    DD_REQUIRE(n <= 65535, DD_E_ARG, "dd_gather_frames: %d frames in one launch (<= 65535)", n);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)frame_bytes;
    if ((bits & 15) == 0) return launch<uint4>(s, src, frame_bytes, d_idx, n, dst);
    if ((bits & 3) == 0) return launch<uint32_t>(s, src, frame_bytes, d_idx, n, dst);
    return launch<uint8_t>(s, src, frame_bytes, d_idx, n, dst);
}

}  // namespace ddk

extern "C" int dd_gather_frames(dd_ctx *ctx, const uint8_t *src_dev, int n_src, int64_t frame_bytes, const int *idx_host, int n, uint8_t *dst_dev,
                                void *stream) {
    DD_REQUIRE(ctx && n_src >= 0 && frame_bytes > 0 && n >= 0 && n <= n_src, DD_E_ARG,
               "dd_gather_frames: bad argument (n_src %d, frame_bytes %lld, n %d)", n_src, (long long)frame_bytes, n);
    if (n == 0) return DD_OK;
    DD_REQUIRE(src_dev && dst_dev && idx_host, DD_E_ARG, "dd_gather_frames: NULL argument");
    for (int i = 0; i < n; ++i)                               // checked here, never by a faulting kernel
        DD_REQUIRE(idx_host[i] >= 0 && idx_host[i] < n_src && (i == 0 || idx_host[i] > idx_host[i - 1]), DD_E_ARG,
                   "dd_gather_frames: idx[%d] = %d -- the list must be strictly increasing and below %d", i, idx_host[i], n_src);
    DD_DEVICE(ctx);
    hipStream_t s = dd_pick_stream(ctx, stream);
    int rc;
    if ((rc = ctx->scratch[0].reserve((size_t)n * sizeof(int))) != DD_OK) return rc;
    if ((rc = ctx->pin[0].reserve((size_t)n * sizeof(int))) != DD_OK) return rc;
    memcpy(ctx->pin[0].p, idx_host, (size_t)n * sizeof(int));
    DD_HIP(hipMemcpyAsync(ctx->scratch[0].p, ctx->pin[0].p, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if ((rc = ddk::gather_frames(s, src_dev, (long long)frame_bytes, ctx->scratch[0].as<int>(), n, dst_dev)) != DD_OK) return rc;
    DD_HIP(hipStreamSynchronize(s));                          // the index list's staging buffers are the context's: free for the next call
    return DD_OK;
}
