// Retained feature rows: with one detector-skip counter per stream (dd_pipeline_detector_skip_streams) a stream on a skip step pairs its
// boxes with the rows of ITS OWN last encoder run (deepdish.py:1003-1014), however many encoder runs of other streams -- each of which
// overwrites the encoder's output buffer -- and steps without a frame lie in between.  The rows live in a store in HBM, compact in stream
// order; this kernel is the one launch a mixed step spends on it:
//   * it assembles the tracker's input rows (streams of the step in order: fresh encoder rows for those that ran the detector, the
//     first min(kept boxes, retained rows) store rows for those that skipped), and
//   * it writes the next store (the fresh rows of the streams that ran the encoder replace what they had; everything else is carried).
// Pure copy.  One block per table entry; an entry reads n = max(n_out, n_store) rows once and writes them to up to two places.  A row is
// 128 f32 = 32 units of 16 bytes: a lane moves up to four units per trip (loads first, then stores), 32 rows per trip of a block.  Row offsets become 64-bit unit offsets
// before they touch a pointer (row 4 194 304 starts at 2^31 bytes).  No LDS, no atomics, nothing reused to tile for; a stream without
// rows has no entry, so it costs nothing.  Algorithmic bytes: 512 read + 512 written per destination, per row.
#include "common.h"
#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr int ROW_UNITS = 32;              // 16-byte units in a 128-f32 row

// table: per entry two int4 -- {sel (0 fresh / 1 store), src row, n_out, dst row in out} {n_store, dst row in store_new, 0, 0}
__global__ __launch_bounds__(256) void feature_rows_carry_k(const uint4 *__restrict__ fresh, const uint4 *__restrict__ store,
                                                            uint4 *__restrict__ out, uint4 *__restrict__ store_new,
                                                            const int4 *__restrict__ table) {
    const int4 a = table[2 * (size_t)blockIdx.x], b = table[2 * (size_t)blockIdx.x + 1];
    const uint4 *sp = (a.x ? store : fresh) + (size_t)a.y * ROW_UNITS;
    const int u_out = a.z * ROW_UNITS, u_store = b.x * ROW_UNITS, u = u_out > u_store ? u_out : u_store;
    uint4 *op = out + (size_t)a.w * ROW_UNITS, *np = store_new + (size_t)b.y * ROW_UNITS;      // (never dereferenced where their count is 0)
    for (int i0 = threadIdx.x; i0 < u; i0 += 1024) {              // four units per lane and trip, all loads issued before the first store
        const int i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
        uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};                  // (four named registers, not an array: see frames_gather_k)
        v0 = sp[i0];
        if (i1 < u) v1 = sp[i1];
        if (i2 < u) v2 = sp[i2];
        if (i3 < u) v3 = sp[i3];
        if (i0 < u_out) op[i0] = v0;
        if (i1 < u_out) op[i1] = v1;
        if (i2 < u_out) op[i2] = v2;
        if (i3 < u_out) op[i3] = v3;
        if (i0 < u_store) np[i0] = v0;
        if (i1 < u_store) np[i1] = v1;
        if (i2 < u_store) np[i2] = v2;
        if (i3 < u_store) np[i3] = v3;
    }
}

}  // namespace

namespace ddk {

// d_table: device, n_entries x 8 ints as above; entries with no rows are not in it.  No range is checked here or by the kernel: the
// pipeline's tables come from ddhost::feature_row_table (host_phases.h), whose every range the sanitizer harness holds to its buffer
// (tests/sanitize/host_harness.cpp); dd_feature_rows_carry below checks a caller's own table.
int feature_rows_carry(hipStream_t s, const float *fresh, const float *store, float *out, float *store_new, const int *d_table, int n_entries) {
    if (n_entries <= 0) return DD_OK;
    hipLaunchKernelGGL(feature_rows_carry_k, dim3((unsigned)n_entries), dim3(256), 0, s, reinterpret_cast<const uint4 *>(fresh),
                       reinterpret_cast<const uint4 *>(store), reinterpret_cast<uint4 *>(out), reinterpret_cast<uint4 *>(store_new),
                       reinterpret_cast<const int4 *>(d_table));
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

// The kernel alone.  table_host: n_streams x 6 ints {sel, src_row, n_out, dst_out_row, n_store, dst_store_row}: stream z reads rows
// [src_row, src_row + max(n_out, n_store)) of fresh_dev (sel 0) or store_dev (sel 1), writes the first n_out of them to rows_out_dev at
// dst_out_row and the first n_store to store_out_dev at dst_store_row.  *_rows: the rows each buffer holds -- every range is checked
// against them here, on the host, never by a faulting kernel.  Destination ranges must not overlap one another.  Synchronous.
extern "C" int dd_feature_rows_carry(dd_ctx *ctx, const float *fresh_dev, int64_t fresh_rows, const float *store_dev, int64_t store_rows,
                                     float *rows_out_dev, int64_t out_rows, float *store_out_dev, int64_t store_out_rows, const int *table_host,
                                     int n_streams, void *stream) {
    DD_REQUIRE(ctx && n_streams >= 0 && fresh_rows >= 0 && store_rows >= 0 && out_rows >= 0 && store_out_rows >= 0, DD_E_ARG,
               "dd_feature_rows_carry: bad argument (n_streams %d)", n_streams);
    if (n_streams == 0) return DD_OK;
    DD_REQUIRE(table_host, DD_E_ARG, "dd_feature_rows_carry: NULL table");
    const uintptr_t bits = reinterpret_cast<uintptr_t>(fresh_dev) | reinterpret_cast<uintptr_t>(store_dev) | reinterpret_cast<uintptr_t>(rows_out_dev) |
                           reinterpret_cast<uintptr_t>(store_out_dev);
    DD_REQUIRE((bits & 15) == 0, DD_E_ARG, "dd_feature_rows_carry: the buffers must be 16-byte aligned");
    std::vector<int> packed;
    std::vector<std::pair<int64_t, int64_t>> w_out, w_store;
    for (int z = 0; z < n_streams; ++z) {
        const int *t = table_host + (size_t)z * 6;
        const int sel = t[0], n_out = t[2], n_store = t[4], n = std::max(n_out, n_store);
        DD_REQUIRE((sel == 0 || sel == 1) && n_out >= 0 && n_store >= 0 && n <= (1 << 20), DD_E_ARG,
                   "dd_feature_rows_carry: stream %d: sel %d, n_out %d, n_store %d", z, sel, n_out, n_store);
        if (n == 0) continue;
        const int64_t have = sel ? store_rows : fresh_rows;
        DD_REQUIRE((sel ? store_dev : fresh_dev) && t[1] >= 0 && (int64_t)t[1] + n <= have, DD_E_ARG,
                   "dd_feature_rows_carry: stream %d reads rows [%d, %d) of source %d, which holds %lld", z, t[1], t[1] + n, sel, (long long)have);
        DD_REQUIRE(n_out == 0 || (rows_out_dev && t[3] >= 0 && (int64_t)t[3] + n_out <= out_rows), DD_E_ARG,
                   "dd_feature_rows_carry: stream %d writes rows [%d, %d) of an output of %lld", z, t[3], t[3] + n_out, (long long)out_rows);
        DD_REQUIRE(n_store == 0 || (store_out_dev && t[5] >= 0 && (int64_t)t[5] + n_store <= store_out_rows), DD_E_ARG,
                   "dd_feature_rows_carry: stream %d writes rows [%d, %d) of a store of %lld", z, t[5], t[5] + n_store, (long long)store_out_rows);
        if (n_out) w_out.emplace_back(t[3], t[3] + n_out);
        if (n_store) w_store.emplace_back(t[5], t[5] + n_store);
        const int e[8] = {sel, t[1], n_out, n_out ? t[3] : 0, n_store, n_store ? t[5] : 0, 0, 0};
        packed.insert(packed.end(), e, e + 8);
    }
    for (auto *w : {&w_out, &w_store}) {
        std::sort(w->begin(), w->end());
        for (size_t i = 1; i < w->size(); ++i)
            DD_REQUIRE((*w)[i].first >= (*w)[i - 1].second, DD_E_ARG, "dd_feature_rows_carry: two streams write overlapping rows [%lld, %lld) and [%lld, %lld)",
                       (long long)(*w)[i - 1].first, (long long)(*w)[i - 1].second, (long long)(*w)[i].first, (long long)(*w)[i].second);
    }
    if (packed.empty()) return DD_OK;
    DD_DEVICE(ctx);
    hipStream_t s = dd_pick_stream(ctx, stream);
    int rc;
    const size_t bytes = packed.size() * sizeof(int);
    if ((rc = ctx->scratch[0].reserve(bytes)) != DD_OK) return rc;
    if ((rc = ctx->pin[0].reserve(bytes)) != DD_OK) return rc;
    memcpy(ctx->pin[0].p, packed.data(), bytes);
    DD_HIP(hipMemcpyAsync(ctx->scratch[0].p, ctx->pin[0].p, bytes, hipMemcpyHostToDevice, s));
    if ((rc = ddk::feature_rows_carry(s, fresh_dev, store_dev, rows_out_dev, store_out_dev, ctx->scratch[0].as<int>(), (int)(packed.size() / 8))) != DD_OK) return rc;
    DD_HIP(hipStreamSynchronize(s));                          // the table's staging buffers are the context's: free for the next call
    return DD_OK;
}
