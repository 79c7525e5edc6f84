// Stream snapshots: the two kernels that move galleries between their chunk lists and one dense buffer (dd_pipeline_snapshot /
// dd_pipeline_restore, csrc/pipeline.hip).  A gallery is a list of 32-row chunks scattered over the pool's 64 MiB arenas (csrc/tracker.hip);
// at 1 536 streams a snapshot moves gigabytes of them, and one copy per chunk would be tens of thousands of calls.
//   chunk_rows_gather_k : every listed track's rows, in storage order, to rows [dense row, + n) of one dense buffer -- and, for the
//                         pipeline, its mean and covariance (72 f64 = 36 units) to the state block behind the rows; one copy to the host follows
//   chunk_rows_scatter_k: the inverse, after restore has placed fresh chunks
// Pure copies in the style of feature_rows_carry_k (csrc/featrows.hip): one block per table entry; a row is 128 f32 = 32 units of 16
// bytes and a chunk 1 024 units that lie contiguously, so a trip of a block (four units per lane, loads first, then stores) moves one
// whole chunk with every wave on 1 KiB of consecutive addresses.  Row offsets become 64-bit unit offsets before they touch a pointer
// (dense row 4 194 304 starts at 2^31 bytes).  No LDS, no atomics.  Nothing is checked here: every range is checked on the host --
// dd_chunk_rows_gather / dd_chunk_rows_scatter check a caller's tables, the pipeline builds its own from the pool's chunk lists.
#include "common.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int ROW_UNITS = 32, CH_ROWS = 32;   // 16-byte units in a 128-f32 row; rows in a chunk (GAL_CH)
constexpr int STATE_UNITS = 36;               // mean 8 f64 + covariance 64 f64

// unit u of an entry's rows -> where it lies in the arenas
__device__ __forceinline__ size_t chunk_unit(const int *__restrict__ list, int u, int arena_shift, int *arena) {
    const int row = u >> 5, c = list[row >> 5];
    *arena = c >> arena_shift;
    return ((size_t)(c & ((1 << arena_shift) - 1)) * CH_ROWS + (row & (CH_ROWS - 1))) * ROW_UNITS + (u & (ROW_UNITS - 1));
}

// table: per entry int4 {offset of its chunk list in `chunks`, rows, first dense row, state slot or -1}
__global__ __launch_bounds__(256) void chunk_rows_gather_k(const uint4 *const *__restrict__ arenas, int arena_shift, const int *__restrict__ chunks,
                                                           const int4 *__restrict__ table, uint4 *__restrict__ dense,
                                                           const uint4 *__restrict__ means, const uint4 *__restrict__ covs, uint4 *__restrict__ state) {
    const int4 e = table[blockIdx.x];
    const int u = e.y * ROW_UNITS;
    const int *list = chunks + e.x;
    uint4 *dp = dense + (size_t)e.z * ROW_UNITS;
    for (int i0 = threadIdx.x; i0 < u; i0 += 1024) {
        const int i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
        uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
        int a;
        size_t o = chunk_unit(list, i0, arena_shift, &a);
        v0 = arenas[a][o];
        if (i1 < u) { o = chunk_unit(list, i1, arena_shift, &a); v1 = arenas[a][o]; }
        if (i2 < u) { o = chunk_unit(list, i2, arena_shift, &a); v2 = arenas[a][o]; }
        if (i3 < u) { o = chunk_unit(list, i3, arena_shift, &a); v3 = arenas[a][o]; }
        dp[i0] = v0;
        if (i1 < u) dp[i1] = v1;
        if (i2 < u) dp[i2] = v2;
        if (i3 < u) dp[i3] = v3;
    }
    if (e.w >= 0 && threadIdx.x < STATE_UNITS) {
        const int t = threadIdx.x;
        state[(size_t)blockIdx.x * STATE_UNITS + t] = t < 4 ? means[(size_t)e.w * 4 + t] : covs[(size_t)e.w * 32 + (t - 4)];
    }
}

__global__ __launch_bounds__(256) void chunk_rows_scatter_k(uint4 *const *__restrict__ arenas, int arena_shift, const int *__restrict__ chunks,
                                                            const int4 *__restrict__ table, const uint4 *__restrict__ dense,
                                                            uint4 *__restrict__ means, uint4 *__restrict__ covs, const uint4 *__restrict__ state) {
    const int4 e = table[blockIdx.x];
    const int u = e.y * ROW_UNITS;
    const int *list = chunks + e.x;
    const uint4 *sp = dense + (size_t)e.z * ROW_UNITS;
    for (int i0 = threadIdx.x; i0 < u; i0 += 1024) {
        const int i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
        uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
        v0 = sp[i0];
        if (i1 < u) v1 = sp[i1];
        if (i2 < u) v2 = sp[i2];
        if (i3 < u) v3 = sp[i3];
        int a;
        size_t o = chunk_unit(list, i0, arena_shift, &a);
        arenas[a][o] = v0;
        if (i1 < u) { o = chunk_unit(list, i1, arena_shift, &a); arenas[a][o] = v1; }
        if (i2 < u) { o = chunk_unit(list, i2, arena_shift, &a); arenas[a][o] = v2; }
        if (i3 < u) { o = chunk_unit(list, i3, arena_shift, &a); arenas[a][o] = v3; }
    }
    if (e.w >= 0 && threadIdx.x < STATE_UNITS) {
        const int t = threadIdx.x;
        const uint4 v = state[(size_t)blockIdx.x * STATE_UNITS + t];
        if (t < 4) means[(size_t)e.w * 4 + t] = v; else covs[(size_t)e.w * 32 + (t - 4)] = v;
    }
}

}  // namespace

namespace ddk {

// d_chunks / d_table: device; table n_entries x 4 ints as above.  means / covs / state may be NULL when no entry names a state slot.
int chunk_rows_gather(hipStream_t s, float *const *d_arenas, int arena_shift, const int *d_chunks, const int *d_table, int n_entries,
                      float *dense, const double *means, const double *covs, double *state) {
    if (n_entries <= 0) return DD_OK;
    hipLaunchKernelGGL(chunk_rows_gather_k, dim3((unsigned)n_entries), dim3(256), 0, s, reinterpret_cast<const uint4 *const *>(d_arenas), arena_shift,
                       d_chunks, reinterpret_cast<const int4 *>(d_table), reinterpret_cast<uint4 *>(dense), reinterpret_cast<const uint4 *>(means),
                       reinterpret_cast<const uint4 *>(covs), reinterpret_cast<uint4 *>(state));
    DD_LAUNCH_CHECK();
    return DD_OK;
}

int chunk_rows_scatter(hipStream_t s, float *const *d_arenas, int arena_shift, const int *d_chunks, const int *d_table, int n_entries,
                       const float *dense, double *means, double *covs, const double *state) {
    if (n_entries <= 0) return DD_OK;
    hipLaunchKernelGGL(chunk_rows_scatter_k, dim3((unsigned)n_entries), dim3(256), 0, s, reinterpret_cast<uint4 *const *>(d_arenas), arena_shift,
                       d_chunks, reinterpret_cast<const int4 *>(d_table), reinterpret_cast<const uint4 *>(dense), reinterpret_cast<uint4 *>(means),
                       reinterpret_cast<uint4 *>(covs), reinterpret_cast<const uint4 *>(state));
    DD_LAUNCH_CHECK();
    return DD_OK;
}

}  // namespace ddk

namespace {

// The stand-alone entries: every range of the caller's tables against the stated sizes, then the tables to the device and one launch.
int chunk_rows_alone(const char *name, bool scatter, dd_ctx *ctx, const void *const *arenas_host, int n_arenas, int64_t arena_rows, const int *chunks_host,
                     int n_chunks, const int64_t *table_host, int n_entries, float *dense_dev, int64_t dense_rows, void *stream) {
    DD_REQUIRE(ctx && n_arenas >= 0 && n_chunks >= 0 && n_entries >= 0 && dense_rows >= 0 && dense_rows < (1ll << 31), DD_E_ARG,
               "%s: bad argument (n_arenas %d, n_chunks %d, n_entries %d, dense_rows %lld)", name, n_arenas, n_chunks, n_entries, (long long)dense_rows);
    if (n_entries == 0) return DD_OK;
    DD_REQUIRE(table_host && (n_chunks == 0 || chunks_host) && (n_arenas == 0 || arenas_host), DD_E_ARG, "%s: NULL table", name);
    int shift = 0;
    while (shift < 26 && ((int64_t)CH_ROWS << shift) < arena_rows) ++shift;
    DD_REQUIRE(arena_rows == ((int64_t)CH_ROWS << shift), DD_E_ARG, "%s: arena_rows %lld is not 32 x a power of two", name, (long long)arena_rows);
    DD_REQUIRE((int64_t)n_arenas << shift < (1ll << 31), DD_E_ARG, "%s: %d arenas of %lld rows hold more chunks than an int counts", name, n_arenas, (long long)arena_rows);
    const int64_t total_chunks = (int64_t)n_arenas << shift;
    for (int a = 0; a < n_arenas; ++a)
        DD_REQUIRE(arenas_host[a] && (reinterpret_cast<uintptr_t>(arenas_host[a]) & 15) == 0, DD_E_ARG, "%s: arena %d is NULL or not 16-byte aligned", name, a);
    DD_REQUIRE((reinterpret_cast<uintptr_t>(dense_dev) & 15) == 0, DD_E_ARG, "%s: the dense buffer must be 16-byte aligned", name);
    for (int c = 0; c < n_chunks; ++c)
        DD_REQUIRE(chunks_host[c] >= 0 && chunks_host[c] < total_chunks, DD_E_ARG, "%s: chunks[%d] = %d of %lld", name, c, chunks_host[c], (long long)total_chunks);
    std::vector<int> table;
    std::vector<std::pair<int64_t, int64_t>> w_dense;
    std::vector<int> w_chunks;
    for (int i = 0; i < n_entries; ++i) {
        const int64_t off = table_host[3 * (size_t)i], rows = table_host[3 * (size_t)i + 1], drow = table_host[3 * (size_t)i + 2];
        DD_REQUIRE(rows >= 0 && rows <= (1 << 24), DD_E_ARG, "%s: entry %d has %lld rows", name, i, (long long)rows);
        if (rows == 0) continue;
        const int64_t nc = (rows + CH_ROWS - 1) / CH_ROWS;
        DD_REQUIRE(off >= 0 && off + nc <= n_chunks, DD_E_ARG, "%s: entry %d reads chunks [%lld, %lld) of a list of %d", name, i, (long long)off, (long long)(off + nc), n_chunks);
        DD_REQUIRE(dense_dev && drow >= 0 && drow + rows <= dense_rows, DD_E_ARG, "%s: entry %d takes rows [%lld, %lld) of a dense buffer of %lld", name, i,
                   (long long)drow, (long long)(drow + rows), (long long)dense_rows);
        if (scatter) w_chunks.insert(w_chunks.end(), chunks_host + off, chunks_host + off + nc);
        else w_dense.emplace_back(drow, drow + rows);
        const int e[4] = {(int)off, (int)rows, (int)drow, -1};
        table.insert(table.end(), e, e + 4);
    }
    std::sort(w_dense.begin(), w_dense.end());
    for (size_t i = 1; i < w_dense.size(); ++i)
        DD_REQUIRE(w_dense[i].first >= w_dense[i - 1].second, DD_E_ARG, "%s: two entries write overlapping dense rows [%lld, %lld) and [%lld, %lld)", name,
                   (long long)w_dense[i - 1].first, (long long)w_dense[i - 1].second, (long long)w_dense[i].first, (long long)w_dense[i].second);
    std::sort(w_chunks.begin(), w_chunks.end());
    for (size_t i = 1; i < w_chunks.size(); ++i)
        DD_REQUIRE(w_chunks[i] != w_chunks[i - 1], DD_E_ARG, "%s: chunk %d is written twice", name, w_chunks[i]);
    if (table.empty()) return DD_OK;
    DD_DEVICE(ctx);
    hipStream_t s = dd_pick_stream(ctx, stream);
    int rc;
    // staging: [arena pointers][table][chunks]
    const size_t b_ar = (size_t)n_arenas * sizeof(void *), b_tab = table.size() * sizeof(int), b_ch = (size_t)n_chunks * sizeof(int);
    const size_t o_tab = (b_ar + 15) / 16 * 16, o_ch = o_tab + b_tab, bytes = o_ch + b_ch;
    if ((rc = ctx->scratch[0].reserve(bytes)) != DD_OK) return rc;
    if ((rc = ctx->pin[0].reserve(bytes)) != DD_OK) return rc;
    char *h = ctx->pin[0].as<char>(), *d = ctx->scratch[0].as<char>();
    memcpy(h, arenas_host, b_ar);
    memcpy(h + o_tab, table.data(), b_tab);
    if (b_ch) memcpy(h + o_ch, chunks_host, b_ch);
    DD_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    float *const *d_ar = reinterpret_cast<float *const *>(d);
    const int *d_tab = reinterpret_cast<const int *>(d + o_tab), *d_ch = reinterpret_cast<const int *>(d + o_ch);
    const int n = (int)(table.size() / 4);
    rc = scatter ? ddk::chunk_rows_scatter(s, d_ar, shift, d_ch, d_tab, n, dense_dev, nullptr, nullptr, nullptr)
                 : ddk::chunk_rows_gather(s, d_ar, shift, d_ch, d_tab, n, dense_dev, nullptr, nullptr, nullptr);
    if (rc != DD_OK) return rc;
    DD_HIP(hipStreamSynchronize(s));                          // the staging buffers are the context's: free for the next call
    return DD_OK;
}

}  // namespace

extern "C" int dd_chunk_rows_gather(dd_ctx *ctx, const void *const *arenas_host, int n_arenas, int64_t arena_rows, const int *chunks_host, int n_chunks,
                                    const int64_t *table_host, int n_entries, float *dense_dev, int64_t dense_rows, void *stream) {
    return chunk_rows_alone("dd_chunk_rows_gather", false, ctx, arenas_host, n_arenas, arena_rows, chunks_host, n_chunks, table_host, n_entries, dense_dev,
                            dense_rows, stream);
}

extern "C" int dd_chunk_rows_scatter(dd_ctx *ctx, void *const *arenas_host, int n_arenas, int64_t arena_rows, const int *chunks_host, int n_chunks,
                                     const int64_t *table_host, int n_entries, const float *dense_dev, int64_t dense_rows, void *stream) {
    return chunk_rows_alone("dd_chunk_rows_scatter", true, ctx, arenas_host, n_arenas, arena_rows, chunks_host, n_chunks, table_host, n_entries,
                            const_cast<float *>(dense_dev), dense_rows, stream);
}
