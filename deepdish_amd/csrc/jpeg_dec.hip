// JPEG decoder for files that arrive in host memory: BGR frames in HBM, byte for byte what libjpeg gives for them (Pillow's
// Image.open(f).convert('RGB'), channels swapped; tests/jpeg_dec_ref.py, jpeg_scaled_ref.py and jpeg_prog_ref.py are the definition).
// Serves the frame_%06d.jpg sequence the reference reads under --input-cvat-dir (deepdish.py:685-689, :727) and MJPEG cameras, through the
// ingest ring (csrc/ingest.hip) or on its own.  All integer arithmetic.  Files of one call may differ in tables, sampling, restart
// interval and kind; a file that is refused or damaged sets its own status and writes nothing outside its own frame.
//
// One call, in order (jpegdec_launch; nothing waits on the host):
//   parse     csrc/jpeg_parse.h, on the host, bounded by the header: one dd_jpeg_info per file, and for a DD_JPEGDEC_PROGRESSIVE decoder
//             the file walked into a scan script (dd_jpeg_scans), every scan at a level one above the highest earlier scan of the same
//             component whose band overlaps its own.  DD_JPEGDEC_STD_TABLES stops here: the Annex K tables where a file has none.
//             DD_JPEGDEC_ANY_SIZE makes the decoder's h x w the largest size accepted and no longer the only one.
//   plan      csrc/jpeg_dec_plan.h jd_plan_call, on the host: every live file's place in the interval arrays, its pixel path and scale,
//             its route through the entropy stage, and the sizes of every launch below (JdCall).  It holds every record to the decoder's
//             buffers, so after it the kernels index with the records' fields as they are; it is the only stage that can refuse a call.
//   upload    records, file bytes and (progressive files in the call) scan scripts, one copy each.
//   markers   jpeg_markers_k        one workgroup per file finds the RSTn markers in its scan and writes each restart interval's bounds,
//                                   and sets mark[f], the status the later kernels go by;
//             jpeg_prog_markers_k   the same per (file, scan) of the progressive files.
//   entropy   into the zeroed coefficient buffer: int16, natural order, MCU-interleaved blocks, a frame coef_stride apart.
//             jpeg_split_entropy_k  DD_JPEGDEC_SPLIT: one workgroup per baseline file that is a single restart interval longer than a
//                                   subsequence (no restart markers: what cameras and cv2.imencode write).  The lanes decode its
//                                   subsequences from guessed states, then from their predecessors' end states until none changes;
//             jpeg_entropy_k        one lane per restart interval of every other baseline file (Huffman decoding is serial inside one);
//             jpeg_prog_entropy_k   once per level, one lane per (scan, restart interval) of that level over all files of the call
//                                   (libjpeg's default script: 10 scans, 3 launches): jdphuff.c's four scan kinds.  Scans of one level
//                                   write different words; what a scan refines was written by an earlier launch.
//   pixels    one workgroup per band (one MCU row) of a frame (csrc/jpeg_dec_pix.h): jpeg_pixels_k at scale 1, jpeg_pixels_scaled_k<S> at
//             1/2, 1/4, 1/8 (the frames are ceil(H / S) x ceil(W / S)), in front of either jpeg_planes_k / jpeg_planes_scaled_k<S> where a
//             file of the call is too wide for a band in LDS (DD_JPEGDEC_PLANES); a DD_JPEGDEC_ANY_SIZE decoder runs
//             jpeg_pixels_any_k<S> / jpeg_planes_any_k<S> (csrc/jpeg_dec_any.hip) once per scale that occurs in the call.
// The statements the entropy kernels run are csrc/jpeg_dec_dev.h, __host__ __device__, so that the scripts/jpeg_*_check.cpp programs run
// them over hostile files on the host.
#include "common.h"
#include "jpeg_dec_dev.h"
#include "jpeg_dec_pix.h"
#include "jpeg_dec_plan.h"
#include <cstdlib>
#include <new>

namespace {

constexpr int JD_CHUNK = 16;                   // scan bytes per thread and pass of jpeg_markers_k

// ------------------------------------------------------------------------------------------------ device

// Exclusive prefix sum over the workgroup's threads; total: the sum.  sc: 4 words of LDS.
__device__ __forceinline__ int jd_scan(int v, int *sc, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) sc[w] = x;
    __syncthreads();
    int base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < JD_T / 64; ++i) {
        const int s = sc[i];
        if (i < w) base += s;
        t += s;
    }
    total = t;
    return base + x - v;
}

// One workgroup per file.  iv_start / iv_end: per restart interval, offsets into the file's scan bytes.  mark[f]: the status the
// later kernels go by (the host's, or DD_JPEG_ST_DATA for a wrong marker count or sequence); status[f]: the caller's copy.
__global__ __launch_bounds__(JD_T) void jpeg_markers_k(const dd_jpeg_info *__restrict__ recs, const uint8_t *__restrict__ bytes, uint32_t *__restrict__ iv_start,
                                                       uint32_t *__restrict__ iv_end, int *__restrict__ mark, int *__restrict__ status) {
    __shared__ int sc[4];
    __shared__ int bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    const dd_jpeg_info &r = recs[f];
    if (r.status != DD_JPEG_ST_OK) {
        if (tid == 0) mark[f] = r.status, status[f] = r.status;
        return;
    }
    if (r.sof == 0xC2) {                                        // only a decoder that takes progressive files hands one on: jpeg_prog_markers_k walks its scans
        if (tid == 0) mark[f] = DD_JPEG_ST_OK, status[f] = DD_JPEG_ST_OK;
        return;
    }
    const uint8_t *scan = bytes + r.file_offset + r.scan_offset;
    const uint32_t len = (uint32_t)r.scan_length;
    const int n_int = r.n_intervals;
    uint32_t *st = iv_start + r.interval_base, *en = iv_end + r.interval_base;
    if (tid == 0) bad = 0, st[0] = 0;
    int found = 0;                                              // markers in front of this pass
    for (uint32_t w0 = 0; w0 + 1 < len; w0 += JD_T * JD_CHUNK) {
        const uint32_t p0 = w0 + (uint32_t)tid * JD_CHUNK;
        int cnt = 0;
        for (uint32_t p = p0; p < p0 + JD_CHUNK && p + 1 < len; ++p) cnt += jpd_rst_at(scan, p) >= 0 ? 1 : 0;
        int all;
        int k = found + jd_scan(cnt, sc, all);
        if (cnt)
            for (uint32_t p = p0; p < p0 + JD_CHUNK && p + 1 < len; ++p) {
                const int m = jpd_rst_at(scan, p);
                if (m < 0) continue;
                if (m != (k & 7) || k + 1 >= n_int) bad = 1;    // RSTn out of sequence, or more markers than intervals
                else en[k] = p, st[k + 1] = p + 2;
                ++k;
            }
        found += all;
    }
    __syncthreads();
    if (tid == 0) {
        en[n_int - 1] = len;
        const int s = bad || found != n_int - 1 ? DD_JPEG_ST_DATA : DD_JPEG_ST_OK;
        mark[f] = s, status[f] = s;
    }
}

// One lane per restart interval, `per` of them in a wave.  Intervals of frames whose status is set are not decoded.
__global__ __launch_bounds__(64) void jpeg_entropy_k(const dd_jpeg_info *__restrict__ recs, int n, int total, int per, const uint8_t *__restrict__ bytes,
                                                     const uint32_t *__restrict__ iv_start, const uint32_t *__restrict__ iv_end, const int *__restrict__ mark,
                                                     int16_t *__restrict__ coef, long long coef_stride, int *__restrict__ status) {
    if ((int)threadIdx.x >= per) return;
    const long long idx = (long long)blockIdx.x * per + threadIdx.x;
    if (idx >= total) return;
    int lo = 0, hi = n - 1;                                     // the last frame whose first interval is at or before idx
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].interval_base <= idx) lo = mid;
        else hi = mid - 1;
    }
    const int f = lo;
    const dd_jpeg_info &r = recs[f];
    const int iv = (int)(idx - r.interval_base);
    if (iv >= r.n_intervals || mark[f] != DD_JPEG_ST_OK) return;
    if (r.reserved) return;                                     // DD_JPEGDEC_SPLIT: jpeg_split_entropy_k decodes this file
    const int mcus = r.mcus_x * r.mcus_y, ri = r.restart_interval ? r.restart_interval : mcus;
    const int m0 = iv * ri, nm = min(ri, mcus - m0);
    const uint8_t *scan = bytes + r.file_offset + r.scan_offset;
    const uint32_t len = (uint32_t)r.scan_length;
    const uint32_t s = min(iv_start[idx], len), e = min(iv_end[idx], len);
    if (jpd_decode_interval(r, scan, s, e, m0, nm, coef + (size_t)f * coef_stride) != DD_JPEG_ST_OK) status[f] = DD_JPEG_ST_DATA;
}

// ---- DD_JPEGDEC_SPLIT: only a decoder made with the flag launches this one.

constexpr int JD_SPLIT_WORDS = 7;              // 32-bit words of LDS per subsequence

// One workgroup per file whose record names a subsequence size (reserved = its log2; the call plan's routing): a baseline file
// without restart intervals, which jpeg_entropy_k would give to a single lane.  The lanes stride over the file's subsequences
// (csrc/jpeg_dec_dev.h jpd_decode_span).  Round 0 decodes every subsequence from its guess; in round r every lane first reads its
// predecessor's end state and, behind a barrier, decodes again where that is known and is not the start it used last -- so a round reads only
// what the round before wrote, and the outcome does not depend on the order the lanes run in.  Subsequence 0 starts from the truth, so after
// round r subsequences 0 .. r are final and the loop is over after at most n_sub + 1 rounds, which is also its hard limit.  Then one
// exclusive scan gives every subsequence its first block and its DC predictors (kept to 16 bits: all that is ever stored of them), and a
// last decode writes the coefficients.  Only a lane in front of which every end state is known can end the frame well; when none does, the
// file is DD_JPEG_ST_DATA.  An error met from a guess is not an error: that lane's successor keeps its own start.
// LDS: per subsequence the start used last, the end state, the blocks begun and the DC sums, JD_SPLIT_WORDS words, max_sub of each.
// stats: subsequences, the most rounds a file took, decodes of a subsequence in the rounds (the entropy stage zeroes them).
__global__ __launch_bounds__(JD_T) void jpeg_split_entropy_k(const dd_jpeg_info *__restrict__ recs, const uint8_t *__restrict__ bytes, const int *__restrict__ mark,
                                                             int16_t *__restrict__ coef, long long coef_stride, int *__restrict__ status, int max_sub,
                                                             unsigned int *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint8_t jd_lds[];
    __shared__ dd_jpeg_huff huff[4];
    __shared__ int sc[4];
    __shared__ uint32_t s_end, s_first_bad, s_decodes;
    __shared__ int s_ok;
    const int f = blockIdx.x, tid = threadIdx.x;
    const dd_jpeg_info &r = recs[f];
    const int log2b = r.reserved;
    if (log2b < 4 || log2b > 30 || r.status != DD_JPEG_ST_OK || mark[f] != DD_JPEG_ST_OK) return;
    const uint8_t *scan = bytes + r.file_offset + r.scan_offset;
    const uint32_t len = (uint32_t)r.scan_length;
    uint32_t *used_pos = reinterpret_cast<uint32_t *>(jd_lds), *used_kj = used_pos + max_sub, *end_pos = used_kj + max_sub, *end_kj = end_pos + max_sub;
    uint32_t *blocks = end_kj + max_sub, *dc01 = blocks + max_sub, *dc2 = dc01 + max_sub;          // dc2: bit 31 marks a decode due in this round
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(r.huff);
        uint32_t *dst = reinterpret_cast<uint32_t *>(huff);
        for (int i = tid; i < (int)(sizeof(huff) / 4); i += JD_T) dst[i] = src[i];
    }
    if (tid == 0) s_end = len, s_first_bad = 0xFFFFFFFFu, s_decodes = 0, s_ok = 0;
    __syncthreads();
    // where the data ends: the first 0xFF that no 0x00 follows
    {
        uint32_t e = len;
        for (uint32_t p = (uint32_t)tid * 4; p < len && e == len; p += JD_T * 4) {
            bool look = true;
            if (p + 4 <= len) {
                uint32_t w;
                __builtin_memcpy(&w, scan + p, 4);
                look = ((~w - 0x01010101u) & w & 0x80808080u) != 0;
            }
            if (look)
                for (uint32_t q = p; q < p + 4 && q < len; ++q)
                    if (jpd_marker_at(scan, q, len)) {
                        e = q;
                        break;
                    }
        }
        if (e < len) atomicMin(&s_end, e);
    }
    __syncthreads();
    const uint32_t end = s_end;
    const int n_sub = (int)min((unsigned long long)max_sub, ((unsigned long long)end + (1ull << log2b) - 1) >> log2b);
    const uint32_t n_blocks = (uint32_t)r.mcus_x * (uint32_t)r.mcus_y * (uint32_t)r.blocks_per_mcu;
    int decodes = 0;
    for (int i = tid; i < n_sub; i += JD_T) {                                   // round 0
        JpdState st = jpd_span_guess(scan, (uint32_t)i, log2b, end);
        JpdSpanSums sums;
        used_pos[i] = st.pos, used_kj[i] = st.kj;
        jpd_decode_span(r, huff, scan, end, (uint32_t)min((unsigned long long)end, ((unsigned long long)i + 1) << log2b), st, JPD_SPAN_COUNT, sums, nullptr, 0, 0, nullptr);
        end_pos[i] = st.pos, end_kj[i] = st.kj;
        blocks[i] = sums.blocks, dc01[i] = (uint32_t)sums.dc[0] | (uint32_t)sums.dc[1] << 16, dc2[i] = sums.dc[2];
        ++decodes;
    }
    __syncthreads();
    int rounds = 1;
    for (int round = 1; round <= n_sub; ++round) {
        int due = 0;
        for (int i = tid; i < n_sub; i += JD_T) {
            if (i == 0) continue;
            JpdState p, u;
            p.pos = end_pos[i - 1], p.kj = end_kj[i - 1];
            u.pos = used_pos[i], u.kj = used_kj[i];
            if (p.kj == JPD_STATE_UNKNOWN || jpd_state_eq(p, u)) continue;
            used_pos[i] = p.pos, used_kj[i] = p.kj;
            dc2[i] |= 0x80000000u;
            due = 1;
        }
        ++rounds;
        if (!__syncthreads_or(due)) break;
        for (int i = tid; i < n_sub; i += JD_T) {
            if (!(dc2[i] & 0x80000000u)) continue;
            JpdState st;
            JpdSpanSums sums;
            st.pos = used_pos[i], st.kj = used_kj[i];
            jpd_decode_span(r, huff, scan, end, (uint32_t)min((unsigned long long)end, ((unsigned long long)i + 1) << log2b), st, JPD_SPAN_COUNT, sums, nullptr, 0, 0, nullptr);
            end_pos[i] = st.pos, end_kj[i] = st.kj;
            blocks[i] = sums.blocks, dc01[i] = (uint32_t)sums.dc[0] | (uint32_t)sums.dc[1] << 16, dc2[i] = sums.dc[2];
            ++decodes;
        }
        __syncthreads();
    }
    // the first subsequence whose end is not known, and every subsequence's first block and predictors
    for (int i = tid; i < n_sub; i += JD_T)
        if (end_kj[i] == JPD_STATE_UNKNOWN) atomicMin(&s_first_bad, (uint32_t)i);
    int carry[4] = {0, 0, 0, 0};
    for (int base = 0; base < n_sub; base += JD_T) {
        const int i = base + tid;
        const bool in = i < n_sub;
        const int v[4] = {in ? (int)blocks[i] : 0, in ? (int)(dc01[i] & 0xFFFFu) : 0, in ? (int)(dc01[i] >> 16) : 0, in ? (int)(dc2[i] & 0xFFFFu) : 0};
        int x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int all;
            x[q] = carry[q] + jd_scan(v[q], sc, all);
            carry[q] += all;
        }
        if (in) blocks[i] = (uint32_t)x[0], dc01[i] = ((uint32_t)x[1] & 0xFFFFu) | (uint32_t)x[2] << 16, dc2[i] = (uint32_t)x[3] & 0xFFFFu;
    }
    __syncthreads();
    const uint32_t first_bad = s_first_bad;
    int16_t *out = coef + (size_t)f * coef_stride;
    for (int i = tid; i < n_sub; i += JD_T) {
        JpdState st;
        JpdSpanSums sums;
        st.pos = used_pos[i], st.kj = used_kj[i];
        const uint32_t pred[3] = {dc01[i] & 0xFFFFu, dc01[i] >> 16, dc2[i]};
        const bool done = jpd_decode_span(r, huff, scan, end, (uint32_t)min((unsigned long long)end, ((unsigned long long)i + 1) << log2b), st, JPD_SPAN_WRITE, sums, out, blocks[i],
                                          n_blocks, pred);
        if (done && (uint32_t)i <= first_bad) s_ok = 1;
    }
    if (decodes) atomicAdd(&s_decodes, (uint32_t)decodes);
    __syncthreads();
    if (tid == 0) {
        if (!s_ok) status[f] = DD_JPEG_ST_DATA;
        atomicAdd(&stats[0], (unsigned int)n_sub);
        atomicMax(&stats[1], (unsigned int)rounds);
        atomicAdd(&stats[2], s_decodes);
    }
}

// ---- progressive files (SOF2): only a decoder made with DD_JPEGDEC_PROGRESSIVE launches these two.

// jpeg_markers_k for the scans of progressive files: one workgroup per (file, scan), `max_scans` of them a file.  iv_start / iv_end: per
// restart interval of the scan, offsets into the scan's bytes, at the scan's interval_base.  A wrong marker count or sequence in any scan
// sets the file's mark and status to DD_JPEG_ST_DATA (jpeg_markers_k has set them to OK).
__global__ __launch_bounds__(JD_T) void jpeg_prog_markers_k(const dd_jpeg_info *__restrict__ recs, const dd_jpeg_scans *__restrict__ scans, int max_scans,
                                                            const uint8_t *__restrict__ bytes, uint32_t *__restrict__ iv_start, uint32_t *__restrict__ iv_end,
                                                            int *__restrict__ mark, int *__restrict__ status) {
    __shared__ int sc[4];
    __shared__ int bad;
    const int f = blockIdx.x / max_scans, si = blockIdx.x - f * max_scans, tid = threadIdx.x;
    const dd_jpeg_info &r = recs[f];
    if (r.status != DD_JPEG_ST_OK || r.sof != 0xC2 || si >= scans[f].n_scans) return;
    const dd_jpeg_scan &s = scans[f].scan[si];
    const uint8_t *scan = bytes + r.file_offset + s.offset;
    const uint32_t len = (uint32_t)s.length;
    const int n_int = s.n_intervals;
    uint32_t *st = iv_start + s.interval_base, *en = iv_end + s.interval_base;
    if (tid == 0) bad = 0, st[0] = 0;
    int found = 0;
    for (uint32_t w0 = 0; w0 + 1 < len; w0 += JD_T * JD_CHUNK) {
        const uint32_t p0 = w0 + (uint32_t)tid * JD_CHUNK;
        int cnt = 0;
        for (uint32_t p = p0; p < p0 + JD_CHUNK && p + 1 < len; ++p) cnt += jpd_rst_at(scan, p) >= 0 ? 1 : 0;
        int all;
        int k = found + jd_scan(cnt, sc, all);
        if (cnt)
            for (uint32_t p = p0; p < p0 + JD_CHUNK && p + 1 < len; ++p) {
                const int m = jpd_rst_at(scan, p);
                if (m < 0) continue;
                if (m != (k & 7) || k + 1 >= n_int) bad = 1;
                else en[k] = p, st[k + 1] = p + 2;
                ++k;
            }
        found += all;
    }
    __syncthreads();
    if (tid == 0) {
        en[n_int - 1] = len;
        if (bad || found != n_int - 1) mark[f] = DD_JPEG_ST_DATA, status[f] = DD_JPEG_ST_DATA;
    }
}

// One lane per (scan, restart interval) of level `level`, `per` of them in a wave; `total` lanes over all files of the call.  A file's
// lanes of this level start at its level_base[level], its scans of the level following each other in file order.  Scans of one level write
// different int16 words of the frame's coefficients (csrc/jpeg_parse.h gives the levels), so the lanes of a launch do not race; what a
// scan refines was written by an earlier launch.  Files whose mark is set are not decoded.
__global__ __launch_bounds__(64) void jpeg_prog_entropy_k(const dd_jpeg_info *__restrict__ recs, const dd_jpeg_scans *__restrict__ scans, int n, int level, int total, int per,
                                                          const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ iv_start, const uint32_t *__restrict__ iv_end,
                                                          const int *__restrict__ mark, int16_t *__restrict__ coef, long long coef_stride, int *__restrict__ status) {
    if ((int)threadIdx.x >= per) return;
    const long long idx = (long long)blockIdx.x * per + threadIdx.x;
    if (idx >= total) return;
    int lo = 0, hi = n - 1;                                     // the last file whose lanes of this level start at or before idx
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scans[mid].level_base[level] <= idx) lo = mid;
        else hi = mid - 1;
    }
    const int f = lo;
    const dd_jpeg_info &r = recs[f];
    const dd_jpeg_scans &S = scans[f];
    if (r.status != DD_JPEG_ST_OK || r.sof != 0xC2 || mark[f] != DD_JPEG_ST_OK) return;
    int iv = (int)(idx - S.level_base[level]), si = 0;
    const int n_scans = min(S.n_scans, DD_JPEG_MAX_SCANS);
    for (; si < n_scans; ++si) {
        if (S.scan[si].level != level) continue;
        if (iv < S.scan[si].n_intervals) break;
        iv -= S.scan[si].n_intervals;
    }
    if (si >= n_scans) return;
    const dd_jpeg_scan &sc = S.scan[si];
    const int units = sc.blocks_x * sc.blocks_y, ri = sc.restart_interval ? sc.restart_interval : units;
    const int u0 = iv * ri, nu = min(ri, units - u0);
    const uint32_t len = (uint32_t)sc.length;
    const uint32_t s = min(iv_start[sc.interval_base + iv], len), e = min(iv_end[sc.interval_base + iv], len);
    if (jpd_prog_decode_interval(r, sc, S.pool, bytes + r.file_offset + sc.offset, s, e, u0, nu, coef + (size_t)f * coef_stride) != DD_JPEG_ST_OK) status[f] = DD_JPEG_ST_DATA;
}

// DD_JPEGDEC_PLANES only: one workgroup per band transforms it into the frame's planes in HBM.
__global__ __launch_bounds__(JD_T) void jpeg_planes_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                      uint8_t *__restrict__ planes) {
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || r.path != DD_JPEGDEC_PLANES || band >= r.mcus_y) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax);
    uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * 8 * b.Wc;
    jd_transform_band(r, coef + (size_t)f * g.coef_stride, band, b, Y + (size_t)band * b.yrows * b.Wy, Cb + (size_t)band * 8 * b.Wc, Cr + (size_t)band * 8 * b.Wc, false);
}

// One workgroup per band of a frame.
__global__ __launch_bounds__(JD_T) void jpeg_pixels_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                      const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t jd_lds[];
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || band >= r.mcus_y) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax);
    const int y_first = band * b.yrows, rows = min(b.yrows, r.height - y_first);
    uint8_t *frame = out + (size_t)f * g.H * g.W * 3;
    if (r.path == DD_JPEGDEC_LDS) {
        uint8_t *Y = jd_lds, *Cb = Y + (size_t)b.yrows * b.Wy, *Cr = Cb + (size_t)b.crows * b.Wc;
        jd_transform_band(r, coef + (size_t)f * g.coef_stride, band, b, Y, Cb, Cr, b.halo != 0);
        __syncthreads();
        jd_paint(r, b, Y, Cb, Cr, y_first, band * 8 - b.halo, y_first, rows, frame, vec != 0);
    } else {
        const uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * 8 * b.Wc;
        jd_paint(r, b, Y, Cb, Cr, 0, 0, y_first, rows, frame, vec != 0);
    }
}

template <int S>
__global__ __launch_bounds__(JD_T) void jpeg_planes_scaled_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                             uint8_t *__restrict__ planes) {
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || r.path != DD_JPEGDEC_PLANES || band >= r.mcus_y) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, S);
    uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * b.crows * b.Wc;
    jd_transform_band_scaled<S>(r, coef + (size_t)f * g.coef_stride, band, b, Y + (size_t)band * b.yrows * b.Wy, Cb + (size_t)band * b.crows * b.Wc,
                                Cr + (size_t)band * b.crows * b.Wc);
}

// One workgroup per band of a frame; the frames are ceil(H / S) x ceil(W / S), dense.
template <int S>
__global__ __launch_bounds__(JD_T) void jpeg_pixels_scaled_k(const dd_jpeg_info *__restrict__ recs, JdGeom g, const int *__restrict__ mark, const int16_t *__restrict__ coef,
                                                             const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t jd_lds[];
    const int f = blockIdx.x / g.max_bands, band = blockIdx.x - f * g.max_bands;
    const dd_jpeg_info &r = recs[f];
    if (mark[f] != DD_JPEG_ST_OK || band >= r.mcus_y) return;
    const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, S);
    const int oh = (g.H + S - 1) / S, ow = (g.W + S - 1) / S;
    const int y_first = band * b.yrows, rows = min(b.yrows, oh - y_first);
    if (rows <= 0) return;
    uint8_t *frame = out + (size_t)f * oh * ow * 3;
    if (r.path == DD_JPEGDEC_LDS) {
        uint8_t *Y = jd_lds, *Cb = Y + (size_t)b.yrows * b.Wy, *Cr = Cb + (size_t)b.crows * b.Wc;
        jd_transform_band_scaled<S>(r, coef + (size_t)f * g.coef_stride, band, b, Y, Cb, Cr);
        __syncthreads();
        jd_paint_scaled<S>(r, b, Y, Cb, Cr, 0, y_first, rows, ow, frame, vec != 0);
    } else {
        const uint8_t *Y = planes + (size_t)f * g.plane_stride, *Cb = Y + (size_t)r.mcus_y * b.yrows * b.Wy, *Cr = Cb + (size_t)r.mcus_y * b.crows * b.Wc;
        jd_paint_scaled<S>(r, b, Y, Cb, Cr, y_first, y_first, rows, ow, frame, vec != 0);
    }
}

// ------------------------------------------------------------------------------------------------ host

// A refusal of csrc/jpeg_dec_plan.h, which knows no dd_set_error, into the library's last error.
int jd_fail(int rc, const char *msg) {
    if (rc != DD_OK) dd_set_error("%s", msg);
    return rc;
}

}  // namespace

struct dd_jpegdec {
    dd_ctx *ctx = nullptr;
    JdConfig cfg{};                         // what the call plan goes by: geometry, scale, flags, capacities
    int oh = 0, ow = 0;                     // the frames (DD_JPEGDEC_ANY_SIZE: the slots) a decode writes are oh x ow
    DevBuf recs, bytes, coef, starts, mark, planes;
    PinBuf recs_host;
    hipEvent_t uploaded = nullptr;
    struct {                                // DD_JPEGDEC_PROGRESSIVE: the scan scripts beside the records, and the scans' interval bounds
        DevBuf scans, starts;
        PinBuf scans_host;
    } prog;
    struct {                                // DD_JPEGDEC_SPLIT: jpeg_split_entropy_k's counters, their copy in pinned memory, the event behind
        DevBuf stats;                       // that copy, whether a decode has queued one, and how many files the last decode routed to the kernel
        PinBuf stats_host;
        hipEvent_t done = nullptr;
        bool queued = false;
        int files = 0;
    } split;
    struct {                                // dd_jpegdec_profile: events at call start, uploads done, markers, entropy, pixels, and around
        bool on = false, done = false;      // each level of jpeg_prog_entropy_k; done: the last decode recorded them all
        hipEvent_t ev[5] = {};
        hipEvent_t lev[DD_JPEG_MAX_LEVELS + 1] = {};
        int levels_run = 0;
    } profile;
};

namespace {

// One call on its way through the stages: the plan, the stream, and where the kernels read and write.
struct JdRun {
    dd_jpegdec *d;
    const JdCall &c;
    int n;
    hipStream_t s;
    dd_jpeg_info *recs;
    dd_jpeg_scans *scans;
    uint8_t *bytes;
    uint32_t *iv_start, *iv_end, *piv_start, *piv_end;      // the bounds of the baseline files' intervals, and of the progressive scans'
    int *mark;
    int16_t *coef;
    uint8_t *planes, *out;
    int *status;
};

int jd_profile_mark(const JdRun &r, hipEvent_t e) {
    if (r.d->profile.on) DD_HIP(hipEventRecord(e, r.s));
    return DD_OK;
}

int jd_stage_reserve(dd_jpegdec *d, const JdCall &c, int n) {
    if (int rc = d->starts.reserve((size_t)(c.total + 1) * 2 * sizeof(uint32_t))) return rc;
    if (jd_call_has_progressive(c))
        if (int rc = d->prog.starts.reserve((size_t)(c.ptotal + 1) * 2 * sizeof(uint32_t))) return rc;
    if (c.any_planes)
        if (int rc = d->planes.reserve((size_t)n * (size_t)d->cfg.g.plane_stride)) return rc;
    return DD_OK;
}

// Records and bytes in one copy each, the scan scripts where a file of the call has one; then `uploaded`, if given.
int jd_stage_upload(const JdRun &r, const dd_jpeg_info *recs_host, const dd_jpeg_scans *scans_host, const uint8_t *bytes_host, size_t n_bytes, hipEvent_t uploaded) {
    DD_HIP(hipMemcpyAsync(r.recs, recs_host, (size_t)r.n * sizeof(dd_jpeg_info), hipMemcpyHostToDevice, r.s));
    if (n_bytes) DD_HIP(hipMemcpyAsync(r.bytes, bytes_host, n_bytes, hipMemcpyHostToDevice, r.s));
    if (jd_call_has_progressive(r.c)) DD_HIP(hipMemcpyAsync(r.scans, scans_host, (size_t)r.n * sizeof(dd_jpeg_scans), hipMemcpyHostToDevice, r.s));
    if (uploaded) DD_HIP(hipEventRecord(uploaded, r.s));
    return DD_OK;
}

int jd_stage_markers(const JdRun &r) {
    hipLaunchKernelGGL(jpeg_markers_k, dim3((unsigned)r.n), dim3(JD_T), 0, r.s, r.recs, r.bytes, r.iv_start, r.iv_end, r.mark, r.status);
    DD_LAUNCH_CHECK();
    if (jd_call_has_progressive(r.c)) {
        hipLaunchKernelGGL(jpeg_prog_markers_k, dim3((unsigned)r.n * (unsigned)r.c.max_scans), dim3(JD_T), 0, r.s, r.recs, r.scans, r.c.max_scans, r.bytes, r.piv_start, r.piv_end,
                           r.mark, r.status);
        DD_LAUNCH_CHECK();
    }
    return DD_OK;
}

// Split files, then the other baseline files, then the progressive files level by level, into the zeroed coefficients.  A
// DD_JPEGDEC_SPLIT decoder reads the split kernel's counters back behind it in every call, also one with nothing to decode.
int jd_stage_entropy(const JdRun &r) {
    dd_jpegdec *d = r.d;
    const JdCall &c = r.c;
    const long long coef_stride = d->cfg.g.coef_stride;
    unsigned int *stats = d->cfg.has(DD_JPEGDEC_SPLIT) ? d->split.stats.as<unsigned int>() : nullptr;
    d->profile.levels_run = 0;
    if (stats) {
        d->split.files = c.n_split;
        DD_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned int), r.s));
    }
    if (c.any) DD_HIP(hipMemsetAsync(r.coef, 0, (size_t)r.n * (size_t)coef_stride * sizeof(int16_t), r.s));
    if (jd_call_has_split(c)) {
        const size_t split_lds = (size_t)c.max_sub * JD_SPLIT_WORDS * sizeof(uint32_t);
        hipLaunchKernelGGL(jpeg_split_entropy_k, dim3((unsigned)r.n), dim3(JD_T), split_lds, r.s, r.recs, r.bytes, r.mark, r.coef, coef_stride, r.status, c.max_sub, stats);
        DD_LAUNCH_CHECK();
    }
    if (stats) {
        DD_HIP(hipMemcpyAsync(d->split.stats_host.as<unsigned int>(), stats, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, r.s));
        DD_HIP(hipEventRecord(d->split.done, r.s));
        d->split.queued = true;
    }
    if (!c.any) return DD_OK;
    if (jd_call_has_baseline_lanes(c)) {
        const int per = jd_lanes_per_wave(c.total, d->cfg.lanes);
        hipLaunchKernelGGL(jpeg_entropy_k, dim3((unsigned)((c.total + per - 1) / per)), dim3(64), 0, r.s, r.recs, r.n, (int)c.total, per, r.bytes, r.iv_start, r.iv_end, r.mark, r.coef,
                           coef_stride, r.status);
        DD_LAUNCH_CHECK();
    }
    if (jd_call_has_progressive(c)) {
        if (int rc = jd_profile_mark(r, d->profile.lev[0])) return rc;
        for (int l = 0; l < c.n_levels; ++l) {
            const long long lt = c.level_total[l];
            const int per = jd_lanes_per_wave(lt, d->cfg.lanes);
            if (lt) {
                hipLaunchKernelGGL(jpeg_prog_entropy_k, dim3((unsigned)((lt + per - 1) / per)), dim3(64), 0, r.s, r.recs, r.scans, r.n, l, (int)lt, per, r.bytes, r.piv_start, r.piv_end,
                                   r.mark, r.coef, coef_stride, r.status);
                DD_LAUNCH_CHECK();
            }
            if (int rc = jd_profile_mark(r, d->profile.lev[l + 1])) return rc;
        }
        d->profile.levels_run = c.n_levels;
    }
    return DD_OK;
}

// One workgroup per band of every frame: the planes kernel first where a file of the call takes DD_JPEGDEC_PLANES.  A DD_JPEGDEC_ANY_SIZE
// decoder does that once per scale that occurs (csrc/jpeg_dec_any.hip); every other decoder has one scale, and dense frames of oh x ow.
int jd_stage_pixels(const JdRun &r) {
    const dd_jpegdec *d = r.d;
    const JdGeom &g = d->cfg.g;
    if (d->cfg.has(DD_JPEGDEC_ANY_SIZE))
        return ddk::jpegdec_pixels_any(r.s, r.n, g.max_bands, g.coef_stride, g.plane_stride, r.c.per_scale, r.recs, r.mark, r.coef, r.planes, r.out, d->oh, d->ow);
    const unsigned grid = (unsigned)r.n * (unsigned)g.max_bands;
    const int vec = (d->ow & 3) == 0 && (reinterpret_cast<uintptr_t>(r.out) & 3) == 0;
    return jd_with_scale(d->cfg.scale, [&](auto scale) -> int {
        constexpr int S = decltype(scale)::value;
        if (r.c.any_planes) {
            if constexpr (S == 1) hipLaunchKernelGGL(jpeg_planes_k, dim3(grid), dim3(JD_T), 0, r.s, r.recs, g, r.mark, r.coef, r.planes);
            else hipLaunchKernelGGL(jpeg_planes_scaled_k<S>, dim3(grid), dim3(JD_T), 0, r.s, r.recs, g, r.mark, r.coef, r.planes);
            DD_LAUNCH_CHECK();
        }
        if constexpr (S == 1) hipLaunchKernelGGL(jpeg_pixels_k, dim3(grid), dim3(JD_T), r.c.lds, r.s, r.recs, g, r.mark, r.coef, r.planes, r.out, vec);
        else hipLaunchKernelGGL(jpeg_pixels_scaled_k<S>, dim3(grid), dim3(JD_T), r.c.lds, r.s, r.recs, g, r.mark, r.coef, r.planes, r.out, vec);
        DD_LAUNCH_CHECK();
        return DD_OK;
    });
}

// What the three parsers of the C API share.  flags: 0 or DD_JPEGDEC_STD_TABLES.
int jd_parse_api(const uint8_t *file_host, int64_t n, int flags, dd_jpeg_info *info, dd_jpeg_scans *scans) {
    char msg[320];
    if ((scans ? jpd_parse_scans(file_host, (size_t)n, info, scans, msg, sizeof(msg), flags) : jpd_parse(file_host, (size_t)n, info, msg, sizeof(msg), flags)) != DD_JPEG_R_OK)
        return jd_fail(DD_E_FORMAT, msg);
    return DD_OK;
}

}  // namespace

namespace ddk {

// The header of one file into *rec, with the status a decoder of h x w gives it (a NULL or empty file: DD_JPEG_ST_NO_FRAME).  scans: NULL,
// or where a decoder that takes progressive files keeps this file's scan script (n_scans 0 for every other file).
// flags: the decoder's.  DD_JPEGDEC_STD_TABLES goes to the parser; with DD_JPEGDEC_ANY_SIZE h x w is the largest size accepted.
int jpegdec_parse(const uint8_t *file, size_t n, int h, int w, dd_jpeg_info *rec, dd_jpeg_scans *scans, int flags) {
    char msg[320];
    const int pf = flags & DD_JPEGDEC_STD_TABLES;
    if (scans) scans->n_scans = scans->n_tables = scans->n_levels = 0;
    if (!file || n == 0) {
        memset(rec, 0, sizeof(*rec));
        rec->status = DD_JPEG_ST_NO_FRAME;
        return rec->status;
    }
    if ((scans ? jpd_parse_scans(file, n, rec, scans, msg, sizeof(msg), pf) : jpd_parse(file, n, rec, msg, sizeof(msg), pf)) != DD_JPEG_R_OK) {
        dd_set_error("%s", msg);
        rec->status = DD_JPEG_ST_HEADER;
    } else if (flags & DD_JPEGDEC_ANY_SIZE) {
        if (rec->height > h || rec->width > w) {
            dd_set_error("jpeg decoder: a %d x %d file for a decoder of at most %d x %d", rec->width, rec->height, w, h);
            rec->status = DD_JPEG_ST_SIZE;
        }
    } else if (rec->height != h || rec->width != w) {
        dd_set_error("jpeg decoder: a %d x %d file for a decoder of %d x %d", rec->width, rec->height, w, h);
        rec->status = DD_JPEG_ST_SIZE;
    }
    return rec->status;
}

// recs_host: n records from jpegdec_parse, in memory that stays as it is until the stream has run the upload (pinned: the copy is then
// asynchronous); file i lies at bytes_host + recs_host[i].file_offset, all within n_bytes.  Plans the call (which fills the records'
// decoder fields, or refuses), uploads (then records `uploaded`, if given), and queues the kernels on s.  No host wait.
// scans_host: NULL, or n scan scripts from jpegdec_parse, kept like the records (a decoder that takes progressive files).
// scales: NULL, or (a decoder made with DD_JPEGDEC_ANY_SIZE) one scale denominator per file, none below the decoder's own.
int jpegdec_launch(dd_jpegdec *d, dd_jpeg_info *recs_host, dd_jpeg_scans *scans_host, const uint8_t *bytes_host, size_t n_bytes, int n, uint8_t *out_dev, int *status_dev,
                   hipStream_t s, hipEvent_t uploaded, const int *scales) {
    JdCall c;
    char msg[320];
    if (int rc = jd_plan_call(d->cfg, recs_host, scans_host, n_bytes, n, scales, &c, msg, sizeof(msg))) return jd_fail(rc, msg);
    if (int rc = jd_stage_reserve(d, c, n)) return rc;
    const bool prog = jd_call_has_progressive(c);
    uint32_t *iv = d->starts.as<uint32_t>(), *piv = prog ? d->prog.starts.as<uint32_t>() : nullptr;
    const JdRun r = {d, c, n, s,
                     d->recs.as<dd_jpeg_info>(), d->prog.scans.as<dd_jpeg_scans>(), d->bytes.as<uint8_t>(),
                     iv, iv + c.total + 1, piv, prog ? piv + c.ptotal + 1 : nullptr,
                     d->mark.as<int>(), d->coef.as<int16_t>(), d->planes.as<uint8_t>(), out_dev, status_dev};
    auto &ev = d->profile.ev;
    d->profile.done = false;
    if (int rc = jd_profile_mark(r, ev[0])) return rc;
    if (int rc = jd_stage_upload(r, recs_host, scans_host, bytes_host, n_bytes, uploaded)) return rc;
    if (int rc = jd_profile_mark(r, ev[1])) return rc;
    if (int rc = jd_stage_markers(r)) return rc;
    if (int rc = jd_profile_mark(r, ev[2])) return rc;
    if (int rc = jd_stage_entropy(r)) return rc;
    if (!c.any) return DD_OK;                                   // every file refused or missing: the statuses are set, no frame is written
    if (int rc = jd_profile_mark(r, ev[3])) return rc;
    if (int rc = jd_stage_pixels(r)) return rc;
    if (int rc = jd_profile_mark(r, ev[4])) return rc;
    d->profile.done = d->profile.on;
    return DD_OK;
}

}  // namespace ddk

extern "C" {

int dd_jpeg_parse_scans(const uint8_t *file_host, int64_t n, dd_jpeg_info *info, dd_jpeg_scans *scans) {
    DD_REQUIRE(file_host && info && scans && n >= 0, DD_E_ARG, "dd_jpeg_parse_scans: NULL argument or a negative length");
    return jd_parse_api(file_host, n, 0, info, scans);
}

int dd_jpeg_parse_flags(const uint8_t *file_host, int64_t n, int flags, dd_jpeg_info *info, dd_jpeg_scans *scans) {
    DD_REQUIRE(file_host && info && n >= 0, DD_E_ARG, "dd_jpeg_parse_flags: NULL argument or a negative length");
    DD_REQUIRE((flags & ~DD_JPEGDEC_STD_TABLES) == 0, DD_E_ARG, "dd_jpeg_parse_flags: flags 0x%x (DD_JPEGDEC_STD_TABLES or 0)", flags);
    return jd_parse_api(file_host, n, flags, info, scans);
}

int dd_jpeg_parse(const uint8_t *file_host, int64_t n, dd_jpeg_info *info) {
    DD_REQUIRE(file_host && info && n >= 0, DD_E_ARG, "dd_jpeg_parse: NULL argument or a negative length");
    return jd_parse_api(file_host, n, 0, info, nullptr);
}

static int jd_plan(const char *who, int h, int w, int ncomp, int hs, int vs, int scale, int *path_host, int *band_rows_host, int *bands_host) {
    JdGeom g;
    char msg[320];
    if (int rc = jd_geometry(h, w, who, &g, msg, sizeof(msg))) return jd_fail(rc, msg);
    DD_REQUIRE(jpd_scale_ok(scale), DD_E_ARG, "%s: scale %d is none of 1, 2, 4, 8", who, scale);
    DD_REQUIRE((ncomp == 1 && hs == 1 && vs == 1) || (ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))), DD_E_ARG,
               "%s: %d components with luma sampling %dx%d (1 component, or 3 with 1x1, 2x1 or 2x2)", who, ncomp, hs, vs);
    const JdBand b = jd_band(w, ncomp, hs, vs, scale);
    const int oh = (h + scale - 1) / scale;
    if (path_host) *path_host = b.lds <= (size_t)JD_LDS_MAX ? DD_JPEGDEC_LDS : DD_JPEGDEC_PLANES;
    if (band_rows_host) *band_rows_host = b.yrows;
    if (bands_host) *bands_host = (oh + b.yrows - 1) / b.yrows;
    return DD_OK;
}

int dd_jpegdec_plan(int h, int w, int ncomp, int hs, int vs, int *path_host, int *band_rows_host, int *bands_host) {
    return jd_plan("dd_jpegdec_plan", h, w, ncomp, hs, vs, 1, path_host, band_rows_host, bands_host);
}

int dd_jpegdec_plan_scaled(int h, int w, int ncomp, int hs, int vs, int scale, int *path_host, int *band_rows_host, int *bands_host) {
    return jd_plan("dd_jpegdec_plan_scaled", h, w, ncomp, hs, vs, scale, path_host, band_rows_host, bands_host);
}

int dd_jpeg_draft_scale(int src_w, int src_h, int dst_w, int dst_h) {
    DD_REQUIRE(src_w >= 1 && src_h >= 1 && dst_w >= 1 && dst_h >= 1, DD_E_ARG, "dd_jpeg_draft_scale: %d x %d for %d x %d", src_w, src_h, dst_w, dst_h);
    const int k = src_w / dst_w < src_h / dst_h ? src_w / dst_w : src_h / dst_h;
    return k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1;
}

static int jd_create(const char *who, dd_ctx *ctx, int h, int w, int scale, int flags, int max_frames, int64_t max_bytes, dd_jpegdec **out) {
    DD_REQUIRE(ctx && out, DD_E_ARG, "%s: NULL argument", who);
    JdConfig cfg{};
    char msg[320];
    if (int rc = jd_geometry(h, w, who, &cfg.g, msg, sizeof(msg))) return jd_fail(rc, msg);
    DD_REQUIRE(jpd_scale_ok(scale), DD_E_ARG, "%s: scale %d is none of 1, 2, 4, 8", who, scale);
    DD_REQUIRE((flags & ~(DD_JPEGDEC_PROGRESSIVE | DD_JPEGDEC_SPLIT | DD_JPEGDEC_ANY_SIZE | DD_JPEGDEC_STD_TABLES)) == 0, DD_E_ARG,
               "%s: flags 0x%x (DD_JPEGDEC_PROGRESSIVE, DD_JPEGDEC_SPLIT, DD_JPEGDEC_ANY_SIZE, DD_JPEGDEC_STD_TABLES, any of them or 0)", who, flags);
    cfg.scale = scale, cfg.flags = flags, cfg.max_frames = max_frames, cfg.max_bytes = (size_t)max_bytes;
    cfg.split_log2 = 6, cfg.split_auto = true;                      // 64 bytes, doubled per file until a lane has one subsequence: see the README's table
    const char *sb = cfg.has(DD_JPEGDEC_SPLIT) ? getenv("DD_JPEGDEC_SPLIT_BYTES") : nullptr;
    if (sb) {                                                       // the subsequence size of jpeg_split_entropy_k: a power of two, 16 .. 4096
        char *tail = nullptr;
        const long v = strtol(sb, &tail, 10);
        DD_REQUIRE(tail != sb && *tail == 0 && v >= 16 && v <= 4096 && (v & (v - 1)) == 0, DD_E_ARG, "%s: DD_JPEGDEC_SPLIT_BYTES=%s (a power of two, 16 .. 4096)", who, sb);
        for (cfg.split_log2 = 4; (1l << cfg.split_log2) < v; ++cfg.split_log2) {}
        cfg.split_auto = false;
    }
    const char *lanes = getenv("DD_JPEGDEC_LANES");                 // intervals per wave of the entropy kernels, for A/B runs: 1 .. 64
    if (lanes && atoi(lanes) >= 1 && atoi(lanes) <= 64) cfg.lanes = atoi(lanes);
    DD_REQUIRE(max_frames >= 1 && (long long)max_frames * cfg.g.max_bands <= 0x7fffffffll, DD_E_ARG, "%s: max_frames %d", who, max_frames);
    DD_REQUIRE(max_bytes >= 1, DD_E_ARG, "%s: max_bytes %lld", who, (long long)max_bytes);
    DD_DEVICE(ctx);
    dd_jpegdec *d = new (std::nothrow) dd_jpegdec();
    DD_REQUIRE(d, DD_E_HIP, "%s: out of host memory", who);
    d->ctx = ctx, d->cfg = cfg, d->oh = (h + scale - 1) / scale, d->ow = (w + scale - 1) / scale;
    const bool prog = cfg.has(DD_JPEGDEC_PROGRESSIVE), split = cfg.has(DD_JPEGDEC_SPLIT);
    int rc = d->recs.reserve((size_t)max_frames * sizeof(dd_jpeg_info));
    if (rc == DD_OK) rc = d->bytes.reserve((size_t)max_bytes + 16);
    if (rc == DD_OK) rc = d->coef.reserve((size_t)max_frames * (size_t)cfg.g.coef_stride * sizeof(int16_t));
    if (rc == DD_OK) rc = d->mark.reserve((size_t)max_frames * sizeof(int));
    if (rc == DD_OK) rc = d->recs_host.reserve((size_t)max_frames * sizeof(dd_jpeg_info));
    if (rc == DD_OK && prog) rc = d->prog.scans.reserve((size_t)max_frames * sizeof(dd_jpeg_scans));
    if (rc == DD_OK && prog) rc = d->prog.scans_host.reserve((size_t)max_frames * sizeof(dd_jpeg_scans));
    if (rc == DD_OK && split) rc = d->split.stats.reserve(4 * sizeof(unsigned int));
    if (rc == DD_OK && split) rc = d->split.stats_host.reserve(4 * sizeof(unsigned int));
    if (rc == DD_OK && split && hipEventCreateWithFlags(&d->split.done, hipEventDisableTiming) != hipSuccess) {
        dd_set_error("%s: hipEventCreateWithFlags failed", who);
        rc = DD_E_HIP;
    }
    if (rc == DD_OK && hipEventCreateWithFlags(&d->uploaded, hipEventDisableTiming) != hipSuccess) {
        dd_set_error("%s: hipEventCreateWithFlags failed", who);
        rc = DD_E_HIP;
    }
    if (rc != DD_OK) {
        dd_jpegdec_destroy(d);
        return rc;
    }
    *out = d;
    return DD_OK;
}

int dd_jpegdec_create(dd_ctx *ctx, int h, int w, int max_frames, int64_t max_bytes, dd_jpegdec **out) {
    return jd_create("dd_jpegdec_create", ctx, h, w, 1, 0, max_frames, max_bytes, out);
}

int dd_jpegdec_create_scaled(dd_ctx *ctx, int h, int w, int scale, int max_frames, int64_t max_bytes, dd_jpegdec **out) {
    return jd_create("dd_jpegdec_create_scaled", ctx, h, w, scale, 0, max_frames, max_bytes, out);
}

int dd_jpegdec_create_ex(dd_ctx *ctx, int h, int w, int scale, int flags, int max_frames, int64_t max_bytes, dd_jpegdec **out) {
    return jd_create("dd_jpegdec_create_ex", ctx, h, w, scale, flags, max_frames, max_bytes, out);
}

int dd_jpegdec_output_size(dd_jpegdec *d, int *out_h, int *out_w) {
    DD_REQUIRE(d && out_h && out_w, DD_E_ARG, "dd_jpegdec_output_size: NULL argument");
    *out_h = d->oh, *out_w = d->ow;
    return DD_OK;
}

int dd_jpegdec_destroy(dd_jpegdec *d) {
    if (!d) return DD_OK;
    if (d->ctx) (void)hipSetDevice(d->ctx->device);
    d->recs.release(), d->bytes.release(), d->coef.release(), d->starts.release(), d->mark.release(), d->planes.release();
    d->recs_host.release();
    d->prog.scans.release(), d->prog.starts.release(), d->prog.scans_host.release();
    if (d->uploaded) (void)hipEventDestroy(d->uploaded);
    d->split.stats.release(), d->split.stats_host.release();
    if (d->split.done) (void)hipEventDestroy(d->split.done);
    for (hipEvent_t e : d->profile.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->profile.lev)
        if (e) (void)hipEventDestroy(e);
    delete d;
    return DD_OK;
}

int dd_jpegdec_profile(dd_jpegdec *d, int on) {
    DD_REQUIRE(d, DD_E_ARG, "dd_jpegdec_profile: NULL decoder");
    DD_DEVICE(d->ctx);
    if (on)
        for (hipEvent_t &e : d->profile.ev)
            if (!e) DD_HIP(hipEventCreate(&e));
    if (on && d->cfg.has(DD_JPEGDEC_PROGRESSIVE))
        for (hipEvent_t &e : d->profile.lev)
            if (!e) DD_HIP(hipEventCreate(&e));
    d->profile.on = on != 0;
    d->profile.done = false;
    return DD_OK;
}

int dd_jpegdec_profile_read(dd_jpegdec *d, float *ms_host) {
    DD_REQUIRE(d && ms_host, DD_E_ARG, "dd_jpegdec_profile_read: NULL argument");
    DD_REQUIRE(d->profile.done, DD_E_STATE, "dd_jpegdec_profile_read: no profiled decode (dd_jpegdec_profile(dec, 1), then a decode with a frame to decode)");
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->profile.ev[4]));
    for (int i = 0; i < 4; ++i) DD_HIP(hipEventElapsedTime(&ms_host[i], d->profile.ev[i], d->profile.ev[i + 1]));
    return DD_OK;
}

int dd_jpegdec_profile_levels(dd_jpegdec *d, float *ms_host, int *n_levels_host) {
    DD_REQUIRE(d && ms_host && n_levels_host, DD_E_ARG, "dd_jpegdec_profile_levels: NULL argument");
    DD_REQUIRE(d->profile.done, DD_E_STATE, "dd_jpegdec_profile_levels: no profiled decode (dd_jpegdec_profile(dec, 1), then a decode with a frame to decode)");
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->profile.ev[4]));
    for (int i = 0; i < DD_JPEG_MAX_LEVELS; ++i) ms_host[i] = 0.f;
    for (int i = 0; i < d->profile.levels_run; ++i) DD_HIP(hipEventElapsedTime(&ms_host[i], d->profile.lev[i], d->profile.lev[i + 1]));
    *n_levels_host = d->profile.levels_run;
    return DD_OK;
}

int dd_jpegdec_split_stats(dd_jpegdec *d, int64_t *out_host) {
    DD_REQUIRE(d && out_host, DD_E_ARG, "dd_jpegdec_split_stats: NULL argument");
    for (int i = 0; i < 4; ++i) out_host[i] = 0;
    if (!d->split.queued) return DD_OK;
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->split.done));
    const unsigned int *st = d->split.stats_host.as<unsigned int>();
    out_host[0] = d->split.files, out_host[1] = st[0], out_host[2] = st[1], out_host[3] = st[2];
    return DD_OK;
}

static int jd_decode(const char *who, dd_jpegdec *d, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, const int *scales, int n, uint8_t *out_dev,
                     int *status_dev, void *stream) {
    DD_REQUIRE(d && files_host && offsets && lengths && out_dev && status_dev, DD_E_ARG, "%s: NULL argument", who);
    DD_REQUIRE(n >= 1 && n <= d->cfg.max_frames, DD_E_CAPACITY, "%s: %d frames (1 .. %d)", who, n, d->cfg.max_frames);
    DD_REQUIRE(!scales || d->cfg.has(DD_JPEGDEC_ANY_SIZE), DD_E_STATE, "%s: a scale per file needs a decoder made with DD_JPEGDEC_ANY_SIZE", who);
    for (int i = 0; scales && i < n; ++i)
        DD_REQUIRE(jpd_scale_ok(scales[i]) && scales[i] >= d->cfg.scale, DD_E_ARG, "%s: file %d at scale %d (1, 2, 4 or 8, and at least the decoder's %d)", who, i, scales[i], d->cfg.scale);
    DD_DEVICE(d->ctx);
    hipStream_t s = dd_pick_stream(d->ctx, stream);
    dd_jpeg_info *recs = d->recs_host.as<dd_jpeg_info>();
    dd_jpeg_scans *scans = d->cfg.has(DD_JPEGDEC_PROGRESSIVE) ? d->prog.scans_host.as<dd_jpeg_scans>() : nullptr;
    size_t n_bytes = 0;
    for (int i = 0; i < n; ++i) {
        DD_REQUIRE(offsets[i] >= 0 && lengths[i] >= 0 && lengths[i] <= 0x7fffffffll, DD_E_ARG, "%s: file %d at offset %lld, length %lld", who, i,
                   (long long)offsets[i], (long long)lengths[i]);
        const size_t end = (size_t)offsets[i] + (size_t)lengths[i];
        DD_REQUIRE(end <= d->cfg.max_bytes, DD_E_CAPACITY, "%s: file %d ends at byte %zu, the decoder holds %zu", who, i, end, d->cfg.max_bytes);
        ddk::jpegdec_parse(files_host + offsets[i], (size_t)lengths[i], d->cfg.g.H, d->cfg.g.W, &recs[i], scans ? &scans[i] : nullptr, d->cfg.flags);
        recs[i].file_offset = offsets[i];
        if (lengths[i] && end > n_bytes) n_bytes = end;
    }
    const int rc = ddk::jpegdec_launch(d, recs, scans, files_host, n_bytes, n, out_dev, status_dev, s, d->uploaded, scales);
    // the records' staging and the caller's bytes are free again once the two copies have run
    if (rc != DD_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    DD_HIP(hipEventSynchronize(d->uploaded));
    return DD_OK;
}

int dd_jpegdec_decode(dd_jpegdec *d, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, int n, uint8_t *out_dev, int *status_dev, void *stream) {
    return jd_decode("dd_jpegdec_decode", d, files_host, offsets, lengths, nullptr, n, out_dev, status_dev, stream);
}

int dd_jpegdec_decode_scales(dd_jpegdec *d, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, const int *scales, int n, uint8_t *out_dev,
                             int *status_dev, void *stream) {
    return jd_decode("dd_jpegdec_decode_scales", d, files_host, offsets, lengths, scales, n, out_dev, status_dev, stream);
}

}  // extern "C"
