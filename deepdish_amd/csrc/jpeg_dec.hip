// Baseline JPEG decoder for files that arrive in host memory: BGR frames in HBM, byte for byte what libjpeg gives for them (Pillow's
// Image.open(f).convert('RGB'), channels swapped; tests/jpeg_dec_ref.py is the definition).  Serves the frame_%06d.jpg sequence the
// reference reads under --input-cvat-dir (deepdish.py:685-689, :727) and MJPEG cameras, through the ingest ring (csrc/ingest.hip) or on
// its own.  All integer arithmetic.
//
// The host parses each header (csrc/jpeg_parse.h, bounded by the header) and uploads the records and the file bytes; then
//   jpeg_markers_k   one workgroup per file finds the RSTn markers in its scan bytes and writes each restart interval's start and end;
//   jpeg_entropy_k   one lane per restart interval decodes it (csrc/jpeg_dec_dev.h; Huffman decoding is serial inside an interval) and
//                    stores the non-zero quantised coefficients, int16, natural order, into a zeroed buffer in HBM;
//   jpeg_pixels_k    one workgroup per band (one MCU row) of a frame: dequantisation and the IDCT, one 8x8 block per thread, into sample
//                    planes in LDS; then fancy up-sampling and colour conversion, BGR rows stored in order.  The h2v2 filter's one
//                    chroma row above and below the band comes from transforming those neighbouring chroma blocks again.
// A band too wide for LDS (DD_JPEGDEC_PLANES) takes its planes through HBM: jpeg_planes_k transforms, jpeg_pixels_k reads them back.
// Files of one call may differ in tables, sampling and restart interval; a file that is refused or damaged sets its own status and
// writes nothing outside its own frame.
//
// A decoder made with a scale denominator of 2, 4 or 8 (libjpeg's scale_denom, Pillow's Image.draft; tests/jpeg_scaled_ref.py) runs the
// same markers and entropy kernels and then jpeg_pixels_scaled_k<S> (jpeg_planes_scaled_k<S>) in place of the last: every block goes
// straight to 4x4, 2x2 or 1x1 samples (csrc/jpeg_dec_dev.h), the band's planes shrink with it, 4:2:0 chroma is not up-sampled at all, and
// the frame written is ceil(H / S) x ceil(W / S).  The coefficient buffer keeps its full-size layout.
//
// A decoder made with DD_JPEGDEC_PROGRESSIVE takes progressive (SOF2) files as well, beside baseline ones in the same call.  Such a file
// ends in the same coefficients in the same blocks, so everything behind the entropy stage stays as it is.  The host walks the whole file
// into a scan script (csrc/jpeg_parse.h jpd_parse_scans: dd_jpeg_scans, uploaded beside the records) and gives every scan a level, one
// more than the highest level of an earlier scan of the same component whose band overlaps its own; then
//   jpeg_prog_markers_k   one workgroup per scan finds its RSTn markers;
//   jpeg_prog_entropy_k   launched once per level, one lane per (scan, restart interval) of that level over all files of the call
//                         (libjpeg's default script: 10 scans, 3 launches): jdphuff.c's four scan kinds (csrc/jpeg_dec_dev.h) into the same
//                         zeroed coefficient buffer, in the same MCU-interleaved block order.  Scans of one level write different words.
// A decoder made without the flag hands no such file on (DD_JPEG_ST_HEADER, as ever) and launches neither.
//
// A decoder made with DD_JPEGDEC_SPLIT gives a baseline file that is a single restart interval -- no restart markers: what cameras and
// cv2.imencode write -- to a workgroup, not to one lane of jpeg_entropy_k:
//   jpeg_split_entropy_k  one workgroup per such file cuts its scan into subsequences that the lanes decode from guessed states and then from
//                         their predecessors' end states until none changes (Huffman data re-synchronises by itself), scans the blocks
//                         begun and the DC sums, and decodes once more to store the coefficients: the sequential decode, cut into pieces.
// Everything in front of and behind the entropy stage stays as it is; a decoder made without the flag does not launch it.
//
// A decoder made with DD_JPEGDEC_ANY_SIZE takes files of any size up to its H x W, each at its own scale (dd_jpegdec_decode_scales): the
// kernels up to here are per record and run as they are, jpegdec_launch decides path and scale per file, holds every record to the
// decoder's buffers, and hands the pixel stage to jpeg_pixels_any_k<S> / jpeg_planes_any_k<S> (csrc/jpeg_dec_any.hip), which write each
// frame into the top-left corner of a uniform slot.  DD_JPEGDEC_STD_TABLES goes to the parser alone (csrc/jpeg_parse.h).
#include "common.h"
#include "jpeg_dec_dev.h"
#include "jpeg_dec_pix.h"
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

constexpr int JD_SPLIT_MAX_SUB = 2048;         // subsequences of a file: 28 bytes of LDS each, beside the file's four Huffman tables
constexpr int JD_SPLIT_WORDS = 7;              // 32-bit words of LDS per subsequence

// One workgroup per file whose record names a subsequence size (reserved = its log2; the host's routing, jpegdec_launch): a baseline file
// without restart intervals, which jpeg_entropy_k would give to a single lane.  The lanes stride over the file's subsequences
// (csrc/jpeg_dec_dev.h jpd_decode_span).  Round 0 decodes every subsequence from its guess; in round r every lane first reads its
// predecessor's end state and, behind a barrier, decodes again where that is known and is not the start it used last -- so a round reads only
// what the round before wrote, and the outcome does not depend on the order the lanes run in.  Subsequence 0 starts from the truth, so after
// round r subsequences 0 .. r are final and the loop is over after at most n_sub + 1 rounds, which is also its hard limit.  Then one
// exclusive scan gives every subsequence its first block and its DC predictors (kept to 16 bits: all that is ever stored of them), and a
// last decode writes the coefficients.  Only a lane in front of which every end state is known can end the frame well; when none does, the
// file is DD_JPEG_ST_DATA.  An error met from a guess is not an error: that lane's successor keeps its own start.
// LDS: per subsequence the start used last, the end state, the blocks begun and the DC sums, JD_SPLIT_WORDS words, max_sub of each.
// stats: subsequences, the most rounds a file took, decodes of a subsequence in the rounds (jpegdec_launch zeroes them).
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

template <int S>
int jd_launch_pixels_scaled(unsigned grid, size_t lds, hipStream_t s, bool any_planes, const dd_jpeg_info *recs, const JdGeom &g, const int *mark, const int16_t *coef,
                            uint8_t *planes, uint8_t *out_dev) {
    if (any_planes) {
        hipLaunchKernelGGL(jpeg_planes_scaled_k<S>, dim3(grid), dim3(JD_T), 0, s, recs, g, mark, coef, planes);
        DD_LAUNCH_CHECK();
    }
    const int vec = (((g.W + S - 1) / S) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0;
    hipLaunchKernelGGL(jpeg_pixels_scaled_k<S>, dim3(grid), dim3(JD_T), lds, s, recs, g, mark, coef, planes, out_dev, vec);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// ------------------------------------------------------------------------------------------------ host

int jd_geometry(int h, int w, const char *who, JdGeom *g) {
    DD_REQUIRE(h >= 1 && w >= 1 && h <= JPD_MAX_SIDE && w <= JPD_MAX_SIDE, DD_E_ARG, "%s: a %d x %d frame (h, w: 1 .. %d either way)", who, w, h, JPD_MAX_SIDE);
    g->H = h, g->W = w;
    g->max_bands = (h + 7) / 8;
    const long long b8w = (w + 7) / 8, b8h = (h + 7) / 8, b16w = (w + 15) / 16, b16h = (h + 15) / 16;
    long long blocks = 3 * b8w * b8h;                                            // 4:4:4
    if (4 * b16w * b8h > blocks) blocks = 4 * b16w * b8h;                       // 4:2:2
    if (6 * b16w * b16h > blocks) blocks = 6 * b16w * b16h;                     // 4:2:0
    g->coef_stride = blocks * 64;
    g->plane_stride = 3 * (16 * b16w) * (16 * b16h);                            // every sampling's planes fit in three padded ones
    return DD_OK;
}

}  // namespace

struct dd_jpegdec {
    dd_ctx *ctx = nullptr;
    JdGeom g{};
    int scale = 1, oh = 0, ow = 0;          // the scale denominator; the frames a decode writes are oh x ow
    int max_frames = 0, lanes = 0;
    size_t max_bytes = 0;
    DevBuf recs, bytes, coef, starts, mark, planes;
    PinBuf recs_host;
    hipEvent_t uploaded = nullptr;
    bool profile = false, profiled = false;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // profile: call start, uploads done, markers, entropy, pixels
    // DD_JPEGDEC_PROGRESSIVE only: the scan scripts beside the records, the scans' interval bounds, and the profile's events around each level
    bool progressive = false;
    DevBuf scans, pstarts;
    PinBuf scans_host;
    int levels_run = 0;
    hipEvent_t lev[DD_JPEG_MAX_LEVELS + 1] = {};
    // DD_JPEGDEC_SPLIT only: log2 of the subsequence size, jpeg_split_entropy_k's counters, their copy in pinned memory, the event behind that
    // copy, and how many files the last decode routed to the kernel
    bool split = false, split_auto = true, split_queued = false;
    int split_log2 = 0, split_files = 0;
    DevBuf split_stats;
    PinBuf split_stats_host;
    hipEvent_t split_done = nullptr;
    // DD_JPEGDEC_ANY_SIZE: g.H x g.W is the largest file accepted and `scale` the smallest denominator of a call; DD_JPEGDEC_STD_TABLES goes
    // to the parser with the rest of the flags
    bool any_size = false;
    int flags = 0;
};

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
// asynchronous); file i lies at bytes_host + recs_host[i].file_offset, all within n_bytes.  Fills the records' decoder fields, uploads
// records and bytes in one copy each (then records `uploaded`, if given), and queues the kernels on s.  No host wait.
// scans_host: NULL, or n scan scripts from jpegdec_parse, kept like the records (a decoder that takes progressive files).
// scales: NULL, or (a decoder made with DD_JPEGDEC_ANY_SIZE) one scale denominator per file, none below the decoder's own.
int jpegdec_launch(dd_jpegdec *d, dd_jpeg_info *recs_host, dd_jpeg_scans *scans_host, const uint8_t *bytes_host, size_t n_bytes, int n, uint8_t *out_dev, int *status_dev,
                   hipStream_t s, hipEvent_t uploaded, const int *scales) {
    DD_REQUIRE(n >= 1 && n <= d->max_frames, DD_E_CAPACITY, "jpeg decoder: %d frames in a call (1 .. %d)", n, d->max_frames);
    DD_REQUIRE(n_bytes <= d->max_bytes, DD_E_CAPACITY, "jpeg decoder: %zu bytes of files in a call (at most %zu)", n_bytes, d->max_bytes);
    const JdGeom &g = d->g;
    DD_REQUIRE(!scans_host || d->progressive, DD_E_STATE, "jpeg decoder: scan scripts for a decoder that was not made to take progressive files");
    DD_REQUIRE(!scales || d->any_size, DD_E_STATE, "jpeg decoder: a scale per file for a decoder that was not made with DD_JPEGDEC_ANY_SIZE");
    size_t lds_at[4] = {0, 0, 0, 0};                            // DD_JPEGDEC_ANY_SIZE: per log2 of the scale, the LDS, whether a file takes it
    bool any_at[4] = {false, false, false, false}, planes_at[4] = {false, false, false, false};
    long long total = 0, ptotal = 0, level_total[DD_JPEG_MAX_LEVELS] = {};
    int max_scans = 0, n_levels = 0, n_split = 0, max_sub = 0;
    size_t lds = 0;
    bool any = false, any_planes = false;
    for (int i = 0; i < n; ++i) {
        dd_jpeg_info &r = recs_host[i];
        r.interval_base = (int32_t)total;
        r.reserved = 0;
        if (scans_host) {
            dd_jpeg_scans &S = scans_host[i];
            for (int l = 0; l < DD_JPEG_MAX_LEVELS; ++l) S.level_base[l] = (int32_t)level_total[l];
            if (r.status != DD_JPEG_ST_OK || r.sof != 0xC2) S.n_scans = S.n_levels = 0;
        }
        if (r.status != DD_JPEG_ST_OK) {
            r.n_intervals = 0;
            continue;
        }
        if (scans_host && scans_host[i].n_scans) {
            dd_jpeg_scans &S = scans_host[i];
            DD_REQUIRE(S.n_scans <= DD_JPEG_MAX_SCANS && S.n_levels <= DD_JPEG_MAX_LEVELS, DD_E_ARG, "jpeg decoder: file %d: %d scans at %d levels", i, S.n_scans, S.n_levels);
            for (int k = 0; k < S.n_scans; ++k) {
                dd_jpeg_scan &sc = S.scan[k];
                DD_REQUIRE(r.file_offset >= 0 && sc.offset >= 0 && sc.length >= 0 && (size_t)r.file_offset + (size_t)sc.offset + (size_t)sc.length <= n_bytes, DD_E_ARG,
                           "jpeg decoder: scan %d of file %d lies outside the %zu bytes given", k, i, n_bytes);
                DD_REQUIRE(sc.level >= 0 && sc.level < S.n_levels && sc.n_intervals >= 1, DD_E_ARG, "jpeg decoder: scan %d of file %d: level %d, %d intervals", k, i, sc.level,
                           sc.n_intervals);
                sc.interval_base = (int32_t)ptotal;
                ptotal += sc.n_intervals;
                level_total[sc.level] += sc.n_intervals;
            }
            DD_REQUIRE(ptotal <= 0x7fffffffll, DD_E_CAPACITY, "jpeg decoder: more than 2^31 restart intervals in a call");
            max_scans = S.n_scans > max_scans ? S.n_scans : max_scans;
            n_levels = S.n_levels > n_levels ? S.n_levels : n_levels;
            r.n_intervals = 0, r.restart_interval = 0, r.scan_offset = 0, r.scan_length = 0;          // nothing for jpeg_entropy_k
        }
        DD_REQUIRE(r.file_offset >= 0 && (size_t)r.file_offset + (size_t)r.scan_offset + (size_t)r.scan_length <= n_bytes, DD_E_ARG,
                   "jpeg decoder: file %d lies outside the %zu bytes given", i, n_bytes);
        const int fs = scales ? scales[i] : d->scale;
        DD_REQUIRE(jpd_scale_ok(fs) && fs >= d->scale, DD_E_ARG, "jpeg decoder: file %d at scale %d (1, 2, 4 or 8, and at least the decoder's %d)", i, fs, d->scale);
        const JdBand b = jd_band(r.width, r.ncomp, r.hmax, r.vmax, fs);
        r.path = b.lds <= (size_t)JD_LDS_MAX ? DD_JPEGDEC_LDS : DD_JPEGDEC_PLANES;
        if (r.path == DD_JPEGDEC_LDS) lds = b.lds > lds ? b.lds : lds;
        else any_planes = true;
        if (d->any_size) {
            // these records came from put on other threads: everything the kernels index with is held to the decoder's buffers here,
            // before anything is queued.  jd_geometry's strides are monotone in h and w, so a file that fits the sides fits them.
            const long long blocks = (long long)r.mcus_x * r.mcus_y * r.blocks_per_mcu;
            const long long crows = fs == 1 ? 8 : b.crows;
            const long long plane_bytes = (long long)r.mcus_y * ((long long)b.yrows * b.Wy + (r.ncomp == 3 ? 2 * crows * b.Wc : 0));
            DD_REQUIRE(r.height >= 1 && r.height <= g.H && r.width >= 1 && r.width <= g.W, DD_E_ARG, "jpeg decoder: file %d is %d x %d, the decoder holds at most %d x %d", i,
                       r.width, r.height, g.W, g.H);
            DD_REQUIRE(r.mcus_x == (r.width + 8 * r.hmax - 1) / (8 * r.hmax) && r.mcus_y == (r.height + 8 * r.vmax - 1) / (8 * r.vmax) && r.mcus_y <= g.max_bands, DD_E_ARG,
                       "jpeg decoder: file %d: %d x %d MCUs for %d x %d pixels", i, r.mcus_x, r.mcus_y, r.width, r.height);
            DD_REQUIRE(blocks * 64 <= g.coef_stride, DD_E_ARG, "jpeg decoder: file %d has %lld blocks, a frame's coefficients hold %lld", i, blocks, g.coef_stride / 64);
            DD_REQUIRE(r.path == DD_JPEGDEC_LDS || plane_bytes <= g.plane_stride, DD_E_ARG, "jpeg decoder: file %d needs %lld bytes of planes, a frame holds %lld", i, plane_bytes,
                       g.plane_stride);
            const int lg = fs == 1 ? 0 : fs == 2 ? 1 : fs == 4 ? 2 : 3;
            any_at[lg] = true;
            if (r.path == DD_JPEGDEC_LDS) lds_at[lg] = b.lds > lds_at[lg] ? b.lds : lds_at[lg];
            else planes_at[lg] = true;
            r.path |= lg << 8;
        }
        // DD_JPEGDEC_SPLIT: a baseline file that is one restart interval (no DRI, DRI 0, or a DRI of the MCU count or more) and longer than a
        // subsequence goes to jpeg_split_entropy_k, in subsequences of the decoder's size -- doubled, where DD_JPEGDEC_SPLIT_BYTES did not
        // fix it, until every lane of the workgroup has at most one, and in any case until the file's states fit the kernel's LDS;
        // jpeg_entropy_k passes over it
        if (d->split && r.sof != 0xC2 && r.n_intervals == 1 && (long long)r.scan_length > (1ll << d->split_log2)) {
            int lg = d->split_log2;
            if (d->split_auto)                                              // one subsequence per lane of the file's workgroup: see the README's table
                while ((((long long)r.scan_length + (1ll << lg) - 1) >> lg) > JD_T) ++lg;
            while ((((long long)r.scan_length + (1ll << lg) - 1) >> lg) > JD_SPLIT_MAX_SUB) ++lg;
            r.reserved = lg;
            const int subs = (int)(((long long)r.scan_length + (1ll << lg) - 1) >> lg);
            max_sub = subs > max_sub ? subs : max_sub;
            ++n_split;
        }
        total += r.n_intervals;
        any = true;
        DD_REQUIRE(total <= 0x7fffffffll, DD_E_CAPACITY, "jpeg decoder: more than 2^31 restart intervals in a call");
    }
    if (int rc = d->starts.reserve((size_t)(total + 1) * 2 * sizeof(uint32_t))) return rc;
    if (max_scans)
        if (int rc = d->pstarts.reserve((size_t)(ptotal + 1) * 2 * sizeof(uint32_t))) return rc;
    if (any_planes)
        if (int rc = d->planes.reserve((size_t)n * (size_t)g.plane_stride)) return rc;
    dd_jpeg_info *recs = d->recs.as<dd_jpeg_info>();
    uint8_t *bytes = d->bytes.as<uint8_t>();
    int16_t *coef = d->coef.as<int16_t>();
    uint32_t *iv_start = d->starts.as<uint32_t>(), *iv_end = iv_start + total + 1;
    int *mark = d->mark.as<int>();
    d->profiled = false;
    if (d->profile) DD_HIP(hipEventRecord(d->ev[0], s));
    DD_HIP(hipMemcpyAsync(recs, recs_host, (size_t)n * sizeof(dd_jpeg_info), hipMemcpyHostToDevice, s));
    if (n_bytes) DD_HIP(hipMemcpyAsync(bytes, bytes_host, n_bytes, hipMemcpyHostToDevice, s));
    if (max_scans) DD_HIP(hipMemcpyAsync(d->scans.as<dd_jpeg_scans>(), scans_host, (size_t)n * sizeof(dd_jpeg_scans), hipMemcpyHostToDevice, s));
    if (uploaded) DD_HIP(hipEventRecord(uploaded, s));
    if (d->profile) DD_HIP(hipEventRecord(d->ev[1], s));
    hipLaunchKernelGGL(jpeg_markers_k, dim3((unsigned)n), dim3(JD_T), 0, s, recs, bytes, iv_start, iv_end, mark, status_dev);
    DD_LAUNCH_CHECK();
    const dd_jpeg_scans *scans = d->scans.as<dd_jpeg_scans>();
    uint32_t *piv_start = max_scans ? d->pstarts.as<uint32_t>() : nullptr, *piv_end = max_scans ? piv_start + ptotal + 1 : nullptr;
    if (max_scans) {
        hipLaunchKernelGGL(jpeg_prog_markers_k, dim3((unsigned)n * (unsigned)max_scans), dim3(JD_T), 0, s, recs, scans, max_scans, bytes, piv_start, piv_end, mark, status_dev);
        DD_LAUNCH_CHECK();
    }
    if (d->profile) DD_HIP(hipEventRecord(d->ev[2], s));
    d->levels_run = 0;
    unsigned int *split_stats = d->split ? d->split_stats.as<unsigned int>() : nullptr;
    if (d->split) {
        d->split_files = n_split;
        DD_HIP(hipMemsetAsync(split_stats, 0, 4 * sizeof(unsigned int), s));
    }
    if (!any) {
        if (d->split) {
            DD_HIP(hipMemcpyAsync(d->split_stats_host.as<unsigned int>(), split_stats, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
            DD_HIP(hipEventRecord(d->split_done, s));
            d->split_queued = true;
        }
        return DD_OK;
    }
    DD_HIP(hipMemsetAsync(coef, 0, (size_t)n * (size_t)g.coef_stride * sizeof(int16_t), s));
    if (n_split) {
        const size_t split_lds = (size_t)max_sub * JD_SPLIT_WORDS * sizeof(uint32_t);
        hipLaunchKernelGGL(jpeg_split_entropy_k, dim3((unsigned)n), dim3(JD_T), split_lds, s, recs, bytes, mark, coef, g.coef_stride, status_dev, max_sub, split_stats);
        DD_LAUNCH_CHECK();
    }
    if (d->split) {
        DD_HIP(hipMemcpyAsync(d->split_stats_host.as<unsigned int>(), split_stats, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        DD_HIP(hipEventRecord(d->split_done, s));
        d->split_queued = true;
    }
    // intervals per wave: a lane decodes serially, so few intervals are spread over many waves (one per SIMD and more: 256 CUs of 4 SIMDs),
    // and only a call with very many intervals fills its waves
    int per = 64;
    while (per > 1 && total / per < 2048) per >>= 1;
    if (d->lanes) per = d->lanes;
    if ((total || !max_scans) && !(n_split && total == n_split)) {          // a call of progressive files alone, or of split files alone, has nothing for it
        hipLaunchKernelGGL(jpeg_entropy_k, dim3((unsigned)((total + per - 1) / per)), dim3(64), 0, s, recs, n, (int)total, per, bytes, iv_start, iv_end, mark, coef,
                           g.coef_stride, status_dev);
        DD_LAUNCH_CHECK();
    }
    if (max_scans) {
        if (d->profile) DD_HIP(hipEventRecord(d->lev[0], s));
        for (int l = 0; l < n_levels; ++l) {
            const long long lt = level_total[l];
            int lper = 64;
            while (lper > 1 && lt / lper < 2048) lper >>= 1;
            if (d->lanes) lper = d->lanes;
            if (lt)
                hipLaunchKernelGGL(jpeg_prog_entropy_k, dim3((unsigned)((lt + lper - 1) / lper)), dim3(64), 0, s, recs, scans, n, l, (int)lt, lper, bytes, piv_start, piv_end, mark,
                                   coef, g.coef_stride, status_dev);
            DD_LAUNCH_CHECK();
            if (d->profile) DD_HIP(hipEventRecord(d->lev[l + 1], s));
        }
        d->levels_run = n_levels;
    }
    if (d->profile) DD_HIP(hipEventRecord(d->ev[3], s));
    const unsigned grid = (unsigned)n * (unsigned)g.max_bands;
    if (d->any_size) {                                          // one launch per scale that occurs; each passes over the other scales' files
        const int rc = jpegdec_pixels_any(s, n, g.max_bands, g.coef_stride, g.plane_stride, lds_at, any_at, planes_at, recs, mark, coef, d->planes.as<uint8_t>(), out_dev, d->oh, d->ow);
        if (rc != DD_OK) return rc;
        if (d->profile) {
            DD_HIP(hipEventRecord(d->ev[4], s));
            d->profiled = true;
        }
        return DD_OK;
    }
    if (d->scale != 1) {
        int rc = DD_OK;
        switch (d->scale) {
            case 2: rc = jd_launch_pixels_scaled<2>(grid, lds, s, any_planes, recs, g, mark, coef, d->planes.as<uint8_t>(), out_dev); break;
            case 4: rc = jd_launch_pixels_scaled<4>(grid, lds, s, any_planes, recs, g, mark, coef, d->planes.as<uint8_t>(), out_dev); break;
            default: rc = jd_launch_pixels_scaled<8>(grid, lds, s, any_planes, recs, g, mark, coef, d->planes.as<uint8_t>(), out_dev); break;
        }
        if (rc != DD_OK) return rc;
        if (d->profile) {
            DD_HIP(hipEventRecord(d->ev[4], s));
            d->profiled = true;
        }
        return DD_OK;
    }
    if (any_planes) {
        hipLaunchKernelGGL(jpeg_planes_k, dim3(grid), dim3(JD_T), 0, s, recs, g, mark, coef, d->planes.as<uint8_t>());
        DD_LAUNCH_CHECK();
    }
    const int vec = (g.W & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0;
    hipLaunchKernelGGL(jpeg_pixels_k, dim3(grid), dim3(JD_T), lds, s, recs, g, mark, coef, d->planes.as<uint8_t>(), out_dev, vec);
    DD_LAUNCH_CHECK();
    if (d->profile) {
        DD_HIP(hipEventRecord(d->ev[4], s));
        d->profiled = true;
    }
    return DD_OK;
}

}  // namespace ddk

extern "C" {

int dd_jpeg_parse_scans(const uint8_t *file_host, int64_t n, dd_jpeg_info *info, dd_jpeg_scans *scans) {
    DD_REQUIRE(file_host && info && scans && n >= 0, DD_E_ARG, "dd_jpeg_parse_scans: NULL argument or a negative length");
    char msg[320];
    if (jpd_parse_scans(file_host, (size_t)n, info, scans, msg, sizeof(msg)) != DD_JPEG_R_OK) {
        dd_set_error("%s", msg);
        return DD_E_FORMAT;
    }
    return DD_OK;
}

int dd_jpeg_parse_flags(const uint8_t *file_host, int64_t n, int flags, dd_jpeg_info *info, dd_jpeg_scans *scans) {
    DD_REQUIRE(file_host && info && n >= 0, DD_E_ARG, "dd_jpeg_parse_flags: NULL argument or a negative length");
    DD_REQUIRE((flags & ~DD_JPEGDEC_STD_TABLES) == 0, DD_E_ARG, "dd_jpeg_parse_flags: flags 0x%x (DD_JPEGDEC_STD_TABLES or 0)", flags);
    char msg[320];
    if ((scans ? jpd_parse_scans(file_host, (size_t)n, info, scans, msg, sizeof(msg), flags) : jpd_parse(file_host, (size_t)n, info, msg, sizeof(msg), flags)) != DD_JPEG_R_OK) {
        dd_set_error("%s", msg);
        return DD_E_FORMAT;
    }
    return DD_OK;
}

int dd_jpeg_parse(const uint8_t *file_host, int64_t n, dd_jpeg_info *info) {
    DD_REQUIRE(file_host && info && n >= 0, DD_E_ARG, "dd_jpeg_parse: NULL argument or a negative length");
    char msg[320];
    if (jpd_parse(file_host, (size_t)n, info, msg, sizeof(msg)) != DD_JPEG_R_OK) {
        dd_set_error("%s", msg);
        return DD_E_FORMAT;
    }
    return DD_OK;
}

static int jd_plan(const char *who, int h, int w, int ncomp, int hs, int vs, int scale, int *path_host, int *band_rows_host, int *bands_host) {
    JdGeom g;
    if (int rc = jd_geometry(h, w, who, &g)) return rc;
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
    JdGeom g;
    if (int rc = jd_geometry(h, w, who, &g)) return rc;
    DD_REQUIRE(jpd_scale_ok(scale), DD_E_ARG, "%s: scale %d is none of 1, 2, 4, 8", who, scale);
    DD_REQUIRE((flags & ~(DD_JPEGDEC_PROGRESSIVE | DD_JPEGDEC_SPLIT | DD_JPEGDEC_ANY_SIZE | DD_JPEGDEC_STD_TABLES)) == 0, DD_E_ARG,
               "%s: flags 0x%x (DD_JPEGDEC_PROGRESSIVE, DD_JPEGDEC_SPLIT, DD_JPEGDEC_ANY_SIZE, DD_JPEGDEC_STD_TABLES, any of them or 0)", who, flags);
    int split_log2 = 6;                                             // 64 bytes, doubled per file until a lane has one subsequence: see the README's table
    const char *sb = (flags & DD_JPEGDEC_SPLIT) ? getenv("DD_JPEGDEC_SPLIT_BYTES") : nullptr;
    if (sb) {                                                       // the subsequence size of jpeg_split_entropy_k: a power of two, 16 .. 4096
        char *tail = nullptr;
        const long v = strtol(sb, &tail, 10);
        DD_REQUIRE(tail != sb && *tail == 0 && v >= 16 && v <= 4096 && (v & (v - 1)) == 0, DD_E_ARG, "%s: DD_JPEGDEC_SPLIT_BYTES=%s (a power of two, 16 .. 4096)", who, sb);
        for (split_log2 = 4; (1l << split_log2) < v; ++split_log2) {}
    }
    DD_REQUIRE(max_frames >= 1 && (long long)max_frames * g.max_bands <= 0x7fffffffll, DD_E_ARG, "%s: max_frames %d", who, max_frames);
    DD_REQUIRE(max_bytes >= 1, DD_E_ARG, "%s: max_bytes %lld", who, (long long)max_bytes);
    DD_DEVICE(ctx);
    dd_jpegdec *d = new (std::nothrow) dd_jpegdec();
    DD_REQUIRE(d, DD_E_HIP, "%s: out of host memory", who);
    d->ctx = ctx, d->g = g, d->max_frames = max_frames, d->max_bytes = (size_t)max_bytes;
    d->scale = scale, d->oh = (h + scale - 1) / scale, d->ow = (w + scale - 1) / scale;
    d->flags = flags, d->any_size = (flags & DD_JPEGDEC_ANY_SIZE) != 0;
    const char *lanes = getenv("DD_JPEGDEC_LANES");                 // intervals per wave of jpeg_entropy_k, for A/B runs: 1 .. 64
    if (lanes && atoi(lanes) >= 1 && atoi(lanes) <= 64) d->lanes = atoi(lanes);
    int rc = d->recs.reserve((size_t)max_frames * sizeof(dd_jpeg_info));
    if (rc == DD_OK) rc = d->bytes.reserve((size_t)max_bytes + 16);
    if (rc == DD_OK) rc = d->coef.reserve((size_t)max_frames * (size_t)g.coef_stride * sizeof(int16_t));
    if (rc == DD_OK) rc = d->mark.reserve((size_t)max_frames * sizeof(int));
    if (rc == DD_OK) rc = d->recs_host.reserve((size_t)max_frames * sizeof(dd_jpeg_info));
    d->progressive = (flags & DD_JPEGDEC_PROGRESSIVE) != 0;
    if (rc == DD_OK && d->progressive) rc = d->scans.reserve((size_t)max_frames * sizeof(dd_jpeg_scans));
    if (rc == DD_OK && d->progressive) rc = d->scans_host.reserve((size_t)max_frames * sizeof(dd_jpeg_scans));
    d->split = (flags & DD_JPEGDEC_SPLIT) != 0, d->split_log2 = split_log2, d->split_auto = sb == nullptr;
    if (rc == DD_OK && d->split) rc = d->split_stats.reserve(4 * sizeof(unsigned int));
    if (rc == DD_OK && d->split) rc = d->split_stats_host.reserve(4 * sizeof(unsigned int));
    if (rc == DD_OK && d->split && hipEventCreateWithFlags(&d->split_done, hipEventDisableTiming) != hipSuccess) {
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
    d->scans.release(), d->pstarts.release(), d->scans_host.release();
    if (d->uploaded) (void)hipEventDestroy(d->uploaded);
    d->split_stats.release(), d->split_stats_host.release();
    if (d->split_done) (void)hipEventDestroy(d->split_done);
    for (hipEvent_t e : d->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->lev)
        if (e) (void)hipEventDestroy(e);
    delete d;
    return DD_OK;
}

int dd_jpegdec_profile(dd_jpegdec *d, int on) {
    DD_REQUIRE(d, DD_E_ARG, "dd_jpegdec_profile: NULL decoder");
    DD_DEVICE(d->ctx);
    if (on)
        for (hipEvent_t &e : d->ev)
            if (!e) DD_HIP(hipEventCreate(&e));
    if (on && d->progressive)
        for (hipEvent_t &e : d->lev)
            if (!e) DD_HIP(hipEventCreate(&e));
    d->profile = on != 0;
    d->profiled = false;
    return DD_OK;
}

int dd_jpegdec_profile_read(dd_jpegdec *d, float *ms_host) {
    DD_REQUIRE(d && ms_host, DD_E_ARG, "dd_jpegdec_profile_read: NULL argument");
    DD_REQUIRE(d->profiled, DD_E_STATE, "dd_jpegdec_profile_read: no profiled decode (dd_jpegdec_profile(dec, 1), then a decode with a frame to decode)");
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->ev[4]));
    for (int i = 0; i < 4; ++i) DD_HIP(hipEventElapsedTime(&ms_host[i], d->ev[i], d->ev[i + 1]));
    return DD_OK;
}

int dd_jpegdec_profile_levels(dd_jpegdec *d, float *ms_host, int *n_levels_host) {
    DD_REQUIRE(d && ms_host && n_levels_host, DD_E_ARG, "dd_jpegdec_profile_levels: NULL argument");
    DD_REQUIRE(d->profiled, DD_E_STATE, "dd_jpegdec_profile_levels: no profiled decode (dd_jpegdec_profile(dec, 1), then a decode with a frame to decode)");
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->ev[4]));
    for (int i = 0; i < DD_JPEG_MAX_LEVELS; ++i) ms_host[i] = 0.f;
    for (int i = 0; i < d->levels_run; ++i) DD_HIP(hipEventElapsedTime(&ms_host[i], d->lev[i], d->lev[i + 1]));
    *n_levels_host = d->levels_run;
    return DD_OK;
}

int dd_jpegdec_split_stats(dd_jpegdec *d, int64_t *out_host) {
    DD_REQUIRE(d && out_host, DD_E_ARG, "dd_jpegdec_split_stats: NULL argument");
    for (int i = 0; i < 4; ++i) out_host[i] = 0;
    if (!d->split || !d->split_queued) return DD_OK;
    DD_DEVICE(d->ctx);
    DD_HIP(hipEventSynchronize(d->split_done));
    const unsigned int *st = d->split_stats_host.as<unsigned int>();
    out_host[0] = d->split_files, out_host[1] = st[0], out_host[2] = st[1], out_host[3] = st[2];
    return DD_OK;
}

static int jd_decode(const char *who, dd_jpegdec *d, const uint8_t *files_host, const int64_t *offsets, const int64_t *lengths, const int *scales, int n, uint8_t *out_dev,
                     int *status_dev, void *stream) {
    DD_REQUIRE(d && files_host && offsets && lengths && out_dev && status_dev, DD_E_ARG, "%s: NULL argument", who);
    DD_REQUIRE(n >= 1 && n <= d->max_frames, DD_E_CAPACITY, "%s: %d frames (1 .. %d)", who, n, d->max_frames);
    DD_REQUIRE(!scales || d->any_size, DD_E_STATE, "%s: a scale per file needs a decoder made with DD_JPEGDEC_ANY_SIZE", who);
    for (int i = 0; scales && i < n; ++i)
        DD_REQUIRE(jpd_scale_ok(scales[i]) && scales[i] >= d->scale, DD_E_ARG, "%s: file %d at scale %d (1, 2, 4 or 8, and at least the decoder's %d)", who, i, scales[i], d->scale);
    DD_DEVICE(d->ctx);
    hipStream_t s = dd_pick_stream(d->ctx, stream);
    dd_jpeg_info *recs = d->recs_host.as<dd_jpeg_info>();
    dd_jpeg_scans *scans = d->progressive ? d->scans_host.as<dd_jpeg_scans>() : nullptr;
    size_t n_bytes = 0;
    for (int i = 0; i < n; ++i) {
        DD_REQUIRE(offsets[i] >= 0 && lengths[i] >= 0 && lengths[i] <= 0x7fffffffll, DD_E_ARG, "%s: file %d at offset %lld, length %lld", who, i,
                   (long long)offsets[i], (long long)lengths[i]);
        const size_t end = (size_t)offsets[i] + (size_t)lengths[i];
        DD_REQUIRE(end <= d->max_bytes, DD_E_CAPACITY, "%s: file %d ends at byte %zu, the decoder holds %zu", who, i, end, d->max_bytes);
        ddk::jpegdec_parse(files_host + offsets[i], (size_t)lengths[i], d->g.H, d->g.W, &recs[i], scans ? &scans[i] : nullptr, d->flags);
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
