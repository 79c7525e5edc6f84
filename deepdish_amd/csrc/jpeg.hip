// Baseline JPEG encoder for BGR frames in HBM: whole JFIF files, byte for byte what libjpeg writes for 4:2:0 at a given quality with
// restart markers (Pillow's Image.save(..., 'JPEG', quality=q, subsampling='4:2:0', restart_marker_rows=r)).  Serves the reference's
// cv2.imencode(".jpg", frame) (deepdish.py:168), --output-cvat-dir (:764-766) and --stream-path.  All integer arithmetic.
//
// One workgroup encodes one restart interval (restart_rows MCU rows of one frame): colour conversion and 2x2 chroma down-sampling, the
// accurate-integer forward DCT with quantisation (one thread per 8x8 block), the per-block bit counts, a scan of them, and then the
// bits themselves, laid into an 8 KiB window of LDS at their bit offsets, byte-stuffed and stored.  An interval's length is known only
// after it is coded, so a call is two launches of the same kernel: the first counts each interval's bytes, the second sums the counts
// of the intervals before its own and writes at the final offset.  Two paths (dd_jpeg_plan):
//   DD_JPEG_LDS      the interval's samples and coefficients stay in LDS between the phases;
//   DD_JPEG_STREAM   an interval too large for that: no sample or coefficient store at all, a block is transformed again from the
//                    frame wherever it is needed, and the per-block bit offsets and DC values live in device scratch (6 bytes a block).
#include "common.h"
#include "jpeg_tables.h"
#include <new>

namespace {

constexpr int JP_T = 256;                  // threads per workgroup
constexpr int JP_WIN = 8192;               // bytes of entropy-coded data per window: 32 per thread
constexpr int JP_WIN_DW = JP_WIN / 4;
constexpr int JP_MAX_SIDE = 8192;
constexpr int JP_LDS_MAX = 160 * 1024;

// device tables, 32-bit words: quantiser divisors 8 * q (natural order) [2][64], their reciprocals [2][64], DC codes [2][16], AC codes
// [2][256]; a code word is code << 5 | length
constexpr int JP_TAB_DIV = 0, JP_TAB_RCP = 128, JP_TAB_DC = 256, JP_TAB_AC = 288, JP_TAB_WORDS = 800;
constexpr int JP_FIXED_WORDS = JP_TAB_WORDS + JP_WIN_DW + 8;          // tables, window, scan scratch

struct JpGeom {
    int H, W, mw, mh, R, n_int, bw, bh, ch, hdr_len, nb_max;
};

// words of the bit offsets and DC values of nb blocks (8-byte aligned: the sample planes behind them are read as uint2)
__host__ __device__ inline size_t jp_state_words(int nb) {
    const size_t w = (size_t)nb + 1 + ((size_t)nb + 1) / 2;
    return w + (w & 1);
}

// ------------------------------------------------------------------------------------------------ device

// One 2x2 quad of the padded frame: chroma column cx, chroma row cy (frame coordinates).  Luma: rows and columns past the frame repeat
// the last one.  Chroma: columns likewise, one more row when H is odd, and past ceil(H / 2) rows the plane's own last row.
__device__ __forceinline__ void jp_quad(const uint8_t *__restrict__ frame, const JpGeom &g, int cy, int cx, int (&y)[4], int &cb, int &cr) {
    const int x0 = min(2 * cx, g.W - 1), x1 = min(2 * cx + 1, g.W - 1);
    int r[4], gr[4], b[4];
    auto load = [&](int row0, int row1) {
        const uint8_t *p0 = frame + ((size_t)row0 * g.W) * 3, *p1 = frame + ((size_t)row1 * g.W) * 3;
        b[0] = p0[x0 * 3], gr[0] = p0[x0 * 3 + 1], r[0] = p0[x0 * 3 + 2];
        b[1] = p0[x1 * 3], gr[1] = p0[x1 * 3 + 1], r[1] = p0[x1 * 3 + 2];
        b[2] = p1[x0 * 3], gr[2] = p1[x0 * 3 + 1], r[2] = p1[x0 * 3 + 2];
        b[3] = p1[x1 * 3], gr[3] = p1[x1 * 3 + 1], r[3] = p1[x1 * 3 + 2];
    };
    load(min(2 * cy, g.H - 1), min(2 * cy + 1, g.H - 1));
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = (19595 * r[i] + 38470 * gr[i] + 7471 * b[i] + 32768) >> 16;
    if (cy >= g.ch) load(2 * (g.ch - 1), min(2 * (g.ch - 1) + 1, g.H - 1));
    int sb = 0, sr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sb += (-11059 * r[i] - 21709 * gr[i] + 32768 * b[i] + (128 << 16) + 32767) >> 16;
        sr += (32768 * r[i] - 27439 * gr[i] - 5329 * b[i] + (128 << 16) + 32767) >> 16;
    }
    const int bias = 1 + (cx & 1);
    cb = (sb + bias) >> 2;
    cr = (sr + bias) >> 2;
}

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's jfdctint.c, one pass over 8 values at stride S of d.
template <int S, bool FIRST>
__device__ __forceinline__ void jp_fdct8(int *d) {
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2;
        d[4 * S] = (t10 - t11) << 2;
    } else {
        d[0] = jp_descale(t10 + t11, 2);
        d[4 * S] = jp_descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = jp_descale(z1 + t13 * 6270, N);
    d[6 * S] = jp_descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = jp_descale(u4 + z1 + z3, N);
    d[5 * S] = jp_descale(u5 + z2 + z4, N);
    d[3 * S] = jp_descale(u6 + z2 + z3, N);
    d[S] = jp_descale(u7 + z1 + z4, N);
}

// d: 64 samples (natural order) -> quantised coefficients in zigzag order at dst (LDS, 4-byte aligned).
// The quotient (|c| + d / 2) / d is taken as the high word of n * ceil(2^32 / d).  With m = (2^32 + e) / d, 0 <= e < d, that is
// floor(n / d + n e / (d 2^32)); the true fraction of n / d is at most 1 - 1 / d, so the floor is unchanged while n e < 2^32.  Here
// n < 2^16 (a coefficient is at most 8 * 64 * 128 * 1.42 in magnitude, plus d / 2 <= 1020) and e < d <= 2040 < 2^11: exact.
__device__ __forceinline__ void jp_transform(int (&d)[64], const uint32_t *tab, int sel, int16_t *dst, bool dummy) {
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] -= 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) jp_fdct8<1, true>(&d[8 * r]);
#pragma unroll
    for (int c = 0; c < 8; ++c) jp_fdct8<8, false>(&d[c]);
    int z[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int i = JP_ZIGZAG[k];
        const uint32_t div = tab[JP_TAB_DIV + sel * 64 + i], rcp = tab[JP_TAB_RCP + sel * 64 + i];
        const int c = d[i];
        const uint32_t n = (uint32_t)(c < 0 ? -c : c) + (div >> 1);
        const int q = (int)__umulhi(n, rcp);
        z[k] = dummy ? 0 : (c < 0 ? -q : q);
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
    for (int k = 0; k < 32; ++k) out[k] = ((uint32_t)z[2 * k] & 0xffffu) | ((uint32_t)z[2 * k + 1] << 16);
}

// OR `len` bits (1 .. 27) into the window at bit `rel` from its start, most significant bit first; rel may lie outside on either side.
__device__ __forceinline__ void jp_put(uint32_t *win, int rel, uint32_t code, int len) {
    const int j = rel >> 5, s = rel & 31;
    const unsigned long long v = (unsigned long long)code << (64 - s - len);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (j >= 0 && j < JP_WIN_DW && hi) atomicOr(&win[j], hi);
    if (j + 1 >= 0 && j + 1 < JP_WIN_DW && lo) atomicOr(&win[j + 1], lo);
}

__device__ __forceinline__ int jp_size(int v) { return 32 - __clz(v < 0 ? -v : v); }

// The DC difference's bits, then (AC) the run / size symbols of c[1 .. 63].  Returns the bit count; EMIT also lays the bits at rel.
template <bool DC, bool AC, bool EMIT>
__device__ __forceinline__ int jp_code(const uint32_t *tab, int sel, int diff, const int16_t *c, uint32_t *win, int rel) {
    int bits = 0;
    if (DC) {
        const int size = jp_size(diff);
        const uint32_t e = tab[JP_TAB_DC + sel * 16 + size];
        const int len = (int)(e & 31) + size;
        if (EMIT) jp_put(win, rel, ((e >> 5) << size) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1)), len);
        bits += len;
    }
    if (AC) {
        const uint32_t *ac = tab + JP_TAB_AC + sel * 256;
        int run = 0;
        for (int k = 1; k < 64; ++k) {
            const int v = c[k];
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                const uint32_t e = ac[0xF0];
                if (EMIT) jp_put(win, rel + bits, e >> 5, (int)(e & 31));
                bits += (int)(e & 31);
                run -= 16;
            }
            const int size = jp_size(v);
            const uint32_t e = ac[run * 16 + size];
            const int len = (int)(e & 31) + size;
            if (EMIT) jp_put(win, rel + bits, ((e >> 5) << size) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1)), len);
            bits += len;
            run = 0;
        }
        if (run) {
            const uint32_t e = ac[0];
            if (EMIT) jp_put(win, rel + bits, e >> 5, (int)(e & 31));
            bits += (int)(e & 31);
        }
    }
    return bits;
}

// Exclusive prefix sum over the workgroup's threads; total: the sum.  sc: 4 words of LDS.
__device__ __forceinline__ int jp_scan(int v, uint32_t *sc, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) sc[w] = (uint32_t)x;
    __syncthreads();
    int base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < JP_T / 64; ++i) {
        const int s = (int)sc[i];
        if (i < w) base += s;
        t += s;
    }
    total = t;
    return base + x - v;
}

struct JpBlock {
    int m, k, mrow, mx, sel;
    bool dummy;
};

__device__ __forceinline__ JpBlock jp_block(const JpGeom &g, int iv, int b) {
    JpBlock q;
    q.m = b / 6;
    q.k = b - q.m * 6;
    q.mrow = q.m / g.mw;
    q.mx = q.m - q.mrow * g.mw;
    q.sel = q.k < 4 ? 0 : 1;
    q.dummy = q.k < 4 && (2 * q.mx + (q.k & 1) >= g.bw || 2 * (iv * g.R + q.mrow) + (q.k >> 1) >= g.bh);
    return q;
}

// The predictor of block b's DC: the DC of the block of the same component before it in the interval, 0 at its start.
__device__ __forceinline__ int jp_pred(const int16_t *dcs, const JpBlock &q, int b) {
    if (q.k >= 1 && q.k <= 3) return dcs[b - 1];
    if (q.m == 0) return 0;
    return q.k == 0 ? dcs[b - 3] : dcs[b - 6];
}

// Block q's quantised coefficients -> dst (LDS, 128 bytes, 8-byte aligned).  RES: its samples lie in the LDS planes.  Otherwise they are
// converted from the frame into the first 64 bytes of dst itself (the thread's own slot), quad by quad, and read back from there.
template <bool RES>
__device__ __forceinline__ void jp_block_coefs(const JpGeom &g, const uint8_t *__restrict__ frame, int iv, const uint32_t *tab, const uint8_t *Ys,
                                               const uint8_t *Cs, int Wp, const JpBlock &q, int16_t *dst) {
    const uint8_t *p;
    int stride;
    if (RES) {
        if (q.k < 4) {
            stride = Wp;
            p = Ys + (size_t)(16 * q.mrow + 8 * (q.k >> 1)) * Wp + 16 * q.mx + 8 * (q.k & 1);
        } else {
            stride = Wp / 2;
            p = Cs + (size_t)((q.k - 4) * 8 * g.R + 8 * q.mrow) * stride + 8 * q.mx;
        }
    } else {
        uint8_t *s = reinterpret_cast<uint8_t *>(dst);
        if (q.k < 4) {
            const int cy0 = (iv * g.R + q.mrow) * 8 + 4 * (q.k >> 1), cx0 = q.mx * 8 + 4 * (q.k & 1);
#pragma unroll 1
            for (int i = 0; i < 16; ++i) {
                const int r = i >> 2, c = i & 3;
                int y[4], cb, cr;
                jp_quad(frame, g, cy0 + r, cx0 + c, y, cb, cr);
                s[16 * r + 2 * c] = (uint8_t)y[0], s[16 * r + 2 * c + 1] = (uint8_t)y[1];
                s[16 * r + 8 + 2 * c] = (uint8_t)y[2], s[16 * r + 8 + 2 * c + 1] = (uint8_t)y[3];
            }
        } else {
            const int cy0 = (iv * g.R + q.mrow) * 8, cx0 = q.mx * 8;
#pragma unroll 1
            for (int i = 0; i < 64; ++i) {
                int y[4], cb, cr;
                jp_quad(frame, g, cy0 + (i >> 3), cx0 + (i & 7), y, cb, cr);
                s[i] = (uint8_t)(q.k == 4 ? cb : cr);
            }
        }
        p = s;
        stride = 8;
    }
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p + (size_t)r * stride);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            d[8 * r + c] = (v.x >> (8 * c)) & 255;
            d[8 * r + 4 + c] = (v.y >> (8 * c)) & 255;
        }
    }
    jp_transform(d, tab, q.sel, dst, q.dummy);
}

// RES: the interval's samples and coefficients are resident in LDS.  Otherwise a block is transformed from the frame into the
// thread's own 128-byte slot each time it is needed, and bitoff / dcs are device scratch.
template <bool RES>
__global__ __launch_bounds__(JP_T) void jpeg_encode_k(JpGeom g, const uint8_t *__restrict__ frames, const uint32_t *__restrict__ tables,
                                                      const uint8_t *__restrict__ header, int *__restrict__ iv_bytes, uint32_t *gstate,
                                                      uint8_t *__restrict__ out, long long cap, int *__restrict__ lengths, int write) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / g.n_int, iv = blockIdx.x - f * g.n_int;
    const int nrows = min(g.R, g.mh - iv * g.R);
    const int NB = nrows * g.mw * 6;
    const int Wp = g.mw * 16;
    const uint8_t *frame = frames + (size_t)f * g.H * g.W * 3;

    uint32_t *tab = lds, *win = lds + JP_TAB_WORDS, *sc = win + JP_WIN_DW;
    uint32_t *bitoff;
    int16_t *dcs, *coef;
    uint8_t *Ys = nullptr, *Cs = nullptr;
    if (RES) {
        bitoff = lds + JP_FIXED_WORDS;
        dcs = reinterpret_cast<int16_t *>(bitoff + g.nb_max + 1);
        coef = reinterpret_cast<int16_t *>(bitoff + jp_state_words(g.nb_max));
        Ys = reinterpret_cast<uint8_t *>(coef + (size_t)g.nb_max * 64);
        Cs = Ys + (size_t)16 * g.R * Wp;                 // Cb [8 R][Wp / 2], then Cr
    } else {
        coef = reinterpret_cast<int16_t *>(lds + JP_FIXED_WORDS);            // [JP_T][64]: one slot per thread
        uint32_t *mine = gstate + (size_t)blockIdx.x * jp_state_words(g.nb_max);
        bitoff = mine;
        dcs = reinterpret_cast<int16_t *>(mine + g.nb_max + 1);
    }

    // where this interval goes (second launch): the header, the intervals before it and their markers
    long long base = 0;
    uint8_t *slot = out + (size_t)f * (size_t)cap;
    if (write) {
        int before = 0, all = 0;
        for (int j = tid; j < g.n_int; j += JP_T) {
            const int v = iv_bytes[(size_t)f * g.n_int + j];
            all += v;
            if (j < iv) before += v;
        }
        int t_before, t_all;
        jp_scan(before, sc, t_before);
        jp_scan(all, sc, t_all);
        const long long length = (long long)g.hdr_len + t_all + 2ll * g.n_int;         // RSTn after every interval but the last, then EOI
        if (iv == g.n_int - 1 && tid == 0) lengths[f] = (int)min(length, 0x7fffffffll);
        if (length > cap) return;                                                       // a file that does not fit writes nothing
        base = (long long)g.hdr_len + t_before + 2ll * iv;
        if (iv == 0)
            for (int i = tid; i < g.hdr_len; i += JP_T) slot[i] = header[i];
    }

    for (int i = tid; i < JP_TAB_WORDS; i += JP_T) tab[i] = tables[i];

    if (RES) {      // colour conversion and down-sampling into LDS
        const int half = Wp / 2, nq = 8 * nrows * half;
        for (int q = tid; q < nq; q += JP_T) {
            const int cyl = q / half, cx = q - cyl * half;
            int y[4], cb, cr;
            jp_quad(frame, g, iv * g.R * 8 + cyl, cx, y, cb, cr);
            *reinterpret_cast<uint16_t *>(Ys + (size_t)(2 * cyl) * Wp + 2 * cx) = (uint16_t)(y[0] | (y[1] << 8));
            *reinterpret_cast<uint16_t *>(Ys + (size_t)(2 * cyl + 1) * Wp + 2 * cx) = (uint16_t)(y[2] | (y[3] << 8));
            Cs[(size_t)cyl * half + cx] = (uint8_t)cb;
            Cs[(size_t)(8 * g.R + cyl) * half + cx] = (uint8_t)cr;
        }
    }
    __syncthreads();

    // transform every block; keep its DC and the bits of its AC part
    for (int b = tid; b < NB; b += JP_T) {
        const JpBlock q = jp_block(g, iv, b);
        int16_t *c = RES ? coef + (size_t)b * 64 : coef + tid * 64;
        jp_block_coefs<RES>(g, frame, iv, tab, Ys, Cs, Wp, q, c);
        dcs[b] = c[0];
        bitoff[b] = (uint32_t)jp_code<false, true, false>(tab, q.sel, 0, c, nullptr, 0);
    }
    __syncthreads();
    // a dummy block carries the DC of the block before it in its MCU
    for (int m = tid; m < NB / 6; m += JP_T)
        for (int k = 1; k < 4; ++k)
            if (jp_block(g, iv, m * 6 + k).dummy) dcs[m * 6 + k] = dcs[m * 6 + k - 1];
    __syncthreads();
    for (int b = tid; b < NB; b += JP_T) {
        const JpBlock q = jp_block(g, iv, b);
        bitoff[b] += (uint32_t)jp_code<true, false, false>(tab, q.sel, dcs[b] - jp_pred(dcs, q, b), nullptr, nullptr, 0);
    }
    __syncthreads();
    // bit counts -> bit offsets; bitoff[NB]: the interval's bits
    int total_bits;
    {
        const int per = (NB + JP_T - 1) / JP_T, b0 = min(tid * per, NB), b1 = min(b0 + per, NB);
        int sum = 0;
        for (int b = b0; b < b1; ++b) sum += (int)bitoff[b];
        int run = jp_scan(sum, sc, total_bits);
        for (int b = b0; b < b1; ++b) {
            const int n = (int)bitoff[b];
            bitoff[b] = (uint32_t)run;
            run += n;
        }
        if (tid == 0) bitoff[NB] = (uint32_t)total_bits;
    }
    __syncthreads();

    const int total_bytes = (total_bits + 7) >> 3;
    long long written = 0;                                  // stuffed bytes of the windows before this one
    for (int w0 = 0; w0 < total_bytes; w0 += JP_WIN) {
        const int nbytes = min(JP_WIN, total_bytes - w0);
        const int bit0 = w0 * 8, bit1 = bit0 + nbytes * 8;
#pragma unroll
        for (int i = 0; i < JP_WIN_DW / JP_T; ++i) win[tid * (JP_WIN_DW / JP_T) + i] = 0;
        __syncthreads();
        // the blocks with a bit in this window: the first whose end lies past bit0 .. the last whose start lies before bit1
        int lo = 0, hi = NB;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)bitoff[mid + 1] > bit0) hi = mid;
            else lo = mid + 1;
        }
        const int first = lo;
        hi = NB;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)bitoff[mid] >= bit1) hi = mid;
            else lo = mid + 1;
        }
        const int last = lo;
        for (int b = first + tid; b < last; b += JP_T) {
            const JpBlock q = jp_block(g, iv, b);
            const int16_t *c = coef + (size_t)b * 64;
            if (!RES) {
                jp_block_coefs<RES>(g, frame, iv, tab, Ys, Cs, Wp, q, coef + tid * 64);
                c = coef + tid * 64;
            }
            jp_code<true, true, true>(tab, q.sel, dcs[b] - jp_pred(dcs, q, b), c, win, (int)bitoff[b] - bit0);
        }
        if (tid == 0 && (total_bits & 7) && bit1 >= total_bits)                  // the last byte's padding: 1-bits
            jp_put(win, total_bits - bit0, (1u << (8 - (total_bits & 7))) - 1, 8 - (total_bits & 7));
        __syncthreads();
        // byte stuffing: a 0x00 after every 0xFF
        constexpr int PER = JP_WIN / JP_T;
        const int k0 = tid * PER;
        uint32_t v[PER / 4];
        int ff = 0;
#pragma unroll
        for (int i = 0; i < PER / 4; ++i) {
            v[i] = win[tid * (PER / 4) + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) ff += (k0 + 4 * i + j < nbytes && ((v[i] >> (24 - 8 * j)) & 255) == 255) ? 1 : 0;
        }
        int ff_all;
        const int ff_before = jp_scan(ff, sc, ff_all);
        if (write) {
            long long p = base + written + k0 + ff_before;
#pragma unroll
            for (int i = 0; i < PER / 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + 4 * i + j < nbytes) {
                        const uint32_t byte = (v[i] >> (24 - 8 * j)) & 255;
                        if (p < cap) slot[p] = (uint8_t)byte;
                        ++p;
                        if (byte == 255) {
                            if (p < cap) slot[p] = 0;
                            ++p;
                        }
                    }
        }
        written += nbytes + ff_all;
        __syncthreads();
    }
    if (tid == 0) {
        if (!write) iv_bytes[(size_t)f * g.n_int + iv] = (int)written;
        else {
            const long long p = base + written;
            if (p + 1 < cap) {
                slot[p] = 0xFF;
                slot[p + 1] = iv == g.n_int - 1 ? 0xD9 : (uint8_t)(0xD0 + (iv & 7));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host

int jp_geometry(int h, int w, int restart_rows, const char *who, JpGeom *g) {
    DD_REQUIRE(h >= 1 && w >= 1 && h <= JP_MAX_SIDE && w <= JP_MAX_SIDE, DD_E_ARG, "%s: a %d x %d frame (h, w: 1 .. %d either way)", who, w, h, JP_MAX_SIDE);
    DD_REQUIRE(restart_rows >= 1, DD_E_ARG, "%s: restart_rows %d (>= 1)", who, restart_rows);
    g->H = h, g->W = w;
    g->mw = (w + 15) / 16, g->mh = (h + 15) / 16;
    DD_REQUIRE((long long)restart_rows * g->mw <= 65535, DD_E_ARG, "%s: restart_rows %d makes an interval of %lld MCUs (<= 65535)", who, restart_rows,
               (long long)restart_rows * g->mw);
    g->R = restart_rows < g->mh ? restart_rows : g->mh;          // rows a workgroup holds; the DRI segment states restart_rows itself
    g->n_int = (g->mh + g->R - 1) / g->R;
    g->bw = (w + 7) / 8, g->bh = (h + 7) / 8, g->ch = (h + 1) / 2;
    g->nb_max = g->R * g->mw * 6;
    g->hdr_len = 0;
    return DD_OK;
}

// LDS of the resident path: tables, window, scan scratch, bit offsets, DCs, coefficients, Y, Cb, Cr
size_t jp_lds_resident(const JpGeom &g) {
    const size_t nb = (size_t)g.nb_max;
    return 4 * (size_t)JP_FIXED_WORDS + 4 * jp_state_words(g.nb_max) + 128 * nb + (size_t)24 * g.R * g.mw * 16;
}
constexpr size_t JP_LDS_STREAM = 4 * (size_t)JP_FIXED_WORDS + (size_t)JP_T * 128;

}  // namespace

struct dd_jpeg {
    dd_ctx *ctx = nullptr;
    JpGeom g{};
    int quality = 0, path = 0;
    std::vector<uint8_t> header;
    bool on_device = false;
    DevBuf tables, header_dev, iv_bytes, state;
    PinBuf lengths;
};

extern "C" {

int dd_jpeg_plan(int h, int w, int restart_rows, int *path_out) {
    DD_REQUIRE(path_out, DD_E_ARG, "dd_jpeg_plan: NULL argument");
    JpGeom g;
    const int rc = jp_geometry(h, w, restart_rows, "dd_jpeg_plan", &g);
    if (rc != DD_OK) return rc;
    *path_out = jp_lds_resident(g) <= (size_t)JP_LDS_MAX ? DD_JPEG_LDS : DD_JPEG_STREAM;
    return DD_OK;
}

int dd_jpeg_create(dd_ctx *ctx, int h, int w, int quality, int restart_rows, dd_jpeg **out) {
    DD_REQUIRE(out, DD_E_ARG, "dd_jpeg_create: NULL argument");
    DD_REQUIRE(quality >= 1 && quality <= 100, DD_E_ARG, "dd_jpeg_create: quality %d (1 .. 100)", quality);
    JpGeom g;
    const int rc = jp_geometry(h, w, restart_rows, "dd_jpeg_create", &g);
    if (rc != DD_OK) return rc;
    dd_jpeg *e = new (std::nothrow) dd_jpeg();
    DD_REQUIRE(e, DD_E_HIP, "dd_jpeg_create: out of host memory");
    e->ctx = ctx;
    e->quality = quality;
    jp_build_header(h, w, quality, restart_rows, e->header);
    g.hdr_len = (int)e->header.size();
    e->g = g;
    e->path = jp_lds_resident(g) <= (size_t)JP_LDS_MAX ? DD_JPEG_LDS : DD_JPEG_STREAM;
    *out = e;
    return DD_OK;
}

int dd_jpeg_destroy(dd_jpeg *e) {
    if (!e) return DD_OK;
    if (e->ctx) (void)hipSetDevice(e->ctx->device);
    e->tables.release();
    e->header_dev.release();
    e->iv_bytes.release();
    e->state.release();
    e->lengths.release();
    delete e;
    return DD_OK;
}

int dd_jpeg_header(dd_jpeg *e, uint8_t *buf_host, int cap, int *len_host) {
    DD_REQUIRE(e && len_host, DD_E_ARG, "dd_jpeg_header: NULL argument");
    *len_host = (int)e->header.size();
    if (!buf_host) return DD_OK;
    DD_REQUIRE(cap >= (int)e->header.size(), DD_E_CAPACITY, "dd_jpeg_header: the header is %zu bytes, the buffer %d", e->header.size(), cap);
    memcpy(buf_host, e->header.data(), e->header.size());
    return DD_OK;
}

int dd_jpeg_encode(dd_jpeg *e, const uint8_t *frames_dev, int n, uint8_t *out_dev, int64_t cap, int *lengths_dev, void *stream) {
    DD_REQUIRE(e && frames_dev && out_dev && lengths_dev, DD_E_ARG, "dd_jpeg_encode: NULL argument");
    DD_REQUIRE(e->ctx, DD_E_STATE, "dd_jpeg_encode: the encoder was created without a context (header only)");
    DD_REQUIRE(n >= 1 && (long long)n * e->g.n_int <= 0x7fffffffll, DD_E_ARG, "dd_jpeg_encode: n %d frames of %d intervals", n, e->g.n_int);
    DD_REQUIRE(cap >= 1, DD_E_ARG, "dd_jpeg_encode: cap %lld", (long long)cap);
    DD_DEVICE(e->ctx);
    hipStream_t s = dd_pick_stream(e->ctx, stream);
    const JpGeom &g = e->g;
    if (!e->on_device) {
        uint32_t tab[JP_TAB_WORDS] = {0};
        uint8_t q[2][64];
        jp_quant(e->quality, q);
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < 64; ++i) {
                const uint32_t d = 8u * q[t][i];
                tab[JP_TAB_DIV + t * 64 + i] = d;
                tab[JP_TAB_RCP + t * 64 + i] = (uint32_t)(((1ull << 32) + d - 1) / d);
            }
        jp_huffman(JP_DC_LUMA_BITS, JP_DC_VALS, tab + JP_TAB_DC);
        jp_huffman(JP_DC_CHROMA_BITS, JP_DC_VALS, tab + JP_TAB_DC + 16);
        jp_huffman(JP_AC_LUMA_BITS, JP_AC_LUMA_VALS, tab + JP_TAB_AC);
        jp_huffman(JP_AC_CHROMA_BITS, JP_AC_CHROMA_VALS, tab + JP_TAB_AC + 256);
        if (int rc = e->tables.reserve(sizeof(tab))) return rc;
        if (int rc = e->header_dev.reserve(e->header.size())) return rc;
        DD_HIP(hipMemcpy(e->tables.p, tab, sizeof(tab), hipMemcpyHostToDevice));
        DD_HIP(hipMemcpy(e->header_dev.p, e->header.data(), e->header.size(), hipMemcpyHostToDevice));
        e->on_device = true;
    }
    const size_t groups = (size_t)n * g.n_int;
    if (int rc = e->iv_bytes.reserve(groups * sizeof(int))) return rc;
    if (int rc = e->lengths.reserve((size_t)n * sizeof(int))) return rc;
    size_t lds;
    if (e->path == DD_JPEG_LDS) {
        lds = jp_lds_resident(g);
        static DevOnce once;
        const int rc = once.run(e->ctx->device, [&]() -> int {
            DD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&jpeg_encode_k<true>), hipFuncAttributeMaxDynamicSharedMemorySize, JP_LDS_MAX));
            return DD_OK;
        });
        if (rc != DD_OK) return rc;
    } else {
        lds = JP_LDS_STREAM;
        if (int rc = e->state.reserve(groups * jp_state_words(g.nb_max) * sizeof(uint32_t))) return rc;
    }
    for (int write = 0; write < 2; ++write) {
        if (e->path == DD_JPEG_LDS)
            hipLaunchKernelGGL(jpeg_encode_k<true>, dim3((unsigned)groups), dim3(JP_T), lds, s, g, frames_dev, e->tables.as<uint32_t>(), e->header_dev.as<uint8_t>(),
                               e->iv_bytes.as<int>(), (uint32_t *)nullptr, out_dev, (long long)cap, lengths_dev, write);
        else
            hipLaunchKernelGGL(jpeg_encode_k<false>, dim3((unsigned)groups), dim3(JP_T), lds, s, g, frames_dev, e->tables.as<uint32_t>(), e->header_dev.as<uint8_t>(),
                               e->iv_bytes.as<int>(), e->state.as<uint32_t>(), out_dev, (long long)cap, lengths_dev, write);
        DD_LAUNCH_CHECK();
    }
    // the lengths decide the return code: the one place this call waits for the device
    DD_HIP(hipMemcpyAsync(e->lengths.p, lengths_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    DD_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        DD_REQUIRE(e->lengths.as<int>()[i] <= cap, DD_E_CAPACITY, "dd_jpeg_encode: frame %d is %d bytes, a slot %lld (the other frames are complete)", i,
                   e->lengths.as<int>()[i], (long long)cap);
    return DD_OK;
}

}  // extern "C"
