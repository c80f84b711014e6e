// j2k_device.h -- the JPEG 2000 tile decoder behind the packet headers, in the form the GPU runs: plain __host__ __device__
// routines over flat buffers.  One header, three users: the kernels of kernels_j2k.hip, the host entry bqio_j2k_decode_canvas
// (j2k_host.cpp: the very same routines on the CPU, for the tests and the fuzzer) and tools/fuzz/j2k_fuzz.cpp.
//
// Input is what bqio_j2k_extract (j2k_host.cpp, tier 2) leaves: per segment a descriptor (Seg), per code block a row of the
// block table (Block) and the block's MQ codeword in a packed byte buffer.  The stages:
//   t1_block       the EBCOT bit-plane decoder of one code block (T.800 Annex C and D, code-block style 0) into the
//                  segment's coefficient plane, as signed magnitudes with one fraction bit (value * 2 + the half of the last
//                  decoded plane: OpenJPEG's midpoint reconstruction)
//   dequant_sample value / 2 (reversible) or value * step / 2 (irreversible) by the sample's sub-band
//   synth_1d       one line of one level of the inverse 5/3 (integer) or 9/7 (float) transform, rows first, then columns
//   finish_pixel   inverse RCT / ICT, rounding (half to even), level shift, clamp, and the reader's YCbCr -> RGB (j2k_ycc.h)
//
// Bounds.  t1_block touches samples (x0 + x, y0 + y), x < w, y < h only, and block_ok() has shown that rectangle inside the
// segment's w x h plane before it runs; a neighbour outside the block is never read (its flag bits are simply never set).
// The MQ decoder reads byte i of the codeword through mq_byte(), which answers 0xFF for i >= len -- the two synthetic FF
// bytes of the standard -- and the extractor additionally pads every codeword with them.  Loops: passes <= 3 * 30 - 2, each
// over w * h <= 4096 samples, renormalisation shifts at most 15 times a decision.  synth_1d reads and writes n samples of
// the line it is given.  Nothing else is data dependent.
//
// The float arithmetic of the 9/7 path must give the same bits on both builds: contraction of a * b + c into one fused
// operation is switched off for everything that follows in the translation unit: by the pragma below under clang (hipcc
// contracts by default), by -ffp-contract=off under g++ (the Makefile's libbiscuit_io rule), whose default would contract
// wherever the target has a fused operation -- such a build without the flag is refused below.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "canvas_place.h"
#include "j2k_ycc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQK_HD __host__ __device__ inline
#else
#define BQK_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FP_FAST_FMAF) && !defined(BQK_CONTRACT_OFF)
#error "this target has a fused multiply-add: compile with -ffp-contract=off -DBQK_CONTRACT_OFF"
#endif

namespace bqj2k {

// status of one segment: 0 = decoded
enum { ST_OK = 0,
       ST_DESC = 16,       // a descriptor or block row the decoder does not take (checked again on the device)
       ST_SUBSET = 32,     // a valid-looking stream outside the device's subset (the extractor's refusal)
       ST_DAMAGED = 64 };  // a stream the extractor could not follow: bad marker, a length past the end, truncated packets

constexpr int MAX_SIDE = 512, MAX_LEVELS = 6, MAX_BANDS = 3 * MAX_LEVELS + 1, MAX_CBLK = 64, MAX_BPS = 30;
constexpr int SEG_I32 = 32, BLOCK_I32 = 12;
constexpr uint32_t CW_ALIGN = 4, CW_PAD = 4;      // a codeword starts at a multiple of 4 and has FF FF (and two more) behind it

struct Seg {                 // SEG_I32 int32
    int32_t status, w, h, levels, reversible, mct, first_block, n_blocks;
    float half_step[MAX_BANDS];          // 0.5 * step of sub-band b (LL, then HL LH HH per resolution); unused when reversible
    int32_t guard, layers, progression, reserved[2];
};
static_assert(sizeof(Seg) == SEG_I32 * 4, "Seg is 32 dwords");

struct Block {               // BLOCK_I32 int32
    int32_t seg, comp, band;             // band: index into half_step | orientation << 8 | resolution << 16
    int32_t x0, y0, w, h;                // the block's rectangle in the component's plane (sub-bands in Mallat order)
    int32_t mb, zbp, passes;             // Mb of the sub-band, missing bit-planes, coding passes to decode
    uint32_t off, len;                   // the codeword in the packed buffer
};
static_assert(sizeof(Block) == BLOCK_I32 * 4, "Block is 12 dwords");

BQK_HD int ceil_shift(int v, int s) { return (int)(((int64_t)v + ((int64_t)1 << s) - 1) >> s); }

BQK_HD bool seg_ok(const Seg& s, int seg_w, int seg_h) {
    return s.w == seg_w && s.h == seg_h && s.w >= 1 && s.h >= 1 && s.w <= MAX_SIDE && s.h <= MAX_SIDE && s.levels >= 0 &&
           s.levels <= MAX_LEVELS && (s.reversible == 0 || s.reversible == 1) && (s.mct == 0 || s.mct == 1);
}

BQK_HD bool block_ok(const Block& b, int n_seg, int seg_w, int seg_h, uint64_t bytes) {
    return b.seg >= 0 && b.seg < n_seg && b.comp >= 0 && b.comp < 3 && ((b.band >> 8) & 255) < 4 && b.w >= 1 && b.h >= 1 && b.w <= MAX_CBLK &&
           b.h <= MAX_CBLK && b.x0 >= 0 && b.y0 >= 0 && b.x0 <= seg_w - b.w && b.y0 <= seg_h - b.h && b.zbp >= 0 && b.mb - b.zbp >= 1 &&
           b.mb - b.zbp <= MAX_BPS && b.passes >= 1 && b.passes <= 3 * (b.mb - b.zbp) - 2 && (uint64_t)b.off + b.len + 2 <= bytes;
}

// ---- MQ decoder (T.800 Annex C, software conventions) ----------------------------------------------------------------------
// T.800 Table C.2, a row per state: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
constexpr int MQ_STATES = 47;
#define MQ_ROW(qe, nmps, nlps, sw) ((uint32_t)(qe) | (uint32_t)(nmps) << 16 | (uint32_t)(nlps) << 22 | (uint32_t)(sw) << 28)
#define BQK_MQ_TABLE { \
    MQ_ROW(0x5601, 1, 1, 1), MQ_ROW(0x3401, 2, 6, 0), MQ_ROW(0x1801, 3, 9, 0), MQ_ROW(0x0AC1, 4, 12, 0), \
    MQ_ROW(0x0521, 5, 29, 0), MQ_ROW(0x0221, 38, 33, 0), MQ_ROW(0x5601, 7, 6, 1), MQ_ROW(0x5401, 8, 14, 0), \
    MQ_ROW(0x4801, 9, 14, 0), MQ_ROW(0x3801, 10, 14, 0), MQ_ROW(0x3001, 11, 17, 0), MQ_ROW(0x2401, 12, 18, 0), \
    MQ_ROW(0x1C01, 13, 20, 0), MQ_ROW(0x1601, 29, 21, 0), MQ_ROW(0x5601, 15, 14, 1), MQ_ROW(0x5401, 16, 14, 0), \
    MQ_ROW(0x5101, 17, 15, 0), MQ_ROW(0x4801, 18, 16, 0), MQ_ROW(0x3801, 19, 17, 0), MQ_ROW(0x3401, 20, 18, 0), \
    MQ_ROW(0x3001, 21, 19, 0), MQ_ROW(0x2801, 22, 19, 0), MQ_ROW(0x2401, 23, 20, 0), MQ_ROW(0x2201, 24, 21, 0), \
    MQ_ROW(0x1C01, 25, 22, 0), MQ_ROW(0x1801, 26, 23, 0), MQ_ROW(0x1601, 27, 24, 0), MQ_ROW(0x1401, 28, 25, 0), \
    MQ_ROW(0x1201, 29, 26, 0), MQ_ROW(0x1101, 30, 27, 0), MQ_ROW(0x0AC1, 31, 28, 0), MQ_ROW(0x09C1, 32, 29, 0), \
    MQ_ROW(0x08A1, 33, 30, 0), MQ_ROW(0x0521, 34, 31, 0), MQ_ROW(0x0441, 35, 32, 0), MQ_ROW(0x02A1, 36, 33, 0), \
    MQ_ROW(0x0221, 37, 34, 0), MQ_ROW(0x0141, 38, 35, 0), MQ_ROW(0x0111, 39, 36, 0), MQ_ROW(0x0085, 40, 37, 0), \
    MQ_ROW(0x0049, 41, 38, 0), MQ_ROW(0x0025, 42, 39, 0), MQ_ROW(0x0015, 43, 40, 0), MQ_ROW(0x0009, 44, 41, 0), \
    MQ_ROW(0x0005, 45, 42, 0), MQ_ROW(0x0001, 45, 43, 0), MQ_ROW(0x5601, 46, 46, 0) }
BQK_HD uint32_t mq_table_row(int i) {
    static constexpr uint32_t T[MQ_STATES] = BQK_MQ_TABLE;
    return T[i];
}

enum { CX_ZC = 0, CX_SC = 9, CX_MAG = 14, CX_AGG = 17, CX_UNI = 18, CX_N = 19 };

struct Mq {
    const uint8_t* d;
    const uint32_t* tab;                 // the MQ_STATES rows (the device keeps a copy in LDS)
    uint8_t* cx;                         // CX_N context bytes, state << 1 | mps, context k at cx[k * cxs]
    uint32_t cxs, len, bp, a, c, ct;
};

BQK_HD uint32_t mq_byte(const Mq& m, uint32_t i) { return i < m.len ? m.d[i] : 0xFFu; }

BQK_HD void mq_bytein(Mq& m) {
    if (mq_byte(m, m.bp) == 0xFF) {
        const uint32_t nx = mq_byte(m, m.bp + 1);
        if (nx > 0x8F) { m.c += 0xFF00; m.ct = 8; }
        else { ++m.bp; m.c += nx << 9; m.ct = 7; }
    } else {
        ++m.bp;
        m.c += mq_byte(m, m.bp) << 8;
        m.ct = 8;
    }
}

BQK_HD void mq_init(Mq& m, const uint8_t* d, uint32_t len, const uint32_t* tab, uint8_t* cx, uint32_t cxs) {
    m.d = d; m.len = len; m.bp = 0; m.tab = tab; m.cx = cx; m.cxs = cxs;
    for (int i = 0; i < CX_N; ++i) cx[i * cxs] = 0;
    cx[CX_UNI * cxs] = 46 << 1; cx[CX_AGG * cxs] = 3 << 1; cx[CX_ZC * cxs] = 4 << 1;
    m.c = mq_byte(m, 0) << 16;
    mq_bytein(m);
    m.c <<= 7; m.ct -= 7; m.a = 0x8000;
}

BQK_HD uint32_t mq_decode(Mq& m, int cx) {
    uint8_t* const slot = m.cx + (uint32_t)cx * m.cxs;
    const uint32_t s = *slot, mps = s & 1u, row = m.tab[s >> 1];
    const uint32_t qe = row & 0xFFFF, to_mps = (row >> 16 & 63) << 1 | mps, to_lps = (row >> 22 & 63) << 1 | (mps ^ (row >> 28));
    uint32_t d;
    m.a -= qe;
    if ((m.c >> 16) < qe) {              // LPS exchange
        if (m.a < qe) { d = mps; *slot = (uint8_t)to_mps; }
        else { d = mps ^ 1u; *slot = (uint8_t)to_lps; }
        m.a = qe;
    } else {
        m.c -= qe << 16;
        if (m.a & 0x8000) return mps;
        if (m.a < qe) { d = mps ^ 1u; *slot = (uint8_t)to_lps; }
        else { d = mps; *slot = (uint8_t)to_mps; }
    }
    do {                                 // renormalise: at most 15 shifts (qe >= 1)
        if (m.ct == 0) mq_bytein(m);
        m.a <<= 1; m.c <<= 1; --m.ct;
    } while (!(m.a & 0x8000));
    return d;
}

// ---- tier 1 ----------------------------------------------------------------------------------------------------------------
// a sample's flags: which neighbours are significant, the sign of the four direct ones, and the sample's own state
enum { F_W = 1, F_E = 2, F_N = 4, F_S = 8, F_NW = 16, F_NE = 32, F_SW = 64, F_SE = 128, F_NEG_W = 256, F_NEG_E = 512, F_NEG_N = 1024,
       F_NEG_S = 2048, F_SIG = 4096, F_VISIT = 8192, F_REFINE = 16384, F_NBR = 255 };

BQK_HD int zc_context(uint32_t f, int orient) {
    int h = (int)(f & 1) + (int)(f >> 1 & 1), v = (int)(f >> 2 & 1) + (int)(f >> 3 & 1);
    const int d = (int)(f >> 4 & 1) + (int)(f >> 5 & 1) + (int)(f >> 6 & 1) + (int)(f >> 7 & 1);
    if (orient == 3) {
        const int hv = h + v;
        if (d >= 3) return 8;
        if (d == 2) return hv >= 1 ? 7 : 6;
        if (d == 1) return hv >= 2 ? 5 : hv == 1 ? 4 : 3;
        return hv >= 2 ? 2 : hv;
    }
    if (orient == 1) { const int t = h; h = v; v = t; }
    if (h == 2) return 8;
    if (h == 1) return v >= 1 ? 7 : d >= 1 ? 6 : 5;
    if (v == 2) return 4;
    if (v == 1) return 3;
    return d >= 2 ? 2 : d;
}

// -> context | xor bit << 8
BQK_HD int sc_context(uint32_t f) {
    int h = 0, v = 0;
    if (f & F_W) h += (f & F_NEG_W) ? -1 : 1;
    if (f & F_E) h += (f & F_NEG_E) ? -1 : 1;
    if (f & F_N) v += (f & F_NEG_N) ? -1 : 1;
    if (f & F_S) v += (f & F_NEG_S) ? -1 : 1;
    h = h > 1 ? 1 : h < -1 ? -1 : h;
    v = v > 1 ? 1 : v < -1 ? -1 : v;
    int x = 0;
    if (h < 0) { h = -h; v = -v; x = 1; }
    else if (h == 0 && v < 0) { v = -v; x = 1; }
    const int cx = h == 1 ? 12 + v : 9 + v;          // (1,1) 13, (1,0) 12, (1,-1) 11, (0,1) 10, (0,0) 9
    return cx | x << 8;
}

struct T1 {
    int32_t* coef;                       // the block's first sample in the plane
    uint16_t* flag;
    int stride, w, h, orient;
    Mq mq;
};

BQK_HD void t1_set_significant(T1& t, int x, int y, uint32_t neg) {
    uint16_t* f = t.flag + (size_t)y * t.stride + x;
    const int s = t.stride;
    const bool l = x > 0, r = x + 1 < t.w, u = y > 0, d = y + 1 < t.h;
    f[0] |= F_SIG;
    if (l) f[-1] |= (uint16_t)(F_E | (neg ? F_NEG_E : 0));
    if (r) f[1] |= (uint16_t)(F_W | (neg ? F_NEG_W : 0));
    if (u) {
        f[-s] |= (uint16_t)(F_S | (neg ? F_NEG_S : 0));
        if (l) f[-s - 1] |= F_SE;
        if (r) f[-s + 1] |= F_SW;
    }
    if (d) {
        f[s] |= (uint16_t)(F_N | (neg ? F_NEG_N : 0));
        if (l) f[s - 1] |= F_NE;
        if (r) f[s + 1] |= F_NW;
    }
}

// decode the sign of (x, y), make it significant at the plane whose doubled value is `oneplushalf`
BQK_HD void t1_new_significant(T1& t, int x, int y, int32_t oneplushalf) {
    const size_t i = (size_t)y * t.stride + x;
    const int sc = sc_context(t.flag[i]);
    const uint32_t neg = mq_decode(t.mq, sc & 255) ^ (uint32_t)(sc >> 8);
    t.coef[i] = neg ? -oneplushalf : oneplushalf;
    t1_set_significant(t, x, y, neg);
}

BQK_HD void t1_sigpass(T1& t, int bp1) {
    const int32_t oph = (1 << bp1) | (1 << bp1 >> 1);
    for (int k = 0; k < t.h; k += 4)
        for (int x = 0; x < t.w; ++x)
            for (int y = k; y < k + 4 && y < t.h; ++y) {
                const size_t i = (size_t)y * t.stride + x;
                const uint32_t f = t.flag[i];
                if ((f & F_SIG) || !(f & F_NBR)) continue;
                if (mq_decode(t.mq, CX_ZC + zc_context(f, t.orient))) t1_new_significant(t, x, y, oph);
                t.flag[i] |= F_VISIT;
            }
}

BQK_HD void t1_refpass(T1& t, int bp1) {
    const int32_t half = 1 << bp1 >> 1;
    for (int k = 0; k < t.h; k += 4)
        for (int x = 0; x < t.w; ++x)
            for (int y = k; y < k + 4 && y < t.h; ++y) {
                const size_t i = (size_t)y * t.stride + x;
                const uint32_t f = t.flag[i];
                if ((f & (F_SIG | F_VISIT)) != F_SIG) continue;
                const int cx = (f & F_REFINE) ? CX_MAG + 2 : (f & F_NBR) ? CX_MAG + 1 : CX_MAG;
                const int32_t step = mq_decode(t.mq, cx) ? half : -half;
                t.coef[i] += t.coef[i] < 0 ? -step : step;
                t.flag[i] = (uint16_t)(f | F_REFINE);
            }
}

BQK_HD void t1_clnpass(T1& t, int bp1) {
    const int32_t oph = (1 << bp1) | (1 << bp1 >> 1);
    for (int k = 0; k < t.h; k += 4)
        for (int x = 0; x < t.w; ++x) {
            int y = k;
            if (k + 4 <= t.h) {                              // a whole stripe column: the run-length mode
                const uint16_t* f = t.flag + (size_t)k * t.stride + x;
                const uint32_t any = f[0] | f[t.stride] | f[2 * t.stride] | f[3 * t.stride];
                if (!(any & (F_SIG | F_VISIT | F_NBR))) {
                    if (!mq_decode(t.mq, CX_AGG)) continue;
                    int run = (int)mq_decode(t.mq, CX_UNI) << 1;
                    run |= (int)mq_decode(t.mq, CX_UNI);
                    t1_new_significant(t, x, k + run, oph);
                    y = k + run + 1;
                }
            }
            for (; y < k + 4 && y < t.h; ++y) {
                const size_t i = (size_t)y * t.stride + x;
                const uint32_t f = t.flag[i];
                if (f & (F_SIG | F_VISIT)) continue;
                if (mq_decode(t.mq, CX_ZC + zc_context(f, t.orient))) t1_new_significant(t, x, y, oph);
            }
        }
    for (int y = 0; y < t.h; ++y)
        for (int x = 0; x < t.w; ++x) t.flag[(size_t)y * t.stride + x] &= (uint16_t)~F_VISIT;
}

// One code block: b has passed block_ok; coef and flag are the component's planes (stride = the segment's width), zero where
// the block lies.
// tab: the MQ table's rows; cx, cxs: room for the CX_N context bytes, context k at cx[k * cxs].
BQK_HD void t1_block(const Block& b, const uint8_t* bytes, int32_t* coef, uint16_t* flag, int stride, const uint32_t* tab, uint8_t* cx,
                     uint32_t cxs) {
    T1 t;
    t.coef = coef + (size_t)b.y0 * stride + b.x0;
    t.flag = flag + (size_t)b.y0 * stride + b.x0;
    t.stride = stride; t.w = b.w; t.h = b.h; t.orient = (b.band >> 8) & 255;
    mq_init(t.mq, bytes + b.off, b.len, tab, cx, cxs);
    int bp1 = b.mb - b.zbp, type = 2;
    for (int p = 0; p < b.passes && bp1 >= 1; ++p) {
        if (type == 0) t1_sigpass(t, bp1);
        else if (type == 1) t1_refpass(t, bp1);
        else t1_clnpass(t, bp1);
        if (++type == 3) { type = 0; --bp1; }
    }
}

// ---- dequantisation --------------------------------------------------------------------------------------------------------
// the sub-band (index into half_step) of sample (x, y) of a w x h plane with `levels` decompositions
BQK_HD int band_of(int x, int y, int w, int h, int levels) {
    for (int r = levels; r >= 1; --r) {
        const int rw = ceil_shift(w, levels - r), rh = ceil_shift(h, levels - r);
        const int lw = (rw + 1) >> 1, lh = (rh + 1) >> 1;
        const int o = (x >= lw ? 1 : 0) + (y >= lh ? 2 : 0);
        if (o) return 3 * (r - 1) + o;
    }
    return 0;
}

// tier 1's value -> the transform's input, as the 32 bits the planes hold (int32 reversible, float irreversible)
BQK_HD int32_t dequant_sample(int32_t v, const Seg& s, int x, int y) {
    if (s.reversible) return v / 2;
    const float f = (float)v * s.half_step[band_of(x, y, s.w, s.h, s.levels)];
    int32_t bits;
    memcpy(&bits, &f, 4);
    return bits;
}

// ---- the inverse transforms, one line of one level -------------------------------------------------------------------------
// src: sn low-pass samples, then n - sn high-pass samples (sn = ceil(n / 2)); dst: the n synthesised samples
BQK_HD void synth53_1d(const int32_t* src, int sstride, int32_t* dst, int dstride, int n) {
    const int sn = (n + 1) >> 1;
    for (int i = 0; i < n; ++i) dst[(size_t)i * dstride] = src[(size_t)((i & 1) ? sn + (i >> 1) : (i >> 1)) * sstride];
    if (n == 1) return;
#define X(i) dst[(size_t)(i) * dstride]
    // (sums wrap modulo 2^32: a damaged stream's coefficients may be anything, a valid one's never come near the limit)
    for (int i = 0; i < n; i += 2) {
        const uint32_t l = (uint32_t)X(i > 0 ? i - 1 : 1), r = (uint32_t)X(i + 1 < n ? i + 1 : i - 1);
        X(i) = (int32_t)((uint32_t)X(i) - (uint32_t)((int32_t)(l + r + 2u) >> 2));
    }
    for (int i = 1; i < n; i += 2) {
        const uint32_t l = (uint32_t)X(i - 1), r = (uint32_t)X(i + 1 < n ? i + 1 : i - 1);
        X(i) = (int32_t)((uint32_t)X(i) + (uint32_t)((int32_t)(l + r) >> 1));
    }
#undef X
}

BQK_HD void lift97(float* dst, int dstride, int n, int first, float c) {
    for (int i = first; i < n; i += 2) {
        const float l = dst[(size_t)(i > 0 ? i - 1 : 1) * dstride], r = dst[(size_t)(i + 1 < n ? i + 1 : i - 1) * dstride];
        const float t = (l + r) * c;
        dst[(size_t)i * dstride] = dst[(size_t)i * dstride] + t;
    }
}

BQK_HD void synth97_1d(const float* src, int sstride, float* dst, int dstride, int n) {
    const int sn = (n + 1) >> 1;
    if (n == 1) { dst[0] = src[0]; return; }
    // the high-pass gain of 2 sits in the scaling (2 / K), not in the step sizes: OpenJPEG's convention
    for (int i = 0; i < n; ++i) {
        const float v = src[(size_t)((i & 1) ? sn + (i >> 1) : (i >> 1)) * sstride];
        dst[(size_t)i * dstride] = v * ((i & 1) ? 1.625732422f : 1.230174105f);
    }
    lift97(dst, dstride, n, 0, -0.443506852f);
    lift97(dst, dstride, n, 1, -0.882911075f);
    lift97(dst, dstride, n, 0, 0.052980118f);
    lift97(dst, dstride, n, 1, 1.586134342f);
}

// line `i` of the row pass (a -> b) or column pass (b -> a) of the level that makes resolution rw x rh; stride = plane width
BQK_HD void synth_row(const int32_t* a, int32_t* b, int stride, int rw, int y, int reversible) {
    if (reversible) synth53_1d(a + (size_t)y * stride, 1, b + (size_t)y * stride, 1, rw);
    else synth97_1d((const float*)a + (size_t)y * stride, 1, (float*)b + (size_t)y * stride, 1, rw);
}
BQK_HD void synth_col(const int32_t* b, int32_t* a, int stride, int rh, int x, int reversible) {
    if (reversible) synth53_1d(b + x, stride, a + x, stride, rh);
    else synth97_1d((const float*)b + x, stride, (float*)a + x, stride, rh);
}

// ---- the pixel -------------------------------------------------------------------------------------------------------------
BQK_HD int32_t round_shift_clamp(float v) {
    if (!(v > -1e9f)) return 0;
    if (v > 1e9f) return 255;
    const int32_t i = (int32_t)rintf(v) + 128;
    return i < 0 ? 0 : i > 255 ? 255 : i;
}

// the three samples of one pixel after the transforms (their 32 bits) -> the canvas's bytes
BQK_HD void finish_pixel(int32_t c0, int32_t c1, int32_t c2, const Seg& s, int ycc, uint8_t* rgb) {
    int32_t v[3];
    if (s.reversible) {
        if (s.mct) {
            const uint32_t g = (uint32_t)c0 - (uint32_t)((int32_t)((uint32_t)c1 + (uint32_t)c2) >> 2);      // (wrapping, as synth53_1d)
            v[0] = (int32_t)((uint32_t)c2 + g); v[1] = (int32_t)g; v[2] = (int32_t)((uint32_t)c1 + g);
        } else { v[0] = c0; v[1] = c1; v[2] = c2; }
        for (int k = 0; k < 3; ++k) { const int64_t t = (int64_t)v[k] + 128; v[k] = (int32_t)(t < 0 ? 0 : t > 255 ? 255 : t); }
    } else {
        float y, u, w;
        memcpy(&y, &c0, 4); memcpy(&u, &c1, 4); memcpy(&w, &c2, 4);
        if (s.mct) {
            const float r = y + w * 1.402f;
            const float g = y - u * 0.34413f - w * 0.71414f;
            const float b = y + u * 1.772f;
            y = r; u = g; w = b;
        }
        v[0] = round_shift_clamp(y); v[1] = round_shift_clamp(u); v[2] = round_shift_clamp(w);
    }
    if (ycc) bqycc::ycc_to_rgb(v[0], v[1], v[2], rgb);
    else { rgb[0] = (uint8_t)v[0]; rgb[1] = (uint8_t)v[1]; rgb[2] = (uint8_t)v[2]; }
}

// ---- which pixels of a segment a canvas shows: canvas_place.h ---------------------------------------------------------------
using bqcanvas::Window;
using bqcanvas::place_window;

}  // namespace bqj2k
