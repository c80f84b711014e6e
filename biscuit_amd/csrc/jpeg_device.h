// jpeg_device.h -- the baseline-JPEG decoder of jpeg_baseline.h in the form the GPU runs: the entropy decoder and the pixel
// stage as plain __host__ __device__ routines over flat buffers.  One header, three users: the kernels of kernels_jpeg.hip,
// the host entry bqio_jpeg_decode_extracted (tfrecord_reader.cpp: the very same routines on the CPU, for the tests and the
// fuzzer -- every input can be shown in bounds and terminating before a GPU sees it) and tools/fuzz/jpeg_extract_fuzz.cpp.
//
// Input is what bqio_extract_jpeg leaves: per tile a descriptor (Desc), the entropy-coded segment with the stuffed zeros
// removed and ECS_PAD zero bytes behind it, and a table set (TableSet: Huffman tables in the lookup form of jpeg_baseline.h,
// quantisers in natural order).  The arithmetic is that header's, restated without SIMD and without containers: the IJG
// "islow" IDCT, h2v1 / h2v2 triangle upsampling with alternating rounding and edge replication, BT.601 in 16-bit fixed point.
// tests/test_jpeg_extract.py holds it to Pillow byte for byte.
//
// The entropy decoder is total: on any byte string it terminates after a number of steps the tile size fixes (every MCU of
// the tile, at most 64 symbols a block, at most 7 steps for a long code), reads only [scan, scan + len + ECS_PAD), writes
// only inside the tile's coefficient blocks, and answers with a status instead of guessing.
//
// A tile need not be square: a TIFF page's JPEG segments are w x h (bqio_extract_jpeg_segments, bq_jpeg_decode_canvas), and the
// argument holds for them as stated, with the numbers geom_of(g, w, h) fixes.  Steps: mcux * mcuy MCUs with mcux = ceil(w / 8 hmax)
// and mcuy = ceil(h / 8 vmax), hmax * vmax + 2 blocks each.  Writes: a luma block's index is below bw[0] * bh[0] = (mcux hmax)
// (mcuy vmax) and a chroma block's below base[c] + mcux * mcuy; with hmax, vmax <= 2 every plane has at most 2 ceil(w / 16) x
// 2 ceil(h / 16) blocks (ceil(w / 8) <= 2 ceil(w / 16)), so the three planes end inside tile_blocks(w, h) whatever the
// sampling.  Reads do not depend on the geometry.  The pixel stage reads samples (y, x) with y < h <= 8 bh[c] and x < w <=
// 8 bw[c] only (chroma: y < ch, x < cw), which lie in the same planes.
//
// Which pixels of a segment a canvas shows is canvas_place.h's statement (place_window), brought into this namespace below.
#pragma once
#include <stdint.h>
#include <string.h>

#include "canvas_place.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQJ_HD __host__ __device__ inline
#else
#define BQJ_HD inline
#endif
#if defined(__clang__)
#define BQJ_UNROLL _Pragma("unroll")
#else
#define BQJ_UNROLL
#endif

namespace bqjd {

// status of one tile: 0 = decoded; otherwise the OR of what refused it
enum { ST_OK = 0,
       ST_CODE = 1,      // a Huffman code that does not exist
       ST_RUN = 2,       // a zero run past coefficient 63
       ST_END = 4,       // bits used from beyond the segment's end
       ST_RANGE = 8,     // outside the range in which libjpeg's builds agree: a product beyond 15 bits, an intermediate
                         // beyond 15 bits, a sample beyond -512..511
       ST_DESC = 16 };   // a descriptor this decoder does not take (sampling, component count, table set index)

constexpr int LOOK = 9, FAST = 11;       // as jpeg_baseline.h
// Readable zero bytes behind every segment.  The bit reader loads 4 aligned bytes when it holds 32 bits or fewer, so it is
// at most 8 bytes ahead of the bits it has used; a block starts only while the bits used lie inside the segment and uses
// at most 64 symbols of at most 16 + 15 bits = 248 bytes: 8 + 248 + 4 <= 320 with room to spare.
constexpr uint32_t ECS_PAD = 320;
constexpr uint32_t ECS_ALIGN = 16;       // every segment starts at a multiple of this

struct Desc {
    uint32_t off, len;                   // the segment inside the scan buffer (off a multiple of ECS_ALIGN), without the pad
    uint32_t geom;                       // hmax | vmax << 8 | components << 16
    uint32_t tset;                       // index of the table set
};

struct HuffD {
    uint16_t look[1 << LOOK];            // (length << 8) | symbol, 0 = longer than LOOK bits
    int32_t maxcode[18];
    int32_t valoff[17];
    uint8_t vals[256];
};

// The tables of one tile, by component (0 = Y, 1 = Cb, 2 = Cr): what the frame and scan headers select, resolved.
struct TableSet {
    int16_t fast[3][1 << FAST];          // AC: (value << 8) | (run << 4) | bits used, 0 = take the long way
    HuffD dc[3], ac[3];
    uint16_t q[3][64];                   // natural order
    uint8_t zigzag[64];
};
static_assert(sizeof(TableSet) % 8 == 0, "table sets are copied by words");

struct Geom {
    int hmax, vmax, mcux, mcuy;
    int bw[3], bh[3];                    // blocks per plane row / column (whole MCUs)
    uint32_t base[3];                    // first block of the plane inside the tile's coefficient space
    int cw, ch;                          // chroma samples that exist: ceil(w / hmax), ceil(h / vmax)
};

// Blocks of coefficient space per w x h tile, whatever its sampling (4:2:0 rounds the luma plane up to whole 16 x 16 MCUs).
BQJ_HD uint32_t tile_blocks(int w, int h) {
    return 3u * (2u * (uint32_t)((w + 15) / 16)) * (2u * (uint32_t)((h + 15) / 16));
}
BQJ_HD uint32_t tile_blocks(int px) { return tile_blocks(px, px); }
BQJ_HD size_t tile_coef_bytes(int w, int h) { return (size_t)tile_blocks(w, h) * 128; }
BQJ_HD size_t tile_coef_bytes(int px) { return tile_coef_bytes(px, px); }

// false: not 3 components at 4:4:4 / 4:2:2 / 4:2:0
BQJ_HD bool geom_of(uint32_t g, int w, int h, Geom& G) {
    const int hmax = (int)(g & 255), vmax = (int)((g >> 8) & 255), ncomp = (int)((g >> 16) & 255);
    if (ncomp != 3 || hmax < 1 || hmax > 2 || vmax < 1 || vmax > 2 || (hmax == 1 && vmax == 2) || w <= 0 || h <= 0) return false;
    G.hmax = hmax; G.vmax = vmax;
    G.mcux = (w + 8 * hmax - 1) / (8 * hmax); G.mcuy = (h + 8 * vmax - 1) / (8 * vmax);
    G.bw[0] = G.mcux * hmax; G.bh[0] = G.mcuy * vmax;
    G.bw[1] = G.bw[2] = G.mcux; G.bh[1] = G.bh[2] = G.mcuy;
    G.base[0] = 0;
    G.base[1] = (uint32_t)(G.bw[0] * G.bh[0]);
    G.base[2] = G.base[1] + (uint32_t)(G.mcux * G.mcuy);
    G.cw = (w + hmax - 1) / hmax; G.ch = (h + vmax - 1) / vmax;
    return true;
}
BQJ_HD bool geom_of(uint32_t g, int px, Geom& G) { return geom_of(g, px, px, G); }

// ---- entropy decoder ----------------------------------------------------------------------------------------------------
struct BitsD {
    const uint8_t* base;
    uint64_t acc;
    int have;
    uint32_t words;                      // 4-byte words loaded so far
    int64_t nbits;
    BQJ_HD void open(const uint8_t* p, uint32_t n) { base = p; acc = 0; have = 0; words = 0; nbits = (int64_t)n * 8; }
    BQJ_HD void fill() {                 // to 33..64 bits
        if (have <= 32) {
            uint32_t v;
#if defined(__HIP_DEVICE_COMPILE__)
            v = reinterpret_cast<const uint32_t*>(base)[words];
#else
            memcpy(&v, base + 4 * (size_t)words, 4);
#endif
            ++words;
            acc |= (uint64_t)__builtin_bswap32(v) << (32 - have);
            have += 32;
        }
    }
    BQJ_HD uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }       // 1 <= n <= 32
    BQJ_HD void drop(int n) { acc <<= n; have -= n; }
    BQJ_HD bool inside() const { return (int64_t)words * 32 - have <= nbits; }      // no bit from beyond the end used so far
};

BQJ_HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

BQJ_HD int decode_symbol(BitsD& B, const HuffD& H) {
    const uint32_t e = H.look[B.peek(LOOK)];
    if (e) { B.drop((int)(e >> 8)); return (int)(e & 0xFF); }
    int l = LOOK + 1;
    int32_t code = (int32_t)B.peek(l);
    while (code > H.maxcode[l]) { ++l; if (l > 16) return -1; code = (int32_t)B.peek(l); }
    B.drop(l);
    return H.vals[(code + H.valoff[l]) & 0xFF];
}

// One block: Huffman-decode and dequantise into cf[64] (natural order, zero beforehand).  0 or the status that refuses it.
BQJ_HD int entropy_block(BitsD& B, const TableSet* T, int c, int& pred, int16_t* cf) {
    if (!B.inside()) return ST_END;      // the stream ended before this block: refuse before reading further
    B.fill();
    int s = decode_symbol(B, T->dc[c]);
    if (s < 0) return ST_CODE;
    s &= 15;                             // (a DC table holds no larger value; the mask keeps that true of any table bytes)
    if (s) { const int r = (int)B.peek(s); B.drop(s); pred += extend(r, s); }
    const uint16_t* q = T->q[c];
    bool wide = false;                   // some product outside 15 bits
    int32_t dq = pred * (int32_t)q[0];
    if ((dq + 16384) & ~0x7FFF) wide = true; else cf[0] = (int16_t)dq;
    for (int k = 1; k < 64;) {
        B.fill();
        const int f = T->fast[c][B.peek(FAST)];
        int v;
        if (f) {
            B.drop(f & 15);
            v = f >> 8;
            k += (f >> 4) & 15;
            if (v == 0) {                // no value: sixteen zeros (k advanced by 15 already) or the end of the block
                if ((f & 0xF0) == 0) break;
                ++k;
                continue;
            }
        } else {
            const int rs = decode_symbol(B, T->ac[c]);
            if (rs < 0) return ST_CODE;
            s = rs & 15;
            if (s == 0) {
                if ((rs >> 4) != 15) break;
                k += 16;
                continue;
            }
            k += rs >> 4;
            v = extend((int)B.peek(s), s);
            B.drop(s);
        }
        if (k > 63) return ST_RUN;
        const int nat = T->zigzag[k];
        dq = v * (int32_t)q[nat];
        if ((dq + 16384) & ~0x7FFF) wide = true; else cf[nat] = (int16_t)dq;
        ++k;
    }
    return wide ? ST_RANGE : ST_OK;
}

// All blocks of one tile, MCU by MCU.  coef: the tile's coefficient space (tile_blocks(px) * 64 int16, zero).
BQJ_HD int entropy_tile(const uint8_t* scan, uint32_t len, const Geom& G, const TableSet* T, int16_t* coef) {
    BitsD B;
    B.open(scan, len);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (int my = 0; my < G.mcuy; ++my)
        for (int mx = 0; mx < G.mcux; ++mx) {
            for (int by = 0; by < G.vmax; ++by)
                for (int bx = 0; bx < G.hmax; ++bx) {
                    const uint32_t blk = G.base[0] + (uint32_t)((my * G.vmax + by) * G.bw[0] + mx * G.hmax + bx);
                    const int e = entropy_block(B, T, 0, pred0, coef + (size_t)blk * 64);
                    if (e) return e;
                }
            const uint32_t cb = (uint32_t)(my * G.mcux + mx);
            int e = entropy_block(B, T, 1, pred1, coef + (size_t)(G.base[1] + cb) * 64);
            if (e) return e;
            e = entropy_block(B, T, 2, pred2, coef + (size_t)(G.base[2] + cb) * 64);
            if (e) return e;
        }
    return B.inside() ? ST_OK : ST_END;
}

// ---- inverse DCT (IJG jidctint "islow") ---------------------------------------------------------------------------------
constexpr int CB = 13, P1 = 2;
constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633,
                  F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

BQJ_HD uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// One 1-D transform: in[k] = frequency k, out[k] = sample k, descaled by SHIFT.
template <int SHIFT>
BQJ_HD void idct8(const int32_t* in, int32_t* out) {
    int32_t z2 = in[2], z3 = in[6];
    int32_t z1 = (z2 + z3) * F_0_541;
    int32_t t2 = z1 - z3 * F_1_847, t3 = z1 + z2 * F_0_765;
    z2 = in[0]; z3 = in[4];
    int32_t t0 = (z2 + z3) * (1 << CB), t1 = (z2 - z3) * (1 << CB);
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = in[7]; t1 = in[5]; t2 = in[3]; t3 = in[1];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    int32_t z4 = t1 + t3;
    const int32_t z5 = (z3 + z4) * F_1_175;
    t0 *= F_0_298; t1 *= F_2_053; t2 *= F_3_072; t3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr int32_t R = 1 << (SHIFT - 1);
    out[0] = (t10 + t3 + R) >> SHIFT; out[7] = (t10 - t3 + R) >> SHIFT;
    out[1] = (t11 + t2 + R) >> SHIFT; out[6] = (t11 - t2 + R) >> SHIFT;
    out[2] = (t12 + t1 + R) >> SHIFT; out[5] = (t12 - t1 + R) >> SHIFT;
    out[3] = (t13 + t0 + R) >> SHIFT; out[4] = (t13 - t0 + R) >> SHIFT;
}

// cf: 64 dequantised coefficients (natural order, each within 15 bits); out: the block's 64 samples, row by row.  false: the
// block leaves the range an 8-bit image's blocks stay in (idct_islow of jpeg_baseline.h refuses the same blocks).  A value
// beyond 15 bits between the passes is held at the limit, as the 16-bit SIMD builds hold it, so that the second pass stays
// inside 32 bits whatever the input; the samples are then written all the same and the caller drops the tile.
BQJ_HD bool idct_block(const int16_t* cf, uint8_t* out) {
    int any = 0;
BQJ_UNROLL
    for (int i = 1; i < 64; ++i) any |= cf[i];
    if (!any) {                          // DC only: both passes reduce to one descale
        const int dc = cf[0];
        const uint8_t v = clamp8(((dc * 4 + 16) >> 5) + 128);
BQJ_UNROLL
        for (int i = 0; i < 64; ++i) out[i] = v;
        return dc >= -4096 && dc < 4096;
    }
    int32_t ws[8][8];
    bool ok = true;
BQJ_UNROLL
    for (int c = 0; c < 8; ++c) {        // down the columns
        int32_t in[8], o[8];
BQJ_UNROLL
        for (int k = 0; k < 8; ++k) in[k] = cf[k * 8 + c];
        idct8<CB - P1>(in, o);
BQJ_UNROLL
        for (int k = 0; k < 8; ++k) {
            int32_t v = o[k];
            if (v < -(1 << 14)) { v = -(1 << 14); ok = false; }
            if (v > (1 << 14) - 1) { v = (1 << 14) - 1; ok = false; }
            ws[k][c] = v;
        }
    }
BQJ_UNROLL
    for (int r = 0; r < 8; ++r) {        // along the rows
        int32_t o[8];
        idct8<CB + P1 + 3>(ws[r], o);
BQJ_UNROLL
        for (int k = 0; k < 8; ++k) {
            ok &= o[k] >= -512 && o[k] < 512;
            out[r * 8 + k] = clamp8(o[k] + 128);
        }
    }
    return ok;
}

// The tile's blocks in place: every 128-byte coefficient block becomes its 64 samples (in its first 64 bytes).
BQJ_HD bool idct_in_place(int16_t* blk) {
    int16_t cf[64];
    uint8_t px[64];
BQJ_UNROLL
    for (int i = 0; i < 64; ++i) cf[i] = blk[i];
    const bool ok = idct_block(cf, px);
    uint8_t* o = reinterpret_cast<uint8_t*>(blk);
BQJ_UNROLL
    for (int i = 0; i < 64; ++i) o[i] = px[i];
    return ok;
}

// ---- upsampling and colour ----------------------------------------------------------------------------------------------
// sample (y, x) of plane c after idct_in_place
BQJ_HD int samp(const uint8_t* tile, const Geom& G, int c, int y, int x) {
    return tile[((size_t)G.base[c] + (size_t)((y >> 3) * G.bw[c] + (x >> 3))) * 128 + (size_t)((y & 7) * 8 + (x & 7))];
}

// Chroma plane c at output pixel (y, x): the triangle filter of jpeg_baseline.h, one output at a time.  The missing neighbour
// at an edge is the sample itself; h2v2 weighs the rows first (3 near + far) and rounds once.
BQJ_HD int chroma_at(const uint8_t* tile, const Geom& G, int c, int y, int x) {
    if (G.hmax == 1) return samp(tile, G, c, y, x);
    const int i = x >> 1;
    const int j = (x & 1) ? (i + 1 < G.cw ? i + 1 : i) : (i > 0 ? i - 1 : i);
    if (G.vmax == 1) {
        const int w = samp(tile, G, c, y, i), n = samp(tile, G, c, y, j);
        return (3 * w + n + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int nr = y >> 1;
    int fr = (y & 1) ? nr + 1 : nr - 1;
    fr = fr < 0 ? 0 : fr > G.ch - 1 ? G.ch - 1 : fr;
    const int w = 3 * samp(tile, G, c, nr, i) + samp(tile, G, c, fr, i);
    const int n = 3 * samp(tile, G, c, nr, j) + samp(tile, G, c, fr, j);
    return (3 * w + n + ((x & 1) ? 7 : 8)) >> 4;
}

// YCbCr (BT.601, full range) -> RGB in 16-bit fixed point: R and B rounded per term, G once for the sum.
BQJ_HD void pixel_rgb(const uint8_t* tile, const Geom& G, int y, int x, uint8_t* rgb) {
    const int Y = samp(tile, G, 0, y, x);
    const int cb = chroma_at(tile, G, 1, y, x) - 128, cr = chroma_at(tile, G, 2, y, x) - 128;
    rgb[0] = clamp8(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ---- a segment's place in a canvas: canvas_place.h states which of its pixels the canvas shows -----------------------------
using bqcanvas::Window;
using bqcanvas::place_window;

// The window of one decoded segment (planes: its blocks after idct_in_place) written into the canvas, pixel by pixel: the host's
// form of the colour-and-place stage (the kernel of kernels_jpeg.hip writes the same pixels four at a time).
BQJ_HD void place_segment(const uint8_t* planes, const Geom& G, const Window& w, int px, int py, uint8_t* canvas, int W) {
    for (int y = w.y0; y < w.y1; ++y) {
        uint8_t* row = canvas + ((size_t)(py + y) * (size_t)W + (size_t)(px + w.x0)) * 3;
        for (int x = w.x0; x < w.x1; ++x) pixel_rgb(planes, G, y, x, row + 3 * (size_t)(x - w.x0));
    }
}

}  // namespace bqjd
