// augment_device.h -- the training augmentation 'xyrjb', stated once for the host and the device.  One header, two users: the
// kernels of kernels_augment.hip (bq_augment) and the host entry bqio_augment (augment_host.cpp: the very same routines on the
// CPU, for the tests and as the timing baseline).
//
// A tile t (uint8 [px][px][3], 8 <= px <= 4096) and four parameter bytes (k, flips, quality, blur) give
//
//     out = blur_s( flip_ud^(flips >> 1 & 1)( flip_lr^(flips & 1)( rot90^k( jpeg_q(t) ))))
//
//   jpeg_q   quality 0: t itself.  1..100: the pixels Pillow returns for Image.open(save(t, 'JPEG', quality=q, subsampling=
//            '4:2:0')).  Entropy coding is lossless, so no bitstream is made: bqje::block_coefs (colour, edges, 4:2:0, fDCT,
//            quantisation: the encoder's coefficients), times the quantiser, bqjd::idct_block, and bqjd::pixel_rgb (fancy
//            upsampling, colour) over the samples in the decoder's plane layout.  Both halves are held to Pillow's bytes by their
//            own tests; tests/test_augment.py holds the round trip to Pillow's pixels.  The dummy blocks of an MCU beyond the
//            luma plane are never read by the colour stage and are not computed.  A block that idct_block reports out of range,
//            or a dequantised coefficient beyond 15 bits (what the decoder refuses a tile for), sets ST_RANGE in the tile's
//            status and keeps the clamped samples.
//   rot90^k  numpy.rot90(x, k): counter-clockwise quarter turns, k = 0..3; the flips are x[:, ::-1] (bit 0) and x[::-1] (bit 1).
//   blur_s   blur 0: identity.  1..4: sigma = 0.5 blur, a separable Gaussian in integers: radius r = int(3 sigma + 0.5) (2, 3, 5,
//            6), weights w_i = floor(65536 g_i / sum(g) + 0.5) with the centre tap adjusted so that they sum to exactly 65536,
//            mirror padding that does not repeat the edge sample; along a row h = (sum(w p) + 128) >> 8 (uint16, 8 fractional
//            bits, <= 65280), then down a column (sum(w h) + (1 << 23)) >> 24 (the sum stays below 2^32).  Within one level of
//            the rounded float64 filter (scipy.ndimage.gaussian_filter, mode='mirror', truncate=3).
//
// The four weight tables and the Annex K base quantisers are built on the host (build_blur_tables, quant_base) and reach the
// kernels as arguments; a tile's quantisers follow from its quality by quant_entry, the formula of bqje::build_tables.
#pragma once
#include "jpeg_device.h"
#include "jpeg_encode_device.h"

#include <math.h>

#if defined(__HIPCC__)
#define BQA_HD __host__ __device__ inline
#else
#define BQA_HD inline
#endif

namespace bqaug {

enum { ST_OK = 0,
       ST_RANGE = 1,     // status bit 1: a block of the JPEG round trip left the range libjpeg's builds agree in; samples clamped
       ST_PARAM = 2 };   // (device only) a parameter byte out of range: the tile came out as with all-zero parameters

constexpr int MIN_PX = 8, MAX_PX = 4096;
constexpr int MAX_BLUR = 4;              // blur index 1..4: sigma 0.5, 1, 1.5, 2
constexpr int MAX_TAPS = 13;             // 2 r + 1 at r = 6

struct Params { int k, flips, quality, blur; };

BQA_HD bool valid_px(int px) { return px >= MIN_PX && px <= MAX_PX; }
BQA_HD bool valid_params(const uint8_t* p) { return p[0] <= 3 && p[1] <= 3 && p[2] <= 100 && p[3] <= MAX_BLUR; }
// the row's parameters; all zero (the identity) for a row out of range
BQA_HD Params params_of(const uint8_t* p) {
    if (!valid_params(p)) return Params{0, 0, 0, 0};
    return Params{p[0], p[1], p[2], p[3]};
}

BQA_HD size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
// scratch of one tile: the decoder's planes (128 bytes a block, samples in the first 64) and the row pass of the blur
BQA_HD size_t plane_bytes(int px) { return bqjd::tile_coef_bytes(px); }
BQA_HD size_t row_bytes(int px) { return align16((size_t)px * px * 3 * 2); }
BQA_HD size_t tile_scratch_bytes(int px) { return plane_bytes(px) + row_bytes(px); }

// ---- tables ---------------------------------------------------------------------------------------------------------------
struct BlurTables {
    uint16_t w[MAX_BLUR][MAX_TAPS + 1];  // [blur - 1][d + r], d = -r .. r
    int32_t r[MAX_BLUR];
};

inline void build_blur_tables(BlurTables& B) {
    for (int b = 1; b <= MAX_BLUR; ++b) {
        const double sigma = 0.5 * b;
        const int r = (int)(3.0 * sigma + 0.5);
        double g[MAX_TAPS], sum = 0.0;
        for (int d = -r; d <= r; ++d) sum += g[d + r] = exp(-0.5 * (double)(d * d) / (sigma * sigma));
        int32_t w[MAX_TAPS], total = 0;
        for (int i = 0; i <= 2 * r; ++i) total += w[i] = (int32_t)floor(65536.0 * g[i] / sum + 0.5);
        w[r] += 65536 - total;
        for (int i = 0; i <= MAX_TAPS; ++i) B.w[b - 1][i] = i <= 2 * r ? (uint16_t)w[i] : 0;
        B.r[b - 1] = r;
    }
}

struct QuantBase { uint8_t b[2][64]; };  // ITU-T T.81 Annex K, zigzag order: [0] luma, [1] chroma

inline QuantBase quant_base() {
    QuantBase Q;
    for (int k = 0; k < 64; ++k) { Q.b[0][k] = bqje::K_LUMA_Q[bqje::zigzag(k)]; Q.b[1][k] = bqje::K_CHROMA_Q[bqje::zigzag(k)]; }
    return Q;
}

// the quantiser of a base entry at `quality` (1..100): bqje::build_tables' values
BQA_HD uint16_t quant_entry(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * scale + 50) / 100;
    return (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
}

// ---- jpeg_q ---------------------------------------------------------------------------------------------------------------
BQA_HD bqje::Geom encode_geom(int px) { return bqje::geom_of(px, bqje::SUB_420); }
BQA_HD bqjd::Geom decode_geom(int px) {
    bqjd::Geom G;
    bqjd::geom_of(2u | (2u << 8) | (3u << 16), px, G);
    return G;
}

// Block P (not a dummy) of the round trip: the tile's pixels -> the block's 64 samples at its place in `planes`.  q: the
// component's quantisers, zigzag order.  false: out of range (ST_RANGE).
BQA_HD bool jpeg_block(const uint8_t* tile, const bqje::Geom& Ge, const bqjd::Geom& Gd, const bqje::BlockPos& P, const uint16_t* q,
                       uint8_t* planes) {
    int16_t zz[64], cf[64];
    bqje::block_coefs(tile, Ge, P, q, zz);
    bool ok = true;
    BQE_UNROLL
    for (int k = 0; k < 64; ++k) {
        int32_t dq = (int32_t)zz[k] * (int32_t)q[k];
        if (dq < -16384) { dq = -16384; ok = false; }
        if (dq > 16383) { dq = 16383; ok = false; }
        cf[bqje::zigzag(k)] = (int16_t)dq;
    }
    uint8_t s[64];
    ok &= bqjd::idct_block(cf, s);
    uint8_t* dst = planes + ((size_t)Gd.base[P.comp] + (size_t)(P.by * Gd.bw[P.comp] + P.bx)) * 128;
#if defined(__HIP_DEVICE_COMPILE__)
    uint4* d4 = reinterpret_cast<uint4*>(dst);                     // (planes is 16-byte aligned, a block 128 bytes)
    BQE_UNROLL
    for (int j = 0; j < 4; ++j) {
        uint32_t w[4];
        BQE_UNROLL
        for (int i = 0; i < 4; ++i) {
            const uint8_t* b = s + 16 * j + 4 * i;
            w[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        d4[j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
#else
    memcpy(dst, s, 64);
#endif
    return ok;
}

// ---- rot90, flips -----------------------------------------------------------------------------------------------------------
// The pixel (sy, sx) of jpeg_q(t) that output pixel (y, x) shows: the inverse of flip_ud . flip_lr . rot90^k.
BQA_HD void source_of(int px, const Params& a, int y, int x, int& sy, int& sx) {
    const int last = px - 1;
    if (a.flips & 2) y = last - y;
    if (a.flips & 1) x = last - x;
    switch (a.k) {
        case 1: sy = x; sx = last - y; break;                      // rot90(J)[i][j] = J[j][n - 1 - i]
        case 2: sy = last - y; sx = last - x; break;
        case 3: sy = last - x; sx = y; break;
        default: sy = y; sx = x; break;
    }
}

// Output pixel (y, x) before the blur.  planes: the tile's samples after jpeg_block (read for quality > 0 only).
BQA_HD void placed_pixel(const uint8_t* tile, const uint8_t* planes, const bqjd::Geom& Gd, int px, const Params& a, int y, int x,
                         uint8_t* rgb) {
    int sy, sx;
    source_of(px, a, y, x, sy, sx);
    if (a.quality) {
        bqjd::pixel_rgb(planes, Gd, sy, sx, rgb);
    } else {
        const uint8_t* s = tile + ((size_t)sy * px + sx) * 3;
        rgb[0] = s[0]; rgb[1] = s[1]; rgb[2] = s[2];
    }
}

// ---- blur_s ---------------------------------------------------------------------------------------------------------------
BQA_HD int mirror(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }      // |offset| <= 6 < MIN_PX: one fold

// the row pass at (y, x): img uint8 [px][px][3] -> three uint16 with 8 fractional bits
BQA_HD void blur_row_at(const uint8_t* img, int px, int y, int x, const uint16_t* w, int r, uint16_t* out) {
    uint32_t a0 = 128, a1 = 128, a2 = 128;
    const uint8_t* row = img + (size_t)y * px * 3;
    for (int d = -r; d <= r; ++d) {
        const uint8_t* s = row + 3 * mirror(x + d, px);
        const uint32_t wd = w[d + r];
        a0 += wd * s[0]; a1 += wd * s[1]; a2 += wd * s[2];
    }
    out[0] = (uint16_t)(a0 >> 8); out[1] = (uint16_t)(a1 >> 8); out[2] = (uint16_t)(a2 >> 8);
}

// the column pass at (y, x): h uint16 [px][px][3] (blur_row_at's) -> three bytes.  65536 * 65280 + 2^23 < 2^32.
BQA_HD void blur_col_at(const uint16_t* h, int px, int y, int x, const uint16_t* w, int r, uint8_t* out) {
    uint32_t a0 = 1u << 23, a1 = 1u << 23, a2 = 1u << 23;
    for (int d = -r; d <= r; ++d) {
        const uint16_t* s = h + ((size_t)mirror(y + d, px) * px + x) * 3;
        const uint32_t wd = w[d + r];
        a0 += wd * s[0]; a1 += wd * s[1]; a2 += wd * s[2];
    }
    out[0] = (uint8_t)(a0 >> 24); out[1] = (uint8_t)(a1 >> 24); out[2] = (uint8_t)(a2 >> 24);
}

}  // namespace bqaug
