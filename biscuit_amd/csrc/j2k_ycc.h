// j2k_ycc.h -- full-range YCbCr -> RGB with the bytes of Pillow's Image.merge('YCbCr', ...).convert('RGB'), stated once for
// the slide reader's host path (bqio_ycc_to_rgb, libbiscuit_io) and the device's j2k_store kernel.  Pillow adds table values
// in 1/64 units: table(k)[c] = (int)(k * 64 * (c - 128) + 0.5), the cast truncating toward zero, for k = 1.402, -0.34414,
// -0.71414 and 1.772; R = Y + (tR[Cr] >> 6), G = Y + ((tGb[Cb] + tGr[Cr]) >> 6), B = Y + (tB[Cb] >> 6), shifts arithmetic,
// results clamped to 0..255.  The tables are restated in integers (k * 64 as a fraction over 100 000); no product reaches
// 2^31.  tests/test_j2k.py compares all 2^24 triples with Pillow.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQY_HD __host__ __device__ inline
#else
#define BQY_HD inline
#endif

namespace bqycc {

// (int)(num / 100000 * d + 0.5) with C's truncation, d in -128..127
BQY_HD int32_t term(int32_t num, int32_t d) { return (num * d + 50000) / 100000; }

BQY_HD uint8_t clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

BQY_HD void ycc_to_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t* rgb) {
    const int32_t u = cb - 128, v = cr - 128;
    rgb[0] = clamp8(y + (term(8972800, v) >> 6));
    rgb[1] = clamp8(y + ((term(-2202496, u) + term(-4570496, v)) >> 6));
    rgb[2] = clamp8(y + (term(11340800, u) >> 6));
}

}  // namespace bqycc
