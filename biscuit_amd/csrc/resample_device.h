// Tile resampling as Pillow's 8-bit resampler does it (Image.resize((px, px), Image.LANCZOS) of an RGB image), stated once
// for the host and the device: the routines below are compiled into libbiscuit_io.so (resample_host.cpp: bqio_resample_taps,
// bqio_tile_resample -- the CPU restatement the tests and the sanitizer build run) and into kernels_resample.hip
// (bq_tile_resample), in the pattern of jpeg_device.h.
//
// The arithmetic (Pillow's src/libImaging/Resample.c, 8 bits per channel): per output coordinate a window [first, first +
// count) of source coordinates and `count` taps of 22 fractional bits, built on the host in float64 (resample_host.cpp);
// a pass is  clip8((2^21 + sum tap * byte) >> 22);  the horizontal pass runs first and is rounded to a byte, the vertical
// pass runs over those bytes.  Everything here is integer arithmetic; accumulators fit 32 bits (the host checks
// 255 * sum |tap| + 2^21 < 2^31 when it builds the taps).
//
// The source of a tile is a src_px x src_px window of a canvas uint8 [H][W][3] at (ox, oy); whatever of the window lies outside
// the canvas reads as 255 (the white a slide reader pads with).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQR_HD __host__ __device__ inline
#else
#define BQR_HD inline
#endif

namespace bqrs {

constexpr int PRECISION_BITS = 32 - 8 - 2;       // Pillow's
constexpr int SUPPORT = 3;                       // LANCZOS
constexpr int MAX_RATIO = 8;                     // px / 8 <= src_px <= 8 px
constexpr int MAX_KSIZE = 2 * SUPPORT * MAX_RATIO + 1;
constexpr int OUTSIDE = 255;

// Taps per output coordinate, Pillow's: ksize = 2 ceil(support * filterscale) + 1 with filterscale = max(src_px / px, 1).  The one
// statement of it: bqio_resample_ksize answers with it and bq_tile_resample checks its caller's ksize against it.  A host function (no
// device attribute): the kernels get ksize as an argument.
inline int ksize_of(int src_px, int px) {
    double filterscale = (double)src_px / px;
    if (filterscale < 1.0) filterscale = 1.0;
    double support = SUPPORT * filterscale;
    int c = (int)support;
    if ((double)c < support) ++c;                 // ceil, without <math.h>
    return c * 2 + 1;
}

BQR_HD int clip8(int acc) {                      // Pillow's clip8: an arithmetic shift, then the clamp of its lookup table
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// a tap window as the tables give it, made safe: 0 <= first, first + count <= size, count <= ksize
BQR_HD void window(const int32_t* bounds, int i, int size, int ksize, int& first, int& count) {
    int f = bounds[2 * i], c = bounds[2 * i + 1];
    f = f < 0 ? 0 : (f > size ? size : f);
    c = c < 0 ? 0 : (c > ksize ? ksize : c);
    if (c > size - f) c = size - f;
    first = f;
    count = c;
}

// Horizontal pass of one output pixel: source row `y` of the canvas (any integer), source columns x0 + [0, count), taps k.
// inside: the caller knows row and columns lie in the canvas.
BQR_HD void hpass(const uint8_t* canvas, int H, int W, int y, int x0, int count, const int32_t* k, bool inside, uint8_t out[3]) {
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    if (inside) {
        const uint8_t* p = canvas + ((size_t)y * W + x0) * 3;
        for (int j = 0; j < count; ++j) {
            const int c = k[j];
            a0 += p[3 * j] * c;
            a1 += p[3 * j + 1] * c;
            a2 += p[3 * j + 2] * c;
        }
    } else {
        const bool row_in = y >= 0 && y < H;
        const uint8_t* row = canvas + (size_t)(row_in ? y : 0) * W * 3;
        for (int j = 0; j < count; ++j) {
            const int c = k[j], x = x0 + j;
            const bool in = row_in && x >= 0 && x < W;
            a0 += (in ? row[3 * x] : OUTSIDE) * c;
            a1 += (in ? row[3 * x + 1] : OUTSIDE) * c;
            a2 += (in ? row[3 * x + 2] : OUTSIDE) * c;
        }
    }
    out[0] = (uint8_t)clip8(a0);
    out[1] = (uint8_t)clip8(a1);
    out[2] = (uint8_t)clip8(a2);
}

// Vertical pass of one output byte: `count` bytes of the horizontal pass's result, `pitch` bytes apart, taps k.
BQR_HD uint8_t vpass(const uint8_t* col, int pitch, int count, const int32_t* k) {
    int a = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < count; ++j) a += col[(size_t)j * pitch] * k[j];
    return (uint8_t)clip8(a);
}

// An origin coordinate as the kernels use it: held inside +-2^28, where a window lies outside every canvas the entries accept
// (H, W <= 2^28), so that the sums origin + row / column cannot overflow an int.
BQR_HD int origin_coord(int v) {
    return v < -(1 << 28) ? -(1 << 28) : (v > (1 << 28) ? (1 << 28) : v);
}

// src_px == px: the window itself
BQR_HD uint8_t copy_byte(const uint8_t* canvas, int H, int W, int y, int x, int c) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? canvas[((size_t)y * W + x) * 3 + c] : (uint8_t)OUTSIDE;
}

}  // namespace bqrs
