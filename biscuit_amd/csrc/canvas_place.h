// canvas_place.h -- a decoded segment's place in a slide canvas, stated once for every canvas decoder, host and device:
// jpeg_device.h and j2k_device.h bring Window and place_window into their namespaces, so the kernels (kernels_jpeg.hip,
// kernels_j2k.hip) and the CPU entries (tfrecord_reader.cpp, j2k_host.cpp) all ask the one body below.
//
// A canvas is uint8 [H][W][3]; a seg_w x seg_h segment lies with its top-left pixel at canvas position (px, py), which may be
// negative or beyond the canvas; clip = {x0, y0, x1, y1} is a rectangle in canvas coordinates (the level's image extent: what a
// border segment holds beyond it is padding and is never shown).  The window [x0, x1) x [y0, y1) of the SEGMENT's own pixels
// that lie inside both the canvas and the rectangle: exactly those are written, pixel (y, x) to canvas pixel (py + y, px + x).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQC_HD __host__ __device__ inline
#else
#define BQC_HD inline
#endif

namespace bqcanvas {

// The canvases an entry accepts: with H, W <= 2^28 a flat pixel index and its byte offset stay far inside 64 bits, and a
// window's corners inside an int.
BQC_HD bool canvas_args_ok(int H, int W) { return H > 0 && W > 0 && H <= (1 << 28) && W <= (1 << 28); }

struct Window { int x0, y0, x1, y1; };   // in segment coordinates, half open

// false: the canvas shows none of the segment.  64-bit sums, so that no place or rectangle overflows.
BQC_HD bool place_window(int px, int py, int seg_w, int seg_h, int H, int W, const int32_t* clip, Window& w) {
    auto lo = [](int64_t a, int64_t b) { return a > b ? a : b; };
    auto hi = [](int64_t a, int64_t b) { return a < b ? a : b; };
    const int64_t cx0 = lo(clip[0], 0), cy0 = lo(clip[1], 0), cx1 = hi(clip[2], W), cy1 = hi(clip[3], H);
    const int64_t x0 = lo(cx0 - px, 0), y0 = lo(cy0 - py, 0), x1 = hi(cx1 - px, seg_w), y1 = hi(cy1 - py, seg_h);
    if (x1 <= x0 || y1 <= y0) return false;
    w.x0 = (int)x0; w.y0 = (int)y0; w.x1 = (int)x1; w.y1 = (int)y1;
    return true;
}

}  // namespace bqcanvas
