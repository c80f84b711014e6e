// The heatmap's region-of-interest mask (DESIGN.md "Heatmap input", Region-of-interest mask), stated once for the host and the
// device in the pattern of resample_device.h: the crossing rule below is compiled into libbiscuit_io.so (roi_host.cpp:
// bqio_roi_plane -- the CPU build the tests run) and into kernels_roi.hip (bq_roi_plane), and the table checks are the ones both
// entries make before they touch anything.
//
// Everything is integer arithmetic on DOUBLED level-0 coordinates: a polygon vertex (x, y) arrives as (2 x, 2 y), a sample point
// as one entry of a per-axis table the host built (roi.center_tables / roi.raster_tables), so that a pixel centre at half a
// level-0 pixel is an integer too.  A sample p is inside one polygon iff an odd number of its edges count (even-odd), and inside
// the region iff it is inside any polygon (union).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQROI_HD __host__ __device__ inline
#else
#define BQROI_HD inline
#endif

namespace bqroi {

constexpr int VERTEX_MAX = 1 << 28;              // |doubled vertex coordinate| <= 2^28 (level-0 coordinates in [-2^27, 2^27])
constexpr int SAMPLE_MAX = 1 << 29;              // 0 <= doubled sample coordinate <= 2^29
constexpr int MAX_EDGES = 1 << 20;

// First half of the crossing rule: the edge a -> b straddles the sample's row, half-open -- an end exactly on the row is "not
// above" -- so a vertex on the row is counted once by the two edges that meet there and a horizontal edge never.
BQROI_HD bool straddles(int ay, int by, int py) { return (ay > py) != (by > py); }

// Second half, for an edge that straddles: d = (b.x - a.x)(p.y - a.y) - (p.x - a.x)(b.y - a.y); the edge counts iff p lies
// strictly on its left going up (d > 0 when b.y > a.y) or strictly on its right going down (d < 0 when b.y < a.y); a point on the
// edge (d == 0) does not count.  Bounds: |b.x - a.x|, |b.y - a.y| <= 2^29 and |p - a| <= 2^29 + 2^28 per axis, all inside int32;
// each product is below 3 * 2^57 and |d| below 3 * 2^58 < 2^62, inside int64.
BQROI_HD bool counts_beyond(int ax, int ay, int bx, int by, int px, int py) {
    const int64_t d = (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(px - ax) * (int64_t)(by - ay);
    return by > ay ? d > 0 : d < 0;
}

// The checks of both entries, on HOST memory: 0 < W, H, H * W < 2^31, 3 <= E <= 2^20, 1 <= P, starts from 0 to E in steps of at
// least 3, every vertex coordinate inside +-2^28 and every sample coordinate inside [0, 2^29].  -> nullptr, or what is wrong.
inline const char* check_tables(const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys,
                                int H) {
    if (W <= 0 || H <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return "need 0 < W, H and H * W < 2^31";
    if (E < 3 || E > MAX_EDGES || P < 1 || P > E / 3) return "need 3 <= E <= 2^20 edges in 1 <= P <= E / 3 polygons";
    if (!edges || !starts || !xs || !ys) return "null table";
    if (starts[0] != 0 || starts[P] != E) return "the polygon starts do not run from 0 to E";
    for (int i = 0; i < P; ++i)
        if ((int64_t)starts[i + 1] - starts[i] < 3) return "the polygon starts do not increase by at least 3 edges";
    for (int64_t i = 0; i < (int64_t)4 * E; ++i)
        if (edges[i] < -VERTEX_MAX || edges[i] > VERTEX_MAX) return "a doubled vertex coordinate is outside [-2^28, 2^28]";
    for (int i = 0; i < W; ++i)
        if (xs[i] < 0 || xs[i] > SAMPLE_MAX) return "a doubled sample column is outside [0, 2^29]";
    for (int i = 0; i < H; ++i)
        if (ys[i] < 0 || ys[i] > SAMPLE_MAX) return "a doubled sample row is outside [0, 2^29]";
    return nullptr;
}

}  // namespace bqroi
