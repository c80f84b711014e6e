// kernels_jpeg.hip -- baseline-JPEG tiles decoded on the device (bq_jpeg_decode): the routines of jpeg_device.h, which
// libbiscuit_io runs unchanged on the CPU (bqio_jpeg_decode_extracted), behind three kernels.
//
//   entropy  one LANE per tile, the arrangement of the device inflate (kernels_inflate.hip): Huffman-decode and dequantise the
//            tile's blocks into int16 coefficients, natural order, per component plane, in the caller's scratch (zeroed by a
//            memset in front of the kernel).  The tile's table set -- 21 KB of lookups -- sits in LDS: the workgroup (one wave)
//            loads the set of its first tile; a lane whose tile names another set reads that one from global memory through
//            the same pointer type, so tiles with different tables may stand side by side.
//   idct     one thread per 8 x 8 block: the islow IDCT in registers, the 64 samples written over the block's own
//            coefficients (no second plane buffer); a block outside the range rule sets the tile's status.
//   colour   four output pixels per thread over the flattened NHWC output: h2v1 / h2v2 triangle upsampling of the chroma
//            samples, BT.601 in fixed point, three aligned dword stores.
//
// Integer arithmetic throughout; the result is held to Pillow's bytes (tests/test_gpu_jpeg.py), not to a tolerance.
// A tile costs tile_coef_bytes(px) of scratch (554 KB at 299 px, sized for 4:4:4), so a call works in rounds of as many
// tiles as the caller's scratch holds (round_items of bq_rounds.h).
//
// bq_jpeg_decode_canvas: a TIFF page's own w x h segments (bqio_extract_jpeg_segments) through the same entropy and idct kernels
// -- they need the (w, h) geometry and nothing else -- and, in place of `colour`,
//   place    four pixels of the CANVAS per thread: the window of each segment that the canvas and the clip rectangle show
//            (place_window of canvas_place.h, the host's statement too), row by row, in groups of four flat canvas pixels -- 12
//            bytes at a multiple of 12, so three aligned dword stores wherever the whole group belongs to the row, byte stores
//            at a row's ragged ends (the pitch 3 W is no multiple of 4 in general).  Nothing outside a window is written.
#include "bq_ctx.h"
#include "jpeg_device.h"

namespace {

constexpr int JE_NT = 64;                // entropy kernel: one wave per workgroup, one table set in LDS
constexpr int JP_NT = 256;
constexpr int JPEG_ROUND = 2048;         // tiles per round that bq_jpeg_scratch_bytes asks scratch for

struct JpegParams {
    const uint8_t* scan;
    const bqjd::Desc* desc;              // of the round's first tile
    const bqjd::TableSet* tables;
    int n_tables;
    int n;                               // tiles of this round
    int w, h;                            // a tile's frame (bq_jpeg_decode: w = h = px)
    int16_t* coef;                       // [n][tile_i16]
    size_t tile_i16;
    int* status;                         // of the round's first tile
    uint8_t* out;                        // of the CALL's first tile
    long long p0, p1;                    // the round's pixels within the call's flattened output
    long long t0;                        // the round's first tile within the call
};

__global__ void __launch_bounds__(JE_NT) jpeg_entropy_kernel(const JpegParams p) {
    __shared__ bqjd::TableSet sT;
    const int first = blockIdx.x * JE_NT;
    const uint32_t primary = p.desc[first].tset;
    if (primary < (uint32_t)p.n_tables) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.tables + primary);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&sT);
        for (unsigned w = threadIdx.x; w < sizeof(bqjd::TableSet) / 4; w += JE_NT) dst[w] = src[w];
    }
    __syncthreads();
    const int i = first + (int)threadIdx.x;
    if (i >= p.n) return;
    const bqjd::Desc d = p.desc[i];
    bqjd::Geom G;
    if (!bqjd::geom_of(d.geom, p.w, p.h, G) || d.tset >= (uint32_t)p.n_tables) { p.status[i] = bqjd::ST_DESC; return; }
    const bqjd::TableSet* T = d.tset == primary ? &sT : p.tables + d.tset;
    p.status[i] = bqjd::entropy_tile(p.scan + d.off, d.len, G, T, p.coef + (size_t)i * p.tile_i16);
}

__global__ void __launch_bounds__(JP_NT) jpeg_idct_kernel(const JpegParams p) {
    const int i = blockIdx.y;
    bqjd::Geom G;
    if (!bqjd::geom_of(p.desc[i].geom, p.w, p.h, G)) return;
    const uint32_t nblk = G.base[2] + (uint32_t)(G.mcux * G.mcuy);
    const uint32_t b = blockIdx.x * JP_NT + threadIdx.x;
    if (b >= nblk) return;
    if (!bqjd::idct_in_place(p.coef + (size_t)i * p.tile_i16 + (size_t)b * 64)) atomicOr(&p.status[i], (int)bqjd::ST_RANGE);
}

// The group of four flat pixels that starts at pixel a = 4 q, b[12] their bytes, to o = base + 12 q: three dword stores where
// the whole group lies in [P0, P1) (`all`) and o is aligned, otherwise byte stores of the pixels that do lie in it.
__device__ __forceinline__ void store_group(uint8_t* o, const uint8_t (&b)[12], bool all, long long a, long long P0, long long P1) {
    if (all && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long P = a + j;
            if (P >= P0 && P < P1) { o[3 * j] = b[3 * j]; o[3 * j + 1] = b[3 * j + 1]; o[3 * j + 2] = b[3 * j + 2]; }
        }
    }
}

__global__ void __launch_bounds__(JP_NT) jpeg_colour_kernel(const JpegParams p) {
    const long long q = p.p0 / 4 + (long long)blockIdx.x * JP_NT + threadIdx.x;     // group of four pixels of the call's output
    const long long a = q * 4;
    if (a >= p.p1) return;
    const int px = p.w;
    const long long ppt = (long long)px * px;
    long long tile = a / ppt;
    const int rem = (int)(a - tile * ppt);
    int y = rem / px, x = rem - y * px;
    uint8_t b[12];
    bool all = true;
    long long cur = -1;
    bqjd::Geom G;
    bool gok = false;
    const uint8_t* planes = nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long P = a + j;
        const bool valid = P >= p.p0 && P < p.p1;
        all &= valid;
        b[3 * j] = b[3 * j + 1] = b[3 * j + 2] = 0;
        if (valid) {
            if (tile != cur) {
                cur = tile;
                gok = bqjd::geom_of(p.desc[tile - p.t0].geom, px, G);
                planes = reinterpret_cast<const uint8_t*>(p.coef + (size_t)(tile - p.t0) * p.tile_i16);
            }
            if (gok) bqjd::pixel_rgb(planes, G, y, x, b + 3 * j);
        }
        if (++x == px) { x = 0; if (++y == px) { y = 0; ++tile; } }
    }
    store_group(p.out + 12 * q, b, all, a, p.p0, p.p1);
}

struct PlaceParams {
    const int32_t* place;                // [n][2] of the round's first segment
    uint8_t* canvas;
    int H, W;
    int32_t clip[4];
    int groups;                          // groups of four canvas pixels a segment row can touch: ceil(w / 4) + 1
};

// blockIdx.y = the segment, the x dimension = (row of the segment, group of four flat canvas pixels within the row's run).
__global__ void __launch_bounds__(JP_NT) jpeg_place_kernel(const JpegParams p, const PlaceParams c) {
    const int i = blockIdx.y;
    const unsigned t = blockIdx.x * JP_NT + threadIdx.x;
    const int r = (int)(t / (unsigned)c.groups), g = (int)(t % (unsigned)c.groups);
    if (r >= p.h) return;
    bqjd::Geom G;
    if (!bqjd::geom_of(p.desc[i].geom, p.w, p.h, G)) return;
    const int sx = c.place[2 * i], sy = c.place[2 * i + 1];
    bqjd::Window w;
    if (!bqjd::place_window(sx, sy, p.w, p.h, c.H, c.W, c.clip, w)) return;
    const int y = w.y0 + r;
    if (y >= w.y1) return;
    // the row's run of flat canvas pixels [P0, P1): inside the canvas by place_window
    const long long P0 = (long long)(sy + y) * c.W + (sx + w.x0), P1 = P0 + (w.x1 - w.x0);
    const long long q = P0 / 4 + g, a = q * 4;
    if (a >= P1) return;
    const uint8_t* planes = reinterpret_cast<const uint8_t*>(p.coef + (size_t)i * p.tile_i16);
    uint8_t b[12];
    bool all = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long P = a + j;
        const bool valid = P >= P0 && P < P1;
        all &= valid;
        b[3 * j] = b[3 * j + 1] = b[3 * j + 2] = 0;
        if (valid) bqjd::pixel_rgb(planes, G, y, w.x0 + (int)(P - P0), b + 3 * j);
    }
    store_group(c.canvas + 12 * q, b, all, a, P0, P1);
}

}  // namespace

static size_t jpeg_scratch_bytes(int n, int px) {
    if (n <= 0 || px <= 0) return 0;
    return round_cap(n, JPEG_ROUND) * bqjd::tile_coef_bytes(px);
}

static size_t jpeg_canvas_scratch_bytes(int n, int w, int h) {
    if (n <= 0 || w <= 0 || h <= 0) return 0;
    return round_cap(n, JPEG_ROUND) * bqjd::tile_coef_bytes(w, h);
}

// What both entries do with n packed w x h tiles, in rounds of as many as d_scratch holds (whole workgroups of the entropy
// kernel, once it holds one): the round's JpegParams, the scratch zeroed, the entropy and idct kernels, and then last(p, cnt),
// the entry's own kernel over the round's samples.  `last` may set out, p0 and p1 first: only its kernel reads them.
template <typename Last>
static int launch_jpeg_rounds(const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int w, int h, int* d_status,
                              void* d_scratch, size_t scratch_bytes, hipStream_t s, Last last) {
    if (n <= 0) return 0;
    const size_t per = bqjd::tile_coef_bytes(w, h);
    const size_t m = round_items(scratch_bytes, per, JE_NT);
    if (m < 1) return (int)hipErrorInvalidValue;
    for (long long t0 = 0; t0 < n; t0 += (long long)m) {
        const int cnt = (int)(n - t0 < (long long)m ? n - t0 : (long long)m);
        JpegParams p;
        p.scan = d_scan;
        p.desc = reinterpret_cast<const bqjd::Desc*>(d_desc) + t0;
        p.tables = reinterpret_cast<const bqjd::TableSet*>(d_tables);
        p.n_tables = n_tables; p.n = cnt; p.w = w; p.h = h;
        p.coef = reinterpret_cast<int16_t*>(d_scratch); p.tile_i16 = per / 2;
        p.status = d_status + t0; p.out = nullptr;
        p.p0 = p.p1 = 0; p.t0 = t0;
        if (const hipError_t e = hipMemsetAsync(d_scratch, 0, (size_t)cnt * per, s)) return (int)e;
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((cnt + JE_NT - 1) / JE_NT), dim3(JE_NT), 0, s, p);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((bqjd::tile_blocks(w, h) + JP_NT - 1) / JP_NT, cnt), dim3(JP_NT), 0, s, p);
        last(p, cnt);
    }
    return (int)hipGetLastError();
}

// n tiles as bqio_extract_jpeg packed them -> uint8 NHWC + status
static int launch_jpeg_decode(const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int px, uint8_t* d_out,
                              int* d_status, void* d_scratch, size_t scratch_bytes, hipStream_t s) {
    const long long ppt = (long long)px * px;
    return launch_jpeg_rounds(d_scan, d_desc, d_tables, n_tables, n, px, px, d_status, d_scratch, scratch_bytes, s, [&](JpegParams& p, int cnt) {
        p.out = d_out; p.p0 = p.t0 * ppt; p.p1 = (p.t0 + cnt) * ppt;
        const long long groups = (p.p1 + 3) / 4 - p.p0 / 4;
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((groups + JP_NT - 1) / JP_NT)), dim3(JP_NT), 0, s, p);
    });
}

// n segments of w x h as bqio_extract_jpeg_segments packed them -> their windows in the canvas + status
static int launch_jpeg_decode_canvas(const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int w, int h,
                                     const int32_t* d_place, uint8_t* d_canvas, int H, int W, const int32_t* clip, int* d_status, void* d_scratch,
                                     size_t scratch_bytes, hipStream_t s) {
    PlaceParams c;
    c.canvas = d_canvas; c.H = H; c.W = W;
    for (int k = 0; k < 4; ++k) c.clip[k] = clip[k];
    c.groups = (w + 3) / 4 + 1;
    const unsigned place_blocks = (unsigned)(((long long)h * c.groups + JP_NT - 1) / JP_NT);
    return launch_jpeg_rounds(d_scan, d_desc, d_tables, n_tables, n, w, h, d_status, d_scratch, scratch_bytes, s, [&](JpegParams& p, int cnt) {
        c.place = d_place + 2 * p.t0;
        hipLaunchKernelGGL(jpeg_place_kernel, dim3(place_blocks, cnt), dim3(JP_NT), 0, s, p, c);
    });
}

extern "C" {

size_t bq_jpeg_scratch_bytes(int n, int px) { return jpeg_scratch_bytes(n, px); }

int bq_jpeg_decode(bq_ctx* c, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int px,
                   uint8_t* d_out, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || px <= 0 || px > 4096 || n_tables < 0) return fail(c, BQ_ERR_ARG, "bq_jpeg_decode: bad argument");
    if (n == 0) return BQ_OK;
    if (!d_scan || !d_desc || !d_tables || n_tables == 0 || !d_out || !d_status || !d_scratch || ((uintptr_t)d_tables & 3) ||
        ((uintptr_t)d_scan & 15) || ((uintptr_t)d_desc & 3))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode: bad argument");
    if (scratch_bytes < jpeg_scratch_bytes(n, px)) return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_decode: scratch too small");
    ProfScope ps(c, (hipStream_t)stream, "jpeg_decode", 0.0, (double)n * px * px * 3.0);
    const int e = launch_jpeg_decode(d_scan, d_desc, d_tables, n_tables, n, px, d_out, d_status, d_scratch, scratch_bytes, (hipStream_t)stream);
    if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg decode launch: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
}

size_t bq_jpeg_canvas_scratch_bytes(int n, int seg_w, int seg_h) { return jpeg_canvas_scratch_bytes(n, seg_w, seg_h); }

int bq_jpeg_decode_canvas(bq_ctx* c, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int seg_w,
                          int seg_h, const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0, int clip_x1,
                          int clip_y1, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || seg_w <= 0 || seg_w > 4096 || seg_h <= 0 || seg_h > 4096 || n_tables < 0 || !bqcanvas::canvas_args_ok(H, W))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode_canvas: bad argument (need 0 < seg_w, seg_h <= 4096 and 0 < H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_scan || !d_desc || !d_tables || n_tables == 0 || !d_place || !d_canvas || !d_status || !d_scratch || ((uintptr_t)d_tables & 3) ||
        ((uintptr_t)d_scan & 15) || ((uintptr_t)d_desc & 3) || ((uintptr_t)d_place & 3))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode_canvas: bad argument");
    if (scratch_bytes < jpeg_canvas_scratch_bytes(1, seg_w, seg_h))
        return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_decode_canvas: scratch smaller than one segment's (bq_jpeg_canvas_scratch_bytes(1, seg_w, seg_h))");
    const int32_t clip[4] = {clip_x0, clip_y0, clip_x1, clip_y1};
    ProfScope ps(c, (hipStream_t)stream, "jpeg_decode_canvas", 0.0, (double)n * seg_w * seg_h * 3.0);
    const int e = launch_jpeg_decode_canvas(d_scan, d_desc, d_tables, n_tables, n, seg_w, seg_h, d_place, d_canvas, H, W, clip, d_status,
                                            d_scratch, scratch_bytes, (hipStream_t)stream);
    if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg canvas decode launch: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
}

}  // extern "C"
