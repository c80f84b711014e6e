// The whole-slide heatmap's input stage (DESIGN.md "Heatmap input"): the tile grid of a slide cut out of a canvas in device
// memory, every tile resampled to px x px as Pillow's Image.resize((px, px), Image.LANCZOS) does it -- byte for byte -- and the
// opt-in background filter's grey-pixel count.  The per-pixel arithmetic is resample_device.h's, shared with the CPU
// restatement (bqio_tile_resample); the tap tables come from the host (bqio_resample_taps).
//
// tile_resample_kernel: one workgroup of 256 threads per (tile, strip of R output rows).
//   1. horizontal pass: the source rows the strip's vertical taps read -- [first(r0), first(r1 - 1) + count(r1 - 1)) of the
//      tile's window -- each resampled to px pixels and rounded to bytes (Pillow's order), one (row, x) pixel per thread and
//      step, x fastest so that a wave reads overlapping runs of one canvas row; the result stays in LDS, [rows][3 px] bytes
//   2. vertical pass over LDS: one output dword (four consecutive bytes of the strip, which is contiguous in the NHWC
//      output) per thread and step, aligned dword stores; the few bytes in front of the first and behind the last aligned
//      dword go out as bytes
// Overlapping tiles (stride_div > 1) read the same canvas; nothing but the output goes to global memory.  Source pixels outside
// the canvas read as 255; a tile whose window lies inside the canvas takes the loop without the bounds checks (wave-uniform).
// The tables are caller-owned device memory: every window read from them is clamped (resample_device.h: window) and every LDS
// row index is held inside the strip's rows, so a damaged table gives wrong bytes, never an access out of bounds.
#include "bq_ctx.h"
#include "resample_device.h"

#include <math.h>

namespace {

constexpr int RS_NT = 256;
constexpr int RS_LDS = 64000;            // bytes of the horizontal pass's result a workgroup may hold
constexpr int RS_MAX_R = 32;             // output rows per strip, at most

__global__ void __launch_bounds__(RS_NT) tile_resample_kernel(const uint8_t* __restrict__ canvas, int H, int W,
                                                              const int* __restrict__ origin, int src_px, int px,
                                                              const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                              int R, int max_rows, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t inter[];
    const int tid = threadIdx.x;
    const int strips = (px + R - 1) / R;
    const int t = blockIdx.x / strips, st = blockIdx.x - t * strips;
    const int r0 = st * R, r1 = r0 + R < px ? r0 + R : px;
    const int ox = bqrs::origin_coord(origin[2 * t]), oy = bqrs::origin_coord(origin[2 * t + 1]);
    const int pitch = 3 * px;
    int row_lo, c0, f1, c1;
    bqrs::window(bounds, r0, src_px, ksize, row_lo, c0);
    bqrs::window(bounds, r1 - 1, src_px, ksize, f1, c1);
    int nrows = f1 + c1 - row_lo;
    nrows = nrows < 0 ? 0 : (nrows > max_rows ? max_rows : nrows);
    const bool whole = ox >= 0 && oy >= 0 && ox <= W - src_px && oy <= H - src_px;

    for (int i = tid; i < nrows * px; i += RS_NT) {
        const int r = i / px, x = i - r * px;
        int first, count;
        bqrs::window(bounds, x, src_px, ksize, first, count);
        uint8_t o[3];
        bqrs::hpass(canvas, H, W, oy + row_lo + r, ox + first, count, coef + (size_t)x * ksize, whole, o);
        uint8_t* d = inter + r * pitch + 3 * x;
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
    __syncthreads();

    uint8_t* dst = out + ((size_t)t * px + r0) * pitch;
    const int total = (r1 - r0) * pitch;
    auto vbyte = [&](int f) -> unsigned {
        const int y = f / pitch, b = f - y * pitch;
        int first, count;
        bqrs::window(bounds, r0 + y, src_px, ksize, first, count);
        int off = first - row_lo;
        off = off < 0 ? 0 : off;
        if (off + count > nrows) count = nrows > off ? nrows - off : 0;
        return bqrs::vpass(inter + off * pitch + b, pitch, count, coef + (size_t)(r0 + y) * ksize);
    };
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    head = head < total ? head : total;
    const int nd = (total - head) / 4, tail = head + 4 * nd;
    if (tid < head) dst[tid] = (uint8_t)vbyte(tid);
    for (int d = tid; d < nd; d += RS_NT) {
        const int f = head + 4 * d;
        const unsigned v = vbyte(f) | (vbyte(f + 1) << 8) | (vbyte(f + 2) << 16) | (vbyte(f + 3) << 24);
        *reinterpret_cast<unsigned*>(dst + f) = v;
    }
    if (tid < total - tail) dst[tail + tid] = (uint8_t)vbyte(tail + tid);
}

// src_px == px: the window itself (what the host path does when the level already has the tile's resolution)
__global__ void __launch_bounds__(RS_NT) tile_copy_kernel(const uint8_t* __restrict__ canvas, int H, int W, const int* __restrict__ origin,
                                                          int px, int rows_per_block, uint8_t* __restrict__ out) {
    const int blocks = (px + rows_per_block - 1) / rows_per_block;
    const int t = blockIdx.x / blocks, y0 = (blockIdx.x - t * blocks) * rows_per_block;
    const int y1 = y0 + rows_per_block < px ? y0 + rows_per_block : px;
    const int ox = bqrs::origin_coord(origin[2 * t]), oy = bqrs::origin_coord(origin[2 * t + 1]), pitch = 3 * px;
    uint8_t* dst = out + ((size_t)t * px + y0) * pitch;
    for (int i = threadIdx.x; i < (y1 - y0) * pitch; i += RS_NT) {
        const int y = i / pitch, b = i - y * pitch, x = b / 3;
        dst[i] = bqrs::copy_byte(canvas, H, W, oy + y0 + y, ox + x, b - 3 * x);
    }
}

// The background filter's count (bq_tile_grayspace): pixels of a tile whose HSV saturation is below the threshold, as an
// integer comparison -- mx - mn < limit[mx], the host's table of the float64 definition.  One workgroup per tile.
__global__ void __launch_bounds__(RS_NT) grayspace_kernel(const uint8_t* __restrict__ tiles, int npix, const int* __restrict__ limit256,
                                                          int* __restrict__ count) {
    __shared__ int lim[256];
    __shared__ int wsum[RS_NT / 64];
    const int tid = threadIdx.x;
    lim[tid] = limit256[tid];
    __syncthreads();
    const uint8_t* src = tiles + (size_t)blockIdx.x * npix * 3;
    int c = 0;
    for (int i = tid; i < npix; i += RS_NT) {
        const int r = src[3 * i], g = src[3 * i + 1], b = src[3 * i + 2];
        const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
        c += (mx - mn) < lim[mx] ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < RS_NT / 64; ++w) s += wsum[w];
        count[blockIdx.x] = s;
    }
}

}  // namespace

static int resample_ksize(int src_px, int px) { return bqrs::ksize_of(src_px, px); }      // for bq_tile_resample's argument check

// Output rows per strip for this ratio, or 0 when even one row's taps do not fit the LDS budget.  The rows a strip of R output
// rows reads: first(r0 + R - 1) - first(r0) <= ceil((R - 1) scale) + 1, plus at most ksize taps of the last row.
static int resample_strip_rows(int src_px, int px, int ksize, int* max_rows) {
    const int cap = RS_LDS / (3 * px);
    const double scale = (double)src_px / px;
    for (int R = RS_MAX_R; R >= 1; --R) {
        const int rows = (int)ceil((R - 1) * scale) + 1 + ksize;
        if (rows <= cap) { *max_rows = rows; return R; }
    }
    return 0;
}

// Workgroups a call launches (one grid dimension): n x strips, or n x blocks of 16 rows for the copy; 0 when the ratio does not fit.
static long long resample_grid(int n, int src_px, int px, int ksize) {
    if (src_px == px) return (long long)n * ((px + 15) / 16);
    int rows = 0;
    const int R = resample_strip_rows(src_px, px, ksize, &rows);
    return R > 0 ? (long long)n * ((px + R - 1) / R) : 0;
}

static int launch_tile_resample(const uint8_t* canvas, int H, int W, const int* origin, int n, int src_px, int px, const int* bounds,
                                const int* coef, int ksize, uint8_t* out, hipStream_t s) {
    if (n <= 0) return 0;
    if (src_px == px) {
        const int rows = 16, blocks = (px + rows - 1) / rows;
        hipLaunchKernelGGL(tile_copy_kernel, dim3((unsigned)n * blocks), dim3(RS_NT), 0, s, canvas, H, W, origin, px, rows, out);
        return (int)hipGetLastError();
    }
    int max_rows = 0;
    const int R = resample_strip_rows(src_px, px, ksize, &max_rows);
    if (R <= 0) return (int)hipErrorInvalidValue;
    const int strips = (px + R - 1) / R;
    hipLaunchKernelGGL(tile_resample_kernel, dim3((unsigned)n * strips), dim3(RS_NT), (size_t)max_rows * 3 * px, s, canvas, H, W, origin,
                       src_px, px, bounds, coef, ksize, R, max_rows, out);
    return (int)hipGetLastError();
}

static int launch_tile_grayspace(const uint8_t* tiles, int n, int px, const int* limit256, int* count, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(grayspace_kernel, dim3(n), dim3(RS_NT), 0, s, tiles, px * px, limit256, count);
    return (int)hipGetLastError();
}

extern "C" {

int bq_tile_resample(bq_ctx* c, const uint8_t* d_canvas, int H, int W, const int32_t* d_origin, int n, int src_px, int px,
                     const int32_t* d_bounds, const int32_t* d_coef, int ksize, uint8_t* d_out, bq_stream_t stream) {
    if (!c || n < 0 || n > (1 << 20) || px <= 0 || px > 4096 || src_px <= 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28) ||
        (int64_t)src_px > 8ll * px || (int64_t)px > 8ll * src_px)
        return fail(c, BQ_ERR_ARG, "bq_tile_resample: bad argument (need 0 < px <= 4096, px / 8 <= src_px <= 8 px, 0 <= n <= 2^20, H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_canvas || !d_origin || !d_out || ((uintptr_t)d_origin & 3)) return fail(c, BQ_ERR_ARG, "bq_tile_resample: bad argument");
    if (src_px != px) {
        if (!d_bounds || !d_coef || ((uintptr_t)d_bounds & 3) || ((uintptr_t)d_coef & 3) || ksize != resample_ksize(src_px, px))
            return fail(c, BQ_ERR_ARG, "bq_tile_resample: the tap tables are not bqio_resample_taps(src_px, px)'s");
        int rows = 0;
        if (!resample_strip_rows(src_px, px, ksize, &rows))
            return fail(c, BQ_ERR_ARG, "bq_tile_resample: the taps of one output row do not fit the kernel's LDS at this px and ratio");
    }
    if (resample_grid(n, src_px, px, ksize) > 0x7fffffffll)
        return fail(c, BQ_ERR_ARG, "bq_tile_resample: n x strips of output rows exceeds 2^31 - 1 workgroups; split the call");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tile_resample", 2.0 * 2 * 3 * (double)n * px * px * (src_px == px ? 0 : ksize),
                 (double)n * 3 * ((double)src_px * src_px + (double)px * px));
    if (launch_tile_resample(d_canvas, H, W, d_origin, n, src_px, px, d_bounds, d_coef, ksize, d_out, s))
        return fail(c, BQ_ERR_HIP, "tile resample launch failed");
    return BQ_OK;
}

int bq_tile_grayspace(bq_ctx* c, const uint8_t* d_tiles, int n, int px, const int32_t* d_limit256, int32_t* d_count, bq_stream_t stream) {
    if (!c || n < 0 || px <= 0 || px > 4096) return fail(c, BQ_ERR_ARG, "bq_tile_grayspace: bad argument");
    if (n == 0) return BQ_OK;
    if (!d_tiles || !d_limit256 || !d_count || ((uintptr_t)d_limit256 & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tile_grayspace: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tile_grayspace", 6.0 * n * px * px, 3.0 * n * px * px);
    if (launch_tile_grayspace(d_tiles, n, px, d_limit256, d_count, s)) return fail(c, BQ_ERR_HIP, "grayspace launch failed");
    return BQ_OK;
}

}  // extern "C"
