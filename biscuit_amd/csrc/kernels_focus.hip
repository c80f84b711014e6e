// The whole-slide heatmap's focus mask (DESIGN.md "Heatmap input", Focus mask): Slideflow's Gaussian blur QC on a 4 um / pixel
// thumbnail -- gray, |Laplacian|, a separable Gaussian, one threshold -- restated in integers so that the device and the numpy
// restatement agree integer for integer.  Three kernels.
//
// focus_rows_kernel: thumbnail uint8 [H][W][3] -> A int32 [H][W], the horizontal Gaussian pass over L = |4 G - the four
// neighbours| of G = 2125 r + 7154 g + 721 b.  One workgroup = an FC_TW x FC_TH tile of output pixels.  It stages G of the tile
// with r + 1 columns and one row of halo (13 columns for r = 12), coordinates clamped to the image, then L of the tile with r
// columns of halo: L at a clamped coordinate is taken from the G of that coordinate's own clamped neighbours, which the staged
// tile always holds (its column j is the image column clamp(x0 + j - r - 1), and every neighbour of a clamped column lies inside
// that span).  A thread then sums its 2 r + 1 taps from LDS in a 64-bit accumulator (w <= 2^16, L < 2^24) and stores
// (sum + 2^15) >> 16.
//
// focus_cols_kernel: A -> V, the vertical pass, from a tile of A with r rows of halo (12 for r = 12), rows clamped to the image;
// plane = V > thr (1 = in focus), V itself when asked for, and the number of out-of-focus pixels: reduced over the wave, then
// over the workgroup in LDS, one global add per workgroup.  One workgroup = FC_CW x FC_CH pixels, FC_CH / 8 rows a thread.
//
// LDS layout: every tile is int32 and is read with 32 lanes along a tile row -- a 32-lane half of the wave reads 32 consecutive
// dwords, one bank each (ds_read_b32 banks modulo 32 per half, and the two halves do not conflict), so the row pitch needs no
// padding and is simply the widest tile's (r = 16).  The taps are read at a wave-uniform index from kernel-argument memory: for
// r = 12 the loop is unrolled and they sit in scalar registers; other radii take the same code with a run-time bound.
//
// focus_union_kernel: one wave per grid cell counts the cell's bad pixels over its range of the Otsu plane [Ho][Wo]: a pixel is
// bad iff otsu <= T or focus[ymap[y]][xmap[x]] == 0, the focus plane [Hf][Wf] resized onto the Otsu plane by the two host tables
// (nearest neighbour).  Ranges and maps are checked on the host before they are uploaded (bq_tissue_cells_union); the kernel
// clamps them all the same.
#include "bq_ctx.h"

namespace {

constexpr int FC_MAXR = 16;                                        // the largest radius the tiles are sized for
constexpr int FC_NT = 256;
constexpr int FC_TW = 32, FC_TH = 8;                               // rows kernel: output pixels of a workgroup, one a thread
constexpr int FC_GP = FC_TW + 2 * (FC_MAXR + 1);                   // pitch of the G tile (r + 1 columns of halo each side)
constexpr int FC_LP = FC_TW + 2 * FC_MAXR;                         // pitch of the L tile
constexpr int FC_CW = 32, FC_CH = 32, FC_CPT = FC_CH / (FC_NT / FC_CW);   // columns kernel: output tile, rows a thread (4)
constexpr int FC_WAVE = 64, FC_CELLS = FC_NT / FC_WAVE;            // cells a workgroup of focus_union_kernel counts
constexpr int FC_SHIFT = 16;                                       // the taps sum to 2^16

__device__ __forceinline__ int fclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// R: the radius when it is known at compile time (12: Slideflow's sigma = 3), 0: `r_arg` at run time (1 .. FC_MAXR)
template <int R>
__global__ void __launch_bounds__(FC_NT) focus_rows_kernel(const uint8_t* __restrict__ thumb, int H, int W, const int* __restrict__ taps,
                                                           int r_arg, int tiles_x, int* __restrict__ work) {
    __shared__ int s_g[FC_TH + 2][FC_GP];
    __shared__ int s_l[FC_TH][FC_LP];
    const int r = R ? R : r_arg;
    const int tid = threadIdx.x;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * FC_TW, y0 = by * FC_TH;
    const int gw = FC_TW + 2 * (r + 1), lw = FC_TW + 2 * r;
    for (int i = tid; i < (FC_TH + 2) * gw; i += FC_NT) {
        const int ly = i / gw, lx = i - ly * gw;
        const int y = fclamp(y0 + ly - 1, 0, H - 1), x = fclamp(x0 + lx - (r + 1), 0, W - 1);
        const uint8_t* p = thumb + ((size_t)y * W + x) * 3;
        s_g[ly][lx] = 2125 * p[0] + 7154 * p[1] + 721 * p[2];
    }
    __syncthreads();
    for (int i = tid; i < FC_TH * lw; i += FC_NT) {
        const int ly = i / lw, lx = i - ly * lw;
        const int y = min(y0 + ly, H - 1), x = fclamp(x0 + lx - r, 0, W - 1);        // the image pixel this entry stands for
        const int jy = y - y0 + 1, jx = x - x0 + r + 1;                                // ... and its place in the G tile
        const int ju = max(y - 1, 0) - y0 + 1, jd = min(y + 1, H - 1) - y0 + 1;
        const int jl = max(x - 1, 0) - x0 + r + 1, jr = min(x + 1, W - 1) - x0 + r + 1;
        const int v = 4 * s_g[jy][jx] - s_g[ju][jx] - s_g[jd][jx] - s_g[jy][jl] - s_g[jy][jr];
        s_l[ly][lx] = v < 0 ? -v : v;
    }
    __syncthreads();
    const int ty = tid / FC_TW, tx = tid - ty * FC_TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
        long long acc = 1ll << (FC_SHIFT - 1);
        if (R) {
#pragma unroll
            for (int k = 0; k < 2 * R + 1; ++k) acc += (long long)taps[k] * s_l[ty][tx + k];
        } else {
            for (int k = 0; k < 2 * r + 1; ++k) acc += (long long)taps[k] * s_l[ty][tx + k];
        }
        work[(size_t)y * W + x] = (int)(acc >> FC_SHIFT);
    }
}

template <int R>
__global__ void __launch_bounds__(FC_NT) focus_cols_kernel(const int* __restrict__ work, int H, int W, const int* __restrict__ taps,
                                                           int r_arg, int thr, int tiles_x, int* __restrict__ value,
                                                           uint8_t* __restrict__ plane, int* __restrict__ count) {
    __shared__ int s_a[FC_CH + 2 * FC_MAXR][FC_CW];
    __shared__ int s_count;
    const int r = R ? R : r_arg;
    const int tid = threadIdx.x;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * FC_CW, y0 = by * FC_CH;
    if (tid == 0) s_count = 0;
    for (int i = tid; i < (FC_CH + 2 * r) * FC_CW; i += FC_NT) {
        const int ly = i / FC_CW, lx = i - ly * FC_CW;
        const int y = fclamp(y0 + ly - r, 0, H - 1), x = min(x0 + lx, W - 1);
        s_a[ly][lx] = work[(size_t)y * W + x];
    }
    __syncthreads();
    const int tx = tid & (FC_CW - 1), x = x0 + tx;
    int blurred = 0;
#pragma unroll
    for (int j = 0; j < FC_CPT; ++j) {
        const int ty = (tid / FC_CW) + j * (FC_NT / FC_CW), y = y0 + ty;
        if (x < W && y < H) {
            long long acc = 1ll << (FC_SHIFT - 1);
            if (R) {
#pragma unroll
                for (int k = 0; k < 2 * R + 1; ++k) acc += (long long)taps[k] * s_a[ty + k][tx];
            } else {
                for (int k = 0; k < 2 * r + 1; ++k) acc += (long long)taps[k] * s_a[ty + k][tx];
            }
            const int v = (int)(acc >> FC_SHIFT);
            const size_t o = (size_t)y * W + x;
            if (value) value[o] = v;
            plane[o] = v > thr ? 1 : 0;
            blurred += v > thr ? 0 : 1;
        }
    }
#pragma unroll
    for (int o = FC_WAVE / 2; o > 0; o >>= 1) blurred += __shfl_xor(blurred, o);
    if ((tid & (FC_WAVE - 1)) == 0 && blurred) atomicAdd(&s_count, blurred);
    __syncthreads();
    if (tid == 0 && s_count) atomicAdd(count, s_count);
}

__global__ void __launch_bounds__(FC_NT) focus_union_kernel(const uint8_t* __restrict__ otsu, int Ho, int Wo, int T,
                                                            const uint8_t* __restrict__ focus, int Hf, int Wf, const int* __restrict__ xmap,
                                                            const int* __restrict__ ymap, const int* __restrict__ col,
                                                            const int* __restrict__ row, int gw, int ncell, int* __restrict__ count) {
    const int cell = blockIdx.x * FC_CELLS + (threadIdx.x >> 6), lane = threadIdx.x & (FC_WAVE - 1);
    if (cell >= ncell) return;                                               // (uniform over the wave)
    const int gy = cell / gw, gx = cell - gy * gw;
    const int xa = fclamp(col[2 * gx], 0, Wo), xb = fclamp(col[2 * gx + 1], xa, Wo);
    const int ya = fclamp(row[2 * gy], 0, Ho), yb = fclamp(row[2 * gy + 1], ya, Ho);
    const int w = xb - xa, area = w * (yb - ya);                            // (Ho Wo < 2^31)
    int c = 0;
    for (int i = lane; i < area; i += FC_WAVE) {
        const int dy = i / w, y = ya + dy, x = xa + i - dy * w;
        const int fy = fclamp(ymap[y], 0, Hf - 1), fx = fclamp(xmap[x], 0, Wf - 1);
        c += (otsu[(size_t)y * Wo + x] <= T || focus[(size_t)fy * Wf + fx] == 0) ? 1 : 0;
    }
#pragma unroll
    for (int o = FC_WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) count[cell] = c;
}

}  // namespace

static int launch_tissue_focus(const uint8_t* thumb, int H, int W, const int* taps, int r, int thr, int* work, int* value, uint8_t* plane,
                               int* count, hipStream_t s) {
    if (r < 1 || r > FC_MAXR) return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s)) return (int)e;
    const int rx = (W + FC_TW - 1) / FC_TW, cx = (W + FC_CW - 1) / FC_CW;
    const long long rows = (long long)rx * ((H + FC_TH - 1) / FC_TH), cols = (long long)cx * ((H + FC_CH - 1) / FC_CH);
    if (rows > 0x7fffffffll || cols > 0x7fffffffll) return (int)hipErrorInvalidValue;      // (H W < 2^31: far below)
    if (r == 12) {
        hipLaunchKernelGGL(focus_rows_kernel<12>, dim3((unsigned)rows), dim3(FC_NT), 0, s, thumb, H, W, taps, r, rx, work);
        hipLaunchKernelGGL(focus_cols_kernel<12>, dim3((unsigned)cols), dim3(FC_NT), 0, s, work, H, W, taps, r, thr, cx, value, plane, count);
    } else {
        hipLaunchKernelGGL(focus_rows_kernel<0>, dim3((unsigned)rows), dim3(FC_NT), 0, s, thumb, H, W, taps, r, rx, work);
        hipLaunchKernelGGL(focus_cols_kernel<0>, dim3((unsigned)cols), dim3(FC_NT), 0, s, work, H, W, taps, r, thr, cx, value, plane, count);
    }
    return (int)hipGetLastError();
}

static int launch_tissue_cells_union(const uint8_t* otsu, int Ho, int Wo, int T, const uint8_t* focus, int Hf, int Wf, const int* xmap,
                                     const int* ymap, const int* col, const int* row, int gw, int gh, int* count, hipStream_t s) {
    const int ncell = gw * gh;
    hipLaunchKernelGGL(focus_union_kernel, dim3((unsigned)((ncell + FC_CELLS - 1) / FC_CELLS)), dim3(FC_NT), 0, s, otsu, Ho, Wo, T, focus,
                       Hf, Wf, xmap, ymap, col, row, gw, ncell, count);
    return (int)hipGetLastError();
}

extern "C" {

int bq_tissue_focus(bq_ctx* c, const uint8_t* d_thumb, int H, int W, const int32_t* d_taps, int r, int thr, int32_t* d_work,
                    int32_t* d_value_or_null, uint8_t* d_plane, int32_t* d_count, bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) || r < 1 || r > 16 || thr < 0)
        return fail(c, BQ_ERR_ARG, "bq_tissue_focus: bad argument (need 0 < H, W, H * W < 2^31, 1 <= r <= 16 and 0 <= thr)");
    if (!d_thumb || !d_taps || !d_work || !d_plane || !d_count || ((uintptr_t)d_taps & 3) || ((uintptr_t)d_work & 3) ||
        ((uintptr_t)d_value_or_null & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_focus: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_focus", 2.0 * 2 * (2.0 * r + 1) * (double)H * W, (d_value_or_null ? 16.0 : 12.0) * (double)H * W);
    if (launch_tissue_focus(d_thumb, H, W, d_taps, r, thr, d_work, d_value_or_null, d_plane, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue focus launch failed");
    return BQ_OK;
}

int bq_tissue_cells_union(bq_ctx* c, const uint8_t* d_otsu_plane, int Ho, int Wo, int T, const uint8_t* d_focus_plane, int Hf, int Wf,
                          const int32_t* xmap, const int32_t* ymap, const int32_t* col_ranges, int gw, const int32_t* row_ranges, int gh,
                          int32_t* d_tables, int32_t* d_count, bq_stream_t stream) {
    if (!c || Ho <= 0 || Wo <= 0 || (int64_t)Ho * Wo >= (1ll << 31) || Hf <= 0 || Wf <= 0 || (int64_t)Hf * Wf >= (1ll << 31) || gw <= 0 ||
        gh <= 0 || gw > (1 << 15) || gh > (1 << 15) || T < 0 || T > 255)
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: bad argument (need 0 < H, W and H * W < 2^31 for both planes, 0 < gw, gh <= "
                                   "32768 and 0 <= T <= 255)");
    if (!d_otsu_plane || !d_focus_plane || !xmap || !ymap || !col_ranges || !row_ranges || !d_tables || !d_count ||
        ((uintptr_t)d_tables & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: bad argument");
    const std::string bad = bad_cell_range("Otsu plane", col_ranges, gw, Wo, row_ranges, gh, Ho);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: " + bad);
    for (int i = 0; i < Wo; ++i)
        if (xmap[i] < 0 || xmap[i] >= Wf || (i && xmap[i] < xmap[i - 1]))
            return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: the column map leaves the focus plane or decreases");
    for (int i = 0; i < Ho; ++i)
        if (ymap[i] < 0 || ymap[i] >= Hf || (i && ymap[i] < ymap[i - 1]))
            return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: the row map leaves the focus plane or decreases");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_cells_union", 0.0, 2.0 * (double)Ho * Wo);
    int32_t* d_xmap = d_tables;
    int32_t* d_ymap = d_xmap + Wo;
    int32_t* d_col = d_ymap + Ho;
    int32_t* d_row = d_col + 2 * gw;
    HIPCHK(c, hipMemcpyAsync(d_xmap, xmap, (size_t)Wo * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ymap, ymap, (size_t)Ho * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_col, col_ranges, (size_t)gw * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_row, row_ranges, (size_t)gh * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_tissue_cells_union(d_otsu_plane, Ho, Wo, T, d_focus_plane, Hf, Wf, d_xmap, d_ymap, d_col, d_row, gw, gh, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue cells union launch failed");
    return BQ_OK;
}

}  // extern "C"
