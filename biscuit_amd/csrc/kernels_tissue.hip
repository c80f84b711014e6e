// The whole-slide heatmap's tissue mask (DESIGN.md "Heatmap input", Tissue mask): Otsu QC on the slide's thumbnail, restated in
// integers so that the device and the numpy restatement agree bit for bit.  Two kernels; the Otsu threshold itself is taken on
// the host from the 256 histogram counts between them (tissue.otsu_threshold).
//
// tissue_blur_kernel: thumbnail uint8 [H][W][3] -> the 7 x 7 median of its 8-bit HSV saturation, uint8 [H][W], and that plane's
// 256-bin histogram.  One workgroup = a TS_TW x TS_TH tile of output pixels.  It stages S = ((mx - mn) sdiv[mx] + 2048) >> 12 of
// the tile and its 3-pixel halo in LDS, coordinates clamped to the image (the replicated border; H or W below 7 included), so
// the saturation pass and the median are one launch.  A thread then holds its pixel's 49 neighbours in registers (the two window
// loops are fully unrolled: every index is a constant, nothing goes to scratch) and selects the 25th smallest by bisection over
// the eight bit planes: the median is the largest c with fewer than 25 neighbours below c.  The histogram is built per
// workgroup in LDS; each workgroup then makes at most one global add per bin.
//
// tissue_cells_kernel: one wave per grid cell counts the cell's background pixels (plane <= T) over its column x row range of
// the plane and reduces across the wave.  Cells may overlap and may be one pixel wide.  The ranges are checked on the host
// before they are uploaded (bq_tissue_cells); the kernel clamps them to the plane all the same.
#include "bq_ctx.h"

namespace {

constexpr int TS_TW = 32, TS_TH = 8, TS_NT = TS_TW * TS_TH;       // output pixels of a workgroup: one a thread
constexpr int TS_R = 3, TS_K = 2 * TS_R + 1;                      // the 7 x 7 window
constexpr int TS_LW = TS_TW + 2 * TS_R, TS_LH = TS_TH + 2 * TS_R; // the tile with its halo
constexpr int TS_RANK = (TS_K * TS_K) / 2;                        // 24 neighbours lie below the 25th smallest, at most
constexpr int TS_WAVE = 64, TS_CELLS = TS_NT / TS_WAVE;           // cells a workgroup of tissue_cells_kernel counts

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(TS_NT) tissue_blur_kernel(const uint8_t* __restrict__ thumb, int H, int W, const int* __restrict__ sdiv,
                                                            int tiles_x, uint8_t* __restrict__ plane, int* __restrict__ hist) {
    __shared__ int s_div[256];
    __shared__ int s_hist[256];
    __shared__ uint8_t s_sat[TS_LH][TS_LW + 2];
    const int tid = threadIdx.x;
    s_div[tid] = sdiv[tid];
    s_hist[tid] = 0;
    __syncthreads();
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * TS_TW, y0 = by * TS_TH;
    for (int i = tid; i < TS_LH * TS_LW; i += TS_NT) {
        const int ly = i / TS_LW, lx = i - ly * TS_LW;
        const int y = clampi(y0 + ly - TS_R, 0, H - 1), x = clampi(x0 + lx - TS_R, 0, W - 1);
        const uint8_t* p = thumb + ((size_t)y * W + x) * 3;
        const int r = p[0], g = p[1], b = p[2];
        const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
        s_sat[ly][lx] = (uint8_t)(((mx - mn) * s_div[mx] + 2048) >> 12);
    }
    __syncthreads();
    const int ty = tid / TS_TW, tx = tid - ty * TS_TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
        int v[TS_K * TS_K];
#pragma unroll
        for (int dy = 0; dy < TS_K; ++dy)
#pragma unroll
            for (int dx = 0; dx < TS_K; ++dx) v[dy * TS_K + dx] = s_sat[ty + dy][tx + dx];
        int med = 0;
#pragma unroll
        for (int bit = 128; bit > 0; bit >>= 1) {
            const int c = med | bit;
            int below = 0;
#pragma unroll
            for (int k = 0; k < TS_K * TS_K; ++k) below += v[k] < c ? 1 : 0;
            if (below <= TS_RANK) med = c;
        }
        plane[(size_t)y * W + x] = (uint8_t)med;
        atomicAdd(&s_hist[med], 1);
    }
    __syncthreads();
    if (s_hist[tid]) atomicAdd(&hist[tid], s_hist[tid]);
}

__global__ void __launch_bounds__(TS_NT) tissue_cells_kernel(const uint8_t* __restrict__ plane, int H, int W, int T,
                                                             const int* __restrict__ col, const int* __restrict__ row, int gw, int ncell,
                                                             int* __restrict__ count) {
    const int cell = blockIdx.x * TS_CELLS + (threadIdx.x >> 6), lane = threadIdx.x & (TS_WAVE - 1);
    if (cell >= ncell) return;                                               // (uniform over the wave)
    const int gy = cell / gw, gx = cell - gy * gw;
    const int xa = clampi(col[2 * gx], 0, W), xb = clampi(col[2 * gx + 1], xa, W);
    const int ya = clampi(row[2 * gy], 0, H), yb = clampi(row[2 * gy + 1], ya, H);
    const int w = xb - xa, area = w * (yb - ya);                            // (H W < 2^31)
    int c = 0;
    for (int i = lane; i < area; i += TS_WAVE) {
        const int dy = i / w, dx = i - dy * w;
        c += plane[(size_t)(ya + dy) * W + xa + dx] <= T ? 1 : 0;
    }
#pragma unroll
    for (int o = TS_WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) count[cell] = c;
}

}  // namespace

static int launch_tissue_blur(const uint8_t* thumb, int H, int W, const int* sdiv256, uint8_t* plane, int* hist, hipStream_t s) {
    if (const hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(int), s)) return (int)e;
    const int tiles_x = (W + TS_TW - 1) / TS_TW, tiles_y = (H + TS_TH - 1) / TS_TH;
    const long long blocks = (long long)tiles_x * tiles_y;                   // (H W < 2^31: below 2^29)
    if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tissue_blur_kernel, dim3((unsigned)blocks), dim3(TS_NT), 0, s, thumb, H, W, sdiv256, tiles_x, plane, hist);
    return (int)hipGetLastError();
}

static int launch_tissue_cells(const uint8_t* plane, int H, int W, int T, const int* col, const int* row, int gw, int gh, int* count,
                               hipStream_t s) {
    const int ncell = gw * gh;
    hipLaunchKernelGGL(tissue_cells_kernel, dim3((unsigned)((ncell + TS_CELLS - 1) / TS_CELLS)), dim3(TS_NT), 0, s, plane, H, W, T, col,
                       row, gw, ncell, count);
    return (int)hipGetLastError();
}

// (bq_ctx.h: shared with bq_tissue_cells_union)
std::string bad_cell_range(const char* plane, const int32_t* col_ranges, int gw, int W, const int32_t* row_ranges, int gh, int H) {
    for (int i = 0; i < gw; ++i)
        if (col_ranges[2 * i] < 0 || col_ranges[2 * i] >= col_ranges[2 * i + 1] || col_ranges[2 * i + 1] > W)
            return std::string("a column range is empty or outside the ") + plane;
    for (int i = 0; i < gh; ++i)
        if (row_ranges[2 * i] < 0 || row_ranges[2 * i] >= row_ranges[2 * i + 1] || row_ranges[2 * i + 1] > H)
            return std::string("a row range is empty or outside the ") + plane;
    return std::string();
}

extern "C" {

int bq_tissue_blur(bq_ctx* c, const uint8_t* d_thumb, int H, int W, const int32_t* d_sdiv256, uint8_t* d_plane, int32_t* d_hist,
                   bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31))
        return fail(c, BQ_ERR_ARG, "bq_tissue_blur: bad argument (need 0 < H, W and H * W < 2^31)");
    if (!d_thumb || !d_sdiv256 || !d_plane || !d_hist || ((uintptr_t)d_sdiv256 & 3) || ((uintptr_t)d_hist & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_blur: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_blur", 0.0, 4.0 * (double)H * W);
    if (launch_tissue_blur(d_thumb, H, W, d_sdiv256, d_plane, d_hist, s)) return fail(c, BQ_ERR_HIP, "tissue blur launch failed");
    return BQ_OK;
}

int bq_tissue_cells(bq_ctx* c, const uint8_t* d_plane, int H, int W, int T, const int32_t* col_ranges, int gw, const int32_t* row_ranges,
                    int gh, int32_t* d_ranges, int32_t* d_count, bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) || gw <= 0 || gh <= 0 || gw > (1 << 15) || gh > (1 << 15) || T < 0 || T > 255)
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells: bad argument (need 0 < H, W, H * W < 2^31, 0 < gw, gh <= 32768 and 0 <= T <= 255)");
    if (!d_plane || !col_ranges || !row_ranges || !d_ranges || !d_count || ((uintptr_t)d_ranges & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells: bad argument");
    const std::string bad = bad_cell_range("plane", col_ranges, gw, W, row_ranges, gh, H);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, "bq_tissue_cells: " + bad);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_cells", 0.0, (double)H * W);
    HIPCHK(c, hipMemcpyAsync(d_ranges, col_ranges, (size_t)gw * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ranges + 2 * gw, row_ranges, (size_t)gh * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_tissue_cells(d_plane, H, W, T, d_ranges, d_ranges + 2 * gw, gw, gh, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue cells launch failed");
    return BQ_OK;
}

}  // extern "C"
