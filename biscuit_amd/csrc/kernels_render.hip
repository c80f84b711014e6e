// The whole-slide heatmap's output stage (DESIGN.md "Heatmap output"): one plane of the grid -- hm.logits[:, :, c] or
// hm.uncertainty[:, :, c] -- drawn over the slide's thumbnail through a 256-entry colour table, what sf.Heatmap.save does on the
// host (results.py:217-227).  The geometry comes from the host as two tables, one entry per output column and one per output row
// (render.render_tables); the kernel does no coordinate arithmetic.  One float32 step per cell, v -> q in [0, 65535] with the
// subtraction and the multiplication un-fused (__fsub_rn / __fmul_rn), everything after it integer.
//
// render_kernel<BICUBIC>: blockIdx.y = the output row, blockIdx.x = a run of RD_NT groups of four FLAT output pixels (pixel P =
// y W + x; group q = pixels [4 q, 4 q + 4), 12 bytes at out + 12 q, dword-aligned when `out` is): a thread produces the pixels of
// its group that lie in its row -- three aligned dword loads / stores where all four do, bytes at the row's ends, because the
// pitch 3 W is no multiple of 4 (the store pattern of kernels_jpeg.hip's place kernel).  A thread reads only the thumbnail
// bytes it then writes and nothing else of `thumb`, so out == thumb is allowed.  LDS: the colour table (one packed dword per
// entry) and the block's share of the column table, at most RD_NT * 4 columns; the row's entry is uniform over the block and is
// read from global memory.  A cell's q is recomputed per tap (two float32 operations on a plane that sits in cache) rather than
// staged by a pre-pass: no scratch, one launch.
// The tables are caller-owned device memory: a cell index read from them is clamped to the grid (negative = no cell in the first
// column of an entry), so a damaged table gives wrong colours, never an access out of bounds.
#include "bq_ctx.h"

#include <math.h>
#include <cmath>

namespace {

constexpr int RD_NT = 256;
constexpr int RD_COLS = RD_NT * 4;       // output columns a block can touch
constexpr int RD_ENTRY = 9;              // bicubic table entry: cell, 4 tap cells, 4 weights (12 fractional bits)
constexpr int RD_MASKED = -1;            // heatmap.MASKED

struct RenderParams {
    const float* values;                 // [gh][gw]
    const int32_t* col;                  // [W] ('none') or [W][9] ('bicubic')
    const int32_t* row;                  // [H] or [H][9]
    const uint8_t* lut;                  // [256][3]
    const uint8_t* thumb;                // [H][W][3]
    uint8_t* out;                        // [H][W][3]
    int gh, gw, H, W, A;
    float vmin, inv;
};

// q of a cell's value, or -1 when the cell is not live (MASKED or not finite)
__device__ __forceinline__ int cell_q(float v, float vmin, float inv) {
    if (!isfinite(v) || v == (float)RD_MASKED) return -1;
    float s = floorf(__fmul_rn(__fsub_rn(v, vmin), inv) * 65536.0f);        // (a power of two: exact, or +-inf)
    s = s < 0.0f ? 0.0f : (s > 65535.0f ? 65535.0f : s);
    return (int)s;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool BICUBIC>
__global__ void __launch_bounds__(RD_NT) render_kernel(const RenderParams p) {
    constexpr int E = BICUBIC ? RD_ENTRY : 1;
    __shared__ uint32_t s_lut[256];
    __shared__ int32_t s_col[RD_COLS * E];
    const int tid = threadIdx.x, y = blockIdx.y;
    const long long P0 = (long long)y * p.W, P1 = P0 + p.W;
    const long long qb = P0 / 4 + (long long)blockIdx.x * RD_NT;            // the block's first group
    // the block's columns: [x_lo, x_hi) of the row
    const long long lo = qb * 4 - P0, hi = lo + RD_COLS;
    const int x_lo = lo < 0 ? 0 : (int)lo, x_hi = hi > p.W ? p.W : (int)hi;
    s_lut[tid] = (uint32_t)p.lut[3 * tid] | ((uint32_t)p.lut[3 * tid + 1] << 8) | ((uint32_t)p.lut[3 * tid + 2] << 16);
    for (int i = tid; i < (x_hi - x_lo) * E; i += RD_NT) s_col[i] = p.col[(size_t)x_lo * E + i];
    __syncthreads();

    const long long q = qb + tid, a = q * 4;
    if (a >= P1) return;
    int ry[E];
#pragma unroll
    for (int k = 0; k < E; ++k) ry[k] = p.row[(size_t)y * E + k];
    const int cy = ry[0];

    const uint8_t* t = p.thumb + 12 * q;
    uint8_t* o = p.out + 12 * q;
    const bool all = a >= P0 && a + 4 <= P1;
    const bool wide = all && ((reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(t)) & 3) == 0;
    uint8_t b[12];
    if (wide) {
        const uint32_t* t4 = reinterpret_cast<const uint32_t*>(t);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = t4[k];
            b[4 * k] = (uint8_t)v; b[4 * k + 1] = (uint8_t)(v >> 8); b[4 * k + 2] = (uint8_t)(v >> 16); b[4 * k + 3] = (uint8_t)(v >> 24);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long P = a + j;
            const bool valid = P >= P0 && P < P1;
            b[3 * j] = valid ? t[3 * j] : 0; b[3 * j + 1] = valid ? t[3 * j + 1] : 0; b[3 * j + 2] = valid ? t[3 * j + 2] : 0;
        }
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long P = a + j;
        if (P < P0 || P >= P1 || cy < 0) continue;
        const int32_t* cx = s_col + ((int)(P - P0) - x_lo) * E;
        if (cx[0] < 0) continue;
        const float* vrow = p.values + (size_t)clampi(cy, p.gh - 1) * p.gw;
        const int q0 = cell_q(vrow[clampi(cx[0], p.gw - 1)], p.vmin, p.inv);
        if (q0 < 0) continue;                                               // the pixel's own cell is not live: transparent
        int Q = q0;
        if constexpr (BICUBIC) {
            long long num = 0;
            int S = 0;
#pragma unroll
            for (int jy = 0; jy < 4; ++jy) {
                const float* r = p.values + (size_t)clampi(ry[1 + jy], p.gh - 1) * p.gw;
                const int wy = ry[5 + jy];
#pragma unroll
                for (int jx = 0; jx < 4; ++jx) {
                    const int qq = cell_q(r[clampi(cx[1 + jx], p.gw - 1)], p.vmin, p.inv);
                    const int w = cx[5 + jx] * wy;
                    if (qq >= 0) { num += (long long)w * qq; S += w; }
                }
            }
            if (S > 0) {
                num += S >> 1;
                const long long d = num <= 0 ? 0 : (S == (1 << 24) ? num >> 24 : num / S);
                Q = d > 65535 ? 65535 : (int)d;
            }
        }
        const uint32_t c = s_lut[Q >> 8];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            b[3 * j + k] = (uint8_t)((p.A * (int)((c >> (8 * k)) & 255u) + (256 - p.A) * (int)b[3 * j + k] + 128) >> 8);
    }

    if (wide) {
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

}  // namespace

static int launch_heatmap_render(const float* values, int gh, int gw, const int32_t* col, const int32_t* row, int bicubic, const uint8_t* lut,
                                 const uint8_t* thumb, uint8_t* out, int H, int W, float vmin, float inv, int A, hipStream_t s) {
    RenderParams p;
    p.values = values; p.col = col; p.row = row; p.lut = lut; p.thumb = thumb; p.out = out;
    p.gh = gh; p.gw = gw; p.H = H; p.W = W; p.A = A; p.vmin = vmin; p.inv = inv;
    const int groups = (W + 3) / 4 + 1;                                      // groups of four flat pixels a row can touch
    const dim3 grid((groups + RD_NT - 1) / RD_NT, H);
    if (bicubic) hipLaunchKernelGGL(render_kernel<true>, grid, dim3(RD_NT), 0, s, p);
    else hipLaunchKernelGGL(render_kernel<false>, grid, dim3(RD_NT), 0, s, p);
    return (int)hipGetLastError();
}

extern "C" {

int bq_heatmap_render(bq_ctx* c, const float* d_values, int gh, int gw, const int32_t* d_col, const int32_t* d_row, int interpolation,
                      const uint8_t* d_lut, const uint8_t* d_thumb, uint8_t* d_out, int H, int W, float vmin, float inv_span, int A,
                      bq_stream_t stream) {
    if (!c || gh <= 0 || gw <= 0 || gh > (1 << 15) || gw > (1 << 15) || H <= 0 || W <= 0 || H > 16384 || W > 16384)
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument (need 0 < gh, gw <= 32768 and 0 < H, W <= 16384)");
    if (interpolation != 0 && interpolation != 1) return fail(c, BQ_ERR_ARG, "bq_heatmap_render: interpolation must be 0 (none) or 1 (bicubic)");
    if (!(A >= 0 && A <= 256) || !std::isfinite(vmin) || !std::isnormal(inv_span) || !(inv_span > 0.0f))
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument (need 0 <= A <= 256, vmin finite, inv_span a normal positive float)");
    if (!d_values || !d_col || !d_row || !d_lut || !d_thumb || !d_out || ((uintptr_t)d_values & 3) || ((uintptr_t)d_col & 3) ||
        ((uintptr_t)d_row & 3))
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument");
    const size_t bytes = (size_t)3 * H * W;
    if (d_out != d_thumb && d_out < d_thumb + bytes && d_thumb < d_out + bytes)
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: out must be the thumbnail itself or not overlap it");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "heatmap_render", 0.0, 2.0 * (double)bytes);
    if (launch_heatmap_render(d_values, gh, gw, d_col, d_row, interpolation, d_lut, d_thumb, d_out, H, W, vmin, inv_span, A, s))
        return fail(c, BQ_ERR_HIP, "heatmap render launch failed");
    return BQ_OK;
}

}  // extern "C"
