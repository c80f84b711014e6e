// The data behind the UQ calibration figure over every row of a tile table (biscuit/threshold.py:15-122, plot_uncertainty;
// DESIGN.md section 7 "UQ calibration"): the Gaussian kernel density of the uncertainty per group (correct / incorrect) and the local
// quadratic regression of correct on uncertainty (LOESS: span of the rows, tricube weights, degree 2) fitted directly at a grid of
// vertices, with what its confidence band needs.  Both are dense sums over (grid point x row) in float64: VALU-bound, no matrix cores.
//
// Layout of both sums: the rows are cut into chunks of chunk_rows(n) (a function of n alone); a workgroup of 256 threads takes one
// chunk and a small tile of grid points, keeps every sum of the tile in registers over its rows, adds them across the wave with a
// shuffle butterfly and across the four waves through LDS in wave order, and writes partial[chunk][point][sum].  A finish kernel
// adds the partials in chunk order.  No atomics and no order that depends on timing: the same bits every call.  Every scratch byte
// a kernel reads was written earlier in the same call (DESIGN.md "Buffer contract").
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bq_ctx.h"
#include "chunk_sum.h"

namespace {

constexpr int KDE_PT = 8;            // support points of a density workgroup: 2 groups x 8 sums in registers
constexpr int LO_PT = 4;             // vertices of a regression workgroup: 4 x 13 moments in registers
constexpr int NMOM = 13;             // m0..m4 (sum w u^k), t0..t2 (sum w y u^k), r0..r4 (sum w^2 u^k)
constexpr int MAX_GRID = 1024;       // the residual pass holds three vertex arrays in LDS

// a * b + c in two roundings, as numpy computes it: the grid points must be the host's bit for bit (a row's segment of the
// interpolant is decided by comparing against them), so this product and sum may not contract into an FMA
__device__ inline double mul_add_2r(double a, double b, double c) {
#pragma clang fp contract(off)
    const double p = a * b;
    return p + c;
}

// numpy.linspace(start, stop, G)[j]: j * step + start, the last point stop itself
__device__ inline double linspace_at(double start, double stop, int G, int j) {
    const double step = (stop - start) / (double)(G - 1);
    return j == G - 1 ? stop : mul_add_2r((double)j, step, start);
}

__device__ inline double wave_min(double v) {
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// ---------------------------------------------------------------- density
// group statistics: stat[g][8] = n, min, max, mean, std (ddof 1), bw (Scott), valid, 1 / (n bw sqrt(2 pi))
constexpr int GS = 8;

// pass 1 over a chunk -> part1[chunk][8] = n0, n1, sum0, sum1, min0, min1, max0, max1
__global__ void __launch_bounds__(NT) kde_stats1_kernel(const double* __restrict__ x, const unsigned char* __restrict__ y, long long n,
                                                        long long rows, double* __restrict__ part1) {
    __shared__ double lds[(NW + 1) * 4 + 4 * NW];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double mn[2] = {__builtin_inf(), __builtin_inf()}, mx[2] = {-__builtin_inf(), -__builtin_inf()};
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const double v = x[i];
        const bool g = y[i] != 0;
        s[0] += g ? 0.0 : 1.0; s[1] += g ? 1.0 : 0.0;
        s[2] += g ? 0.0 : v;   s[3] += g ? v : 0.0;
        if (g) { mn[1] = fmin(mn[1], v); mx[1] = fmax(mx[1], v); } else { mn[0] = fmin(mn[0], v); mx[0] = fmax(mx[0], v); }
    }
    double* ext = lds + (NW + 1) * 4;     // [4][NW]: min0, min1, max0, max1 per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double a0 = wave_min(mn[0]), a1 = wave_min(mn[1]), b0 = wave_max(mx[0]), b1 = wave_max(mx[1]);
    if (lane == 0) { ext[0 * NW + wave] = a0; ext[1 * NW + wave] = a1; ext[2 * NW + wave] = b0; ext[3 * NW + wave] = b1; }
    const double* sum = block_sum<4>(s, lds);        // its barriers cover ext as well
    if (threadIdx.x < 4) part1[(size_t)blockIdx.x * 8 + threadIdx.x] = sum[threadIdx.x];
    if (threadIdx.x >= 4 && threadIdx.x < 8) {
        const int k = threadIdx.x - 4;
        double v = ext[k * NW];
        for (int w = 1; w < NW; ++w) v = k < 2 ? fmin(v, ext[k * NW + w]) : fmax(v, ext[k * NW + w]);
        part1[(size_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
}

// one workgroup: part1 over the chunks in order -> stat[g][0..3] = n, min, max, mean
__global__ void __launch_bounds__(NT) kde_stats1_finish_kernel(const double* __restrict__ part1, int chunks, double* __restrict__ stat) {
    if (threadIdx.x >= 2) return;
    const int g = threadIdx.x;
    double cnt = 0.0, sum = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    for (int c = 0; c < chunks; ++c) {
        const double* p = part1 + (size_t)c * 8;
        cnt += p[g]; sum += p[2 + g]; mn = fmin(mn, p[4 + g]); mx = fmax(mx, p[6 + g]);
    }
    stat[g * GS + 0] = cnt; stat[g * GS + 1] = mn; stat[g * GS + 2] = mx; stat[g * GS + 3] = cnt > 0.0 ? sum / cnt : 0.0;
}

// pass 2 over a chunk -> part2[chunk][2]: the sum of squares about the group's mean
__global__ void __launch_bounds__(NT) kde_stats2_kernel(const double* __restrict__ x, const unsigned char* __restrict__ y, long long n,
                                                        long long rows, const double* __restrict__ stat, double* __restrict__ part2) {
    __shared__ double lds[(NW + 1) * 2];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    const double mean0 = stat[0 * GS + 3], mean1 = stat[1 * GS + 3];
    double s[2] = {0.0, 0.0};
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const bool g = y[i] != 0;
        const double d = x[i] - (g ? mean1 : mean0);
        s[0] += g ? 0.0 : d * d; s[1] += g ? d * d : 0.0;
    }
    const double* sum = block_sum<2>(s, lds);
    if (threadIdx.x < 2) part2[(size_t)blockIdx.x * 2 + threadIdx.x] = sum[threadIdx.x];
}

// one workgroup: part2 over the chunks in order -> std, bw, valid, norm; then the support of both groups
__global__ void __launch_bounds__(NT) kde_stats2_finish_kernel(const double* __restrict__ part2, int chunks, double* __restrict__ stat,
                                                               int G, double cut, double* __restrict__ sup) {
    __shared__ double lo[2], hi[2];
    if (threadIdx.x < 2) {
        const int g = threadIdx.x;
        double ss = 0.0;
        for (int c = 0; c < chunks; ++c) ss += part2[(size_t)c * 2 + g];
        const double cnt = stat[g * GS + 0];
        const double sd = cnt >= 2.0 ? sqrt(ss / (cnt - 1.0)) : 0.0;
        const bool valid = cnt >= 2.0 && sd > 0.0;
        const double bw = valid ? sd * pow(cnt, -0.2) : 0.0;
        stat[g * GS + 4] = sd; stat[g * GS + 5] = bw; stat[g * GS + 6] = valid ? 1.0 : 0.0;
        stat[g * GS + 7] = valid ? 1.0 / (cnt * bw * sqrt(2.0 * M_PI)) : 0.0;
        lo[g] = valid ? mul_add_2r(-cut, bw, stat[g * GS + 1]) : 0.0;
        hi[g] = valid ? mul_add_2r(cut, bw, stat[g * GS + 2]) : 0.0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * G; t += NT) {
        const int g = t / G, p = t - g * G;
        sup[t] = linspace_at(lo[g], hi[g], G, p);
    }
}

// a chunk of rows x a tile of KDE_PT support points -> part[chunk][g][point]: the kernel sum of the group's rows of the chunk
__global__ void __launch_bounds__(NT) kde_partial_kernel(const double* __restrict__ x, const unsigned char* __restrict__ y, long long n,
                                                         long long rows, const double* __restrict__ stat, const double* __restrict__ sup,
                                                         int G, double* __restrict__ part) {
    __shared__ double lds[(NW + 1) * 2 * KDE_PT];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    const int p0 = blockIdx.y * KDE_PT;
    const double ib0 = stat[0 * GS + 6] != 0.0 ? 1.0 / stat[0 * GS + 5] : 0.0;
    const double ib1 = stat[1 * GS + 6] != 0.0 ? 1.0 / stat[1 * GS + 5] : 0.0;
    double s0[KDE_PT], s1[KDE_PT], acc[2 * KDE_PT];
#pragma unroll
    for (int p = 0; p < KDE_PT; ++p) {
        const int q = p0 + p < G ? p0 + p : G - 1;        // a tile cut short repeats the last point; nothing of it is written
        s0[p] = sup[q]; s1[p] = sup[G + q];
        acc[p] = 0.0; acc[KDE_PT + p] = 0.0;
    }
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const double v = x[i];
        const bool g = y[i] != 0;
        const double ib = g ? ib1 : ib0;
#pragma unroll
        for (int p = 0; p < KDE_PT; ++p) {
            const double z = (v - (g ? s1[p] : s0[p])) * ib;
            const double e = exp(-0.5 * z * z);
            acc[p] += g ? 0.0 : e;
            acc[KDE_PT + p] += g ? e : 0.0;
        }
    }
    const double* sum = block_sum<2 * KDE_PT>(acc, lds);
    if (threadIdx.x < 2 * KDE_PT) {
        const int g = threadIdx.x / KDE_PT, p = p0 + threadIdx.x % KDE_PT;
        if (p < G) part[((size_t)blockIdx.x * 2 + g) * G + p] = sum[threadIdx.x];
    }
}

// a thread per (group, point): the partials in chunk order -> out = support[2][G], density[2][G] (unscaled: integrates to 1 per
// group), stat[2][8]; NaN support and density for a group without a curve
__global__ void __launch_bounds__(NT) kde_finish_kernel(const double* __restrict__ part, int chunks, const double* __restrict__ stat,
                                                        const double* __restrict__ sup, int G, double* __restrict__ out) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t < 2 * GS) out[4 * (size_t)G + t] = stat[t];
    if (t >= 2 * G) return;
    const int g = t / G;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * 2 * G + t];
    const bool valid = stat[g * GS + 6] != 0.0;
    const double nan = __builtin_nan("");
    out[t] = valid ? sup[t] : nan;
    out[2 * (size_t)G + t] = valid ? s * stat[g * GS + 7] : nan;
}

// ---------------------------------------------------------------- regression
// a thread per vertex: x0 = linspace(min, max, G)[v]; h = the q-th smallest |x - x0| = min_j max(x0 - xs[j], xs[j + q - 1] - x0)
// over the windows of q consecutive sorted rows.  The first term falls and the second rises with j (rounded subtraction is
// monotone), so the minimum is at the first j where the second reaches the first, or one before.
__global__ void __launch_bounds__(NT) loess_vertex_kernel(const double* __restrict__ xs, long long n, long long q, int G,
                                                          double* __restrict__ vert, double* __restrict__ hh) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= G) return;
    const double x0 = linspace_at(xs[0], xs[n - 1], G, v);
    long long lo = 0, hi = n - q + 1;                      // windows start at 0 .. n - q
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;          // <= n - q, so mid + q - 1 <= n - 1
        if (xs[mid + q - 1] - x0 >= x0 - xs[mid]) hi = mid; else lo = mid + 1;
    }
    double h = __builtin_inf();
    if (lo <= n - q) h = fmin(h, fmax(x0 - xs[lo], xs[lo + q - 1] - x0));
    if (lo >= 1) h = fmin(h, fmax(x0 - xs[lo - 1], xs[lo + q - 2] - x0));
    vert[v] = x0;
    hh[v] = h;
}

// a chunk of sorted rows x a tile of LO_PT vertices -> part[chunk][vertex][13]
__global__ void __launch_bounds__(NT) loess_partial_kernel(const double* __restrict__ xs, const unsigned char* __restrict__ ys, long long n,
                                                           long long rows, const double* __restrict__ vert, const double* __restrict__ hh,
                                                           int G, double* __restrict__ part) {
    __shared__ double lds[(NW + 1) * LO_PT * NMOM];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    const int v0 = blockIdx.y * LO_PT;
    const double xlo = xs[base], xhi = xs[end - 1];        // base < n: the grid has ceil(n / rows) chunks
    double x0[LO_PT], ih[LO_PT], acc[LO_PT * NMOM];
    bool any = false;
#pragma unroll
    for (int p = 0; p < LO_PT; ++p) {
        const int v = v0 + p < G ? v0 + p : G - 1;
        const double h = hh[v];
        x0[p] = vert[v];
        // a chunk that lies outside [x0 - h, x0 + h] has weight 0 throughout; h = 0 is a degenerate vertex
        const bool on = h > 0.0 && (xlo - x0[p]) < h && (x0[p] - xhi) < h;
        ih[p] = on ? 1.0 / h : 0.0;
        any = any || on;
#pragma unroll
        for (int k = 0; k < NMOM; ++k) acc[p * NMOM + k] = 0.0;
    }
    if (any) {
        for (long long i = base + threadIdx.x; i < end; i += NT) {
            const double x = xs[i];
            const bool y = ys[i] != 0;
#pragma unroll
            for (int p = 0; p < LO_PT; ++p) {
                const double u = (x - x0[p]) * ih[p];
                const double au = fabs(u);
                const double c = 1.0 - au * au * au;
                const double w = (au < 1.0 && ih[p] != 0.0) ? c * c * c : 0.0;
                double* a = acc + p * NMOM;
                const double w1 = w * u, w2 = w1 * u, w3 = w2 * u, w4 = w3 * u;
                a[0] += w; a[1] += w1; a[2] += w2; a[3] += w3; a[4] += w4;
                a[5] += y ? w : 0.0; a[6] += y ? w1 : 0.0; a[7] += y ? w2 : 0.0;
                const double ww = w * w, r1 = ww * u, r2 = r1 * u, r3 = r2 * u, r4 = r3 * u;
                a[8] += ww; a[9] += r1; a[10] += r2; a[11] += r3; a[12] += r4;
            }
        }
    }
    const double* sum = block_sum<LO_PT * NMOM>(acc, lds);
    if (threadIdx.x < LO_PT * NMOM) {
        const int v = v0 + threadIdx.x / NMOM, k = threadIdx.x % NMOM;
        if (v < G) part[((size_t)blockIdx.x * G + v) * NMOM + k] = sum[threadIdx.x];
    }
}

// a thread per (vertex, moment): the partials in chunk order -> mom[vertex][13]
__global__ void __launch_bounds__(NT) loess_sum_kernel(const double* __restrict__ part, int chunks, int G, double* __restrict__ mom) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= G * NMOM) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * G * NMOM + t];
    mom[t] = s;
}

// a thread per vertex: a = A^-1 e0 by cofactors, fit = a . t, l2 = a' B a, lam = a0; NaN for a degenerate vertex
__global__ void __launch_bounds__(NT) loess_solve_kernel(const double* __restrict__ mom, const double* __restrict__ hh, int G,
                                                         double* __restrict__ fit, double* __restrict__ l2, double* __restrict__ lam) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= G) return;
    const double* m = mom + (size_t)v * NMOM;
    const double* t = m + 5;
    const double* r = m + 8;
    const double c0 = m[2] * m[4] - m[3] * m[3], c1 = m[1] * m[4] - m[2] * m[3], c2 = m[1] * m[3] - m[2] * m[2];
    const double det = m[0] * c0 - m[1] * c1 + m[2] * c2;
    const bool bad = !(hh[v] > 0.0) || !(m[0] > 0.0) || fabs(det) < 1e-12 * m[0] * m[0] * m[0];
    const double nan = __builtin_nan("");
    if (bad) { fit[v] = nan; l2[v] = nan; lam[v] = nan; return; }
    const double a[3] = {c0 / det, -c1 / det, c2 / det};
    fit[v] = a[0] * t[0] + a[1] * t[1] + a[2] * t[2];
    double s = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s += a[i] * a[j] * r[i + j];
    l2[v] = s;
    lam[v] = a[0];
}

// a chunk of sorted rows -> part[chunk][2] = sum (y - z(x))^2, sum lam(x): z and lam the piecewise-linear interpolants over the
// vertices, the segment of a row the last one whose left vertex is <= x (0 .. G - 2)
__global__ void __launch_bounds__(NT) loess_resid_kernel(const double* __restrict__ xs, const unsigned char* __restrict__ ys, long long n,
                                                         long long rows, const double* __restrict__ vert, const double* __restrict__ fit,
                                                         const double* __restrict__ lam, int G, double* __restrict__ part) {
    __shared__ double sv[MAX_GRID], sf[MAX_GRID], sl[MAX_GRID];
    __shared__ double lds[(NW + 1) * 2];
    for (int t = threadIdx.x; t < G; t += NT) { sv[t] = vert[t]; sf[t] = fit[t]; sl[t] = lam[t]; }
    __syncthreads();
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    double s[2] = {0.0, 0.0};
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const double x = xs[i];
        int lo = 0, hi = G - 2;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;            // 1 .. G - 2
            if (sv[mid] <= x) lo = mid; else hi = mid - 1;
        }
        const double w = (x - sv[lo]) / (sv[lo + 1] - sv[lo]);
        const double z = sf[lo] + w * (sf[lo + 1] - sf[lo]);
        const double l = sl[lo] + w * (sl[lo + 1] - sl[lo]);
        const double res = (ys[i] != 0 ? 1.0 : 0.0) - z;
        s[0] += res * res;
        s[1] += l;
    }
    const double* sum = block_sum<2>(s, lds);
    if (threadIdx.x < 2) part[(size_t)blockIdx.x * 2 + threadIdx.x] = sum[threadIdx.x];
}

// one workgroup: the residual partials in chunk order -> tail = nu, rss, degenerate vertices, q
__global__ void __launch_bounds__(NT) loess_final_kernel(const double* __restrict__ part, int chunks, const double* __restrict__ fit, int G,
                                                         long long q, double* __restrict__ tail) {
    if (threadIdx.x == 0) {
        double rss = 0.0, nu = 0.0;
        for (int c = 0; c < chunks; ++c) { rss += part[(size_t)c * 2]; nu += part[(size_t)c * 2 + 1]; }
        int bad = 0;
        for (int v = 0; v < G; ++v) bad += fit[v] != fit[v] ? 1 : 0;
        tail[0] = nu; tail[1] = rss; tail[2] = (double)bad; tail[3] = (double)q;
    }
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

bool calib_args_ok(long long n, int G) { return n >= 1 && n <= 0x7fffffffLL && G >= 2 && G <= MAX_GRID; }

size_t sort_temp_bytes(long long n) {
    size_t b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, b, (double*)nullptr, (double*)nullptr, (unsigned char*)nullptr, (unsigned char*)nullptr,
                                    (size_t)n, 0, 64, (hipStream_t)0);
    return b;
}

size_t kde_workspace_bytes(long long n, int G) {
    if (!calib_args_ok(n, G)) return 0;
    const size_t ch = (size_t)num_chunks(n);
    return al(ch * 8 * 8) + al(ch * 2 * 8) + al(2 * GS * 8) + al((size_t)2 * G * 8) + al(ch * 2 * G * 8);
}

size_t loess_workspace_bytes(long long n, int G) {
    if (!calib_args_ok(n, G)) return 0;
    const size_t ch = (size_t)num_chunks(n);
    return al(sort_temp_bytes(n)) + al((size_t)n * 8) + al((size_t)n) + al(ch * G * NMOM * 8) + al((size_t)G * NMOM * 8) + al(ch * 2 * 8);
}

}  // namespace

extern "C" {

int64_t bq_uq_chunk_rows(int64_t n) { return n >= 1 ? (int64_t)chunk_rows((long long)n) : 0; }

size_t bq_uq_kde_workspace_bytes(int64_t n, int grid) { return kde_workspace_bytes((long long)n, grid); }

size_t bq_uq_loess_workspace_bytes(int64_t n, int grid) { return loess_workspace_bytes((long long)n, grid); }

int bq_uq_kde(bq_ctx* c, const double* d_x, const uint8_t* d_correct, int64_t n, int grid, double cut, double* d_out, void* d_ws,
              size_t ws_bytes, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_uq_kde: null context");
    if (!calib_args_ok(n, grid) || !(cut >= 0.0) || cut > 1e6)
        return fail(c, BQ_ERR_ARG, "bq_uq_kde: 1 <= n <= 2^31 - 1, 2 <= grid <= 1024 and 0 <= cut <= 1e6");
    if (!d_x || !d_correct || !d_out || !d_ws || ((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_ws & 255))
        return fail(c, BQ_ERR_ARG, "bq_uq_kde: bad argument (null pointer, x or out not 8-byte or the workspace not 256-byte aligned)");
    if (ws_bytes < kde_workspace_bytes(n, grid)) return fail(c, BQ_ERR_WORKSPACE, "bq_uq_kde: workspace below bq_uq_kde_workspace_bytes(n, grid)");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(c->device);
    ProfScope ps(c, s, "uq_kde", 30.0 * (double)n * grid, 9.0 * (double)n * (2 + (grid + KDE_PT - 1) / KDE_PT));
    const long long rows = chunk_rows(n);
    const int ch = (int)num_chunks(n);
    unsigned char* p = (unsigned char*)d_ws;
    double* part1 = (double*)p; p += al((size_t)ch * 8 * 8);
    double* part2 = (double*)p; p += al((size_t)ch * 2 * 8);
    double* stat = (double*)p; p += al(2 * GS * 8);
    double* sup = (double*)p; p += al((size_t)2 * grid * 8);
    double* part = (double*)p;
    hipLaunchKernelGGL(kde_stats1_kernel, dim3(ch), dim3(NT), 0, s, d_x, d_correct, (long long)n, rows, part1);
    hipLaunchKernelGGL(kde_stats1_finish_kernel, dim3(1), dim3(NT), 0, s, part1, ch, stat);
    hipLaunchKernelGGL(kde_stats2_kernel, dim3(ch), dim3(NT), 0, s, d_x, d_correct, (long long)n, rows, stat, part2);
    hipLaunchKernelGGL(kde_stats2_finish_kernel, dim3(1), dim3(NT), 0, s, part2, ch, stat, grid, cut, sup);
    hipLaunchKernelGGL(kde_partial_kernel, dim3(ch, (grid + KDE_PT - 1) / KDE_PT), dim3(NT), 0, s, d_x, d_correct, (long long)n, rows, stat,
                       sup, grid, part);
    hipLaunchKernelGGL(kde_finish_kernel, dim3((2 * grid + NT - 1) / NT), dim3(NT), 0, s, part, ch, stat, sup, grid, d_out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bq_uq_loess(bq_ctx* c, const double* d_x, const uint8_t* d_correct, int64_t n, int grid, double span, double* d_out, void* d_ws,
                size_t ws_bytes, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_uq_loess: null context");
    if (!calib_args_ok(n, grid) || !(span > 0.0))
        return fail(c, BQ_ERR_ARG, "bq_uq_loess: 1 <= n <= 2^31 - 1, 2 <= grid <= 1024 and span > 0");
    const long long q = (long long)floor(span * (double)n + 1e-5);
    if (q < 1 || q > n) return fail(c, BQ_ERR_ARG, "bq_uq_loess: the span's window, floor(span n + 1e-5) rows, must hold 1 .. n rows");
    if (!d_x || !d_correct || !d_out || !d_ws || ((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_ws & 255))
        return fail(c, BQ_ERR_ARG, "bq_uq_loess: bad argument (null pointer, x or out not 8-byte or the workspace not 256-byte aligned)");
    if (ws_bytes < loess_workspace_bytes(n, grid)) return fail(c, BQ_ERR_WORKSPACE, "bq_uq_loess: workspace below bq_uq_loess_workspace_bytes(n, grid)");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(c->device);
    ProfScope ps(c, s, "uq_loess", 45.0 * (double)n * grid, 9.0 * (double)n * (4 + (grid + LO_PT - 1) / LO_PT));
    const long long rows = chunk_rows(n);
    const int ch = (int)num_chunks(n);
    size_t sort_b = sort_temp_bytes(n);
    unsigned char* p = (unsigned char*)d_ws;
    void* d_tmp = p; p += al(sort_b);
    double* xs = (double*)p; p += al((size_t)n * 8);
    unsigned char* ys = p; p += al((size_t)n);
    double* part = (double*)p; p += al((size_t)ch * grid * NMOM * 8);
    double* mom = (double*)p; p += al((size_t)grid * NMOM * 8);
    double* rpart = (double*)p;
    double* vert = d_out, *fit = d_out + grid, *l2 = d_out + 2 * (size_t)grid, *lam = d_out + 3 * (size_t)grid, *hh = d_out + 4 * (size_t)grid;
    double* tail = d_out + 5 * (size_t)grid;
    HIPCHK(c, rocprim::radix_sort_pairs(d_tmp, sort_b, d_x, xs, d_correct, ys, (size_t)n, 0, 64, s));
    const int vb = (grid + NT - 1) / NT;
    hipLaunchKernelGGL(loess_vertex_kernel, dim3(vb), dim3(NT), 0, s, xs, (long long)n, q, grid, vert, hh);
    hipLaunchKernelGGL(loess_partial_kernel, dim3(ch, (grid + LO_PT - 1) / LO_PT), dim3(NT), 0, s, xs, ys, (long long)n, rows, vert, hh, grid,
                       part);
    hipLaunchKernelGGL(loess_sum_kernel, dim3((grid * NMOM + NT - 1) / NT), dim3(NT), 0, s, part, ch, grid, mom);
    hipLaunchKernelGGL(loess_solve_kernel, dim3(vb), dim3(NT), 0, s, mom, hh, grid, fit, l2, lam);
    hipLaunchKernelGGL(loess_resid_kernel, dim3(ch), dim3(NT), 0, s, xs, ys, (long long)n, rows, vert, fit, lam, grid, rpart);
    hipLaunchKernelGGL(loess_final_kernel, dim3(1), dim3(NT), 0, s, rpart, ch, fit, grid, q, tail);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
