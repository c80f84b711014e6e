// The feature map (DESIGN.md "Feature map (Figure 6)"), stated once for the host and the device in the pattern of roi_device.h and
// resample_device.h: the per-row arithmetic below is compiled into libbiscuit_io.so (umap_host.cpp: bqio_knn, bqio_umap_smooth,
// bqio_umap_epoch -- the CPU build the tests run) and into kernels_knn.hip / kernels_umap.hip (bq_knn, bq_umap_smooth,
// bq_umap_epoch).  UMAP is restated from memory: unpinned against umap-learn, pinned to tests/_umap_ref.py.
//
// Everything here is fp32 without fused multiply-adds, so that the host build and the kernels round alike wherever they call no
// transcendental function (expf, powf differ between libm and the device library by a few ulp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQU_HD __host__ __device__ inline
#else
#define BQU_HD inline
#endif
#if defined(__clang__)
#define BQU_NO_FMA _Pragma("clang fp contract(off)")
#elif defined(__FP_FAST_FMAF) && !defined(BQK_CONTRACT_OFF)
#error "this target has a fused multiply-add: compile with -ffp-contract=off -DBQK_CONTRACT_OFF"
#else
#define BQU_NO_FMA
#endif

namespace bqumap {

constexpr int K_MAX = 64;                  // neighbours of a row
constexpr int K_SLACK = 16;                // a candidate list keeps k + K_SLACK rows (kernels_knn.hip)
constexpr int SQ_LANES = 64;               // partial sums of the direct form: element e goes to partial e % 64
constexpr int NEG_RATE = 5;                // negative samples of an edge that is due
constexpr float CLIP = 4.f;

// (distance, index) ascending: the order of a row of the table, a strict total order on distinct indices
BQU_HD bool before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// ---- the direct form sum (x - y)^2 --------------------------------------------------------------------------------------
// 64 partial sums, partial p taking the elements p, p + 64, ... in order; then ((p0 + p1) + (p2 + p3)) for each group of four
// and a balanced tree over the 16 groups (g with g ^ 8, then ^ 4, ^ 2, ^ 1): the order a 16-lane group of the kernel takes with
// one float4 per lane and step, so the bits do not depend on who computes them.  D is a multiple of 16.
BQU_HD float sq_term(float acc, float x, float y) {
    BQU_NO_FMA
    const float d = x - y;
    const float q = d * d;
    return acc + q;
}

BQU_HD float sq_fold4(float a0, float a1, float a2, float a3) {
    BQU_NO_FMA
    const float l = a0 + a1, r = a2 + a3;
    return l + r;
}

inline float sqdist_host(const float* x, const float* y, int D) {
    float p[SQ_LANES];
    for (int j = 0; j < SQ_LANES; ++j) p[j] = 0.f;
    for (int e0 = 0; e0 < D; e0 += SQ_LANES) {
        const int m = D - e0 < SQ_LANES ? D - e0 : SQ_LANES;
        for (int j = 0; j < m; ++j) p[j] = sq_term(p[j], x[e0 + j], y[e0 + j]);
    }
    float g[16];
    for (int l = 0; l < 16; ++l) g[l] = sq_fold4(p[4 * l], p[4 * l + 1], p[4 * l + 2], p[4 * l + 3]);
    for (int s = 8; s >= 1; s >>= 1) {
        float t[16];
        for (int l = 0; l < 16; ++l) t[l] = g[l] + g[l ^ s];
        for (int l = 0; l < 16; ++l) g[l] = t[l];
    }
    return g[0];
}

// ---- the GEMM form's error (DESIGN.md "Neighbours": the derivation) -------------------------------------------------------
// nq, nc: the fp32 sums of squares of two rows of D columns, v = fl(fl(nq + nc) - 2 fl(q.c)), every sum in ANY order, fused or
// not.  With u = 2^-24, gamma_m = m u / (1 - m u) and S = |q|^2 + |c|^2 exactly: |nq + nc - S| <= gamma_D S, the dot product is
// off by gamma_D sum |q_i c_i| <= gamma_D S / 2 (doubled: gamma_D S), the two outer roundings add u S (1 + gamma_D) and
// u |v| <= 2 u S (1 + ...), so |v - d^2| <= gamma_(2D + 4) S; 4 u S more pay for rounding v - E itself.  S is not known, only
// nq + nc >= S (1 - gamma_D): with g = (2 D + 8) u the coefficient g / (1 - g)^2 >= gamma_(2D + 8) / (1 - gamma_D), times
// 1 + 2^-18 for the three roundings of E's own arithmetic; 1e-30 covers products that underflow (2 D 2^-126 at most).
// Valid while nothing overflows: a value that is not finite certifies nothing (kernels_knn.hip).
BQU_HD float gemm_err_coeff(int D) {
    const double g = (2.0 * (double)D + 8.0) * 5.9604644775390625e-08;      // (D <= 2^20: g <= 0.126)
    return (float)(g / ((1.0 - g) * (1.0 - g)) * (1.0 + 3.814697265625e-06) * (1.0 + 1.1920928955078125e-07));      // (and the cast's own rounding)
}

BQU_HD float gemm_err_with(float nq, float nc, float coeff) {
    BQU_NO_FMA
    return (nq + nc) * coeff + 1e-30f;
}

// E(nq, nc, D) >= |GEMM-form value - exact d^2|
BQU_HD float gemm_form_err(float nq, float nc, int D) { return gemm_err_with(nq, nc, gemm_err_coeff(D)); }

// The k-th direct-form d2 of a row against the smallest lower bound `floor_` = min (v - E) of the rows that were NOT looked at
// again: true only where every such row's rounded distance lies STRICTLY above the k-th's, so the (distance, index) order cannot
// put it into the table.  The direct form is off by relative gamma_(D + 2) <= eps_for(D) / 2 (plus D 2^-149 where squares
// underflow), and two fp32 roots differ as soon as their squares differ by a factor 1 + 8 u: (2 D + 12) u covers both, in double.
BQU_HD bool knn_certified(float d2_kth, float floor_, int D) {
    const double thr = (double)d2_kth * (1.0 + (2.0 * (double)D + 12.0) * 5.9604644775390625e-08) + 1e-30;
    return thr < (double)floor_;      // (a NaN on either side: not certified)
}

// ---- Philox4x32-10 (oracle/philox.py), for both sides ---------------------------------------------------------------------
BQU_HD uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// ---- the fuzzy graph's row: rho, sigma and the weights ---------------------------------------------------------------------
// d[k]: the row's distances ascending, idx[k] its neighbours, `self` the row's own index.  Local connectivity 1, bandwidth 1:
// rho = the smallest non-zero distance (0 when there is none); sigma by the 64-step bisection for
// sum_{j >= 1} exp(-max(0, d_j - rho) / sigma) = log2(k) (lo 0, hi infinite, mid 1, doubling while hi is infinite, stop at
// |delta| < 1e-5); floored at 1e-3 x the row's mean distance, or 1e-3 x global_mean where rho = 0.  w[j] = 0 for the row
// itself, 1 where d_j - rho <= 0, else exp(-(d_j - rho) / sigma).
BQU_HD void smooth_row(const float* d, const int* idx, int k, int self, float global_mean, float* rho_out, float* sigma_out, float* w) {
    BQU_NO_FMA
    float rho = 0.f, sum_d = 0.f;
    bool found = false;
    for (int j = 0; j < k; ++j) {
        sum_d += d[j];
        if (!found && d[j] > 0.f) { rho = d[j]; found = true; }
    }
    const float target = log2f((float)k);
    float lo = 0.f, hi = INFINITY, mid = 1.f;
    for (int it = 0; it < 64; ++it) {
        float psum = 0.f;
        for (int j = 1; j < k; ++j) {
            const float t = d[j] - rho;
            psum += t > 0.f ? expf(-(t / mid)) : 1.f;
        }
        if (fabsf(psum - target) < 1e-5f) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) * 0.5f;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.f : (lo + hi) * 0.5f;
        }
    }
    const float floor_at = 1e-3f * (rho > 0.f ? sum_d / (float)k : global_mean);
    const float sigma = mid < floor_at ? floor_at : mid;
    *rho_out = rho;
    *sigma_out = sigma;
    for (int j = 0; j < k; ++j) {
        const float t = d[j] - rho;
        w[j] = idx[j] == self ? 0.f : (t <= 0.f ? 1.f : expf(-(t / sigma)));
    }
}

// ---- one epoch of the layout for one vertex (gather form) -----------------------------------------------------------------
BQU_HD float clip4(float v) { return v > CLIP ? CLIP : (v < -CLIP ? -CLIP : v); }

// Vertex i of n: its row of the symmetric CSR is nbr / eps / next [row_len] (neighbours ascending, epochs per sample, the epoch
// of the next sample -- advanced here).  prev: every vertex's position after the previous epoch, float [n][2]; the vertex's own
// new position is returned in out[2].  For every edge that is due (next <= epoch) in the row's order: the attractive step towards
// the neighbour, then NEG_RATE repulsive steps away from vertices drawn by Philox (key seed; counter epoch, vertex, slot, draw);
// each step moves the running position, every other position is the previous epoch's.
BQU_HD void epoch_vertex(const float* prev, int n, int i, const int* nbr, const float* eps, float* next, int row_len, int epoch, float alpha,
                         float a, float b, uint32_t seed_lo, uint32_t seed_hi, float* out) {
    BQU_NO_FMA
    float cx = prev[2 * (size_t)i], cy = prev[2 * (size_t)i + 1];
    for (int s = 0; s < row_len; ++s) {
        if (!(next[s] <= (float)epoch)) continue;
        {
            const int j = nbr[s];
            const float dx = cx - prev[2 * (size_t)j], dy = cy - prev[2 * (size_t)j + 1];
            const float d2 = dx * dx + dy * dy;
            float g = 0.f;
            if (d2 > 0.f) g = (-2.f * a * b * powf(d2, b - 1.f)) / (a * powf(d2, b) + 1.f);
            cx += clip4(g * dx) * alpha;
            cy += clip4(g * dy) * alpha;
        }
        next[s] += eps[s];
        for (int p = 0; p < NEG_RATE; ++p) {
            const int j = (int)(philox_word0((uint32_t)epoch, (uint32_t)i, (uint32_t)s, (uint32_t)p, seed_lo, seed_hi) % (uint32_t)n);
            if (j == i) continue;
            const float dx = cx - prev[2 * (size_t)j], dy = cy - prev[2 * (size_t)j + 1];
            const float d2 = dx * dx + dy * dy;
            float gx = CLIP, gy = CLIP;
            if (d2 > 0.f) {
                const float g = (2.f * b) / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
                gx = clip4(g * dx);
                gy = clip4(g * dy);
            }
            cx += gx * alpha;
            cy += gy * alpha;
        }
    }
    out[0] = cx;
    out[1] = cy;
}

// ---- what both entries check --------------------------------------------------------------------------------------------
inline const char* check_knn(long long n, int D, int k) {
    if (n < 1 || n > 0x7fffffffLL / (2 * (K_MAX + K_SLACK))) return "n outside 1 .. 2^31 / 160";
    if (D < 16 || D % 16 || D > (1 << 20)) return "D must be a multiple of 16 in 16 .. 2^20";
    if (k < 1 || k > K_MAX) return "k outside 1 .. 64";
    if (k > n) return "k exceeds n";
    return nullptr;
}

}  // namespace bqumap
