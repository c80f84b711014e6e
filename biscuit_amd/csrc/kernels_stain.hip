// Macenko stain normalisation (Slideflow's `normalizer='macenko'`; Macenko et al. 2009 in the numpy form of HEnorm_python),
// in front of the staging kernel where `reinhard_fast` sits (results.py:251-252 `wsi_normalizer.rgb_to_rgb`).  DESIGN.md
// "Macenko" states the spec; tests/_macenko_ref.py restates it in float64 numpy.  Unpinned like reinhard_fast: the
// constants below are recalled, not read from Slideflow, and live here and in biscuit_amd/stain.py (MACENKO_*) only.
//
// One workgroup of 1 024 threads per tile; every pass re-reads the 268 KB tile from cache, one pixel per thread and step:
//   1. statistics: OD = -ln((I + 1) / Io) from a 256-entry float64 table in LDS; a pixel is tissue when none of its three OD
//      values is < beta; n, sum x and sum x x^T over tissue pixels in float64, per thread in a fixed pixel map, then a fixed
//      shuffle + LDS tree: bit-reproducible
//   2. one lane: the covariance (divided by n - 1), its 3x3 eigenproblem by cyclic Jacobi in float64, E = the eigenvectors of
//      the middle and the largest eigenvalue, each column's entry of largest magnitude made positive
//   3. exact order statistics of phi = atan2(OD.E1, OD.E0) over tissue pixels: the (floor(v))-th and next of v = 0.01 (n-1)
//      and v = 0.99 (n-1) (numpy's 'linear' percentile), by a radix select (radix_select.h, shared with kernels_reinhard.hip) over the order-preserving 32-bit key of the float32
//      angle -- one pass over a monotone 2 048-bin coarse histogram of the value, then 11 + 11 + 10 key bits restricted to the
//      chosen coarse bin (so LDS atomics only collide inside it), then one pass for the successor when it is a different value
//   4. one lane: numpy's _lerp in float64, vMin / vMax, HE (H first), det(HE^T HE), pinv(HE) = (HE^T HE)^-1 HE^T in float64
//   5. the same select for the 99th percentiles of C = pinv(HE) OD over ALL pixels (both rows at once)
//   6. transform: C2 = C * maxCRef / maxC, Inorm = Io exp(-HERef C2), Inorm > 255 -> 254, truncated to uint8
// Precision contract: float64 for the OD table, the statistics, the eigenproblem, the percentile interpolation, HE and pinv;
// float32 per pixel (the angle, the concentrations, the transform).  The order statistics are exact over the float32 values,
// so a percentile differs from the float64 reference by the float32 rounding of its two neighbours at most.
// Degenerate tiles: status 1 = n_tissue < 2, 2 = |det(HE^T HE)| < 1e-12, 3 = a maxC <= 0 or a non-finite
// intermediate; such a tile passes through unchanged (copied when dst != src).  dst may equal src: every pixel is read and
// written by one thread in the last pass, after every read of the others.
#include "bq_ctx.h"
#include "radix_select.h"

#include <cmath>

namespace {

// ---- the spec's constants (unpinned; mirrored in biscuit_amd/stain.py) ----
constexpr double MK_IO = 255.0;            // transmitted light intensity
constexpr double MK_ALPHA = 1.0;           // percentile of the extreme angles
constexpr double MK_BETA = 0.15;           // OD threshold of a tissue pixel
constexpr double MK_CONC_PCT = 99.0;       // percentile of the concentrations
constexpr float MK_OVER = 255.f;           // HEnorm_python's quirk: Inorm > 255 becomes 254
constexpr float MK_OVER_TO = 254.f;
constexpr double MK_DET_MIN = 1e-12;       // |det(HE^T HE)| below this: status 2

constexpr int MK_NT = RS_NT;               // the workgroup of the shared radix select (radix_select.h)
constexpr int MK_NW = RS_NW;
constexpr int MK_BINS = RS_BINS;

struct MacenkoRef {
    float he[6];      // HERef, row-major 3x2 (columns H, E)
    float maxc[2];    // maxCRef
};

struct MkShared {
    double od64[256];
    float od32[256];
    unsigned char tis[256];
    RadixSel sel;                          // the order statistics of steps 3 and 5 (radix_select.h)
    double red[10][MK_NW];
    float e[6];                            // E row-major 3x2, float32 (angle pass)
    float p[6];                            // pinv(HE) row-major 2x3, float32 (concentrations)
    float scale[2];                        // maxCRef / maxC
    double he[6], maxc[2];
    int status, ntissue;
};

// Cyclic Jacobi on a symmetric 3x3 matrix (float64): a is diagonalised in place, v gets the eigenvectors as columns.
__device__ void mk_jacobi3(double a[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-36 * dia)) break;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (a[p][q] == 0.0) continue;
            const double th = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
            const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            // a <- J^T a J, v <- v J with J = I except J[p][p] = J[q][q] = c, J[p][q] = s, J[q][p] = -s
            for (int k = 0; k < 3; ++k) {
                const double akp = a[k][p], akq = a[k][q];
                a[k][p] = c * akp - s * akq;
                a[k][q] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = a[p][k], aqk = a[q][k];
                a[p][k] = c * apk - s * aqk;
                a[q][k] = s * apk + c * aqk;
            }
            a[p][q] = a[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - s * vkq;
                v[k][q] = s * vkp + c * vkq;
            }
        }
    }
}

__device__ __forceinline__ void mk_read(const uint8_t* src, int i, int& r, int& g, int& b) {
    r = src[3 * i]; g = src[3 * i + 1]; b = src[3 * i + 2];
}

__global__ void __launch_bounds__(MK_NT) macenko_kernel(const uint8_t* tiles, int px, const MacenkoRef ref, uint8_t* dst,
                                                        float* __restrict__ stats8, int* __restrict__ st, int st_stride) {
    const int npix = px * px;
    const uint8_t* src = tiles + (size_t)blockIdx.x * npix * 3;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    __shared__ MkShared sh;
    for (int i = tid; i < 256; i += MK_NT) {
        const double od = -log(((double)i + 1.0) / MK_IO);
        sh.od64[i] = od;
        sh.od32[i] = (float)od;
        sh.tis[i] = od < MK_BETA ? 0 : 1;
    }
    __syncthreads();

    // ---- 1. statistics of the tissue pixels
    {
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int cnt = 0;
        for (int i = tid; i < npix; i += MK_NT) {
            int r, g, b;
            mk_read(src, i, r, g, b);
            if (sh.tis[r] & sh.tis[g] & sh.tis[b]) {
                const double x = sh.od64[r], y = sh.od64[g], z = sh.od64[b];
                ++cnt;
                s[0] += x; s[1] += y; s[2] += z;
                s[3] += x * x; s[4] += x * y; s[5] += x * z; s[6] += y * y; s[7] += y * z; s[8] += z * z;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
            if (lane == 0) sh.red[q][wid] = s[q];
        }
        if (lane == 0) sh.red[9][wid] = (double)cnt;
    }
    __syncthreads();

    // ---- 2. covariance and its eigenproblem (one lane)
    if (tid == 0) {
        double s[10];
        for (int q = 0; q < 10; ++q) {
            double a = 0;
            for (int w = 0; w < MK_NW; ++w) a += sh.red[q][w];
            s[q] = a;
        }
        const int n = (int)s[9];
        for (int i = 0; i < 6; ++i) sh.he[i] = __builtin_nan("");
        sh.maxc[0] = sh.maxc[1] = __builtin_nan("");
        sh.ntissue = n;
        sh.status = n < 2 ? 1 : 0;
        if (n >= 2) {
            const double dn = (double)n, mu[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
            const int ix[3][3] = {{3, 4, 5}, {4, 6, 7}, {5, 7, 8}};
            double a[3][3], v[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) a[i][j] = (s[ix[i][j]] - dn * mu[i] * mu[j]) / (dn - 1.0);
            mk_jacobi3(a, v);
            // ascending order of the eigenvalues: E = (middle, largest)
            int o[3] = {0, 1, 2};
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2 - i; ++j)
                    if (a[o[j]][o[j]] > a[o[j + 1]][o[j + 1]]) { const int tmp = o[j]; o[j] = o[j + 1]; o[j + 1] = tmp; }
            bool fin = true;
            for (int c = 0; c < 2; ++c) {
                const int col = o[c + 1];
                int big = 0;
                for (int i = 1; i < 3; ++i)
                    if (fabs(v[i][col]) > fabs(v[big][col])) big = i;
                const double sg = v[big][col] < 0 ? -1.0 : 1.0;
                for (int i = 0; i < 3; ++i) {
                    const double e = sg * v[i][col];
                    fin = fin && isfinite(e);
                    sh.he[2 * i + c] = e;                 // E, float64, until step 4 replaces it with HE
                    sh.e[2 * i + c] = (float)e;
                }
            }
            if (!fin) sh.status = 3;
            const double vi = (dn - 1.0) * (MK_ALPHA / 100.0), vj = (dn - 1.0) * ((100.0 - MK_ALPHA) / 100.0);
            sh.sel.rank[0] = (unsigned)floor(vi);
            sh.sel.rank[1] = (unsigned)floor(vj);
        }
        sh.sel.coff = 3.14159265f;
        sh.sel.cscl = (float)(MK_BINS / (2.0 * 3.14159265358979323846));
    }
    __syncthreads();
    const unsigned ntis = (unsigned)sh.ntissue;

    // ---- 3. the two extreme angles
    if (sh.status == 0) {
        const float e00 = sh.e[0], e01 = sh.e[1], e10 = sh.e[2], e11 = sh.e[3], e20 = sh.e[4], e21 = sh.e[5];
        rs_select(sh.sel, npix, [&](int i, float v[2], bool ok[2]) {
            int r, g, b;
            mk_read(src, i, r, g, b);
            const bool t = sh.tis[r] & sh.tis[g] & sh.tis[b];
            const float x = sh.od32[r], y = sh.od32[g], z = sh.od32[b];
            const float p0 = x * e00 + y * e10 + z * e20, p1 = x * e01 + y * e11 + z * e21;
            v[0] = v[1] = atan2f(p1, p0);
            ok[0] = ok[1] = t;
        });
        // ---- 4. HE and pinv(HE) (one lane)
        if (tid == 0) {
            const double n1 = (double)ntis - 1.0;
            const double vi[2] = {n1 * (MK_ALPHA / 100.0), n1 * ((100.0 - MK_ALPHA) / 100.0)};
            double ph[2];
            for (int t = 0; t < 2; ++t)
                ph[t] = rs_lerp((double)rs_unkey(sh.sel.key[t]), (double)rs_unkey(sh.sel.succ[t]), vi[t] - floor(vi[t]));
            double vmin[3], vmax[3];
            const double c0 = cos(ph[0]), s0 = sin(ph[0]), c1 = cos(ph[1]), s1 = sin(ph[1]);
            for (int i = 0; i < 3; ++i) {
                vmin[i] = sh.he[2 * i] * c0 + sh.he[2 * i + 1] * s0;
                vmax[i] = sh.he[2 * i] * c1 + sh.he[2 * i + 1] * s1;
            }
            const bool minfirst = vmin[0] > vmax[0];
            double he[3][2];
            for (int i = 0; i < 3; ++i) {
                he[i][0] = minfirst ? vmin[i] : vmax[i];
                he[i][1] = minfirst ? vmax[i] : vmin[i];
                sh.he[2 * i] = he[i][0];
                sh.he[2 * i + 1] = he[i][1];
            }
            double m00 = 0, m01 = 0, m11 = 0;
            for (int i = 0; i < 3; ++i) {
                m00 += he[i][0] * he[i][0];
                m01 += he[i][0] * he[i][1];
                m11 += he[i][1] * he[i][1];
            }
            const double det = m00 * m11 - m01 * m01;
            bool fin = isfinite(det);
            if (fabs(det) < MK_DET_MIN) {
                sh.status = 2;
            } else {
                for (int i = 0; i < 3; ++i) {
                    const double p0 = (m11 * he[i][0] - m01 * he[i][1]) / det;
                    const double p1 = (m00 * he[i][1] - m01 * he[i][0]) / det;
                    fin = fin && isfinite(p0) && isfinite(p1);
                    sh.p[i] = (float)p0;
                    sh.p[3 + i] = (float)p1;
                }
                if (!fin) sh.status = 3;
            }
            const double vc = (double)(npix - 1) * (MK_CONC_PCT / 100.0);
            sh.sel.rank[0] = sh.sel.rank[1] = (unsigned)floor(vc);
            sh.sel.coff = 8.f;                                    // concentrations: 1/128 bins over [-8, 8)
            sh.sel.cscl = 128.f;
        }
        __syncthreads();
    }

    // ---- 5. the 99th percentiles of the concentrations over all pixels
    if (sh.status == 0) {
        const float p00 = sh.p[0], p01 = sh.p[1], p02 = sh.p[2], p10 = sh.p[3], p11 = sh.p[4], p12 = sh.p[5];
        rs_select(sh.sel, npix, [&](int i, float v[2], bool ok[2]) {
            int r, g, b;
            mk_read(src, i, r, g, b);
            const float x = sh.od32[r], y = sh.od32[g], z = sh.od32[b];
            v[0] = p00 * x + p01 * y + p02 * z;
            v[1] = p10 * x + p11 * y + p12 * z;
            ok[0] = ok[1] = true;
        });
        if (tid == 0) {
            const double vc = (double)(npix - 1) * (MK_CONC_PCT / 100.0), g = vc - floor(vc);
            for (int t = 0; t < 2; ++t) {
                const double m = rs_lerp((double)rs_unkey(sh.sel.key[t]), (double)rs_unkey(sh.sel.succ[t]), g);
                sh.maxc[t] = m;
                if (!(m > 0.0) || !isfinite(m)) sh.status = 3;
                const double sc = (double)ref.maxc[t] / m;
                sh.scale[t] = (float)sc;
                if (!isfinite(sc)) sh.status = 3;
            }
        }
        __syncthreads();
    }

    if (tid == 0) {
        const int status = sh.status;
        if (stats8) {
            float* o = stats8 + (size_t)blockIdx.x * 8;
            for (int i = 0; i < 6; ++i) o[i] = (float)sh.he[i];          // NaN where a degenerate tile stopped before
            for (int t = 0; t < 2; ++t) o[6 + t] = (float)sh.maxc[t];
        }
        if (st) {
            st[(size_t)blockIdx.x * st_stride] = status;
            if (st_stride > 1) st[(size_t)blockIdx.x * st_stride + 1] = sh.ntissue;
        }
    }
    if (!dst) return;

    // ---- 6. transform (or pass-through)
    uint8_t* out = dst + (size_t)blockIdx.x * npix * 3;
    if (sh.status != 0) {
        if (out != src)
            for (int i = tid; i < 3 * npix; i += MK_NT) out[i] = src[i];
        return;
    }
    const float s0 = sh.scale[0], s1 = sh.scale[1];
    const float p00 = sh.p[0], p01 = sh.p[1], p02 = sh.p[2], p10 = sh.p[3], p11 = sh.p[4], p12 = sh.p[5];
    for (int i = tid; i < npix; i += MK_NT) {
        int r, g, b;
        mk_read(src, i, r, g, b);
        const float x = sh.od32[r], y = sh.od32[g], z = sh.od32[b];
        const float c0 = (p00 * x + p01 * y + p02 * z) * s0;
        const float c1 = (p10 * x + p11 * y + p12 * z) * s1;
        uint8_t o[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float v = (float)MK_IO * expf(-(ref.he[2 * ch] * c0 + ref.he[2 * ch + 1] * c1));
            v = v > MK_OVER ? MK_OVER_TO : v;
            o[ch] = (uint8_t)(v > 0.f ? (int)v : 0);           // truncation (v is in (0, 255] for a finite fit)
        }
        out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
    }
}

}  // namespace

static int launch_macenko(const uint8_t* tiles, int n, int px, const float* he_ref6, const float* maxc_ref2, uint8_t* dst,
                          float* d_stats8, int* d_status, int status_stride, hipStream_t s) {
    if (n <= 0) return 0;
    MacenkoRef ref;
    for (int i = 0; i < 6; ++i) ref.he[i] = he_ref6 ? he_ref6[i] : 0.f;
    for (int i = 0; i < 2; ++i) ref.maxc[i] = maxc_ref2 ? maxc_ref2[i] : 1.f;
    hipLaunchKernelGGL(macenko_kernel, dim3(n), dim3(MK_NT), 0, s, tiles, px, ref, dst, d_stats8, d_status, status_stride);
    return (int)hipGetLastError();
}

extern "C" {

int bq_stain_macenko(bq_ctx* c, const uint8_t* d_tiles, int n, const float* he_ref6, const float* maxc_ref2,
                     uint8_t* d_out, int* d_status, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || !he_ref6 || !maxc_ref2 || n < 0)
        return fail(c, BQ_ERR_ARG, "bq_stain_macenko: bad argument");
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(he_ref6[i])) return fail(c, BQ_ERR_ARG, "bq_stain_macenko: non-finite stain matrix");
    for (int i = 0; i < 2; ++i)
        if (!std::isfinite(maxc_ref2[i]) || !(maxc_ref2[i] > 0.f))
            return fail(c, BQ_ERR_ARG, "bq_stain_macenko: target concentrations must be finite and > 0");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_macenko", 400.0 * n * 299 * 299, 3.0 * n * kStaged);
    if (launch_macenko(d_tiles, n, 299, he_ref6, maxc_ref2, d_out, nullptr, d_status, 1, s))
        return fail(c, BQ_ERR_HIP, "macenko launch failed");
    return BQ_OK;
}

int bq_stain_macenko_stats(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_stats8, int* d_status2, bq_stream_t stream) {
    if (!c || !d_tiles || !d_stats8 || n < 0) return fail(c, BQ_ERR_ARG, "bq_stain_macenko_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_macenko_stats", 350.0 * n * 299 * 299, 1.0 * n * kStaged);
    if (launch_macenko(d_tiles, n, 299, nullptr, nullptr, nullptr, d_stats8, d_status2, 2, s))
        return fail(c, BQ_ERR_HIP, "macenko stats launch failed");
    return BQ_OK;
}

}  // extern "C"
