// K0 (optional front half): Reinhard-fast stain normalisation, from its tables and constants to its entry points.
// hp.py:19 normalizer='reinhard_fast', applied to the uint8 tile before the standardisation
// (results.py:251-256).  One workgroup per tile: pass 1 converts every pixel to CIE-LAB and reduces
// the six channel statistics in float64 (fixed thread map and tree: bit-reproducible); pass 2
// re-reads the (L2-resident) tile, converts again, applies (lab - mu) * (target_std / sd) + target_mean,
// converts back and stores uint8.  The precision contract (float64 for cbrt / pow / the statistics,
// one float32 rounding per other operation, no FMA contraction) is written out in oracle/stain.py;
// it makes the uint8 result comparable bit for bit.  The rest of Slideflow's Reinhard family (`reinhard`, `reinhard_mask`,
// `reinhard_fast_mask`: a brightness standardisation in front and / or a tissue mask) is reinhard_family_kernel below, on the same
// device helpers ("Reinhard family").
#include "bq_ctx.h"
#include "radix_select.h"

#include <cmath>
#include <string.h>

namespace {
// float32 colour constants of the Reinhard normaliser: XYZ<-RGB, RGB<-XYZ (its float64 inverse rounded),
// D65 white (oracle/stain.py: constants())
const float kReinhardConsts[21] = {
    0.412452996f, 0.357580006f, 0.180423006f, 0.212670997f, 0.715160012f, 0.0721689984f, 0.0193339996f,
    0.119193003f, 0.950227022f,
    3.24048138f, -1.53715158f, -0.498536319f, -0.969254971f, 1.87599003f, 0.0415559262f, 0.0556466393f,
    -0.204041332f, 1.05731106f,
    0.950469971f, 1.0f, 1.08882999f};
}  // namespace

// The tables of the Reinhard normaliser (oracle/stain.py states the same arithmetic), built once per context:
// [0,256)   sRGB -> linear, float64 evaluation rounded to float32
// [256,511) linear -> 8-bit sRGB as 255 switching points: entry v-1 is the smallest float32 c for which
//           clip(trunc(255 * clip(gamma(c), 0, 1)), 0, 255) >= v, gamma(c) = c > 0.0031308 ?
//           1.055f * float(pow(double(c), 1/2.4)) - 0.055f : 12.92f * c, found by bisection on the
//           float bit pattern over [0, 2] (the function is monotone).  Not over [0, 1]: 1.055f * 1 - 0.055f rounds to the
//           float below 1, so c = 1 is level 254 and the last point lies a few ulps ABOVE 1 (oracle/stain.py
//           srgb_switch_points states the same search)
bool reinhard_tables(float** d_lut) {
    float lut[512];
    for (int v = 0; v < 256; ++v) {
        const double x = (double)v / 255.0;
        lut[v] = (float)(x > 0.04045 ? std::pow((x + 0.055) / 1.055, 2.4) : x / 12.92);
    }
    auto level = [](float cf) {
        float g;
        if (cf > 0.0031308f) { const float p = (float)std::pow((double)cf, 1.0 / 2.4); g = 1.055f * p - 0.055f; }
        else g = cf * 12.92f;
        g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
        const float t = truncf(g * 255.0f);
        return (int)(t < 0.f ? 0.f : (t > 255.f ? 255.f : t));
    };
    for (int v = 1; v <= 255; ++v) {
        uint32_t lo = 0, hi = 0x40000000u;               // bit patterns of 0.0f and 2.0f; level(2.0f) = 255
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float f;
            memcpy(&f, &mid, 4);
            if (level(f) >= v) hi = mid; else lo = mid + 1;
        }
        memcpy(&lut[256 + v - 1], &lo, 4);
    }
    lut[511] = 0.f;
    return hipMalloc(d_lut, sizeof lut) == hipSuccess && hipMemcpy(*d_lut, lut, sizeof lut, hipMemcpyHostToDevice) == hipSuccess;
}

// ---- the kernel ----
namespace {

struct ReinhardConst {
    float m[9];        // XYZ from linear RGB
    float minv[9];     // linear RGB from XYZ
    float white[3];
    float rwhite[3];   // RN(1 / white): see divc
    float tgt_mean[3];
    float tgt_std[3];
};

struct Lab { float L, a, b; };

// x / c for a constant c, correctly rounded, in three operations instead of the ~10 of the IEEE division sequence (nine divisions by
// constants per pixel and pass): q = x * rc with rc = RN(1 / c), the exact residual by fma, one correction -- Markstein's theorem:
// RN(x / c) whenever rc is the correctly rounded reciprocal and c's significand is not all ones (0.95047, 1.08883, 116, 500, 200,
// 7.787: checked against the division itself on 56 M values, experiments/r06.md).  The contract of oracle/stain.py -- one float32
// rounding per operation -- is kept to the bit.
__device__ __forceinline__ float divc(float x, float c, float rc) {
    const float q = x * rc;
    const float r = __builtin_fmaf(-q, c, x);
    return __builtin_fmaf(r, rc, q);
}

// cbrt of a float32 t in (0.008856, ~1.1], "evaluated in float64 and rounded to float32" (the contract of oracle/stain.py), without
// the library's cbrt(double) (~80 double-precision operations): a float32 seed exp2(log2(t) / 3) (relative error ~1e-6), then two
// Newton steps y -= (y^3 - t) * r in float64 with ONE approximate reciprocal r ~ 1 / (3 y0^2) taken in float32 -- the error contracts
// by ~1e-6 per step, to the last bits of a double.  The float32 rounding of that differs from the rounding of the exact cube root only
// where the root lies within ~2e-16 (relative) of a float32 rounding boundary: one evaluation in ~3e8.
__device__ __forceinline__ float cbrt_f64_rounded(float t) {
    const float y0 = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(t) * (1.0f / 3.0f));
    const double r = (double)__builtin_amdgcn_rcpf(3.0f * y0 * y0);
    const double td = (double)t;
    double y = (double)y0;
    y = __builtin_fma(-(__builtin_fma(y * y, y, -td)), r, y);
    y = __builtin_fma(-(__builtin_fma(y * y, y, -td)), r, y);
    return (float)y;
}

// (at file scope: it holds from here to the end of this file, the launcher and the entry points included)
#pragma clang fp contract(off)
__device__ __forceinline__ Lab rgb_to_lab(const float* __restrict__ lut, const ReinhardConst& k, unsigned r8,
                                          unsigned g8, unsigned b8) {
    const float r = lut[r8], g = lut[g8], b = lut[b8];
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float xyz = (k.m[3 * i] * r + k.m[3 * i + 1] * g) + k.m[3 * i + 2] * b;
        const float t = divc(xyz, k.white[i], k.rwhite[i]);
        f[i] = t > 0.008856f ? cbrt_f64_rounded(t) : 7.787f * t + (float)(16.0 / 116.0);
    }
    Lab o;
    o.L = 116.0f * f[1] - 16.0f;
    o.a = 500.0f * (f[0] - f[1]);
    o.b = 200.0f * (f[1] - f[2]);
    return o;
}

#pragma clang fp contract(off)
__device__ __forceinline__ void lab_to_rgb8(const ReinhardConst& k, const float* __restrict__ thr, float L, float a,
                                            float b, uint8_t* out) {
    const float fy = divc(L + 16.0f, 116.0f, 1.0f / 116.0f);
    const float fx = divc(a, 500.0f, 1.0f / 500.0f) + fy;
    const float fz = fy - divc(b, 200.0f, 1.0f / 200.0f);
    const float fv[3] = {fx, fy, fz};
    float xyz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float v = fv[i];
        const float t = v > 0.2068966f ? (v * v) * v : divc(v - (float)(16.0 / 116.0), 7.787f, 1.0f / 7.787f);
        xyz[i] = t * k.white[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float c = (k.minv[3 * i] * xyz[0] + k.minv[3 * i + 1] * xyz[1]) + k.minv[3 * i + 2] * xyz[2];
        // out = clip(trunc(255 * clip(gamma(c), 0, 1)), 0, 255) is a monotone step function of c: the host evaluates the reference
        // formula (float64 power rounded to float32, then float32 steps) once per output level and hands over the 255 switching
        // points: thr[v-1] = smallest float32 c whose output is >= v.  Round 6: a fast float32 gamma gives the level to within one,
        // and two corrections against the switching points (two pairs of independent LDS reads) make it the formula's own result --
        // rounds 2-5 ran a bisection, eight DEPENDENT LDS reads per channel, which was most of this kernel's time.
        const float gam = c > 0.0031308f ? 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(c) * (float)(1.0 / 2.4)) - 0.055f : 12.92f * c;
        int lo = gam > 0.f ? (int)(255.0f * fminf(gam, 1.0f)) : 0;          // (NaN -> 0, like the clip; and it stays 0 below)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const float t_hi = thr[lo < 255 ? lo : 254], t_lo = thr[lo > 0 ? lo - 1 : 0];
            const int up = (lo < 255 && c >= t_hi) ? 1 : 0;
            const int dn = (lo > 0 && !(c >= t_lo)) ? 1 : 0;
            lo += up - dn;
        }
        out[i] = (uint8_t)lo;
    }
}

// stats_out (optional): [n][6] = mean L, a, b, std L, a, b.  dst may be null (statistics only) or == src.
// One workgroup of 1 024 threads per tile (round 6: 512 left every SIMD with two waves and the kernel waiting on its own LDS reads).
constexpr int RH_NT = 1024;
__global__ void __launch_bounds__(RH_NT) reinhard_kernel(const uint8_t* __restrict__ tiles, int px,
                                                         const float* __restrict__ lut, const ReinhardConst k,
                                                         uint8_t* dst, float* __restrict__ stats_out) {
    const int npix = px * px;
    const uint8_t* src = tiles + (size_t)blockIdx.x * npix * 3;
    const int tid = threadIdx.x, nt = blockDim.x;
    __shared__ float slut[256];
    __shared__ float sthr[256];
    __shared__ double red[6][RH_NT / 64];
    __shared__ float stat[6];
    for (int i = tid; i < 256; i += nt) { slut[i] = lut[i]; sthr[i] = lut[256 + i]; }
    __syncthreads();

    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < npix; i += nt) {
        const Lab v = rgb_to_lab(slut, k, src[3 * i], src[3 * i + 1], src[3 * i + 2]);
        s[0] += (double)v.L; s[1] += (double)v.a; s[2] += (double)v.b;
        s[3] += (double)v.L * (double)v.L; s[4] += (double)v.a * (double)v.a; s[5] += (double)v.b * (double)v.b;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
        if ((tid & 63) == 0) red[q][tid >> 6] = s[q];
    }
    __syncthreads();
    if (tid < 3) {
        double a = 0, b = 0;
        for (int i = 0; i < nt / 64; ++i) { a += red[tid][i]; b += red[tid + 3][i]; }
        const double mu = a / (double)npix;
        double var = b / (double)npix - mu * mu;
        if (var < 0) var = 0;
        stat[tid] = (float)mu;
        stat[tid + 3] = (float)sqrt(var);
        if (stats_out) {
            stats_out[(size_t)blockIdx.x * 6 + tid] = (float)mu;
            stats_out[(size_t)blockIdx.x * 6 + tid + 3] = (float)sqrt(var);
        }
    }
    __syncthreads();
    if (!dst) return;
    uint8_t* o = dst + (size_t)blockIdx.x * npix * 3;
    float sc[3];
    {
#pragma clang fp contract(off)
        sc[0] = k.tgt_std[0] / stat[3]; sc[1] = k.tgt_std[1] / stat[4]; sc[2] = k.tgt_std[2] / stat[5];
    }
    for (int i = tid; i < npix; i += nt) {
#pragma clang fp contract(off)
        const Lab v = rgb_to_lab(slut, k, src[3 * i], src[3 * i + 1], src[3 * i + 2]);
        const float L = (v.L - stat[0]) * sc[0] + k.tgt_mean[0];
        const float a = (v.a - stat[1]) * sc[1] + k.tgt_mean[1];
        const float b = (v.b - stat[2]) * sc[2] + k.tgt_mean[2];
        uint8_t rgb[3];
        lab_to_rgb8(k, sthr, L, a, b, rgb);
        o[3 * i] = rgb[0]; o[3 * i + 1] = rgb[1]; o[3 * i + 2] = rgb[2];
    }
}

// ---- the Reinhard family ("Reinhard family"): reinhard_fast plus two optional stages ----
// flags: RF_BRIGHTNESS = brightness standardisation in front (Slideflow's `reinhard` / `reinhard_mask`), RF_MASK = statistics and
// transform over the tissue pixels only, L < mask_L (`reinhard_fast_mask` / `reinhard_mask`).  One workgroup per tile, the tile
// re-read from cache in every pass:
//   0. (RF_BRIGHTNESS) p = the 90th percentile of the tile's float32 L, numpy's 'linear' rule over the exact order statistics
//      (radix_select.h); p not finite or <= 0: status RF_DARK, the tile passes through
//   1. the brightness table b -> trunc(min(b * (100 / p), 255)) in LDS (the identity without RF_BRIGHTNESS); every pixel through
//      it, to LAB, the mask test; the count and the six sums over tissue pixels in float64, the thread map and the tree of
//      reinhard_kernel (so flags 0 reports that kernel's statistics bit for bit); no tissue pixel: status RF_NO_TISSUE
//   2. tissue pixels transformed as reinhard_kernel transforms, the others stored as the table left them
// dst may be null (statistics only) or == src: in pass 2 every pixel is read and written by one thread, after every other read.
constexpr int RF_BRIGHTNESS = 1, RF_MASK = 2;
constexpr int RF_OK = 0, RF_NO_TISSUE = 1, RF_DARK = 2;
constexpr double RF_PCT = 0.9;             // the percentile of L that becomes L = 100 (unpinned; stain.py REINHARD_BRIGHT_PCT)
static_assert(RS_NT == RH_NT, "the radix select runs in the workgroup of the Reinhard kernels");

struct RfShared {
    float slut[256];
    float sthr[256];
    unsigned char btab[256];
    RadixSel sel;
    double red[6][RH_NT / 64];
    int cnt[RH_NT / 64];
    float stat[6];
    float p;
    int status, m;
};

__global__ void __launch_bounds__(RH_NT) reinhard_family_kernel(const uint8_t* tiles, int px, const float* __restrict__ lut,
                                                                const ReinhardConst k, int flags, float mask_L, uint8_t* dst,
                                                                float* __restrict__ stats8, int* __restrict__ st) {
    const int npix = px * px;
    const uint8_t* src = tiles + (size_t)blockIdx.x * npix * 3;
    const int tid = threadIdx.x, nt = blockDim.x;
    __shared__ RfShared sh;
    for (int i = tid; i < 256; i += nt) { sh.slut[i] = lut[i]; sh.sthr[i] = lut[256 + i]; }
    if (tid == 0) {
        sh.p = 100.0f;
        sh.status = RF_OK;
        sh.m = 0;
        // the select's second target is not used: an empty histogram, which leaves bin and before as they are set here
        sh.sel.rank[0] = (unsigned)floor(RF_PCT * (double)(npix - 1));
        sh.sel.rank[1] = sh.sel.bin[1] = sh.sel.before[1] = 0u;
        sh.sel.bin[0] = sh.sel.before[0] = 0u;
        sh.sel.coff = 0.f;                                    // L: 100 / 2 048 bins over [0, 100]
        sh.sel.cscl = (float)RS_BINS / 100.0f;
    }
    __syncthreads();

    // ---- 0. the 90th percentile of L
    if (flags & RF_BRIGHTNESS) {
        rs_select(sh.sel, npix, [&](int i, float v[2], bool ok[2]) {
            v[0] = v[1] = rgb_to_lab(sh.slut, k, src[3 * i], src[3 * i + 1], src[3 * i + 2]).L;
            ok[0] = true;
            ok[1] = false;
        });
        if (tid == 0) {
            const double v = RF_PCT * (double)(npix - 1), lo = floor(v);
            const double a = (double)rs_unkey(sh.sel.key[0]);
            const double b = lo + 1.0 < (double)npix ? (double)rs_unkey(sh.sel.succ[0]) : a;       // L[min(lo + 1, N - 1)]
            const float p = (float)rs_lerp(a, b, v - lo);
            sh.p = p;
            if (!(p > 0.f) || !isfinite(p)) sh.status = RF_DARK;
        }
        __syncthreads();
    }

    // ---- 1. brightness table, mask, statistics
    if (sh.status == RF_OK) {
        {
#pragma clang fp contract(off)
            const float s = 100.0f / sh.p;
            for (int i = tid; i < 256; i += nt)
                sh.btab[i] = (flags & RF_BRIGHTNESS) ? (unsigned char)(int)fminf((float)i * s, 255.0f) : (unsigned char)i;
        }
        __syncthreads();
        double s[6] = {0, 0, 0, 0, 0, 0};
        int cnt = 0;
        for (int i = tid; i < npix; i += nt) {
            const Lab v = rgb_to_lab(sh.slut, k, sh.btab[src[3 * i]], sh.btab[src[3 * i + 1]], sh.btab[src[3 * i + 2]]);
            if (!(flags & RF_MASK) || v.L < mask_L) {
                ++cnt;
                s[0] += (double)v.L; s[1] += (double)v.a; s[2] += (double)v.b;
                s[3] += (double)v.L * (double)v.L; s[4] += (double)v.a * (double)v.a; s[5] += (double)v.b * (double)v.b;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if ((tid & 63) == 0) sh.cnt[tid >> 6] = cnt;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
            if ((tid & 63) == 0) sh.red[q][tid >> 6] = s[q];
        }
        __syncthreads();
        if (tid < 3) {
            int m = 0;
            double a = 0, b = 0;
            for (int i = 0; i < nt / 64; ++i) { m += sh.cnt[i]; a += sh.red[tid][i]; b += sh.red[tid + 3][i]; }
            const double mu = a / (double)m;                  // (m == 0: NaN, and the status says so)
            double var = b / (double)m - mu * mu;
            if (var < 0) var = 0;
            sh.stat[tid] = (float)mu;
            sh.stat[tid + 3] = (float)sqrt(var);
            if (tid == 0) {
                sh.m = m;
                if (m == 0) sh.status = RF_NO_TISSUE;
            }
        }
        __syncthreads();
    }

    const int status = sh.status;
    if (tid == 0) {
        if (stats8) {
            float* o = stats8 + (size_t)blockIdx.x * 8;
            for (int i = 0; i < 6; ++i) o[i] = status == RF_OK ? sh.stat[i] : __builtin_nanf("");
            o[6] = sh.p;
            o[7] = (float)((double)sh.m / (double)npix);
        }
        if (st) st[blockIdx.x] = status;
    }
    if (!dst) return;

    // ---- 2. transform (or pass-through)
    uint8_t* out = dst + (size_t)blockIdx.x * npix * 3;
    if (status == RF_DARK) {
        if (out != src)
            for (int i = tid; i < 3 * npix; i += nt) out[i] = src[i];
        return;
    }
    if (status == RF_NO_TISSUE) {
        for (int i = tid; i < 3 * npix; i += nt) out[i] = sh.btab[src[i]];
        return;
    }
    float sc[3];
    {
#pragma clang fp contract(off)
        sc[0] = k.tgt_std[0] / sh.stat[3]; sc[1] = k.tgt_std[1] / sh.stat[4]; sc[2] = k.tgt_std[2] / sh.stat[5];
    }
    for (int i = tid; i < npix; i += nt) {
#pragma clang fp contract(off)
        const unsigned r8 = sh.btab[src[3 * i]], g8 = sh.btab[src[3 * i + 1]], b8 = sh.btab[src[3 * i + 2]];
        const Lab v = rgb_to_lab(sh.slut, k, r8, g8, b8);
        uint8_t rgb[3] = {(uint8_t)r8, (uint8_t)g8, (uint8_t)b8};
        if (!(flags & RF_MASK) || v.L < mask_L) {
            const float L = (v.L - sh.stat[0]) * sc[0] + k.tgt_mean[0];
            const float a = (v.a - sh.stat[1]) * sc[1] + k.tgt_mean[1];
            const float b = (v.b - sh.stat[2]) * sc[2] + k.tgt_mean[2];
            lab_to_rgb8(k, sh.sthr, L, a, b, rgb);
        }
        out[3 * i] = rgb[0]; out[3 * i + 1] = rgb[1]; out[3 * i + 2] = rgb[2];
    }
}

}  // namespace

static void reinhard_consts(ReinhardConst& k, const float* consts27, const float* tgt_mean, const float* tgt_std) {
    for (int i = 0; i < 9; ++i) { k.m[i] = consts27[i]; k.minv[i] = consts27[9 + i]; }
    for (int i = 0; i < 3; ++i) {
        k.white[i] = consts27[18 + i];
        k.rwhite[i] = 1.0f / consts27[18 + i];
        k.tgt_mean[i] = tgt_mean ? tgt_mean[i] : 0.f;
        k.tgt_std[i] = tgt_std ? tgt_std[i] : 1.f;
    }
}

static int launch_reinhard_family(const uint8_t* tiles, int n, int px, int flags, float mask_L, const float* d_lut,
                                  const float* tgt_mean, const float* tgt_std, uint8_t* dst, float* d_stats8, int* d_status,
                                  hipStream_t s) {
    if (n <= 0) return 0;
    ReinhardConst k;
    reinhard_consts(k, kReinhardConsts, tgt_mean, tgt_std);
    hipLaunchKernelGGL(reinhard_family_kernel, dim3(n), dim3(RH_NT), 0, s, tiles, px, d_lut, k, flags, mask_L, dst, d_stats8,
                       d_status);
    return (int)hipGetLastError();
}

static int launch_reinhard(const uint8_t* tiles, int n, int px, const float* d_lut, const float* consts27,
                           const float* tgt_mean, const float* tgt_std, uint8_t* dst, float* d_stats, hipStream_t s) {
    if (n <= 0) return 0;
    ReinhardConst k;
    reinhard_consts(k, consts27, tgt_mean, tgt_std);
    hipLaunchKernelGGL(reinhard_kernel, dim3(n), dim3(RH_NT), 0, s, tiles, px, d_lut, k, dst, d_stats);
    return (int)hipGetLastError();
}

extern "C" {

int bq_stain_reinhard_fast(bq_ctx* c, const uint8_t* d_tiles, int n, const float* target_means3,
                           const float* target_stds3, uint8_t* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || !target_means3 || !target_stds3 || n < 0)
        return fail(c, BQ_ERR_ARG, "bq_stain_reinhard_fast: bad argument");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(target_stds3[i]) || !std::isfinite(target_means3[i]))      // (a std of 0 or below is defined arithmetic)
            return fail(c, BQ_ERR_ARG, "bq_stain_reinhard_fast: non-finite target statistics");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_reinhard_fast", 300.0 * n * 299 * 299, 3.0 * n * kStaged);
    if (launch_reinhard(d_tiles, n, 299, c->d_srgb_lut, kReinhardConsts, target_means3, target_stds3, d_out, nullptr, s))
        return fail(c, BQ_ERR_HIP, "reinhard launch failed");
    return BQ_OK;
}

int bq_stain_lab_stats(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_stats6, bq_stream_t stream) {
    if (!c || !d_tiles || !d_stats6 || n < 0) return fail(c, BQ_ERR_ARG, "bq_stain_lab_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (launch_reinhard(d_tiles, n, 299, c->d_srgb_lut, kReinhardConsts, nullptr, nullptr, nullptr, d_stats6, s))
        return fail(c, BQ_ERR_HIP, "lab stats launch failed");
    return BQ_OK;
}

static int reinhard_family_args(bq_ctx* c, const char* who, const void* d_tiles, int n, int px, int flags, float mask_L) {
    if (!c || !d_tiles || n < 0) return fail(c, BQ_ERR_ARG, std::string(who) + ": bad argument");
    if (px < 1 || px > 1024) return fail(c, BQ_ERR_ARG, std::string(who) + ": px must be in 1..1024");
    if (flags < 0 || flags > 3) return fail(c, BQ_ERR_ARG, std::string(who) + ": flags must be in 0..3 (1 = brightness, 2 = mask)");
    if (!std::isfinite(mask_L)) return fail(c, BQ_ERR_ARG, std::string(who) + ": non-finite mask_L");
    return BQ_OK;
}

int bq_stain_reinhard(bq_ctx* c, const uint8_t* d_tiles, int n, int px, int flags, float mask_L, const float* target_means3,
                      const float* target_stds3, uint8_t* d_out, int* d_status, bq_stream_t stream) {
    if (const int e = reinhard_family_args(c, "bq_stain_reinhard", d_tiles, n, px, flags, mask_L)) return e;
    if (!d_out || !target_means3 || !target_stds3) return fail(c, BQ_ERR_ARG, "bq_stain_reinhard: bad argument");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(target_stds3[i]) || !std::isfinite(target_means3[i]))      // (a std of 0 or below is defined arithmetic)
            return fail(c, BQ_ERR_ARG, "bq_stain_reinhard: non-finite target statistics");
    hipStream_t s = (hipStream_t)stream;
    const double pixels = (double)n * px * px;
    ProfScope ps(c, s, "stain_reinhard", ((flags & 1) ? 500.0 : 300.0) * pixels, 3.0 * 3.0 * pixels);
    if (launch_reinhard_family(d_tiles, n, px, flags, mask_L, c->d_srgb_lut, target_means3, target_stds3, d_out, nullptr, d_status, s))
        return fail(c, BQ_ERR_HIP, "reinhard family launch failed");
    return BQ_OK;
}

int bq_stain_reinhard_stats(bq_ctx* c, const uint8_t* d_tiles, int n, int px, int flags, float mask_L, float* d_stats8,
                            int* d_status, bq_stream_t stream) {
    if (const int e = reinhard_family_args(c, "bq_stain_reinhard_stats", d_tiles, n, px, flags, mask_L)) return e;
    if (!d_stats8) return fail(c, BQ_ERR_ARG, "bq_stain_reinhard_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const double pixels = (double)n * px * px;
    ProfScope ps(c, s, "stain_reinhard_stats", ((flags & 1) ? 350.0 : 150.0) * pixels, 3.0 * pixels);
    if (launch_reinhard_family(d_tiles, n, px, flags, mask_L, c->d_srgb_lut, nullptr, nullptr, nullptr, d_stats8, d_status, s))
        return fail(c, BQ_ERR_HIP, "reinhard family stats launch failed");
    return BQ_OK;
}

}  // extern "C"
