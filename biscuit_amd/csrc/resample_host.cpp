// Host side of the tile resampler (include/biscuit_io.h: bqio_resample_ksize, bqio_resample_taps, bqio_tile_resample):
// Pillow's coefficient construction for its LANCZOS filter in C++ double with libm -- which is what Pillow itself does --
// and the CPU restatement of the two passes over the routines of resample_device.h, the ones the GPU kernel is compiled from.
#include "../../include/biscuit_io.h"
#include "resample_device.h"

#include <math.h>
#include <stdlib.h>

#include <vector>

namespace {

#if defined(__GNUC__) && !defined(__clang__)
#define BQR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))     // the taps are a bit-level contract: no fused multiply-add
#else
#define BQR_NO_CONTRACT
#endif

double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

double lanczos_filter(double x) {                 // truncated sinc
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

bool ratio_ok(int src_px, int px) {
    return px > 0 && src_px > 0 && px <= 4096 && src_px <= 4096 * bqrs::MAX_RATIO && (int64_t)src_px <= (int64_t)bqrs::MAX_RATIO * px &&
           (int64_t)px <= (int64_t)bqrs::MAX_RATIO * src_px;
}

using bqrs::ksize_of;

// precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c for the box (0, src_px)
BQR_NO_CONTRACT int build_taps(int src_px, int px, int32_t* bounds, int32_t* coef, int ksize) {
    const double scale = (double)src_px / px;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = bqrs::SUPPORT * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < px; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > src_px) xmax = src_px;
        xmax -= xmin;
        if (xmax < 0 || xmax > ksize) return BQIO_ERR_ARG;
        for (int x = 0; x < xmax; ++x) {
            const double w = lanczos_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        int32_t* out = coef + (size_t)xx * ksize;
        int64_t mag = 0;
        for (int x = 0; x < ksize; ++x) {
            const double v = x < xmax ? k[x] : 0.0;
            out[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << bqrs::PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << bqrs::PRECISION_BITS));
            mag += llabs((long long)out[x]);
        }
        // the accumulators of both passes are 32-bit: 2^21 + 255 * sum |tap| must stay below 2^31
        if (255 * mag + (1 << (bqrs::PRECISION_BITS - 1)) >= (int64_t)1 << 31) return BQIO_ERR_UNSUPPORTED;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return BQIO_OK;
}

}  // namespace

extern "C" {

int bqio_resample_ksize(int src_px, int px) {
    if (!ratio_ok(src_px, px)) return BQIO_ERR_ARG;
    return ksize_of(src_px, px);
}

int bqio_resample_taps(int src_px, int px, int32_t* bounds, int32_t* coef, int ksize_cap) {
    if (!ratio_ok(src_px, px) || !bounds || !coef) return BQIO_ERR_ARG;
    const int ksize = ksize_of(src_px, px);
    if (ksize > ksize_cap || ksize > bqrs::MAX_KSIZE) return BQIO_ERR_ARG;
    const int e = build_taps(src_px, px, bounds, coef, ksize);
    return e == BQIO_OK ? ksize : e;
}

int bqio_tile_resample(const uint8_t* canvas, int H, int W, const int32_t* origin, int n, int src_px, int px, uint8_t* out) {
    if (n < 0 || !ratio_ok(src_px, px) || H <= 0 || W <= 0 || (int64_t)H * W > ((int64_t)1 << 40) / 3) return BQIO_ERR_ARG;
    if (n == 0) return BQIO_OK;
    if (!canvas || !origin || !out) return BQIO_ERR_ARG;
    for (int t = 0; t < 2 * n; ++t)
        if (origin[t] < -(1 << 28) || origin[t] > (1 << 28)) return BQIO_ERR_ARG;
    const size_t tile = (size_t)px * px * 3;
    if (src_px == px) {
        for (int t = 0; t < n; ++t) {
            const int ox = origin[2 * t], oy = origin[2 * t + 1];
            uint8_t* o = out + (size_t)t * tile;
            for (int y = 0; y < px; ++y)
                for (int x = 0; x < px; ++x)
                    for (int c = 0; c < 3; ++c) o[((size_t)y * px + x) * 3 + c] = bqrs::copy_byte(canvas, H, W, oy + y, ox + x, c);
        }
        return BQIO_OK;
    }
    const int ksize = ksize_of(src_px, px);
    std::vector<int32_t> bounds((size_t)2 * px), coef((size_t)px * ksize);
    const int e = build_taps(src_px, px, bounds.data(), coef.data(), ksize);
    if (e != BQIO_OK) return e;
    const int pitch = 3 * px;
    std::vector<uint8_t> inter((size_t)src_px * pitch);                     // the horizontal pass, one row per source row
    for (int t = 0; t < n; ++t) {
        const int ox = origin[2 * t], oy = origin[2 * t + 1];
        const bool whole = ox >= 0 && oy >= 0 && ox <= W - src_px && oy <= H - src_px;
        int f0, c0, f1, c1;
        bqrs::window(bounds.data(), 0, src_px, ksize, f0, c0);
        bqrs::window(bounds.data(), px - 1, src_px, ksize, f1, c1);
        for (int r = f0; r < f1 + c1; ++r)                                    // the rows the vertical pass reads (Pillow's ybox)
            for (int x = 0; x < px; ++x) {
                int first, count;
                bqrs::window(bounds.data(), x, src_px, ksize, first, count);
                bqrs::hpass(canvas, H, W, oy + r, ox + first, count, coef.data() + (size_t)x * ksize, whole, &inter[(size_t)r * pitch + 3 * x]);
            }
        uint8_t* o = out + (size_t)t * tile;
        for (int y = 0; y < px; ++y) {
            int first, count;
            bqrs::window(bounds.data(), y, src_px, ksize, first, count);
            for (int b = 0; b < pitch; ++b)
                o[(size_t)y * pitch + b] = bqrs::vpass(&inter[(size_t)first * pitch + b], pitch, count, coef.data() + (size_t)y * ksize);
        }
    }
    return BQIO_OK;
}

}  // extern "C"
