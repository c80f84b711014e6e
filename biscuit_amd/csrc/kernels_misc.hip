// HBM-bound kernels around the MFMA path: tile staging (K0), the 3->32 stem conv (K1a),
// max-pool + residual add (K4), global average pool (K5), the MC head's last layer with
// softmax + Welford fold (K6 tail) and the slide-level segmented reduce (K7); the entry points of K0 and K7 at the end.
#include "bq_ctx.h"

namespace {

template <typename T> __device__ __forceinline__ T from_f32(float f);
template <> __device__ __forceinline__ float from_f32<float>(float f) { return f; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float f) { return (bf16_t)f; }
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float f) { return (f16_t)f; }   // FP16_OVFL: saturates
template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) { return (float)v; }
template <> __device__ __forceinline__ float to_f32<f16_t>(f16_t v) { return (float)v; }

template <typename T>
__device__ __forceinline__ unsigned pk16(float lo, float hi) {
    const unsigned short a = __builtin_bit_cast(unsigned short, from_f32<T>(lo));
    const unsigned short b = __builtin_bit_cast(unsigned short, from_f32<T>(hi));
    return (unsigned)a | ((unsigned)b << 16);
}
template <typename T> __device__ __forceinline__ void f16_mode() {
    if constexpr (sizeof(T) == 2 && !__is_same(T, bf16_t)) bq_f16_saturate();
}

// ---------------------------------------------------------------- K0 staging
// Two kernels with SLICES workgroups per tile (one workgroup per tile leaves the chip at one workgroup per
// CU for an HBM-bound pass: 0.157 ms per 256 tiles against a 0.04 ms roofline): exact integer sum / sum of
// squares of the uint8 bytes into two 64-bit atomics per tile (order-independent, so the statistics are
// bit-reproducible), then the standardisation pass, which writes three contiguous planes.
constexpr int kStageSlices = 8;

__global__ void __launch_bounds__(256) stage_stats_kernel(const uint8_t* __restrict__ tiles, int px,
                                                          unsigned long long* __restrict__ stats) {
    const int nbytes = px * px * 3;
    const int tile = blockIdx.x / kStageSlices, sl = blockIdx.x - tile * kStageSlices;
    const uint8_t* src = tiles + (size_t)tile * nbytes;
    const int tid = threadIdx.x, nt = blockDim.x;
    // A thread's share of a slice is ~130 bytes: 32-bit partial sums cannot overflow (130 x 255^2 < 2^24).  Four bytes per
    // instruction: v_sad_u8 against zero is their sum, v_dot4_u32_u8 of a word with itself the sum of their squares (round 4:
    // 16-byte loads and these two instead of shifts, masks and 64-bit adds per byte: 0.036 -> 0.02 ms per batch, same integers).
    unsigned p1 = 0, p2 = 0;
    const int head = (int)((4 - ((uintptr_t)src & 3)) & 3);
    const int body = (nbytes - head) >> 2;
    const int d0 = (int)((long long)body * sl / kStageSlices), d1 = (int)((long long)body * (sl + 1) / kStageSlices);
    if (sl == 0 && tid < head) { const unsigned v = src[tid]; p1 += v; p2 += v * v; }
    const unsigned* w = reinterpret_cast<const unsigned*>(src + head);
    const int nq = (d1 - d0) >> 2;                      // whole groups of four words (16 bytes: dword alignment is all it needs)
    for (int i = tid; i < nq; i += nt) {
        const uint4 u = *reinterpret_cast<const uint4*>(w + d0 + 4 * i);
        p1 = __builtin_amdgcn_sad_u8(u.x, 0u, p1); p2 = __builtin_amdgcn_udot4(u.x, u.x, p2, false);
        p1 = __builtin_amdgcn_sad_u8(u.y, 0u, p1); p2 = __builtin_amdgcn_udot4(u.y, u.y, p2, false);
        p1 = __builtin_amdgcn_sad_u8(u.z, 0u, p1); p2 = __builtin_amdgcn_udot4(u.z, u.z, p2, false);
        p1 = __builtin_amdgcn_sad_u8(u.w, 0u, p1); p2 = __builtin_amdgcn_udot4(u.w, u.w, p2, false);
    }
    for (int i = d0 + 4 * nq + tid; i < d1; i += nt) {
        const unsigned u = w[i];
        p1 = __builtin_amdgcn_sad_u8(u, 0u, p1); p2 = __builtin_amdgcn_udot4(u, u, p2, false);
    }
    const int tail0 = head + body * 4;
    if (sl == kStageSlices - 1 && tid < nbytes - tail0) { const unsigned v = src[tail0 + tid]; p1 += v; p2 += v * v; }
    unsigned long long s1 = p1, s2 = p2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&stats[2 * tile], s1);
        atomicAdd(&stats[2 * tile + 1], s2);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) stage_apply_kernel(const uint8_t* __restrict__ tiles, int px,
                                                          const unsigned long long* __restrict__ stats,
                                                          T* __restrict__ out) {
    f16_mode<T>();
    const int npix = px * px, nbytes = npix * 3;
    const int tile = blockIdx.x / kStageSlices, sl = blockIdx.x - tile * kStageSlices;
    const uint8_t* src = tiles + (size_t)tile * nbytes;
    // float64 statistics from the exact integer sums
    const double n = (double)nbytes;
    const double mean_d = (double)stats[2 * tile] / n;
    double var = (double)stats[2 * tile + 1] / n - mean_d * mean_d;
    if (var < 0) var = 0;
    const double sd = sqrt(var), floor_sd = 1.0 / sqrt(n);   // tf.image.per_image_standardization
    const float mean = (float)mean_d, inv = (float)(1.0 / (sd > floor_sd ? sd : floor_sd));
    T* o0 = out + (size_t)tile * nbytes;
    const int p0 = (int)((long long)npix * sl / kStageSlices), p1 = (int)((long long)npix * (sl + 1) / kStageSlices);
    for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const uint8_t* q = src + p * 3;
        o0[p] = from_f32<T>(((float)q[0] - mean) * inv);
        o0[npix + p] = from_f32<T>(((float)q[1] - mean) * inv);
        o0[2 * npix + p] = from_f32<T>(((float)q[2] - mean) * inv);
    }
}

template <typename T>
__global__ void stage_f32_kernel(const float* __restrict__ tiles, long long total_pix, int npix,
                                 T* __restrict__ out) {
    f16_mode<T>();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_pix) return;
    const long long img = i / npix;
    const int p = (int)(i - img * npix);
    const float* q = tiles + i * 3;
    T* o0 = out + img * 3 * npix;
    o0[p] = from_f32<T>(q[0]);
    o0[npix + p] = from_f32<T>(q[1]);
    o0[2 * npix + p] = from_f32<T>(q[2]);
}

// ---------------------------------------------------------------- K1a stem conv1
// Conv2D(32, 3x3, strides 2, 'valid', no bias) + folded BN + ReLU on the planar staged
// tile.  0.2 % of the FLOPs: vector ALU, one output pixel x 32 channels per lane, weights
// through the scalar cache (uniform addresses), NHWC store of 32 contiguous channels.
template <typename T>
__global__ void __launch_bounds__(256) stem1_kernel(const T* __restrict__ in, int n, int px,
                                                    const float* __restrict__ w,
                                                    const float* __restrict__ scale,
                                                    const float* __restrict__ bias,
                                                    T* __restrict__ out) {
    f16_mode<T>();
    const int po = (px - 3) / 2 + 1;  // 149
    const long long total = (long long)n * po * po;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int img = (int)(gid / (po * po));
    const int rem = (int)(gid - (long long)img * po * po);
    const int yo = rem / po, xo = rem - yo * po;
    const T* base = in + (size_t)img * 3 * px * px;
    float x[27];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                x[(dy * 3 + dx) * 3 + c] = to_f32<T>(base[(size_t)c * px * px + (2 * yo + dy) * px + 2 * xo + dx]);
    // two output channels per v_pk_fma_f32 (weights as scalar-register pairs, the pixel value splat): the
    // kernel is bound by its 864 multiply-adds per pixel, not by memory
    typedef float f32x2s __attribute__((ext_vector_type(2)));
    f32x2s acc2[16];
#pragma unroll
    for (int co = 0; co < 16; ++co) acc2[co] = (f32x2s){0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const f32x2s xs = {x[k], x[k]};
#pragma unroll
        for (int co = 0; co < 16; ++co)
            acc2[co] = __builtin_elementwise_fma(xs, (f32x2s){w[k * 32 + 2 * co], w[k * 32 + 2 * co + 1]}, acc2[co]);
    }
    float acc[32];
#pragma unroll
    for (int co = 0; co < 16; ++co) {
        acc[2 * co] = fmaxf(fmaf(acc2[co].x, scale[2 * co], bias[2 * co]), 0.f);
        acc[2 * co + 1] = fmaxf(fmaf(acc2[co].y, scale[2 * co + 1], bias[2 * co + 1]), 0.f);
    }
    T* o = out + (size_t)gid * 32;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int j = 0; j < 32; j += 8)
            *reinterpret_cast<uint4*>(o + j) =
                make_uint4(pk16<T>(acc[j], acc[j + 1]), pk16<T>(acc[j + 2], acc[j + 3]),
                           pk16<T>(acc[j + 4], acc[j + 5]), pk16<T>(acc[j + 6], acc[j + 7]));
    } else {
#pragma unroll
        for (int j = 0; j < 32; j += 4)
            *reinterpret_cast<float4*>(o + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
    }
}

// ---------------------------------------------------------------- K4 maxpool + add
// MaxPooling2D(3, strides 2, 'same') with TensorFlow's asymmetric padding (odd input:
// pad (1,1); even input: pad (0,1); padded value -inf) fused with the residual add.
template <typename T, int VEC>
__global__ void __launch_bounds__(256) pool_add_kernel(const T* __restrict__ y, const T* __restrict__ res,
                                                       T* __restrict__ out, int n, int Hi, int Wi,
                                                       int Ho, int Wo, int C) {
    f16_mode<T>();
    const int chunks = C / VEC;
    const long long total = (long long)n * Ho * Wo * chunks;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % chunks);
    const long long pix = gid / chunks;
    const int xo = (int)(pix % Wo);
    const int yo = (int)((pix / Wo) % Ho);
    const int img = (int)(pix / ((long long)Wo * Ho));
    const int pt = (Hi & 1) ? 1 : 0, pl = (Wi & 1) ? 1 : 0;
    float m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = 2 * yo + dy - pt;
        if ((unsigned)yy >= (unsigned)Hi) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = 2 * xo + dx - pl;
            if ((unsigned)xx >= (unsigned)Wi) continue;
            const T* q = y + ((size_t)(img * Hi + yy) * Wi + xx) * C + c * VEC;
            const uint4 u = *reinterpret_cast<const uint4*>(q);
            const T* e = reinterpret_cast<const T*>(&u);
#pragma unroll
            for (int j = 0; j < VEC; ++j) m[j] = fmaxf(m[j], to_f32<T>(e[j]));
        }
    }
    const size_t o = (size_t)pix * C + c * VEC;
    const uint4 ru = *reinterpret_cast<const uint4*>(res + o);
    const T* re = reinterpret_cast<const T*>(&ru);
    uint4 ou;
    T* oe = reinterpret_cast<T*>(&ou);
#pragma unroll
    for (int j = 0; j < VEC; ++j) oe[j] = from_f32<T>(m[j] + to_f32<T>(re[j]));
    *reinterpret_cast<uint4*>(out + o) = ou;
}

// ---------------------------------------------------------------- K5 global average pool
template <typename T>
__global__ void __launch_bounds__(256) gap_kernel(const T* __restrict__ x, int n, int HW, int C, int ld,
                                                  float* __restrict__ feat, float mul) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n * C) return;
    const int img = (int)(gid / C), c = (int)(gid - (long long)img * C);
    const T* p = x + (size_t)img * HW * ld + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += to_f32<T>(p[(size_t)i * ld]);
    feat[gid] = s / (float)HW * mul;
}

// ---------------------------------------------------------------- K6 tail
// One workgroup of eight waves per tile.  Wave w takes MC passes w, w + 8, ...: dropout(hidden_1 row) . W2 -> 2 logits ->
// softmax; the two probabilities of a block of eight passes meet in LDS and ONE lane folds them into the Welford state (count,
// mean[2], M2[2]) in pass order -- the arithmetic, and its order, of the one-wave-per-tile form this replaces (round 4: that
// form ran 256 waves on the whole chip, each through 30 passes of ~500 vector instructions: 0.036 ms; the passes are
// independent, only the fold is sequential).  W2 lives in registers (16 k per lane x 2 classes).  state layout [n][5] fp32.
constexpr int kHeadFinalWaves = 8;
__global__ void __launch_bounds__(64 * kHeadFinalWaves) head_final_kernel(const float* __restrict__ h1, int n, int mc_n,
                                                         int pass0, long long tile0_imm,
                                                         const long long* __restrict__ tile0_dev,
                                                         const long long* __restrict__ tile_idx, unsigned seed_lo,
                                                         unsigned seed_hi, unsigned thresh, float dscale,
                                                         const float* __restrict__ w2,
                                                         const float* __restrict__ b2, int init,
                                                         int finalize, float* __restrict__ state,
                                                         float* __restrict__ mean2,
                                                         float* __restrict__ std2) {
    __shared__ float probs[kHeadFinalWaves][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x;
    const unsigned tctr = (unsigned)(tile0_imm + (tile0_dev ? *tile0_dev : 0) + (tile_idx ? tile_idx[tile] : (long long)tile));
    float wa[16], wb[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 4 * (lane + 64 * j) + e;
            wa[j * 4 + e] = w2[k * 2];
            wb[j * 4 + e] = w2[k * 2 + 1];
        }
    float cnt = 0.f, mu0 = 0.f, mu1 = 0.f, q0 = 0.f, q1 = 0.f;       // (kept by thread 0 only)
    if (!init && threadIdx.x == 0) {
        const float* st = state + (size_t)tile * 5;
        cnt = st[0]; mu0 = st[1]; mu1 = st[2]; q0 = st[3]; q1 = st[4];
    }
    for (int base = 0; base < mc_n; base += kHeadFinalWaves) {
        const int p = base + wave;
        if (p < mc_n) {
            const float* row = h1 + ((size_t)tile * mc_n + p) * 1024;
            float z0 = 0.f, z1 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = lane + 64 * j;  // Philox group = unit / 4
                const float4 v = *reinterpret_cast<const float4*>(row + 4 * g);
                unsigned r[4];
                philox4x32_10((unsigned)g, 2u, (unsigned)(pass0 + p), tctr, seed_lo,
                              seed_hi, r);
                const float f0 = r[0] >= thresh ? v.x * dscale : 0.f;
                const float f1 = r[1] >= thresh ? v.y * dscale : 0.f;
                const float f2 = r[2] >= thresh ? v.z * dscale : 0.f;
                const float f3 = r[3] >= thresh ? v.w * dscale : 0.f;
                z0 = fmaf(f0, wa[j * 4], z0); z0 = fmaf(f1, wa[j * 4 + 1], z0);
                z0 = fmaf(f2, wa[j * 4 + 2], z0); z0 = fmaf(f3, wa[j * 4 + 3], z0);
                z1 = fmaf(f0, wb[j * 4], z1); z1 = fmaf(f1, wb[j * 4 + 1], z1);
                z1 = fmaf(f2, wb[j * 4 + 2], z1); z1 = fmaf(f3, wb[j * 4 + 3], z1);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                z0 += __shfl_xor(z0, o);
                z1 += __shfl_xor(z1, o);
            }
            z0 += b2[0];
            z1 += b2[1];
            const float zm = fmaxf(z0, z1);
            const float e0 = expf(z0 - zm), e1 = expf(z1 - zm);
            const float inv = 1.f / (e0 + e1);
            if (lane == 0) { probs[wave][0] = e0 * inv; probs[wave][1] = e1 * inv; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int np = mc_n - base < kHeadFinalWaves ? mc_n - base : kHeadFinalWaves;
            for (int k = 0; k < np; ++k) {
                float p0 = probs[k][0], p1 = probs[k][1];
                // Pin the rounded probabilities: if the compiler contracts a product into the Welford differences below
                // (fma(e, inv, -mean)), p - mean keeps the product's rounding error instead of an exact 0 and a single pass
                // reports std ~1e-4 instead of 0.
                asm volatile("" : "+v"(p0), "+v"(p1));
                cnt += 1.f;
                const float d0 = p0 - mu0, d1 = p1 - mu1;
                mu0 += d0 / cnt;
                mu1 += d1 / cnt;
                q0 = fmaf(d0, p0 - mu0, q0);
                q1 = fmaf(d1, p1 - mu1, q1);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* st = state + (size_t)tile * 5;
        st[0] = cnt; st[1] = mu0; st[2] = mu1; st[3] = q0; st[4] = q1;
        if (finalize) {
            mean2[tile * 2] = mu0;
            mean2[tile * 2 + 1] = mu1;
            // population std (ddof = 0); a NaN tile keeps its NaN (fmaxf(NaN, 0) would report 0)
            std2[tile * 2] = sqrtf((q0 != q0 ? q0 : fmaxf(q0, 0.f)) / cnt);
            std2[tile * 2 + 1] = sqrtf((q1 != q1 ? q1 : fmaxf(q1, 0.f)) / cnt);
        }
    }
}

// ---------------------------------------------------------------- K7 slide reduce
// Fixed-point (2^-40) 64-bit integer atomics: the sum is exact per addend and associative,
// so slide means are bit-reproducible whatever the arrival order.
__global__ void __launch_bounds__(256) slide_reduce_kernel(const float* __restrict__ mean2,
                                                           const float* __restrict__ std2,
                                                           const int32_t* __restrict__ slide_idx, int n,
                                                           int n_slides, float tile_uq, int use_uq,
                                                           unsigned long long* acc_pred,
                                                           unsigned long long* acc_unc, int32_t* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slide_idx[i];
    if ((unsigned)s >= (unsigned)n_slides) return;
    const float yp = mean2[i * 2 + 1];  // P(class 1): utils.py:27-28 y_pred1
    const float un = std2[i * 2 + 1];   // utils.py:19-20 uncertainty1
    if (use_uq && !(un < tile_uq)) return;  // strict '<' (threshold.py:298)
    const double sc = (double)(1ull << BQ_FIXED_SHIFT);
    const long long a = __double2ll_rn((double)yp * sc);
    const long long b = __double2ll_rn((double)un * sc);
    atomicAdd(acc_pred + s, (unsigned long long)a);
    atomicAdd(acc_unc + s, (unsigned long long)b);
    atomicAdd(count + s, 1);
}

__global__ void slide_finish_kernel(const long long* acc_pred, const long long* acc_unc,
                                    const int32_t* count, int n_slides, double* mean_pred,
                                    double* mean_unc) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slides) return;
    const double inv = 1.0 / (double)(1ull << BQ_FIXED_SHIFT);
    const int c = count[s];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    mean_pred[s] = c > 0 ? ((double)acc_pred[s] * inv) / (double)c : nan;
    mean_unc[s] = c > 0 ? ((double)acc_unc[s] * inv) / (double)c : nan;
}

// ---------------------------------------------------------------- debug copies
template <typename T>
__global__ void to_f32_nhwc_kernel(const T* __restrict__ x, long long rows, int C, int ld,
                                   float* __restrict__ out) {
    // grid-stride: a launch has fewer than 2^32 threads (the runtime truncates a larger one), a tap can have more elements --
    // 147 x 147 x 128 from n = 1 553
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < rows * C; gid += (long long)gridDim.x * blockDim.x) {
        const long long r = gid / C;
        const int c = (int)(gid - r * C);
        out[gid] = to_f32<T>(x[r * ld + c]);
    }
}

template <typename T>
__global__ void nchw_to_f32_nhwc_kernel(const T* __restrict__ x, int n, int C, int HW,
                                        float* __restrict__ out) {
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < (long long)n * C * HW; gid += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % C);
        const long long pix = gid / C;
        const int p = (int)(pix % HW);
        const long long img = pix / HW;
        out[gid] = to_f32<T>(x[(img * C + c) * HW + p]);
    }
}

inline int grid_for(long long total, int block) { return (int)((total + block - 1) / block); }
// of a grid-stride kernel: at most 2^30 threads per launch
inline int grid_stride_for(long long total, int block) {
    const long long g = (total + block - 1) / block, cap = (1ll << 30) / block;
    return (int)(g < cap ? g : cap);
}

}  // namespace

// CALL is written for the type name T_; instantiated for bf16 (dtype 1), f16 (2) and fp32 (0)
#define BQ_DISPATCH_T(dtype, ...)                                              \
    do {                                                                       \
        if ((dtype) == 1) { using T_ = bf16_t; __VA_ARGS__; }                  \
        else if ((dtype) == 2) { using T_ = f16_t; __VA_ARGS__; }              \
        else { using T_ = float; __VA_ARGS__; }                                \
    } while (0)

// stats_scratch: 2 x 64-bit per tile, zeroed here
static int launch_stage_u8(const uint8_t* tiles, int n, int px, void* out, int dtype, double* stats_scratch, hipStream_t s) {
    if (n <= 0) return 0;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats_scratch);
    hipError_t e = hipMemsetAsync(st, 0, (size_t)n * 16, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(stage_stats_kernel, dim3(n * kStageSlices), dim3(256), 0, s, tiles, px, st);
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(stage_apply_kernel<T_>, dim3(n * kStageSlices), dim3(256), 0, s, tiles, px,
                                     st, (T_*)out));
    return (int)hipGetLastError();
}

// the per-tile integer sums alone (2 x 64-bit per tile, zeroed here): the pre-pass of the fused front kernel (kernels_front.hip)
int launch_stage_stats(const uint8_t* tiles, int n, int px, double* stats_scratch, hipStream_t s) {
    if (n <= 0) return 0;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats_scratch);
    hipError_t e = hipMemsetAsync(st, 0, (size_t)n * 16, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(stage_stats_kernel, dim3(n * kStageSlices), dim3(256), 0, s, tiles, px, st);
    return (int)hipGetLastError();
}

static int launch_stage_f32(const float* tiles, int n, int px, void* out, int dtype, hipStream_t s) {
    if (n <= 0) return 0;
    const long long total = (long long)n * px * px;
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(stage_f32_kernel<T_>, dim3(grid_for(total, 256)), dim3(256), 0, s,
                                     tiles, total, px * px, (T_*)out));
    return (int)hipGetLastError();
}

int launch_stem1(const void* in, int n, const float* w, const float* scale, const float* bias, void* out,
                 int dtype, hipStream_t s) {
    const int px = 299, po = 149;
    const long long total = (long long)n * po * po;
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(stem1_kernel<T_>, dim3(grid_for(total, 256)), dim3(256), 0, s,
                                     (const T_*)in, n, px, w, scale, bias, (T_*)out));
    return (int)hipGetLastError();
}

int launch_pool_add(const void* y, const void* res, void* out, int n, int Hi, int Wi, int C, int dtype,
                    hipStream_t s) {
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    if (dtype == 1) {
        const long long total = (long long)n * Ho * Wo * (C / 8);
        hipLaunchKernelGGL((pool_add_kernel<bf16_t, 8>), dim3(grid_for(total, 256)), dim3(256), 0, s,
                           (const bf16_t*)y, (const bf16_t*)res, (bf16_t*)out, n, Hi, Wi, Ho, Wo, C);
    } else if (dtype == 2) {
        const long long total = (long long)n * Ho * Wo * (C / 8);
        hipLaunchKernelGGL((pool_add_kernel<f16_t, 8>), dim3(grid_for(total, 256)), dim3(256), 0, s,
                           (const f16_t*)y, (const f16_t*)res, (f16_t*)out, n, Hi, Wi, Ho, Wo, C);
    } else {
        const long long total = (long long)n * Ho * Wo * (C / 4);
        hipLaunchKernelGGL((pool_add_kernel<float, 4>), dim3(grid_for(total, 256)), dim3(256), 0, s,
                           (const float*)y, (const float*)res, (float*)out, n, Hi, Wi, Ho, Wo, C);
    }
    return (int)hipGetLastError();
}

int launch_gap(const void* x, int n, int HW, int C, int ld, float* feat, float mul, int dtype, hipStream_t s) {
    const long long total = (long long)n * C;
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(gap_kernel<T_>, dim3(grid_for(total, 256)), dim3(256), 0, s,
                                     (const T_*)x, n, HW, C, ld, feat, mul));
    return (int)hipGetLastError();
}

int launch_head_final(const float* h1, int n, int mc_n, int pass0, long long tile0, const long long* tile0_dev, const long long* tile_idx,
                      unsigned seed_lo,
                      unsigned seed_hi, unsigned thresh, float dscale, const float* w2, const float* b2,
                      int init, int finalize, float* state, float* mean2, float* std2, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(head_final_kernel, dim3(n), dim3(64 * kHeadFinalWaves), 0, s, h1, n, mc_n, pass0, tile0, tile0_dev, tile_idx,
                       seed_lo, seed_hi, thresh, dscale, w2, b2, init, finalize, state, mean2, std2);
    return (int)hipGetLastError();
}

static int launch_slide_reduce(const float* mean2, const float* std2, const int32_t* slide_idx, int n,
                               int n_slides, float tile_uq, long long* acc_pred, long long* acc_unc,
                               int32_t* count, hipStream_t s) {
    if (n <= 0) return 0;
    const int use_uq = (tile_uq == tile_uq) && tile_uq != 0.f;  // NaN / 0 disable the filter
    hipLaunchKernelGGL(slide_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, mean2, std2, slide_idx,
                       n, n_slides, tile_uq, use_uq, (unsigned long long*)acc_pred,
                       (unsigned long long*)acc_unc, count);
    return (int)hipGetLastError();
}

static int launch_slide_finish(const long long* acc_pred, const long long* acc_unc, const int32_t* count,
                               int n_slides, double* mean_pred, double* mean_unc, hipStream_t s) {
    if (n_slides <= 0) return 0;
    hipLaunchKernelGGL(slide_finish_kernel, dim3(grid_for(n_slides, 256)), dim3(256), 0, s, acc_pred,
                       acc_unc, count, n_slides, mean_pred, mean_unc);
    return (int)hipGetLastError();
}

int launch_to_f32_nhwc(const void* x, long long rows, int C, int ld, float* out, int dtype, hipStream_t s) {
    const long long total = rows * C;
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(to_f32_nhwc_kernel<T_>, dim3(grid_stride_for(total, 256)), dim3(256), 0, s,
                                     (const T_*)x, rows, C, ld, out));
    return (int)hipGetLastError();
}

// x *= mul in place (mul a power of two: exact), grid-stride
__global__ void scale_f32_kernel(float* __restrict__ x, long long count, float mul) {
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < count; gid += (long long)gridDim.x * blockDim.x) x[gid] *= mul;
}

int launch_scale_f32(float* x, long long count, float mul, hipStream_t s) {
    hipLaunchKernelGGL(scale_f32_kernel, dim3(grid_stride_for(count, 256)), dim3(256), 0, s, x, count, mul);
    return (int)hipGetLastError();
}

// out[r][c] = x[r][c] of a 16-bit tensor of either type, rows of ld elements made compact: eight elements, 16 bytes, per load and
// store (C and ld multiples of 8, both pointers 16-byte aligned), grid-stride
__global__ void copy16_nhwc_kernel(const uint4* __restrict__ x, long long rows, int C8, int ld8, uint4* __restrict__ out) {
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < rows * C8; gid += (long long)gridDim.x * blockDim.x) {
        const long long r = gid / C8;
        out[gid] = x[r * ld8 + (gid - r * C8)];
    }
}

int launch_copy16_nhwc(const void* x, long long rows, int C, int ld, void* out, hipStream_t s) {
    if (C % 8 || ld % 8 || ((uintptr_t)x | (uintptr_t)out) % 16) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(copy16_nhwc_kernel, dim3(grid_stride_for(rows * (C / 8), 256)), dim3(256), 0, s, (const uint4*)x, rows, C / 8, ld / 8,
                       (uint4*)out);
    return (int)hipGetLastError();
}

int launch_nchw_to_f32_nhwc(const void* x, int n, int C, int HW, float* out, int dtype, hipStream_t s) {
    const long long total = (long long)n * C * HW;
    BQ_DISPATCH_T(dtype,
                  hipLaunchKernelGGL(nchw_to_f32_nhwc_kernel<T_>, dim3(grid_stride_for(total, 256)), dim3(256), 0,
                                     s, (const T_*)x, n, C, HW, out));
    return (int)hipGetLastError();
}

extern "C" {

int bq_stage(bq_ctx* c, const uint8_t* d_tiles, int n, void* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || n < 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_stage: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stage_u8_standardize", 4.0 * n * kStaged, (double)n * kStaged * (1.0 + esize(c)));
    if (launch_stage_u8(d_tiles, n, 299, d_out, c->cfg.dtype, c->d_stage_stats, s))
        return fail(c, BQ_ERR_HIP, "stage launch failed");
    return BQ_OK;
}

int bq_stage_f32(bq_ctx* c, const float* d_tiles, int n, void* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || n < 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_stage_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stage_f32_to_planar", 0.0, (double)n * kStaged * (4.0 + esize(c)));
    if (launch_stage_f32(d_tiles, n, 299, d_out, c->cfg.dtype, s)) return fail(c, BQ_ERR_HIP, "stage launch failed");
    return BQ_OK;
}

int bq_slide_reduce(bq_ctx* c, const float* d_mean2, const float* d_std2, const int32_t* d_slide_idx, int n,
                    int n_slides, float tile_uq, int64_t* d_acc_pred, int64_t* d_acc_unc, int32_t* d_count,
                    bq_stream_t stream) {
    if (!c || !d_mean2 || !d_std2 || !d_slide_idx || !d_acc_pred || !d_acc_unc || !d_count || n < 0 || n_slides <= 0)
        return fail(c, BQ_ERR_ARG, "bq_slide_reduce: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "slide_reduce", 2.0 * n, 20.0 * n);
    if (launch_slide_reduce(d_mean2, d_std2, d_slide_idx, n, n_slides, tile_uq, (long long*)d_acc_pred,
                            (long long*)d_acc_unc, d_count, s))
        return fail(c, BQ_ERR_HIP, "slide_reduce launch failed");
    return BQ_OK;
}

int bq_slide_finish(bq_ctx* c, const int64_t* d_acc_pred, const int64_t* d_acc_unc, const int32_t* d_count,
                    int n_slides, double* d_mean_pred, double* d_mean_unc, bq_stream_t stream) {
    if (!c || !d_acc_pred || !d_acc_unc || !d_count || !d_mean_pred || !d_mean_unc || n_slides <= 0)
        return fail(c, BQ_ERR_ARG, "bq_slide_finish: bad argument");
    if (launch_slide_finish((const long long*)d_acc_pred, (const long long*)d_acc_unc, d_count, n_slides,
                            d_mean_pred, d_mean_unc, (hipStream_t)stream))
        return fail(c, BQ_ERR_HIP, "slide_finish launch failed");
    return BQ_OK;
}

}  // extern "C"
