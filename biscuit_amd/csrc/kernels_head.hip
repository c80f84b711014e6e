// MC-dropout head, the two Dense(1024, relu) layers (K6; biscuit/hp.py:11,13,21; the UQ loop of results.py:257-258):
//     out[row][n] = relu( bias[n] + sum_k dropout(x[row][k]) * W[k][n] ),   rows = tiles x passes
// Round 3.  Rounds 1-2 ran these as exact-fp32 MFMAs (v_mfma_f32_32x32x2_f32, 1/16 of the 16-bit matrix rate): 0.48 ms
// per batch, 68 % of that pipe's peak.  Here every fp32 operand is split on the fly into two IEEE halves,
//     v = hi + lo / 2^11,   hi = f16(v),   lo = f16((v - hi) * 2^11)      (22 significand bits together; the scale keeps
//                                                                          lo out of the subnormals)
// and the product is three f16 MFMAs with fp32 accumulation,
//     x * w  ~  hi_x hi_w  +  2^-11 (hi_x lo_w + lo_x hi_w)               (the dropped lo lo term is 2^-22 of the product)
// into two accumulator sets that are combined once at the end.  Every f16 x f16 product is exact in fp32, so the result
// carries the rounding of the fp32 accumulation only: measured against float64 on this network's own tensors the
// three-term form is as close as a plain fp32 GEMM (rms 4.6e-7 both, oracle tolerance of the tests 1e-6).  It is the
// head of ALL three storage types -- the backbone's type never reaches it.
//
// Workgroup = 8 waves = 64 rows x 512 columns (grid: row tiles x 2 column halves: 240 workgroups at 7 680 rows, and half
// the weight traffic of 32-row tiles); wave w owns the 2 x 2 fragments of 32x32 at columns [64 w, 64 w + 64).  K is
// walked in chunks of 512: the producer draws the Philox4x32-10 masks (counter = (unit / 4, layer, pass, global tile),
// key = seed: the contract of oracle/philox.py), applies the inverted dropout, splits and writes the two A planes to
// LDS; the matrix stage reads A fragments from LDS and streams the pre-split weight fragments (host-packed hi / lo in
// fragment order) from L2 through a register ring.
//
// Range.  The split is fp32-grade only for about 2^-14 <= |v| < 2^16: below, hi and lo turn subnormal and lose bits; above,
// both saturate (MODE.FP16_OVFL) and 1e5 would be read as 65536.  So both operands carry power-of-two exponents:
//   * per row, e: the producer multiplies by dscale * 2^-e instead of dscale.  Layer 0 takes e from max |x| * dscale of the
//     row's feature row (a prologue over the 1-64 tiles of the workgroup); layer 1 from max |h0| * dscale, which the layer-0
//     epilogue leaves in rmax[row][column half];
//   * per layer, s: the weights are stored as W * 2^-s (weights.py: head_weight_exponent, "hidden_N/wexp" of the blob).
// The epilogue multiplies the accumulator by 2^(e + s) before the bias.  Both scalings are exact.  An exponent is 0 whenever
// its peak lies in [2^-8, 2^14] (today's networks: the same bits as without exponents); otherwise it brings the peak to
// [2^13, 2^14).
//
// Non-finite operands.  The f16 MFMAs do not carry a NaN operand into the sum (a NaN feature acted as 0; an inf one gave inf,
// its NaN lo part dropped), so the producer notes a kept operand that is not finite (fma(f, 0, nf) turns NaN once one is met)
// and the epilogue writes NaN for the whole row; the ReLU passes NaN through.  A non-finite input never gives a plausible result.
#include "gemm_common.h"

namespace {
using namespace bqk;

constexpr int HM = 64, HN = 512;            // rows, columns per workgroup
constexpr float HSCALE = 2048.f, HINV = 1.f / 2048.f;

struct HeadParams {
    const float* in;        // [tiles][K] (in_row_is_tile) or [rows][K]
    const float* rmax_in;   // layer 1: [rows][2] max |h0| per row and column half (written by layer 0), else null
    float* rmax_out;        // layer 0: where to write it, else null
    const uint4* wh;        // f16(W) in fragment order [1024 / 32][K / 16][64] x 16 B
    const uint4* wl;        // f16((W - hi) * 2^11), same order
    const float* bias;      // [1024]
    float* out;             // [rows][1024]
    int rows, K;
    int mc_n, pass0, in_row_is_tile, layer;
    unsigned seed_lo, seed_hi, thresh;
    float dscale;
    int wexp;               // the weights are stored as W * 2^-wexp
    long long tile0;
    const long long* tile0_dev;
    const long long* tile_idx;  // per-tile Philox indices [tiles] (bq_set_tile_index_array) or null: tile i counts as tile0 + i
};

// Power-of-two exponent of a row whose largest split operand is `peak`: 0 in [2^-8, 2^14] (and for 0, NaN, inf), else the e that
// brings the peak to [2^13, 2^14), within [-64, 64] so that dscale * 2^-e stays a normal float.
__device__ __forceinline__ int head_row_exp(float peak) {
    if (!(peak > 0.f) || !__builtin_isfinite(peak) || (peak >= 0x1p-8f && peak <= 0x1p14f)) return 0;
    const int e = ilogbf(peak) - 13;
    return e < -64 ? -64 : (e > 64 ? 64 : e);
}

// ReLU that keeps NaN (fmaxf(NaN, 0) is 0); the same bits as fmaxf(v, 0) otherwise.
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

__device__ __forceinline__ float max4(float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float4 fabs4(float4 v) { return make_float4(fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)); }

__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
    hi = H16<f16_t>::pack2(a, b);
    const float ra = (a - H16<f16_t>::lo(hi)) * HSCALE, rb = (b - H16<f16_t>::hi(hi)) * HSCALE;
    lo = H16<f16_t>::pack2(ra, rb);
}

// Producer and matrix stage overlapped (round 5; rounds 3-4 ran them in lock step -- barrier, every wave draws Philox masks and
// splits (vector ALU, ~9 us per 512-deep chunk), barrier, every wave multiplies (matrix pipe, ~12 us) -- so each pipe idled while the
// other worked: 0.155 ms for layer 0 where this takes 0.123).  The A planes are double-buffered (chunks of 256: 2 x 2 x 33 KB of
// LDS) and a chunk step is "produce chunk c + 1, multiply chunk c" for waves 0-3 and "multiply chunk c, produce chunk c + 1" for
// waves 4-7: waves w and w + 4 of a workgroup share a SIMD, so the two waves of a SIMD are in opposite stages; one barrier per chunk.
constexpr int PKC = 256;
constexpr int PSTR = PKC * 2 + 16;          // 33 slots of 16 B
constexpr int PPLANE = HM * PSTR;

__global__ void __launch_bounds__(512) head_dense_pipe_kernel(const HeadParams p) {
    bq_f16_saturate();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [buffer][hi | lo] planes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * HM;
    const int nf0 = blockIdx.y * (HN / 32) + wave * 2;
    const int KB = p.K / 16;
    const long long tile0 = p.tile0 + (p.tile0_dev ? *p.tile0_dev : 0);
    const int prow = tid >> 3, pseg = tid & 7;
    const int pm = m0 + prow;
    const bool plive = pm < p.rows;
    const int ptile = plive ? pm / p.mc_n : 0;
    const int ppass = p.pass0 + (plive ? pm - ptile * p.mc_n : 0);
    const unsigned pctr = (unsigned)(tile0 + (p.tile_idx ? p.tile_idx[ptile] : (long long)ptile));   // the Philox tile counter of this row
    const float* prow_ptr = p.in + (size_t)(p.in_row_is_tile ? ptile : (plive ? pm : 0)) * p.K;

    // Row exponents (see the header).  Layer 0: max |x| of each of the tiles the 64 rows belong to, one tile per pass of the
    // whole workgroup over its K / 4 float4 (K / 4 is a multiple of 64, so every wave stays on one tile and loops as a whole).
    __shared__ int rexp[HM];
    __shared__ int rbad[HM];                        // the row met a kept operand that is not finite
    if (tid < HM) rbad[tid] = 0;
    if (p.in_row_is_tile) {
        __shared__ unsigned tmax[HM];               // float bits of non-negative maxima order as unsigned integers
        const int t0 = m0 / p.mc_n;
        const int nt = ((m0 + HM < p.rows ? m0 + HM : p.rows) - 1) / p.mc_n - t0 + 1;
        const int kq = p.K >> 2;
        if (tid < HM) tmax[tid] = 0u;
        __syncthreads();
        for (int j = tid; j < nt * kq; j += 512) {
            const int lt = j / kq;
            float a = max4(fabs4(*reinterpret_cast<const float4*>(p.in + (size_t)(t0 + lt) * p.K + (size_t)(j - lt * kq) * 4)));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
            if (lane == 0) atomicMax(&tmax[lt], __float_as_uint(a));
        }
        __syncthreads();
        if (tid < HM) rexp[tid] = m0 + tid < p.rows ? head_row_exp(__uint_as_float(tmax[(m0 + tid) / p.mc_n - t0]) * p.dscale) : 0;
    } else if (tid < HM) {
        const int m = m0 + tid;
        rexp[tid] = m < p.rows ? head_row_exp(fmaxf(p.rmax_in[2 * (size_t)m], p.rmax_in[2 * (size_t)m + 1]) * p.dscale) : 0;
    }
    __syncthreads();
    const float pscale = ldexpf(p.dscale, -rexp[prow]);     // dscale * 2^-e of the producer's row (exact)
    float nf = 0.f;                                          // NaN once a kept operand of this thread was not finite

    f32x16 acc1[2][2], acc2[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc1[i][j][e] = 0.f; acc2[i][j][e] = 0.f; }
    const uint4* bh0 = p.wh + (size_t)nf0 * KB * 64 + lane;
    const uint4* bl0 = p.wl + (size_t)nf0 * KB * 64 + lane;
    constexpr int PF = 2;
    uint4 bh[PF][2], bl[PF][2];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            bh[d][j] = bh0[((size_t)j * KB + d) * 64];
            bl[d][j] = bl0[((size_t)j * KB + d) * 64];
        }

    auto produce = [&](int k0, int buf) {
        unsigned char* const base = smem + buf * 2 * PPLANE;
        float4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float4*>(prow_ptr + k0 + (i * 8 + pseg) * 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gi = i * 8 + pseg;
            const int g = (k0 >> 2) + gi;
            unsigned rnd[4];
            philox4x32_10((unsigned)g, (unsigned)p.layer, (unsigned)ppass, pctr, p.seed_lo, p.seed_hi, rnd);
            const float f0 = (plive && rnd[0] >= p.thresh) ? v[i].x * pscale : 0.f;
            const float f1 = (plive && rnd[1] >= p.thresh) ? v[i].y * pscale : 0.f;
            const float f2 = (plive && rnd[2] >= p.thresh) ? v[i].z * pscale : 0.f;
            const float f3 = (plive && rnd[3] >= p.thresh) ? v[i].w * pscale : 0.f;
            nf = fmaf(f0, 0.f, fmaf(f1, 0.f, fmaf(f2, 0.f, fmaf(f3, 0.f, nf))));
            uint2 hi, lo;
            split2(f0, f1, hi.x, lo.x);
            split2(f2, f3, hi.y, lo.y);
            const int off = prow * PSTR + gi * 8;
            *reinterpret_cast<uint2*>(base + off) = hi;
            *reinterpret_cast<uint2*>(base + PPLANE + off) = lo;
        }
        if (nf != nf) rbad[prow] = 1;                        // (read after the loop's last barrier)
    };
    auto multiply = [&](int k0, int buf) {
        const unsigned char* a_hi = smem + buf * 2 * PPLANE + r32 * PSTR + h * 16;
        const unsigned char* a_lo = a_hi + PPLANE;
        const int kb0 = k0 / 16;
#pragma unroll 2
        for (int kl = 0; kl < PKC / 16; ++kl) {
            const int d = kl & (PF - 1);
            uint4 ah[2], al[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const uint4*>(a_hi + i * 32 * PSTR + kl * 32);
                al[i] = *reinterpret_cast<const uint4*>(a_lo + i * 32 * PSTR + kl * 32);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    mma<f16_t>(acc1[i][j], bh[d][j], ah[i]);
                    mma<f16_t>(acc2[i][j], bh[d][j], al[i]);
                    mma<f16_t>(acc2[i][j], bl[d][j], ah[i]);
                }
            const int nx = kb0 + kl + PF;
            const int idx = nx < KB ? nx : KB - 1;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bh[d][j] = bh0[((size_t)j * KB + idx) * 64];
                bl[d][j] = bl0[((size_t)j * KB + idx) * 64];
            }
        }
    };

    const int NC = p.K / PKC;
    produce(0, 0);
    __syncthreads();
    const bool first_produce = (wave >> 2) == 0;      // (wave-uniform)
    for (int c = 0; c < NC; ++c) {
        const bool more = c + 1 < NC;
        if (first_produce) {
            if (more) produce((c + 1) * PKC, (c + 1) & 1);
            multiply(c * PKC, c & 1);
        } else {
            multiply(c * PKC, c & 1);
            if (more) produce((c + 1) * PKC, (c + 1) & 1);
        }
        __syncthreads();
    }
    int oexp[2];                                    // 2^(e + s) of the two rows this lane writes
    bool bad[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        oexp[i] = rexp[i * 32 + r32] + p.wexp;
        bad[i] = rbad[i * 32 + r32] != 0;
    }
    float rmax[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n0 = (nf0 + j) * 32 + g * 8 + h * 4;
            const float4 b = *reinterpret_cast<const float4*>(p.bias + n0);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + i * 32 + r32;
                if (m < p.rows) {
                    float4 o;
                    o.x = relu_nan(ldexpf(fmaf(acc2[i][j][g * 4 + 0], HINV, acc1[i][j][g * 4 + 0]), oexp[i]) + b.x);
                    o.y = relu_nan(ldexpf(fmaf(acc2[i][j][g * 4 + 1], HINV, acc1[i][j][g * 4 + 1]), oexp[i]) + b.y);
                    o.z = relu_nan(ldexpf(fmaf(acc2[i][j][g * 4 + 2], HINV, acc1[i][j][g * 4 + 2]), oexp[i]) + b.z);
                    o.w = relu_nan(ldexpf(fmaf(acc2[i][j][g * 4 + 3], HINV, acc1[i][j][g * 4 + 3]), oexp[i]) + b.w);
                    if (bad[i]) o = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
                    *reinterpret_cast<float4*>(p.out + (size_t)m * 1024 + n0) = o;
                    rmax[i] = fmaxf(rmax[i], max4(o));
                }
            }
        }
    if (p.rmax_out) {
        // max over this workgroup's 512 columns of each row: the two lane halves, then the eight waves through LDS (the A planes
        // are free since the loop's last barrier)
        float* red = reinterpret_cast<float*>(smem);          // [8 waves][64 rows]
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rmax[i] = fmaxf(rmax[i], __shfl_xor(rmax[i], 32));
            if (h == 0) red[wave * HM + i * 32 + r32] = rmax[i];
        }
        __syncthreads();
        if (tid < HM && m0 + tid < p.rows) {
            float r = red[tid];
#pragma unroll
            for (int w = 1; w < 8; ++w) r = fmaxf(r, red[w * HM + tid]);
            p.rmax_out[2 * (size_t)(m0 + tid) + blockIdx.y] = r;
        }
    }
}

}  // namespace

// One Dense(1024, relu) layer of the MC head over `rows` = tiles x passes rows.  K = 2048 (layer 0) or 1024 (layer 1).
// Layer 0 (in_row_is_tile) writes rmax [rows][2], layer 1 reads it (see the header).
int launch_head_dense(const float* in, const void* wh, const void* wl, const float* bias, int wexp, float* out, float* rmax,
                      int rows, int K, int mc_n, int pass0, int in_row_is_tile, int layer, unsigned seed_lo, unsigned seed_hi,
                      unsigned thresh, float dscale, long long tile0, const long long* tile0_dev, const long long* tile_idx,
                      hipStream_t s) {
    if (rows <= 0) return 0;
    if (K % PKC != 0 || !wh || !wl || !bias || !rmax) return (int)hipErrorInvalidValue;
    HeadParams p;
    p.in = in; p.rmax_in = in_row_is_tile ? nullptr : rmax; p.rmax_out = in_row_is_tile ? rmax : nullptr; p.wexp = wexp;
    p.wh = reinterpret_cast<const uint4*>(wh); p.wl = reinterpret_cast<const uint4*>(wl);
    p.bias = bias; p.out = out; p.rows = rows; p.K = K;
    p.mc_n = mc_n; p.pass0 = pass0; p.in_row_is_tile = in_row_is_tile; p.layer = layer;
    p.seed_lo = seed_lo; p.seed_hi = seed_hi; p.thresh = thresh; p.dscale = dscale;
    p.tile0 = tile0; p.tile0_dev = tile0_dev; p.tile_idx = tile_idx;
    constexpr size_t ldsp = 4 * (size_t)PPLANE;
    static BqLdsAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(head_dense_pipe_kernel), ldsp)) return e;
    hipLaunchKernelGGL(head_dense_pipe_kernel, dim3((rows + HM - 1) / HM, 1024 / HN), dim3(512), ldsp, s, p);
    return (int)hipGetLastError();
}
