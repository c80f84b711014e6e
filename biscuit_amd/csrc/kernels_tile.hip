// block1_conv2 (3x3 valid convolution 32 -> 64, 149x149 -> 147x147) of the float / planar entry in a 16-bit context: bq_backbone
// (UncertaintyInterface: standardised float tiles), bq_debug_activation, and a blob without "block1_conv1/w16" /
// "block1_conv2/wp16".  choose_route (biscuit_hip.hip) names it "TILE kind=0".  The uint8 entry -- the headline path -- runs this
// layer inside kernels_front.hip, bit-compatible with this kernel (same tap order, same rounding points): tests/test_gpu_parity.py
// runs both entries.
//
// Persistent 2-D tile kernel for a big, HBM-bound layer with a tiny GEMM (K = 288, N = 64): what matters is that
// every input byte is fetched once, in coalesced 16-byte pieces, with enough loads in flight,
// and that nothing but the final activations is written.  Design:
//  * Persistent workgroups (4 waves) walk 8x16-pixel output tiles of the image grid.
//  * The layer's weights are copied ONCE per workgroup into LDS in MFMA fragment order
//    (18 KB) and stay there: no per-tile weight stream from L2.
//  * Per tile the (8+2)x(16+2) input halo is loaded with all of a thread's 16-byte loads in
//    flight at once, zero-filled outside the image, and the loads of
//    tile t+1 are issued before tile t is computed (register prefetch across the tile loop).
//  * No A tile: the MFMA operand layout D[cout][pixel] = W[cout][k] * Act[k][pixel]
//    wants, per lane, 8 consecutive k of ONE pixel -- 16 bytes of a shifted halo pixel.  Each wave
//    owns two tile rows (32 pixels = one 32x32 fragment) and reads its operands straight from the
//    halo in LDS.
//  * Epilogue: folded BN + ReLU in registers, tile parked in LDS (aliasing the dead halo),
//    streamed out as 16 x Cout x 2 B contiguous row segments.
#include "gemm_common.h"

namespace {
using namespace bqk;

constexpr int TH = 8, TW = 16, RH = TH + 2, RW = TW + 2, RPIX = RH * RW;   // 180 halo pixels

__device__ __forceinline__ unsigned relu2(unsigned x) { return relu_pk16(x); }   // ReLU on two packed bf16 / f16

template <typename T>
struct TileParams {
    const T* in;           // NHWC [n][Hi][Wi][CIN]
    const uint4* wp;       // fragment-packed weights [NF][KB][64] x 16 B
    const float* unused0;  // of the retired separable kernels; kept, as unused1: without them hipcc schedules this kernel differently
    const float* scale;    // [NF*32]
    const float* bias;
    T* out;                // NHWC [n][H][W][NF*32]
    int n, H, W, Hi, Wi;   // output / input maps
    int tyn, txn;          // tiles per image
    int relu;
    int unused1;
};

// 3x3 valid convolution (block1_conv2).  WPE = waves per SIMD the register budget is set for (= persistent workgroups per CU).
template <typename T, int CIN, int NF, bool RELU_IN, int WPE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
tile_conv_kernel(const TileParams<T> p) {
    if constexpr (H16<T>::F16) bq_f16_saturate();
    constexpr int NT = 256;
    constexpr int CC = CIN < 64 ? CIN : 64;            // channels staged per pass (<= 64)
    constexpr int NPASS = CIN / CC;
    constexpr int PPP = CC / 8;                        // 16-byte pieces per halo pixel and pass
    constexpr int PS = CC * 2 + 16;                    // halo pixel stride in LDS (odd # of 16-B slots)
    // Halo row pitch padded to a multiple of 16 slots: a ds_read_b128 lane group mixes pixels
    // 0-3/12-15 of one tile row with 4-11 of the next; with pitch = 0 (mod 16 slots) the second
    // row lands exactly on the slots the first leaves free (measured 24 % conflict cycles before)
    constexpr int RP = (RW * PS + 255) / 256 * 256;
    constexpr int KB = 9 * CIN / 16;
    constexpr int KBP = KB / NPASS;                    // k-blocks per pass
    constexpr int NLOAD = (RPIX * PPP + NT - 1) / NT;  // raw 16-byte loads per thread and pass
    constexpr int N = NF * 32;
    constexpr int SST = N * 2 + 16;                    // staging row stride
    constexpr int W_BYTES = NF * KB * 1024;
    // folded-BN scale | bias as fp32 [2][N] in LDS -- unless three workgroups per CU leave no room for it (LDS is
    // handed out in 1280-byte granules: +1 KB can cost the third workgroup)
    constexpr bool SB_LDS = WPE < 3;
    constexpr int SB_OFF = W_BYTES;
    constexpr int BUF_OFF = SB_OFF + (SB_LDS ? 2 * N * 4 : 0);   // raw halo / output staging share this region
    static_assert(NPASS == 1, "the 3x3 conv stages all its channels at once");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;

    // ---- one-time: weights (fragment order) -> LDS
    for (int i = tid; i < W_BYTES / 16; i += NT)
        *reinterpret_cast<uint4*>(smem + i * 16) = p.wp[i];

    if (SB_LDS) {
        for (int i = tid; i < N; i += NT) {
            reinterpret_cast<float*>(smem + SB_OFF)[i] = p.scale[i];
            reinterpret_cast<float*>(smem + SB_OFF)[N + i] = p.bias[i];
        }
    }

    const int tiles_per_img = p.tyn * p.txn;
    const int ntiles = p.n * tiles_per_img;

    // tile-independent part of this thread's halo pieces: (ry, rx) and the element offset
    int rel[NLOAD], ryx[NLOAD];
#pragma unroll
    for (int q = 0; q < NLOAD; ++q) {
        const int idx = tid + q * NT;
        const int pix = idx / PPP, j = idx - pix * PPP;
        const int ry = pix / RW, rx = pix - ry * RW;
        rel[q] = (ry * p.Wi + rx) * CIN + j * 8;
        ryx[q] = pix < RPIX ? ((ry << 8) | rx) : -1;
    }
    uint4 rreg[NLOAD];
    // issue the halo loads of (tile, pass) into registers; zeros outside the image
    auto load_pass = [&](int tile, int pass) {
        const int img = tile / tiles_per_img;
        const int trem = tile - img * tiles_per_img;
        const int ty = trem / p.txn, tx = trem - ty * p.txn;
        const int gy0 = ty * TH, gx0 = tx * TW;         // valid convolution: the halo starts at the tile origin
        const long long base = ((long long)(img * p.Hi + gy0) * p.Wi + gx0) * CIN + pass * CC;
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int gy = gy0 + (ryx[q] >> 8), gx = gx0 + (ryx[q] & 255);
            const bool ok = ryx[q] >= 0 && (unsigned)gy < (unsigned)p.Hi && (unsigned)gx < (unsigned)p.Wi;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *reinterpret_cast<const uint4*>(p.in + base + rel[q]);
            if (RELU_IN) { v.x = relu2(v.x); v.y = relu2(v.y); v.z = relu2(v.z); v.w = relu2(v.w); }
            rreg[q] = v;
        }
    };
    auto store_pass = [&]() {
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int idx = tid + q * NT;
            const int pix = idx / PPP, j = idx - pix * PPP;
            if (ryx[q] >= 0)
                *reinterpret_cast<uint4*>(smem + BUF_OFF + (ryx[q] >> 8) * RP + (ryx[q] & 255) * PS + j * 16) = rreg[q];
        }
    };

    int tile = blockIdx.x;
    if (tile < ntiles) load_pass(tile, 0);
    // this wave's pixels: tile rows 2*wave and 2*wave+1, lane&31 -> (row, column)
    const int py = 2 * wave + (r32 >> 4), px = r32 & 15;
    const int raw_lane = BUF_OFF + py * RP + px * PS;          // halo pixel of tap (0,0)

    for (; tile < ntiles; tile += gridDim.x) {
        f32x16 acc[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

#pragma unroll 1
        for (int pass = 0; pass < NPASS; ++pass) {
            __syncthreads();             // previous readers of the halo / staging region are done
            store_pass();
            __syncthreads();             // halo (and, first time, weights) visible
            // next halo in flight while this one is computed
            if (pass + 1 < NPASS) load_pass(tile, pass + 1);
            else if (tile + (int)gridDim.x < ntiles) load_pass(tile + gridDim.x, 0);

#pragma unroll 2
            for (int kl = 0; kl < KBP; ++kl) {
                const int kb = pass * KBP + kl;
                // k = tap*CIN + channel: this k-block is 16 channels of one tap
                const int tap = (kb * 16) / CIN, c0 = (kb * 16) % CIN;
                const int dy = tap / 3, dx = tap - dy * 3;
                const uint4 opnd = *reinterpret_cast<const uint4*>(smem + raw_lane + dy * RP + dx * PS + (c0 + h * 8) * 2);
#pragma unroll
                for (int j = 0; j < NF; ++j) {
                    const uint4 wf = *reinterpret_cast<const uint4*>(smem + ((j * KB + kb) * 64 + lane) * 16);
                    mma<T>(acc[j], wf, opnd);
                }
            }
        }

        // ---- epilogue: BN + ReLU in registers -> LDS staging (aliases the halo) -> row segments.
        // Scale and bias come from LDS (per tile they would be 32 KB of L1 traffic per wave, more than the
        // tile's own pixels); ReLU is a packed int16 max on the converted pair (0x8000 = no-op).
        __syncthreads();                 // every wave is done reading the halo
        {
            const unsigned lo2 = p.relu ? 0u : 0x80008000u;
            const float* sbl = (SB_LDS ? reinterpret_cast<const float*>(smem + SB_OFF) : p.scale) + h * 4;
            const float* bbl = (SB_LDS ? reinterpret_cast<const float*>(smem + SB_OFF) + N : p.bias) + h * 4;
            unsigned char* row = smem + BUF_OFF + (wave * 32 + r32) * SST + h * 8;
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ng = j * 32 + g * 8;
                    const float4 sc = *reinterpret_cast<const float4*>(sbl + ng);
                    const float4 bi = *reinterpret_cast<const float4*>(bbl + ng);
                    const float v0 = fmaf(acc[j][g * 4 + 0], sc.x, bi.x), v1 = fmaf(acc[j][g * 4 + 1], sc.y, bi.y);
                    const float v2 = fmaf(acc[j][g * 4 + 2], sc.z, bi.z), v3 = fmaf(acc[j][g * 4 + 3], sc.w, bi.w);
                    uint2 o;
                    o.x = H16<T>::pack2(v0, v1);
                    o.y = H16<T>::pack2(v2, v3);
                    asm("v_pk_max_i16 %0, %1, %2" : "=v"(o.x) : "v"(o.x), "v"(lo2));
                    asm("v_pk_max_i16 %0, %1, %2" : "=v"(o.y) : "v"(o.y), "v"(lo2));
                    *reinterpret_cast<uint2*>(row + ng * 2) = o;
                }
        }
        __syncthreads();
        {
            const int img = tile / tiles_per_img;
            const int trem = tile - img * tiles_per_img;
            const int ty = trem / p.txn, tx = trem - ty * p.txn;
            constexpr int PPR = N * 2 / 16;            // 16-byte pieces per output pixel
            for (int idx = tid; idx < TH * TW * PPR; idx += NT) {
                const int pix = idx / PPR, pc = idx - pix * PPR;
                const int oy = ty * TH + (pix >> 4), ox = tx * TW + (pix & 15);
                if (oy < p.H && ox < p.W)
                    *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(p.out) +
                                              (((size_t)(img * p.H + oy) * p.W + ox) * N) * 2 + pc * 16) =
                        *reinterpret_cast<const uint4*>(smem + BUF_OFF + pix * SST + pc * 16);
            }
        }
    }
}

template <typename T, int CIN, int NF, bool RELU_IN, int WPE>
int launch_tile(const TileParams<T>& p, int num_cus, hipStream_t s) {
    constexpr int KB = 9 * CIN / 16;
    constexpr size_t W_BYTES = (size_t)NF * KB * 1024;
    constexpr size_t RAW_BYTES = (size_t)RH * ((RW * ((CIN < 64 ? CIN : 64) * 2 + 16) + 255) / 256 * 256);
    constexpr size_t STAGE_BYTES = (size_t)TH * TW * (NF * 64 + 16);
    constexpr size_t lds = W_BYTES + (WPE < 3 ? (size_t)NF * 32 * 8 : 0) + (RAW_BYTES > STAGE_BYTES ? RAW_BYTES : STAGE_BYTES);
    static_assert(lds <= 160 * 1024, "tile kernel LDS budget");
    auto kern = tile_conv_kernel<T, CIN, NF, RELU_IN, WPE>;
    static BqLdsAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(kern), lds)) return e;
    const int per_cu = (int)((160 * 1024) / lds) < 1 ? 1 : (int)((160 * 1024) / lds);
    const int wgs = per_cu > WPE ? WPE : per_cu;     // persistent workgroups per CU = waves per SIMD
    const int ntiles = p.n * p.tyn * p.txn;
    int grid = num_cus * wgs;
    if (grid > ntiles) grid = ntiles;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, p);
    return (int)hipGetLastError();
}

template <typename T>
int launch_tile_conv_t(const void* in, const void* wp, const float* scale, const float* bias, void* out, int n, int H, int W, int Hi,
                       int Wi, int relu, int num_cus, hipStream_t s) {
    TileParams<T> p{};
    p.in = reinterpret_cast<const T*>(in);
    p.wp = reinterpret_cast<const uint4*>(wp);
    p.scale = scale; p.bias = bias;
    p.out = reinterpret_cast<T*>(out);
    p.n = n; p.H = H; p.W = W; p.Hi = Hi; p.Wi = Wi;
    p.tyn = (H + TH - 1) / TH; p.txn = (W + TW - 1) / TW;
    p.relu = relu;
    return launch_tile<T, 32, 2, false, 2>(p, num_cus, s);
}

}  // namespace

int launch_tile_conv(int dtype, const void* in, const void* wp, const float* scale, const float* bias, void* out, int n, int H,
                     int W, int Hi, int Wi, int relu, int num_cus, hipStream_t s) {
    return dtype == 2 ? launch_tile_conv_t<f16_t>(in, wp, scale, bias, out, n, H, W, Hi, Wi, relu, num_cus, s)
                      : launch_tile_conv_t<bf16_t>(in, wp, scale, bias, out, n, H, W, Hi, Wi, relu, num_cus, s);
}
