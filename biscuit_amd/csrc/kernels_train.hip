// Training the MC-dropout head on cached features (DESIGN.md section 7 "Head training"): one step is the gradient of the mean sparse
// categorical cross-entropy of n <= 1024 gathered feature rows through
//     x [n][2048] -> drop -> Dense 1024 + ReLU -> drop -> Dense 1024 + ReLU -> drop -> Dense 2 -> softmax
// (bq_head_grad) and one fused Keras-Adam pass over the P = 3 149 826 parameters (bq_head_adam); bq_head_train_steps is those two in a
// loop, one linear chain of launches on one stream.  The keep masks are the contract of oracle/philox.py -- counter (unit / 4, layer,
// step, row index in the feature cache), key seed -- drawn by bq_common.h's philox4x32_10 wherever a dropped operand is formed, forward
// and backward: no mask and no copied batch is stored.  State is plain fp32 [K][N] tensors in the caller's arrays (the packed hi / lo
// fragments of the inference head, kernels_head.hip, are not touched).
//
// The five GEMMs -- two forward, dx = dz W^T, and dW = drop(x)^T dz of both hidden layers with K = n -- run on the exact f32-input
// MFMA (v_mfma_f32_32x32x2_f32: an fmaf chain in k order, one rounding per product) from 64 x 64 x 32 LDS tiles, four waves of one 32 x 32
// output tile each (four accumulators: the groups of 8 k of a chunk sum separately and are added pairwise at the end); the operands come in either orientation, "k contiguous" (read as ds_read_b128 from rows of 36 floats: the sixteen
// lanes of a read group then cover all 64 banks) or "row contiguous" (four ds_read_b32 of 32 consecutive floats).  Inside a group of 8 k
// the lane half h takes k = 4 h + t in MFMA t, for both operands alike: a fixed order.  The [., 2] logits layer, its softmax, the loss
// and its gradients stay on the vector ALU; the softmax and the loss of a row are evaluated in float64 from the fp32 logits and the
// rows' losses are summed in float64, so the loss carries one rounding beyond the logits' own.
//
// Every sum runs in a fixed order -- the MFMA chains, dW over the batch (the K loop), the bias column sums and the loss (eight row
// groups, then the groups in order), the logits' dot products (an xor tree and four waves in order) -- and there are no floating-point atomics: a repeated
// call gives the same bits.  ReLU's derivative is 0 at 0.  A feature that is not finite reaches the first GEMM as NaN whether its unit is
// kept or dropped, a row index outside the cache or a label above 1 likewise: the loss is then NaN, never a plausible number.
//
// Adam evaluates the update of an element in float64 from its fp32 state and rounds once per stored value, so m', v' and w' are the
// correctly rounded values of the Keras formulas; an element with g = 0 and m = v = 0 keeps its bits.
//
// bq_head_validate (DESIGN.md section 7 "Training schedule") is the forward half alone over n <= 4096 rows, for the validation checks in
// the middle of a training: the same two GEMMs (at rate 0 in the A mode that draws nothing), the same logits and float64 row loss, a hit
// per row, and the two sums in a fixed order.  A row's loss and hit depend on the row only, not on n or on its place in the batch.
//
// Exit-flow fine-tuning (bq_exit_*, bq_adam_n; the section at the end of the file) trains Xception's block 14 in front of this head on
// cached block13_out: its pointwise products are further instantiations of train_gemm_kernel, which is why it lives here.
#include <cmath>
#include <hip/hip_runtime.h>

#include "bq_ctx.h"

namespace {

constexpr int D_IN = 2048, D_H = 1024, D_OUT = 2;
constexpr long long OFF_W0 = 0, OFF_B0 = OFF_W0 + (long long)D_IN * D_H, OFF_W1 = OFF_B0 + D_H, OFF_B1 = OFF_W1 + (long long)D_H * D_H,
                    OFF_W2 = OFF_B1 + D_H, OFF_B2 = OFF_W2 + D_H * D_OUT, P_TOTAL = OFF_B2 + D_OUT;
static_assert(P_TOTAL == 3149826, "the head's parameter count");
constexpr int MAX_N = 1024;

constexpr int TM = 64, TN = 64, TK = 32;        // the workgroup's tile
constexpr int KSTR = TK + 4;                    // floats of a k-contiguous row in LDS
constexpr int TILE_FLOATS = TM * KSTR;          // >= TK * TM, the row-contiguous image

struct Drop {
    unsigned layer, step, seed_lo, seed_hi, thresh;
    float scale;
};

// Inverted dropout of the four units 4 g .. 4 g + 3 of the row whose Philox tile counter is ctr; a value that is not finite becomes NaN
// whether kept or not.
__device__ __forceinline__ float4 drop4(float4 v, unsigned g, unsigned ctr, const Drop& d) {
    unsigned r[4];
    philox4x32_10(g, d.layer, d.step, ctr, d.seed_lo, d.seed_hi, r);
    const float nan = __builtin_nanf("");
    float4 o;
    o.x = __builtin_isfinite(v.x) ? (r[0] >= d.thresh ? v.x * d.scale : 0.f) : nan;
    o.y = __builtin_isfinite(v.y) ? (r[1] >= d.thresh ? v.y * d.scale : 0.f) : nan;
    o.z = __builtin_isfinite(v.z) ? (r[2] >= d.thresh ? v.z * d.scale : 0.f) : nan;
    o.w = __builtin_isfinite(v.w) ? (r[3] >= d.thresh ? v.w * d.scale : 0.f) : nan;
    return o;
}

// The derivative v of drop4's four units through their dropout and the ReLU in front of it, whose output there was h: scale v where
// the unit was kept and h > 0, else 0.
__device__ __forceinline__ float4 drop_relu_grad4(float4 h, float4 v, unsigned g, unsigned ctr, const Drop& d) {
    unsigned r[4];
    philox4x32_10(g, d.layer, d.step, ctr, d.seed_lo, d.seed_hi, r);
    float4 o;
    o.x = (h.x > 0.f && r[0] >= d.thresh) ? v.x * d.scale : 0.f;
    o.y = (h.y > 0.f && r[1] >= d.thresh) ? v.y * d.scale : 0.f;
    o.z = (h.z > 0.f && r[2] >= d.thresh) ? v.z * d.scale : 0.f;
    o.w = (h.w > 0.f && r[3] >= d.thresh) ? v.w * d.scale : 0.f;
    return o;
}

// The derivative v of drop4's four units through their dropout alone: scale v where the unit was kept, else 0.
__device__ __forceinline__ float4 drop_grad4(float4 v, unsigned g, unsigned ctr, const Drop& d) {
    unsigned r[4];
    philox4x32_10(g, d.layer, d.step, ctr, d.seed_lo, d.seed_hi, r);
    return make_float4(r[0] >= d.thresh ? v.x * d.scale : 0.f, r[1] >= d.thresh ? v.y * d.scale : 0.f,
                       r[2] >= d.thresh ? v.z * d.scale : 0.f, r[3] >= d.thresh ? v.w * d.scale : 0.f);
}

// what drop4 gives at rate 0 (every unit kept, scale 1), without the draw
__device__ __forceinline__ float4 finite4(float4 v) {
    const float nan = __builtin_nanf("");
    return make_float4(__builtin_isfinite(v.x) ? v.x : nan, __builtin_isfinite(v.y) ? v.y : nan, __builtin_isfinite(v.z) ? v.z : nan,
                       __builtin_isfinite(v.w) ? v.w : nan);
}

// ReLU that keeps NaN, as the inference head's
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// drop(src)[m][k]; src[m][k]; drop(src)[k = batch row][m = unit]; A_DROP_K at rate 0 without its draws (bq_head_validate): src[m][k], NaN for not finite
// A_MAT_K / A_MAT_T (exit-flow fine-tuning): a plain matrix src[m][k] / src[k][m] of any number of rows, no row table behind it
enum AMode : int { A_DROP_K = 0, A_PLAIN_K = 1, A_DROP_T = 2, A_FINITE_K = 3, A_MAT_K = 4, A_MAT_T = 5 };
enum BMode : int { B_ROWS = 0, B_KCONT = 1 };                     // b[k][n]; b[n][k]
// EPI_DX0: EPI_DX without a ReLU in front of the dropout -- the gradient with respect to the head's input
enum Epi : int { EPI_RELU = 0, EPI_DX = 1, EPI_STORE = 2, EPI_DX0 = 3 };

struct TrainGemm {
    const float* a;             // A's source, rows of lda floats
    const float* b;             // B's source, rows of ldb floats
    float* out;                 // [M][ldo]
    const float* bias;          // EPI_RELU: [N]
    const float* h;             // EPI_DX: the layer's own forward output [M][ldo]
    const long long* rows;      // [batch]: the rows' indices in the feature cache, the Philox tile counters
    long long n_feat;           // rows of the feature cache (gather)
    int gather;                 // A's rows are a[rows[i]] (the feature cache) instead of a[i]
    int lda, ldb, ldo;
    int M, N, K;                // M rows x N columns, K summed; N a multiple of 64; K a multiple of 32 unless A_DROP_T / A_MAT_T (then any, M a multiple of 64)
    Drop drop;                  // of A (A_DROP_*) or of the epilogue (EPI_DX, EPI_DX0)
};

// source row of batch row i, or null for one outside the cache
__device__ __forceinline__ const float* a_row(const TrainGemm& p, int i, unsigned& ctr) {
    const long long r = p.rows[i];
    ctr = (unsigned)r;
    if (!p.gather) return p.a + (size_t)i * p.lda;
    return (r >= 0 && r < p.n_feat) ? p.a + (size_t)r * p.lda : nullptr;
}

template <int AM, int BM, int EPI>
__global__ void __launch_bounds__(256) train_gemm_kernel(const TrainGemm p) {
    __shared__ __attribute__((aligned(16))) float As[TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) float Bs[TILE_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const int n0 = blockIdx.x * TN, m0 = blockIdx.y * TM;
    const float nan = __builtin_nanf("");
    constexpr bool AT = AM == A_DROP_T || AM == A_MAT_T;          // A comes as [k][m]
    constexpr bool DXT = EPI == EPI_DX || EPI == EPI_DX0;         // the transposed output tile

    // what this thread brings in per chunk: two float4 of each operand
    // k-contiguous image [64 rows][32 k]: float4 f -> row f >> 3, k 4 (f & 7); row-contiguous [32 k][64 rows]: k f >> 4, row 4 (f & 15)
    const float* arow[2] = {nullptr, nullptr};
    unsigned actr[2] = {0u, 0u};
    bool alive[2] = {false, false};
    if (!AT) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + ((tid + i * 256) >> 3);
            alive[i] = m < p.M;
            if (alive[i]) arow[i] = AM == A_MAT_K ? p.a + (size_t)m * p.lda : a_row(p, m, actr[i]);
        }
    }
    float4 ra0, ra1, rb0, rb1;
    auto fetch = [&](int k0, int i, float4& ra, float4& rb) {
        {
            const int f = tid + i * 256;
            if (AM == A_MAT_T) {
                const int kk = k0 + (f >> 4), u = m0 + (f & 15) * 4;
                ra = kk < p.K ? *reinterpret_cast<const float4*>(p.a + (size_t)kk * p.lda + u) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else if (AM == A_DROP_T) {
                const int kk = k0 + (f >> 4), u = m0 + (f & 15) * 4;       // batch row, first of four units (u + 3 < M: M a multiple of 64)
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kk < p.K) {
                    unsigned ctr;
                    const float* src = a_row(p, kk, ctr);
                    v = src ? *reinterpret_cast<const float4*>(src + u) : make_float4(nan, nan, nan, nan);
                    v = drop4(v, (unsigned)(u >> 2), ctr, p.drop);
                }
                ra = v;
            } else {
                const int k = k0 + (f & 7) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (alive[i]) {
                    v = arow[i] ? *reinterpret_cast<const float4*>(arow[i] + k) : make_float4(nan, nan, nan, nan);
                    if (AM == A_DROP_K) v = drop4(v, (unsigned)(k >> 2), actr[i], p.drop);
                    if (AM == A_FINITE_K) v = finite4(v);
                }
                ra = v;
            }
            if (BM == B_ROWS) {
                const int kk = k0 + (f >> 4), n = n0 + (f & 15) * 4;
                rb = kk < p.K ? *reinterpret_cast<const float4*>(p.b + (size_t)kk * p.ldb + n) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int n = n0 + (f >> 3), k = k0 + (f & 7) * 4;
                rb = *reinterpret_cast<const float4*>(p.b + (size_t)n * p.ldb + k);
            }
        }
    };
    auto stash = [&](int i, const float4& ra, const float4& rb) {
        {
            const int f = tid + i * 256;
            if (AT) *reinterpret_cast<float4*>(As + (f >> 4) * TM + (f & 15) * 4) = ra;
            else *reinterpret_cast<float4*>(As + (f >> 3) * KSTR + (f & 7) * 4) = ra;
            if (BM == B_ROWS) *reinterpret_cast<float4*>(Bs + (f >> 4) * TN + (f & 15) * 4) = rb;
            else *reinterpret_cast<float4*>(Bs + (f >> 3) * KSTR + (f & 7) * 4) = rb;
        }
    };

    // four accumulators, one per group of 8 k of a chunk: four interleaved partial sums of K / 4 terms each, added pairwise at the end
    // (a shorter chain per sum than one accumulator over all of K)
    f32x16 acc4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc4[j][e] = 0.f;

    fetch(0, 0, ra0, rb0);
    fetch(0, 1, ra1, rb1);
    for (int k0 = 0; k0 < p.K; k0 += TK) {
        stash(0, ra0, rb0);
        stash(1, ra1, rb1);
        __syncthreads();
        if (k0 + TK < p.K) {
            fetch(k0 + TK, 0, ra0, rb0);
            fetch(k0 + TK, 1, ra1, rb1);
        }
#pragma unroll
        for (int j = 0; j < TK / 8; ++j) {
            const int kb = 8 * j + 4 * h;
            float a[4], b[4];
            if (AT) {
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] = As[(kb + t) * TM + wm * 32 + r32];
            } else {
                const float4 v = *reinterpret_cast<const float4*>(As + (wm * 32 + r32) * KSTR + kb);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            }
            if (BM == B_ROWS) {
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t] = Bs[(kb + t) * TN + wn * 32 + r32];
            } else {
                const float4 v = *reinterpret_cast<const float4*>(Bs + (wn * 32 + r32) * KSTR + kb);
                b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)     // EPI_DX takes the transposed tile: a lane then holds groups of four units of one batch row
                acc4[j] = DXT ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[t], a[t], acc4[j], 0, 0, 0)
                                        : __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc4[j], 0, 0, 0);
        }
        __syncthreads();
    }

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = (acc4[0][e] + acc4[1][e]) + (acc4[2][e] + acc4[3][e]);
    // D: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    if (DXT) {                  // transposed: column = the batch row, rows = units 8 q + 4 h .. + 3, one Philox draw per group
        const int m = m0 + wm * 32 + r32;
        if (m < p.M) {
            const unsigned ctr = (unsigned)p.rows[m];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 32 + 8 * q + 4 * h;
                const size_t o = (size_t)m * p.ldo + n;
                const float4 dv = make_float4(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
                if (EPI == EPI_DX0) *reinterpret_cast<float4*>(p.out + o) = drop_grad4(dv, (unsigned)(n >> 2), ctr, p.drop);
                else *reinterpret_cast<float4*>(p.out + o) =
                    drop_relu_grad4(*reinterpret_cast<const float4*>(p.h + o), dv, (unsigned)(n >> 2), ctr, p.drop);
            }
        }
    } else {
        const int n = n0 + wn * 32 + r32;
        const float bias = EPI == EPI_RELU ? p.bias[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            const float v = acc[e];
            if (m < p.M) p.out[(size_t)m * p.ldo + n] = EPI == EPI_RELU ? relu_nan(v + bias) : v;
        }
    }
}

// the sum over a workgroup of 256 threads, the same order every time: an xor tree in each wave, then the four waves in order
__device__ __forceinline__ float block_sum_256(float v, float* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// The softmax and the row's loss in float64 from the fp32 logits, each rounded once (a few operations per row); all NaN for a label
// above 1 or a logit that is NaN.
__device__ __forceinline__ double row_loss(float z0, float z1, unsigned y, double& p0, double& p1) {
    const double zd0 = (double)z0, zd1 = (double)z1, mx = fmax(zd0, zd1);
    const double e0 = exp(zd0 - mx), e1 = exp(zd1 - mx), sum = e0 + e1;
    p0 = e0 / sum;
    p1 = e1 / sum;
    double loss = log(sum) - ((y ? zd1 : zd0) - mx);
    if (y > 1u || z0 != z0 || z1 != z1) { loss = __builtin_nan(""); p0 = loss; p1 = loss; }
    return loss;
}

// What both row kernels open with, a workgroup of 256 threads per row, thread t on the units 4 t .. 4 t + 3: the loads (hv: the row's
// h1 there; wa, wb: W2's rows of those units), the logits z = drop(h1) W2 + b2 -- an fmaf chain per thread, then block_sum_256; DROP
// false is rate 0 without the draw --, the label y and, in the threads that `score`, row_loss (loss, p0, p1; 0 in the others).
struct Row { float4 hv, wa, wb; unsigned ctr, y; float z0, z1; double loss, p0, p1; };

template <bool DROP>
__device__ __forceinline__ Row row_forward(const float* __restrict__ h1, const float* __restrict__ w2, const float* __restrict__ b2,
                                           const long long* __restrict__ rows, const unsigned char* __restrict__ label, const Drop& d,
                                           float* lds, bool score) {
    const int m = blockIdx.x, tid = threadIdx.x;
    Row r;
    r.ctr = (unsigned)rows[m];
    r.hv = *reinterpret_cast<const float4*>(h1 + (size_t)m * D_H + tid * 4);
    r.wa = *reinterpret_cast<const float4*>(w2 + tid * 8);
    r.wb = *reinterpret_cast<const float4*>(w2 + tid * 8 + 4);
    const float4 u = DROP ? drop4(r.hv, (unsigned)tid, r.ctr, d) : finite4(r.hv);
    // units 4 tid .. 4 tid + 3: (wa.x, wa.y), (wa.z, wa.w), (wb.x, wb.y), (wb.z, wb.w)
    const float s0 = fmaf(u.w, r.wb.z, fmaf(u.z, r.wb.x, fmaf(u.y, r.wa.z, u.x * r.wa.x)));
    const float s1 = fmaf(u.w, r.wb.w, fmaf(u.z, r.wb.y, fmaf(u.y, r.wa.w, u.x * r.wa.y)));
    r.z0 = block_sum_256(s0, lds) + b2[0];
    r.z1 = block_sum_256(s1, lds) + b2[1];
    r.y = label[m];
    r.loss = r.p0 = r.p1 = 0.0;
    if (score) r.loss = row_loss(r.z0, r.z1, r.y, r.p0, r.p1);
    return r;
}

// A workgroup per batch row: logits = drop(h1) W2 + b2, softmax, the row's loss, dlog = (p - onehot) / n, and
// dz1 = (h1 > 0 and kept) ? scale (dlog . W2[k]) : 0.
__global__ void __launch_bounds__(256) train_logits_kernel(const float* __restrict__ h1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const long long* __restrict__ rows,
                                                           const unsigned char* __restrict__ label, int n, Drop d,
                                                           float* __restrict__ dz1, float* __restrict__ dlog, double* __restrict__ rowloss) {
    __shared__ float lds[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const Row r = row_forward<true>(h1, w2, b2, rows, label, d, lds, true);
    const float g0 = (float)((r.p0 - (r.y == 0u ? 1.0 : 0.0)) / (double)n), g1 = (float)((r.p1 - (r.y == 1u ? 1.0 : 0.0)) / (double)n);
    if (tid == 0) {
        dlog[2 * m] = g0;
        dlog[2 * m + 1] = g1;
        rowloss[m] = r.loss;
    }
    const float4 dv = make_float4(fmaf(g1, r.wa.y, g0 * r.wa.x), fmaf(g1, r.wa.w, g0 * r.wa.z), fmaf(g1, r.wb.y, g0 * r.wb.x),
                                  fmaf(g1, r.wb.w, g0 * r.wb.z));
    float4 o = drop_relu_grad4(r.hv, dv, (unsigned)tid, r.ctr, d);
    if (g0 != g0 || g1 != g1) o = make_float4(g0, g0, g0, g0);       // a NaN row stays NaN where its ReLU would have cut it
    *reinterpret_cast<float4*>(dz1 + (size_t)m * D_H + tid * 4) = o;
}

// bq_head_validate's row kernel, a workgroup per row: train_logits_kernel's logits and loss, and hit = the larger logit is the label's
// (a tie goes to class 0; a NaN row hits nothing).  A row's values depend on nothing but the row.  out_loss / out_hit: the caller's, or null.
template <bool DROP>
__global__ void __launch_bounds__(256) validate_logits_kernel(const float* __restrict__ h1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, const long long* __restrict__ rows,
                                                              const unsigned char* __restrict__ label, Drop d, double* __restrict__ rowloss,
                                                              unsigned char* __restrict__ hit, double* __restrict__ out_loss,
                                                              unsigned char* __restrict__ out_hit) {
    __shared__ float lds[4];
    const int m = blockIdx.x;
    const Row r = row_forward<DROP>(h1, w2, b2, rows, label, d, lds, threadIdx.x == 0);
    if (threadIdx.x == 0) {
        const unsigned char ok = (r.loss == r.loss && (r.z1 > r.z0 ? 1u : 0u) == r.y) ? 1 : 0;
        rowloss[m] = r.loss;
        hit[m] = ok;
        if (out_loss) out_loss[m] = r.loss;
        if (out_hit) out_hit[m] = ok;
    }
}

// stats[0] = the sum of the rows' losses, stats[1] = the number of hits: thread t takes the rows t, t + 256, ... in order, then thread
// 0 the 256 partial sums in order.  One workgroup.
__global__ void __launch_bounds__(256) validate_sums_kernel(const double* __restrict__ rowloss, const unsigned char* __restrict__ hit, int n,
                                                            double* __restrict__ stats) {
    __shared__ double lpart[256];
    __shared__ unsigned cpart[256];
    double l = 0.0;
    unsigned c = 0u;
    for (int i = threadIdx.x; i < n; i += 256) {
        l += rowloss[i];
        c += hit[i];
    }
    lpart[threadIdx.x] = l;
    cpart[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        l = 0.0; c = 0u;
        for (int t = 0; t < 256; ++t) {
            l += lpart[t];
            c += cpart[t];
        }
        stats[0] = l;
        stats[1] = (double)c;
    }
}

// The small sums over the batch.  A workgroup is 8 row groups x 32 lanes: row group q sums the rows q, q + 8, ... in order, then the
// eight partial sums are added in the order of q -- a fixed order.  Workgroups 0-7: the logits kernel's gradient, a lane per group of four
// units (g_w2[k][c] = sum_i drop(h1)[i][k] dlog[i][c]).  Workgroup 8: the logits bias gradient and the loss (the rows' losses summed in
// float64, rounded once).  Workgroups 9-40 and 41-72: the column sums of dz1 and dz0, the hidden layers' bias gradients, a lane per column.
constexpr int SUM_BLOCKS = 8 + 1 + 2 * (D_H / 32);
__global__ void __launch_bounds__(256) train_sums_kernel(const float* __restrict__ h1, const float* __restrict__ dz1,
                                                         const float* __restrict__ dz0, const float* __restrict__ dlog,
                                                         const double* __restrict__ rowloss, const long long* __restrict__ rows, int n, Drop d,
                                                         float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_b1,
                                                         float* __restrict__ g_b0, float* __restrict__ loss) {
    __shared__ float part[8][32][9];                 // (9: the eight values of a lane on distinct banks)
    __shared__ double lpart[8][32];
    const int q = threadIdx.x >> 5, c = threadIdx.x & 31, b = blockIdx.x;
    if (b < 8) {
        const int ug = b * 32 + c;                   // units 4 ug .. 4 ug + 3
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i = q; i < n; i += 8) {
            const float4 u = drop4(*reinterpret_cast<const float4*>(h1 + (size_t)i * D_H + ug * 4), (unsigned)ug, (unsigned)rows[i], d);
            const float g0 = dlog[2 * i], g1 = dlog[2 * i + 1];
            a[0] = fmaf(u.x, g0, a[0]); a[1] = fmaf(u.x, g1, a[1]);
            a[2] = fmaf(u.y, g0, a[2]); a[3] = fmaf(u.y, g1, a[3]);
            a[4] = fmaf(u.z, g0, a[4]); a[5] = fmaf(u.z, g1, a[5]);
            a[6] = fmaf(u.w, g0, a[6]); a[7] = fmaf(u.w, g1, a[7]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) part[q][c][e] = a[e];
        __syncthreads();
        if (q == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float s = part[0][c][e];
                for (int k = 1; k < 8; ++k) s += part[k][c][e];
                g_w2[ug * 8 + e] = s;
            }
        }
    } else if (b == 8) {
        float s0 = 0.f, s1 = 0.f;
        double l = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) {
            s0 += dlog[2 * i];
            s1 += dlog[2 * i + 1];
            l += rowloss[i];
        }
        part[q][c][0] = s0;
        part[q][c][1] = s1;
        lpart[q][c] = l;
        __syncthreads();
        if (threadIdx.x == 0) {
            s0 = 0.f; s1 = 0.f; l = 0.0;
            for (int t = 0; t < 256; ++t) {
                s0 += part[t >> 5][t & 31][0];
                s1 += part[t >> 5][t & 31][1];
                l += lpart[t >> 5][t & 31];
            }
            g_b2[0] = s0;
            g_b2[1] = s1;
            loss[0] = (float)(l / (double)n);
        }
    } else {
        const bool first = b < 9 + D_H / 32;
        const int col = (b - (first ? 9 : 9 + D_H / 32)) * 32 + c;
        const float* dz = first ? dz1 : dz0;
        float s = 0.f;
        for (int i = q; i < n; i += 8) s += dz[(size_t)i * D_H + col];
        part[q][c][0] = s;
        __syncthreads();
        if (q == 0) {
            s = part[0][c][0];
            for (int k = 1; k < 8; ++k) s += part[k][c][0];
            (first ? g_b1 : g_b0)[col] = s;
        }
    }
}

// Keras Adam of one element, t = step + 1 folded into alpha = lr sqrt(1 - b2^t) / (1 - b1^t) on the host
__global__ void __launch_bounds__(256) train_adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ g, long long count, double b1, double b2, double eps,
                                                         double alpha) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double gi = (double)g[i];
    const double mi = b1 * (double)m[i] + (1.0 - b1) * gi;
    const double vi = b2 * (double)v[i] + (1.0 - b2) * (gi * gi);
    m[i] = (float)mi;
    v[i] = (float)vi;
    w[i] = (float)((double)w[i] - alpha * (mi / (sqrt(vi) + eps)));
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int VALIDATE_MAX_N = 4096;            // the reference's validation_steps x batch_size, 32 x 128

// The two layouts: the regions in order, each rounded up to 256 bytes, and their total (all a null ws gives).
struct TrainWs { float *h0, *h1, *dz1, *dz0, *dlog; double* rowloss; size_t total; };
TrainWs train_ws(void* ws, size_t n) {          // bq_head_grad's: h0 | h1 | dz1 | dz0, each [n][1024] | dlog [n][2] | rowloss f64 [n]
    uintptr_t p = (uintptr_t)ws;
    TrainWs w{};
    w.h0 = (float*)p; p += al(n * D_H * 4);
    w.h1 = (float*)p; p += al(n * D_H * 4);
    w.dz1 = (float*)p; p += al(n * D_H * 4);
    w.dz0 = (float*)p; p += al(n * D_H * 4);
    w.dlog = (float*)p; p += al(n * 2 * 4);
    w.rowloss = (double*)p; p += al(n * 8);
    w.total = p - (uintptr_t)ws;
    return w;
}
struct ValidateWs { float *h0, *h1; double* rowloss; unsigned char* hit; size_t total; };
ValidateWs validate_ws(void* ws, size_t n) {    // bq_head_validate's: h0 | h1, each [n][1024] | rowloss f64 [n] | hit u8 [n]
    uintptr_t p = (uintptr_t)ws;
    ValidateWs w{};
    w.h0 = (float*)p; p += al(n * D_H * 4);
    w.h1 = (float*)p; p += al(n * D_H * 4);
    w.rowloss = (double*)p; p += al(n * 8);
    w.hit = (unsigned char*)p; p += al(n);
    w.total = p - (uintptr_t)ws;
    return w;
}

// What the entries over gathered rows take alike.
struct Batch {
    const float* params; const float* feats; long long n_feat; const long long* rows; const unsigned char* labels; int n;
    long long step;             // the Philox pass: bq_head_validate's `pass`
    double rate; void* ws;
    int gather = 1;             // feats[rows[i]]; 0 (bq_exit_grad): feats[i], the rows being the Philox counters only
};

inline bool aligned(const void* p, uintptr_t a) { return p && !((uintptr_t)p & (a - 1)); }

// The refusal of a gathered batch, "" for none.  max_n: the entry's row limit; counter: what the entry calls the Philox pass; own_ok:
// the pointers that are the entry's own are there and aligned; pointers: the entry's text for one, of the batch or its own, that is not.
std::string bad_batch(bq_ctx* c, const char* entry, const Batch& b, int max_n, const char* counter, bool own_ok, const char* pointers) {
    const std::string e(entry);
    if (!c) return e + ": null context";
    if (b.n < 1 || b.n > max_n) return e + ": 1 <= n <= " + std::to_string(max_n);
    if (b.n_feat < 1 || b.step < 0 || b.step > 0xffffffffLL) return e + ": an empty feature cache, or a " + counter + " outside 0 .. 2^32 - 1";
    if (!(b.rate >= 0.0) || !(b.rate < 1.0)) return e + ": the rate must lie in [0, 1)";
    if (!aligned(b.params, 16) || !aligned(b.feats, 16) || !aligned(b.rows, 8) || !b.labels || !aligned(b.ws, 256) || !own_ok) return e + pointers;
    return "";
}

// bq_head_grad's and bq_head_train_steps': grad and loss are their own
std::string bad_grad_args(bq_ctx* c, const char* entry, const Batch& b, const void* grad, const void* loss) {
    return bad_batch(c, entry, b, MAX_N, "step", aligned(grad, 16) && aligned(loss, 4),
                     ": bad argument (null pointer, params, feats or grad not 16-byte, rows not 8-byte or the workspace not 256-byte aligned)");
}

// The masks of a batch: set_dropout's rule (biscuit_hip.hip), the contract of oracle/philox.py, at pass b.step; the layer is the launch's.
Drop drop_of(const Batch& b, uint64_t seed) {
    const double t = std::floor(b.rate * 4294967296.0);
    return Drop{0u, (unsigned)b.step, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), t > 4294967295.0 ? 4294967295u : (unsigned)t,
                (float)(1.0 / (1.0 - b.rate))};
}

struct ASrc { const float* p; int ld, gather; };   // A's source: rows of ld floats, a[rows[i]] (the feature cache) or a[i]

// out [M][1024] = A [M][K] B, every operand in rows of 1024 floats but A; the launch names the orientations and the epilogue, `layer`
// the mask of A (A_DROP_*) or of the epilogue (EPI_DX), epi the epilogue's operand: the bias (EPI_RELU), the layer's forward output (EPI_DX).
template <int AM, int BM, int EPI>
void launch_gemm(const Batch& b, Drop d, unsigned layer, ASrc a, const float* bm, const float* epi, float* out, int M, int K, hipStream_t s) {
    TrainGemm p{};
    p.a = a.p; p.lda = a.ld; p.gather = a.gather; p.b = bm; p.ldb = D_H; p.out = out; p.ldo = D_H;
    p.bias = EPI == EPI_RELU ? epi : nullptr; p.h = EPI == EPI_DX ? epi : nullptr;
    p.rows = b.rows; p.n_feat = b.n_feat; p.M = M; p.N = D_H; p.K = K; p.drop = d; p.drop.layer = layer;
    hipLaunchKernelGGL((train_gemm_kernel<AM, BM, EPI>), dim3(p.N / TN, (p.M + TM - 1) / TM), dim3(256), 0, s, p);
}

// The forward half of a gradient and of a validation, two launches under the profiling classes fwd0 and fwd1.  AM: A_DROP_K, or
// A_FINITE_K -- rate 0 without its draws.
template <int AM>
void enqueue_forward(bq_ctx* c, const Batch& b, const Drop& d, float* h0, float* h1, const char* fwd0, const char* fwd1, hipStream_t s) {
    const double fn = (double)b.n;
    {   // h0 = relu(drop_0(x[rows]) W0 + b0)
        ProfScope ps(c, s, fwd0, 2.0 * fn * D_IN * D_H, 4.0 * (fn * D_IN + (double)D_IN * D_H + fn * D_H));
        launch_gemm<AM, B_ROWS, EPI_RELU>(b, d, 0u, ASrc{b.feats, D_IN, b.gather}, b.params + OFF_W0, b.params + OFF_B0, h0, b.n, D_IN, s);
    }
    {   // h1 = relu(drop_1(h0) W1 + b1)
        ProfScope ps(c, s, fwd1, 2.0 * fn * D_H * D_H, 4.0 * (2.0 * fn * D_H + (double)D_H * D_H));
        launch_gemm<AM, B_ROWS, EPI_RELU>(b, d, 1u, ASrc{h0, D_H, 0}, b.params + OFF_W1, b.params + OFF_B1, h1, b.n, D_H, s);
    }
}

// The seven launches of one gradient, each a profiling class of its own (Adam's is the eighth of a step).
int enqueue_grad(bq_ctx* c, const Batch& b, const Drop& d, float* grad, float* loss, hipStream_t s) {
    const int n = b.n;
    const TrainWs w = train_ws(b.ws, n);
    const double fn = (double)n;
    enqueue_forward<A_DROP_K>(c, b, d, w.h0, w.h1, "head_train_fwd0", "head_train_fwd1", s);
    Drop d2 = d; d2.layer = 2u;
    {   // logits, softmax, loss per row, dlog, dz1
        ProfScope ps(c, s, "head_train_logits", 8.0 * fn * D_H, 4.0 * (2.0 * fn * D_H + 2.0 * D_H));
        hipLaunchKernelGGL(train_logits_kernel, dim3(n), dim3(256), 0, s, w.h1, b.params + OFF_W2, b.params + OFF_B2, b.rows, b.labels, n, d2,
                           w.dz1, w.dlog, w.rowloss);
    }
    {   // dz0 = (h0 > 0 and kept_1) ? scale (dz1 W1^T) : 0
        ProfScope ps(c, s, "head_train_dx1", 2.0 * fn * D_H * D_H, 4.0 * (3.0 * fn * D_H + (double)D_H * D_H));
        launch_gemm<A_PLAIN_K, B_KCONT, EPI_DX>(b, d, 1u, ASrc{w.dz1, D_H, 0}, b.params + OFF_W1, w.h0, w.dz0, n, D_H, s);
    }
    {   // g_W1 = drop_1(h0)^T dz1
        ProfScope ps(c, s, "head_train_dw1", 2.0 * fn * D_H * D_H, 4.0 * (2.0 * fn * D_H + (double)D_H * D_H));
        launch_gemm<A_DROP_T, B_ROWS, EPI_STORE>(b, d, 1u, ASrc{w.h0, D_H, 0}, w.dz1, nullptr, grad + OFF_W1, D_H, n, s);
    }
    {   // g_W0 = drop_0(x[rows])^T dz0
        ProfScope ps(c, s, "head_train_dw0", 2.0 * fn * D_IN * D_H, 4.0 * (fn * D_IN + fn * D_H + (double)D_IN * D_H));
        launch_gemm<A_DROP_T, B_ROWS, EPI_STORE>(b, d, 0u, ASrc{b.feats, D_IN, b.gather}, w.dz0, nullptr, grad + OFF_W0, D_IN, n, s);
    }
    {   // g_W2, g_b2, the loss, g_b1, g_b0
        ProfScope ps(c, s, "head_train_sums", 4.0 * fn * D_H + 2.0 * fn * D_H, 4.0 * 3.0 * fn * D_H);
        hipLaunchKernelGGL(train_sums_kernel, dim3(SUM_BLOCKS), dim3(256), 0, s, w.h1, w.dz1, w.dz0, w.dlog, w.rowloss, b.rows, n, d2,
                           grad + OFF_W2, grad + OFF_B2, grad + OFF_B1, grad + OFF_B0, loss);
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

std::string bad_adam_args(const char* entry, const void* params, const void* m, const void* v, const void* grad, int64_t step, double lr,
                          double b1, double b2, double eps) {
    const std::string e(entry);
    if (!params || !m || !v || !grad || (((uintptr_t)params | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad) & 3))
        return e + ": bad argument (null or misaligned pointer)";
    if (step < 0 || step > 0xffffffffLL || !std::isfinite(lr) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps > 0.0) ||
        !std::isfinite(eps))
        return e + ": a step outside 0 .. 2^32 - 1, a learning rate that is not finite, b1 or b2 outside [0, 1), or eps <= 0";
    return "";
}

// one Adam pass over `count` elements under the profiling class `cls` (the head's: P_TOTAL, "head_train_adam")
int enqueue_adam(bq_ctx* c, float* params, float* m, float* v, const float* grad, long long step, double lr, double b1, double b2, double eps,
                 hipStream_t s, long long count = P_TOTAL, const char* cls = "head_train_adam") {
    const double t = (double)(step + 1);
    const double alpha = lr * std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t));
    ProfScope ps(c, s, cls, 12.0 * (double)count, 28.0 * (double)count);
    hipLaunchKernelGGL(train_adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, params, m, v, grad, count, b1, b2, eps,
                       alpha);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// bq_head_validate: the forward half of enqueue_grad over up to 4096 rows (the forward GEMMs then launch 16 x 64 workgroups), four
// launches, each a profiling class of its own.  DROP false (rate 0): no mask is drawn anywhere.
template <bool DROP>
int enqueue_validate(bq_ctx* c, const Batch& b, const Drop& d, double* stats, double* out_loss, unsigned char* out_hit, hipStream_t s) {
    const int n = b.n;
    const ValidateWs w = validate_ws(b.ws, n);
    const double fn = (double)n;
    enqueue_forward<DROP ? A_DROP_K : A_FINITE_K>(c, b, d, w.h0, w.h1, "head_validate_fwd0", "head_validate_fwd1", s);
    {   // logits, the row's loss and hit
        ProfScope ps(c, s, "head_validate_logits", 4.0 * fn * D_H, 4.0 * (fn * D_H + 2.0 * D_H));
        Drop d2 = d; d2.layer = 2u;
        hipLaunchKernelGGL((validate_logits_kernel<DROP>), dim3(n), dim3(256), 0, s, w.h1, b.params + OFF_W2, b.params + OFF_B2, b.rows, b.labels,
                           d2, w.rowloss, w.hit, out_loss, out_hit);
    }
    {   // the two sums
        ProfScope ps(c, s, "head_validate_sums", fn, 9.0 * fn);
        hipLaunchKernelGGL(validate_sums_kernel, dim3(1), dim3(256), 0, s, w.rowloss, w.hit, n, stats);
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ================================================================================================ exit-flow fine-tuning
// DESIGN.md section 7 "Exit-flow fine-tuning": block 14 in front of the head, trained with it.  For a tile's cached
// x = block13_out [10][10][1024], in fp32 and NHWC:
//     u1 = dw(x, D1)   z1 = u1 P1 [1024 x 1536]   h1 = relu(a1 z1 + b1)
//     u2 = dw(h1, D2)  z2 = u2 P2 [1536 x 2048]   h2 = relu(a2 z2 + b2)      f = mean over the 100 positions of h2 -> the head above
// with a = gamma / sqrt(var + eps), b = beta - a mean and the moving statistics frozen -- or, in training mode (bq_exit_grad_bn: the
// kernels under "Training-mode batch norm" below, launched by a host-side branch on ExitBatch::bstats), mean and var the batch's own
// over the 100 n rows of the layer's z, with the gradient through them.  Only u and z are stored: every reader of h
// forms relu(fmaf(a, z, b)) again (bn_relu, one function).  The four pointwise products and their four transposes are
// train_gemm_kernel (A_MAT_K / A_MAT_T: dP = u^T dz sums over K = 100 n rows), as is the head's input gradient (EPI_DX0); the
// depthwise kernel, its two transposes, the pool and the BN backward are vector-ALU kernels over a tile's 100 positions x 256
// channels per workgroup, a lane on four consecutive channels (float4), wave q on the positions q, q + 4, ... in order, the four
// waves' partial sums then added in the order of q.  Sums over the batch (dD, dgamma, dbeta) go through per-tile partials in the
// workspace and exit_colsum_kernel: eight row groups, then the groups in order.  No floating-point atomics anywhere.
constexpr int X_POS = 100, X_HW = 10, X_C0 = 1024, X_C1 = 1536, X_C2 = 2048;
constexpr long long X_ROW = (long long)X_POS * X_C0;            // floats of a tile in the activation cache
constexpr long long E_D1 = 0, E_P1 = E_D1 + 9 * X_C0, E_G1 = E_P1 + (long long)X_C0 * X_C1, E_B1 = E_G1 + X_C1, E_D2 = E_B1 + X_C1,
                    E_P2 = E_D2 + 9 * X_C1, E_G2 = E_P2 + (long long)X_C1 * X_C2, E_B2 = E_G2 + X_C2, P_EXIT = E_B2 + X_C2;
static_assert(P_EXIT == 4748800 && P_EXIT % 4 == 0, "the exit vector's parameter count");
constexpr long long P_ALL = P_EXIT + P_TOTAL;
constexpr int S_M1 = 0, S_V1 = X_C1, S_M2 = 2 * X_C1, S_V2 = 2 * X_C1 + X_C2;      // d_bn_stats: mean1 | var1 | mean2 | var2
constexpr int EXIT_MAX_N = 256;
constexpr float BN_EPS = 1e-3f;

__device__ __forceinline__ float bn_relu(float z, float a, float b) { return relu_nan(fmaf(a, z, b)); }
__device__ __forceinline__ float4 bn_relu4(float4 z, float4 a, float4 b) {
    return make_float4(bn_relu(z.x, a.x, b.x), bn_relu(z.y, a.y, b.y), bn_relu(z.z, a.z, b.z), bn_relu(z.w, a.w, b.w));
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// the four waves' partial sums in the order of q
__device__ __forceinline__ float4 sum_q(const float4* l, int stride) { return add4(add4(add4(l[0], l[stride]), l[2 * stride]), l[3 * stride]); }

// a = gamma / sqrt(var + eps), b = beta - a mean, inv = 1 / sqrt(var + eps) of one layer
__global__ void __launch_bounds__(256) exit_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ mean, const float* __restrict__ var, int C,
                                                        float* __restrict__ a, float* __restrict__ b, float* __restrict__ inv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float sd = sqrtf(var[c] + BN_EPS), ac = gamma[c] / sd;
    a[c] = ac;
    b[c] = beta[c] - ac * mean[c];
    inv[c] = 1.f / sd;
}

// What a depthwise kernel reads: the activation cache through the row table (a row outside it is never read and reads as NaN, a
// value that is not finite as NaN), relu(a z + b) of a stored z, or a plain [100 n][C] tensor.
// IN_STAGE: the host tier's staging copy of a float32 cache, the batch's rows in order (exit_gather_kernel has checked the rows: one
// outside the cache is NaN there).  IN_CACHE_F16 / IN_CACHE_BF16: a cache in the engine's 16-bit type, stored value h, the network's
// value float(h) mul with mul a power of two -- the float32 cache's number exactly; a null row table: the staging copy, rows in order.
enum DwIn : int { IN_CACHE = 0, IN_BN = 1, IN_PLAIN = 2, IN_STAGE = 3, IN_CACHE_F16 = 4, IN_CACHE_BF16 = 5 };
struct DwSrc { const float* p; const long long* rows; long long n_act; const float* a; const float* b; };
struct DwSrc16 { const unsigned short* p; const long long* rows; long long n_act; float mul; };
template <int IN> struct DwOf { using Src = DwSrc; using Elt = float; };
template <> struct DwOf<IN_CACHE_F16> { using Src = DwSrc16; using Elt = unsigned short; };
template <> struct DwOf<IN_CACHE_BF16> { using Src = DwSrc16; using Elt = unsigned short; };
constexpr bool dw_is16(int in) { return in == IN_CACHE_F16 || in == IN_CACHE_BF16; }
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <int IN, int C>
__device__ __forceinline__ const typename DwOf<IN>::Elt* dw_tile(const typename DwOf<IN>::Src& s, int i) {
    if constexpr (dw_is16(IN)) {
        const long long r = s.rows ? s.rows[i] : (long long)i;
        return (r >= 0 && r < s.n_act) ? s.p + (size_t)r * (size_t)X_ROW : nullptr; // 64-bit: a row is 102 400 elements, 204 800 bytes
    } else {
        if (IN != IN_CACHE) return s.p + (size_t)i * X_POS * C;
        const long long r = s.rows[i];
        return (r >= 0 && r < s.n_act) ? s.p + (size_t)r * (size_t)X_ROW : nullptr;     // 64-bit: a row is 102 400 floats
    }
}
// a, b: the BN coefficients of IN_BN; a.x of a 16-bit cache: its mul
template <int IN, int C>
__device__ __forceinline__ float4 dw_at(const typename DwOf<IN>::Elt* tile, int pos, int c, const float4& a, const float4& b) {
    if constexpr (dw_is16(IN)) {
        if (!tile) { const float nan = __builtin_nanf(""); return make_float4(nan, nan, nan, nan); }
        const unsigned short* p = tile + (size_t)pos * C + c;          // four channels: one 8-byte load
        float4 v;
        if (IN == IN_CACHE_F16) {
            const f16x4 h = *reinterpret_cast<const f16x4*>(p);
            v = make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
        } else {
            const uint2 h = *reinterpret_cast<const uint2*>(p);
            v = make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xffff0000u), __uint_as_float(h.y << 16),
                            __uint_as_float(h.y & 0xffff0000u));
        }
        return finite4(make_float4(v.x * a.x, v.y * a.x, v.z * a.x, v.w * a.x));
    } else {
        if (IN == IN_CACHE && !tile) { const float nan = __builtin_nanf(""); return make_float4(nan, nan, nan, nan); }
        const float4 v = ld4(tile + (size_t)pos * C + c);
        return IN == IN_CACHE || IN == IN_STAGE ? finite4(v) : IN == IN_BN ? bn_relu4(v, a, b) : v;
    }
}
// a and b of dw_at
template <int IN>
__device__ __forceinline__ void dw_coef(const typename DwOf<IN>::Src& s, int c, float4& a, float4& b) {
    a = b = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (dw_is16(IN)) a.x = s.mul;
    else if (IN == IN_BN) { a = ld4(s.a + c); b = ld4(s.b + c); }
}

// out[i][y][x][c] = sum over the taps (ky, kx) in order of in[i][y + ky - 1][x + kx - 1][c] w[ky][kx][c], an fmaf chain; zero padding 1
// (a tap outside the map adds nothing).  FLIP: the taps reversed -- the transpose, the gradient with respect to the input.
template <int IN, int C, bool FLIP>
__global__ void __launch_bounds__(256) exit_dw_kernel(const typename DwOf<IN>::Src s, const float* __restrict__ w, float* __restrict__ out) {
    const int i = blockIdx.y, c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, q = threadIdx.x >> 6;
    const auto* tile = dw_tile<IN, C>(s, i);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a, b;
    dw_coef<IN>(s, c, a, b);
    float4 wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = ld4(w + (size_t)(FLIP ? 8 - t : t) * C + c);
    for (int pos = q; pos < X_POS; pos += 4) {
        const int y = pos / X_HW, x = pos - y * X_HW;
        float4 acc = zero;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y + ky - 1, xx = x + kx - 1;
                if (yy >= 0 && yy < X_HW && xx >= 0 && xx < X_HW) acc = fma4(dw_at<IN, C>(tile, yy * X_HW + xx, c, a, b), wt[ky * 3 + kx], acc);
            }
        st4(out + ((size_t)i * X_POS + pos) * C + c, acc);
    }
}

// part[i][ky][kx][c] = sum over tile i's positions of in[i][y + ky - 1][x + kx - 1][c] du[i][y][x][c]: the depthwise kernel's weight
// gradient of one tile (exit_colsum_kernel adds the tiles).
template <int IN, int C>
__global__ void __launch_bounds__(256) exit_dw_wgrad_kernel(const typename DwOf<IN>::Src s, const float* __restrict__ du,
                                                            float* __restrict__ part) {
    __shared__ float4 lds[4][9][64];
    const int i = blockIdx.y, cq = threadIdx.x & 63, c = (blockIdx.x * 64 + cq) * 4, q = threadIdx.x >> 6;
    const auto* tile = dw_tile<IN, C>(s, i);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a, b;
    dw_coef<IN>(s, c, a, b);
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = zero;
    for (int pos = q; pos < X_POS; pos += 4) {
        const int y = pos / X_HW, x = pos - y * X_HW;
        const float4 g = ld4(du + ((size_t)i * X_POS + pos) * C + c);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y + ky - 1, xx = x + kx - 1;
                if (yy >= 0 && yy < X_HW && xx >= 0 && xx < X_HW)
                    acc[ky * 3 + kx] = fma4(dw_at<IN, C>(tile, yy * X_HW + xx, c, a, b), g, acc[ky * 3 + kx]);
            }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) lds[q][t][cq] = acc[t];
    __syncthreads();
    for (int e = threadIdx.x; e < 9 * 64; e += 256) {
        const int t = e >> 6, k = e & 63;
        st4(part + ((size_t)i * 9 + t) * C + (blockIdx.x * 64 + k) * 4, sum_q(&lds[0][t][k], 9 * 64));
    }
}

// f[i][c] = (sum over tile i's positions of relu(a z2 + b)) / 100
__global__ void __launch_bounds__(256) exit_pool_kernel(const float* __restrict__ z, const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ f) {
    __shared__ float4 lds[4][64];
    const int i = blockIdx.y, cq = threadIdx.x & 63, c = (blockIdx.x * 64 + cq) * 4, q = threadIdx.x >> 6;
    const float4 av = ld4(a + c), bv = ld4(b + c);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int pos = q; pos < X_POS; pos += 4) acc = add4(acc, bn_relu4(ld4(z + ((size_t)i * X_POS + pos) * X_C2 + c), av, bv));
    lds[q][cq] = acc;
    __syncthreads();
    if (q == 0) {
        const float4 v = sum_q(&lds[0][cq], 64);
        st4(f + (size_t)i * X_C2 + c, make_float4(v.x / 100.f, v.y / 100.f, v.z / 100.f, v.w / 100.f));
    }
}

// The BN + ReLU backward of one layer over tile i: with h = relu(a z + b) and g = dh [h > 0] (a NaN h keeps its NaN),
// dz = g a, and the tile's partial sums part[i][0][c] = sum g (z - mean) inv (dgamma), part[i][1][c] = sum g (dbeta).  BCAST: dh is the
// pool's transpose, df[i][c] / 100 at every position; otherwise dh [100 n][C], which dz may overwrite in place.
template <bool BCAST, int C>
__global__ void __launch_bounds__(256) exit_bn_back_kernel(const float* __restrict__ z, const float* dh, const float* __restrict__ a,
                                                           const float* __restrict__ b, const float* __restrict__ mean,
                                                           const float* __restrict__ inv, float* dz, float* __restrict__ part) {
    __shared__ float4 lds[4][2][64];
    const int i = blockIdx.y, cq = threadIdx.x & 63, c = (blockIdx.x * 64 + cq) * 4, q = threadIdx.x >> 6;
    const float4 av = ld4(a + c), bv = ld4(b + c), mv = ld4(mean + c), iv = ld4(inv + c);
    float4 top = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BCAST) {
        top = ld4(dh + (size_t)i * C + c);
        top = make_float4(top.x / 100.f, top.y / 100.f, top.z / 100.f, top.w / 100.f);
    }
    float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sb = sg;
    for (int pos = q; pos < X_POS; pos += 4) {
        const size_t o = ((size_t)i * X_POS + pos) * C + c;
        const float4 zv = ld4(z + o), h = bn_relu4(zv, av, bv), d = BCAST ? top : ld4(dh + o);
        const float4 g = make_float4(h.x > 0.f ? d.x : (h.x != h.x ? h.x : 0.f), h.y > 0.f ? d.y : (h.y != h.y ? h.y : 0.f),
                                     h.z > 0.f ? d.z : (h.z != h.z ? h.z : 0.f), h.w > 0.f ? d.w : (h.w != h.w ? h.w : 0.f));
        st4(dz + o, make_float4(g.x * av.x, g.y * av.y, g.z * av.z, g.w * av.w));
        sg = fma4(g, make_float4((zv.x - mv.x) * iv.x, (zv.y - mv.y) * iv.y, (zv.z - mv.z) * iv.z, (zv.w - mv.w) * iv.w), sg);
        sb = add4(sb, g);
    }
    lds[q][0][cq] = sg;
    lds[q][1][cq] = sb;
    __syncthreads();
    if (q < 2) st4(part + ((size_t)i * 2 + q) * C + c, sum_q(&lds[0][q][cq], 2 * 64));
}

// dst[j] = sum over the n rows of src[i][j], j < W (a multiple of 32): a workgroup is 8 row groups x 32 columns, row group q sums the
// rows q, q + 8, ... in order, then the eight partial sums are added in the order of q.
__global__ void __launch_bounds__(256) exit_colsum_kernel(const float* __restrict__ src, int n, int W, float* __restrict__ dst) {
    __shared__ float part[8][33];
    const int q = threadIdx.x >> 5, l = threadIdx.x & 31, j = blockIdx.x * 32 + l;
    float s = 0.f;
    for (int i = q; i < n; i += 8) s += src[(size_t)i * W + j];
    part[q][l] = s;
    __syncthreads();
    if (q == 0) {
        s = part[0][l];
        for (int k = 1; k < 8; ++k) s += part[k][l];
        dst[j] = s;
    }
}

// Training-mode batch norm (bq_exit_grad_bn; DESIGN.md section 7 "Exit-flow fine-tuning", Two modes): the statistics of a layer are
// the batch's own, over the M = 100 n rows of its stored z.  part[i][c] = (the sum over tile i's positions of z, or with SQ of
// (z - mu)^2) / M, so that exit_colsum_kernel over the tiles gives mu, then var: two passes, never E[z^2] - mu^2.
template <bool SQ, int C>
__global__ void __launch_bounds__(256) exit_stat_kernel(const float* __restrict__ z, const float* __restrict__ mu, float m,
                                                        float* __restrict__ part) {
    __shared__ float4 lds[4][64];
    const int i = blockIdx.y, cq = threadIdx.x & 63, c = (blockIdx.x * 64 + cq) * 4, q = threadIdx.x >> 6;
    float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), acc = mv;
    if (SQ) mv = ld4(mu + c);
    for (int pos = q; pos < X_POS; pos += 4) {
        const float4 v = ld4(z + ((size_t)i * X_POS + pos) * C + c);
        if (SQ) {
            const float4 d = make_float4(v.x - mv.x, v.y - mv.y, v.z - mv.z, v.w - mv.w);
            acc = fma4(d, d, acc);
        } else {
            acc = add4(acc, v);
        }
    }
    lds[q][cq] = acc;
    __syncthreads();
    if (q == 0) {
        const float4 v = sum_q(&lds[0][cq], 64);
        st4(part + (size_t)i * C + c, make_float4(v.x / m, v.y / m, v.z / m, v.w / m));
    }
}

// What the batch statistics add to exit_bn_back_kernel's dz = g a, in place over tile i: with xhat = (z - mu) inv and the layer's
// finished sums dgb = dgamma [C] | dbeta [C],  dz -= a (dbeta / M + xhat dgamma / M).
template <int C>
__global__ void __launch_bounds__(256) exit_bn_fix_kernel(const float* __restrict__ z, const float* __restrict__ a, const float* __restrict__ mean,
                                                          const float* __restrict__ inv, const float* __restrict__ dgb, float m,
                                                          float* __restrict__ dz) {
    const int i = blockIdx.y, c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, q = threadIdx.x >> 6;
    const float4 av = ld4(a + c), mv = ld4(mean + c), iv = ld4(inv + c), dg = ld4(dgb + c), db = ld4(dgb + C + c);
    const float4 na = make_float4(-av.x, -av.y, -av.z, -av.w);
    const float4 cg = make_float4(dg.x / m, dg.y / m, dg.z / m, dg.w / m), cb = make_float4(db.x / m, db.y / m, db.z / m, db.w / m);
    for (int pos = q; pos < X_POS; pos += 4) {
        const size_t o = ((size_t)i * X_POS + pos) * C + c;
        const float4 zv = ld4(z + o);
        const float4 xh = make_float4((zv.x - mv.x) * iv.x, (zv.y - mv.y) * iv.y, (zv.z - mv.z) * iv.z, (zv.w - mv.w) * iv.w);
        st4(dz + o, fma4(na, fma4(xh, cg, cb), ld4(dz + o)));
    }
}

// moving <- 0.99 moving + 0.01 batch over mean1 | var1 | mean2 | var2, the variances with the unbiased batch variance: their factor
// fu = 0.01 M / (M - 1).  Two products and a sum per element, evaluated in float64 from the fp32 values and rounded once, as Adam's
// update is: a moving mean whose two terms nearly cancel is still the correctly rounded value of the formula.
constexpr int BN_STATS = 2 * X_C1 + 2 * X_C2;
__global__ void __launch_bounds__(256) exit_bn_move_kernel(float* __restrict__ moving, const float* __restrict__ batch, double fu) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= BN_STATS) return;
    const bool var = (j >= S_V1 && j < S_M2) || j >= S_V2;
    moving[j] = (float)(0.99 * (double)moving[j] + (var ? fu : 0.01) * (double)batch[j]);
}

// The host tier's gather: stage[i] = cache[rows[i]], whole rows of row16 16-byte pieces, one load and one store each; `cache` is the
// device pointer of mapped pinned host memory, which this kernel alone reads (once per piece: fine-grained memory is not cached).  A row
// outside 0 .. n_rows - 1 is never read: its copy is `nan`, the NaN pattern of the cache's type in every element.
constexpr int GATHER_BLOCKS = 50;
__global__ void __launch_bounds__(256) exit_gather_kernel(const uint4* __restrict__ cache, long long n_rows, const long long* __restrict__ rows,
                                                          int row16, unsigned nan, uint4* __restrict__ stage) {
    const long long r = rows[blockIdx.y];
    const bool in = r >= 0 && r < n_rows;
    const uint4* src = cache + (in ? (size_t)r * (size_t)row16 : (size_t)0);      // 64-bit: a row is 204 800 or 409 600 bytes
    uint4* dst = stage + (size_t)blockIdx.y * (size_t)row16;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < row16; k += GATHER_BLOCKS * 256) dst[k] = in ? src[k] : make_uint4(nan, nan, nan, nan);
}

constexpr size_t act_elt_bytes(int type) { return type == BQ_ACT_F32 ? 4 : 2; }
constexpr size_t act_row_bytes(int type) { return (size_t)X_ROW * act_elt_bytes(type); }

// The layout of both exit workspaces, the regions in order, each rounded up to 256 bytes; `train`: the backward regions and the
// head's own workspace behind the forward ones.  du1 takes du2's place once du2 is spent.  The host tier's staging copy of the
// batch's rows lies behind either (exit_stage).
struct ExitWs {
    float *a1, *b1, *i1, *a2, *b2, *i2, *u1, *z1, *u2, *z2, *f;           // forward
    float *df, *dz2, *du, *dz1, *part; void* head;                         // backward
    size_t total;
};
ExitWs exit_ws(void* ws, size_t n, bool train) {
    uintptr_t p = (uintptr_t)ws;
    ExitWs w{};
    auto take = [&](size_t floats) { float* r = (float*)p; p += al(floats * 4); return r; };
    w.a1 = take(X_C1); w.b1 = take(X_C1); w.i1 = take(X_C1);
    w.a2 = take(X_C2); w.b2 = take(X_C2); w.i2 = take(X_C2);
    w.u1 = take(n * X_POS * X_C0); w.z1 = take(n * X_POS * X_C1); w.u2 = take(n * X_POS * X_C1); w.z2 = take(n * X_POS * X_C2);
    w.f = take(n * X_C2);
    if (train) {
        w.df = take(n * X_C2); w.dz2 = take(n * X_POS * X_C2); w.du = take(n * X_POS * X_C1); w.dz1 = take(n * X_POS * X_C1);
        w.part = take(n * 9 * X_C1);                // (9 C1 >= 9 C0, 2 C2, 2 C1)
        w.head = (void*)p; p += train_ws(nullptr, n).total;
    }
    w.total = p - (uintptr_t)ws;
    return w;
}

// a plain product on train_gemm_kernel: out [M][N] = A B; rows, d: of EPI_DX0
template <int AM, int BM, int EPI>
void launch_mat(const float* a, int lda, const float* bm, int ldb, float* out, int ldo, int M, int N, int K, hipStream_t s,
                const long long* rows = nullptr, Drop d = Drop{}) {
    TrainGemm p{};
    p.a = a; p.lda = lda; p.b = bm; p.ldb = ldb; p.out = out; p.ldo = ldo; p.rows = rows; p.M = M; p.N = N; p.K = K; p.drop = d;
    hipLaunchKernelGGL((train_gemm_kernel<AM, BM, EPI>), dim3(N / TN, (M + TM - 1) / TM), dim3(256), 0, s, p);
}

// acts: the cache, n_act rows of `type` (BQ_ACT_*) holding value / mul; stage: null for a cache on the device, the staging copy --
// n rows of the cache's type -- for one in host memory, which acts then addresses through its mapped device pointer
struct ExitBatch {
    const float* params; const float* stats; const void* acts; long long n_act; const long long* rows; int n;
    int type = BQ_ACT_F32; float mul = 1.f; void* stage = nullptr;
    float* bstats = nullptr;    // training-mode BN: the batch statistics mu1 | var1 | mu2 | var2, written here; `stats` is then this
};
ExitBatch exit_batch(const float* params, const float* stats, const bq_act_cache& a, const long long* rows, int n) {
    ExitBatch b{params, stats, a.p, (long long)a.n_rows, rows, n};
    b.type = a.type; b.mul = a.mul;
    return b;
}

// The two readers of the cache, exit_dw_kernel (x: the taps) and exit_dw_wgrad_kernel (WGRAD; x: du), by the cache's type and place
template <int IN, bool WGRAD>
void launch_cache_reader(const typename DwOf<IN>::Src& src, const float* x, float* out, int n, hipStream_t s) {
    if (WGRAD) hipLaunchKernelGGL((exit_dw_wgrad_kernel<IN, X_C0>), dim3(X_C0 / 256, n), dim3(256), 0, s, src, x, out);
    else hipLaunchKernelGGL((exit_dw_kernel<IN, X_C0, false>), dim3(X_C0 / 256, n), dim3(256), 0, s, src, x, out);
}
template <bool WGRAD>
void enqueue_cache_reader(const ExitBatch& b, const float* x, float* out, hipStream_t s) {
    if (b.type == BQ_ACT_F32) {
        if (b.stage) launch_cache_reader<IN_STAGE, WGRAD>(DwSrc{(const float*)b.stage, nullptr, 0, nullptr, nullptr}, x, out, b.n, s);
        else launch_cache_reader<IN_CACHE, WGRAD>(DwSrc{(const float*)b.acts, b.rows, b.n_act, nullptr, nullptr}, x, out, b.n, s);
        return;
    }
    const DwSrc16 src = b.stage ? DwSrc16{(const unsigned short*)b.stage, nullptr, (long long)b.n, b.mul}
                                : DwSrc16{(const unsigned short*)b.acts, b.rows, b.n_act, b.mul};
    if (b.type == BQ_ACT_F16) launch_cache_reader<IN_CACHE_F16, WGRAD>(src, x, out, b.n, s);
    else launch_cache_reader<IN_CACHE_BF16, WGRAD>(src, x, out, b.n, s);
}

// Training-mode BN of one layer, under the class `cls`: the batch's mu and var over the n tiles of the stored z (per-tile partial sums in
// w.part -- the backward pass has no use for it yet --, then exit_colsum_kernel; the mean first, the variance around it), written where
// the caller reads them, and exit_coef_kernel on those: the frozen call's coefficients, had it been given these statistics.
template <int C>
void enqueue_bn_stats(bq_ctx* c, const char* cls, const float* z, int n, const float* gamma, const float* beta, float* mu, float* var,
                      const ExitWs& w, float* a, float* bb, float* inv, hipStream_t s) {
    const double fm = (double)n * X_POS;
    ProfScope ps(c, s, cls, 5.0 * fm * C, 8.0 * fm * C);
    hipLaunchKernelGGL((exit_stat_kernel<false, C>), dim3(C / 256, n), dim3(256), 0, s, z, (const float*)nullptr, (float)(n * X_POS), w.part);
    hipLaunchKernelGGL(exit_colsum_kernel, dim3(C / 32), dim3(256), 0, s, w.part, n, C, mu);
    hipLaunchKernelGGL((exit_stat_kernel<true, C>), dim3(C / 256, n), dim3(256), 0, s, z, (const float*)mu, (float)(n * X_POS), w.part);
    hipLaunchKernelGGL(exit_colsum_kernel, dim3(C / 32), dim3(256), 0, s, w.part, n, C, var);
    hipLaunchKernelGGL(exit_coef_kernel, dim3(C / 256), dim3(256), 0, s, gamma, beta, (const float*)mu, (const float*)var, C, a, bb, inv);
}

// The forward half, seven launches under the classes `pre`coef, dw1, pw1, dw2, pw2, pool: acts[rows] -> w.f [n][2048] (u and z stay in w);
// in front of them for a cache in host memory, under exit_gather, the batch's rows into b.stage, which both readers of the cache then read.
// With b.bstats (training-mode BN; a training workspace) no coef launch opens the chain: each layer's statistics and coefficients
// follow its pointwise product (enqueue_bn_stats).
void enqueue_exit_forward(bq_ctx* c, const ExitBatch& b, const ExitWs& w, const std::string& pre, hipStream_t s) {
    const int n = b.n, M = n * X_POS;
    const double fm = (double)M;
    const float* e = b.params;
    if (b.stage) {
        const unsigned nan = b.type == BQ_ACT_F32 ? 0x7fc00000u : b.type == BQ_ACT_F16 ? 0x7e007e00u : 0x7fc07fc0u;
        ProfScope ps(c, s, "exit_gather", 0.0, 2.0 * n * (double)act_row_bytes(b.type));
        hipLaunchKernelGGL(exit_gather_kernel, dim3(GATHER_BLOCKS, n), dim3(256), 0, s, (const uint4*)b.acts, b.n_act, b.rows,
                           (int)(act_row_bytes(b.type) / 16), nan, (uint4*)b.stage);
    }
    if (!b.bstats) {
        ProfScope ps(c, s, pre + "coef", 8.0 * (X_C1 + X_C2), 28.0 * (X_C1 + X_C2));
        hipLaunchKernelGGL(exit_coef_kernel, dim3(X_C1 / 256), dim3(256), 0, s, e + E_G1, e + E_B1, b.stats + S_M1, b.stats + S_V1, X_C1, w.a1,
                           w.b1, w.i1);
        hipLaunchKernelGGL(exit_coef_kernel, dim3(X_C2 / 256), dim3(256), 0, s, e + E_G2, e + E_B2, b.stats + S_M2, b.stats + S_V2, X_C2, w.a2,
                           w.b2, w.i2);
    }
    {
        ProfScope ps(c, s, pre + "dw1", 18.0 * fm * X_C0, (4.0 + act_elt_bytes(b.type)) * fm * X_C0);
        enqueue_cache_reader<false>(b, e + E_D1, w.u1, s);
    }
    {
        ProfScope ps(c, s, pre + "pw1", 2.0 * fm * X_C0 * X_C1, 4.0 * (fm * X_C0 + fm * X_C1 + (double)X_C0 * X_C1));
        launch_mat<A_MAT_K, B_ROWS, EPI_STORE>(w.u1, X_C0, e + E_P1, X_C1, w.z1, X_C1, M, X_C1, X_C0, s);
    }
    if (b.bstats) enqueue_bn_stats<X_C1>(c, "exit_train_stat1", w.z1, n, e + E_G1, e + E_B1, b.bstats + S_M1, b.bstats + S_V1, w, w.a1, w.b1, w.i1, s);
    {
        ProfScope ps(c, s, pre + "dw2", 20.0 * fm * X_C1, 8.0 * fm * X_C1);
        hipLaunchKernelGGL((exit_dw_kernel<IN_BN, X_C1, false>), dim3(X_C1 / 256, n), dim3(256), 0, s, DwSrc{w.z1, nullptr, 0, w.a1, w.b1},
                           e + E_D2, w.u2);
    }
    {
        ProfScope ps(c, s, pre + "pw2", 2.0 * fm * X_C1 * X_C2, 4.0 * (fm * X_C1 + fm * X_C2 + (double)X_C1 * X_C2));
        launch_mat<A_MAT_K, B_ROWS, EPI_STORE>(w.u2, X_C1, e + E_P2, X_C2, w.z2, X_C2, M, X_C2, X_C1, s);
    }
    if (b.bstats) enqueue_bn_stats<X_C2>(c, "exit_train_stat2", w.z2, n, e + E_G2, e + E_B2, b.bstats + S_M2, b.bstats + S_V2, w, w.a2, w.b2, w.i2, s);
    {
        ProfScope ps(c, s, pre + "pool", 3.0 * fm * X_C2, 4.0 * fm * X_C2);
        hipLaunchKernelGGL(exit_pool_kernel, dim3(X_C2 / 256, n), dim3(256), 0, s, w.z2, w.a2, w.b2, w.f);
    }
}

// One gradient over [exit | head]: the forward half, the head's seven launches on w.f (the same kernels as bq_head_grad: its rows
// are the batch's own, the row table the Philox counters), the head's input gradient, then block 14 backwards.
int enqueue_exit_grad(bq_ctx* c, const ExitBatch& b, const unsigned char* labels, long long step, uint64_t seed, double rate, void* ws,
                      float* grad, float* loss, hipStream_t s) {
    const int n = b.n, M = n * X_POS;
    const double fm = (double)M, fn = (double)n;
    const ExitWs w = exit_ws(ws, n, true);
    const float* e = b.params;
    enqueue_exit_forward(c, b, w, "exit_train_", s);
    Batch hb{b.params + P_EXIT, w.f, (long long)n, b.rows, labels, n, step, rate, w.head};
    hb.gather = 0;
    const Drop d = drop_of(hb, seed);
    RUN(enqueue_grad(c, hb, d, grad + P_EXIT, loss, s));
    const TrainWs hw = train_ws(w.head, n);
    {   // df = drop_0'(dz0 W0^T)
        ProfScope ps(c, s, "exit_train_dfeat", 2.0 * fn * D_IN * D_H, 4.0 * (fn * D_H + fn * D_IN + (double)D_IN * D_H));
        Drop d0 = d; d0.layer = 0u;
        launch_mat<A_MAT_K, B_KCONT, EPI_DX0>(hw.dz0, D_H, b.params + P_EXIT + OFF_W0, D_H, w.df, D_IN, n, D_IN, D_H, s, b.rows, d0);
    }
    {   // dz2, and the tiles' parts of dgamma2 | dbeta2
        ProfScope ps(c, s, "exit_train_bn2", 8.0 * fm * X_C2, 8.0 * fm * X_C2);
        hipLaunchKernelGGL((exit_bn_back_kernel<true, X_C2>), dim3(X_C2 / 256, n), dim3(256), 0, s, w.z2, w.df, w.a2, w.b2, b.stats + S_M2,
                           w.i2, w.dz2, w.part);
        hipLaunchKernelGGL(exit_colsum_kernel, dim3(2 * X_C2 / 32), dim3(256), 0, s, w.part, n, 2 * X_C2, grad + E_G2);
    }
    if (b.bstats) {   // dz2 -= a2 (dbeta2 / M + xhat2 dgamma2 / M): the gradient through the batch's own statistics
        ProfScope ps(c, s, "exit_train_bnfix2", 6.0 * fm * X_C2, 12.0 * fm * X_C2);
        hipLaunchKernelGGL((exit_bn_fix_kernel<X_C2>), dim3(X_C2 / 256, n), dim3(256), 0, s, w.z2, w.a2, b.stats + S_M2, w.i2, grad + E_G2,
                           (float)M, w.dz2);
    }
    {   // dP2 = u2^T dz2
        ProfScope ps(c, s, "exit_train_dp2", 2.0 * fm * X_C1 * X_C2, 4.0 * (fm * X_C1 + fm * X_C2 + (double)X_C1 * X_C2));
        launch_mat<A_MAT_T, B_ROWS, EPI_STORE>(w.u2, X_C1, w.dz2, X_C2, grad + E_P2, X_C2, X_C1, X_C2, M, s);
    }
    {   // du2 = dz2 P2^T
        ProfScope ps(c, s, "exit_train_du2", 2.0 * fm * X_C1 * X_C2, 4.0 * (fm * X_C1 + fm * X_C2 + (double)X_C1 * X_C2));
        launch_mat<A_MAT_K, B_KCONT, EPI_STORE>(w.dz2, X_C2, e + E_P2, X_C2, w.du, X_C1, M, X_C1, X_C2, s);
    }
    {   // dD2 over h1 = relu(a1 z1 + b1)
        ProfScope ps(c, s, "exit_train_dd2", 20.0 * fm * X_C1, 8.0 * fm * X_C1);
        hipLaunchKernelGGL((exit_dw_wgrad_kernel<IN_BN, X_C1>), dim3(X_C1 / 256, n), dim3(256), 0, s, DwSrc{w.z1, nullptr, 0, w.a1, w.b1}, w.du,
                           w.part);
        hipLaunchKernelGGL(exit_colsum_kernel, dim3(9 * X_C1 / 32), dim3(256), 0, s, w.part, n, 9 * X_C1, grad + E_D2);
    }
    {   // dh1 = dw^T(du2, D2)
        ProfScope ps(c, s, "exit_train_dh1", 18.0 * fm * X_C1, 8.0 * fm * X_C1);
        hipLaunchKernelGGL((exit_dw_kernel<IN_PLAIN, X_C1, true>), dim3(X_C1 / 256, n), dim3(256), 0, s, DwSrc{w.du, nullptr, 0, nullptr, nullptr},
                           e + E_D2, w.dz1);
    }
    {   // dz1 in place, and the tiles' parts of dgamma1 | dbeta1
        ProfScope ps(c, s, "exit_train_bn1", 8.0 * fm * X_C1, 12.0 * fm * X_C1);
        hipLaunchKernelGGL((exit_bn_back_kernel<false, X_C1>), dim3(X_C1 / 256, n), dim3(256), 0, s, w.z1, w.dz1, w.a1, w.b1, b.stats + S_M1,
                           w.i1, w.dz1, w.part);
        hipLaunchKernelGGL(exit_colsum_kernel, dim3(2 * X_C1 / 32), dim3(256), 0, s, w.part, n, 2 * X_C1, grad + E_G1);
    }
    if (b.bstats) {
        ProfScope ps(c, s, "exit_train_bnfix1", 6.0 * fm * X_C1, 12.0 * fm * X_C1);
        hipLaunchKernelGGL((exit_bn_fix_kernel<X_C1>), dim3(X_C1 / 256, n), dim3(256), 0, s, w.z1, w.a1, b.stats + S_M1, w.i1, grad + E_G1,
                           (float)M, w.dz1);
    }
    {   // dP1 = u1^T dz1
        ProfScope ps(c, s, "exit_train_dp1", 2.0 * fm * X_C0 * X_C1, 4.0 * (fm * X_C0 + fm * X_C1 + (double)X_C0 * X_C1));
        launch_mat<A_MAT_T, B_ROWS, EPI_STORE>(w.u1, X_C0, w.dz1, X_C1, grad + E_P1, X_C1, X_C0, X_C1, M, s);
    }
    {   // du1 = dz1 P1^T, where du2 was
        ProfScope ps(c, s, "exit_train_du1", 2.0 * fm * X_C0 * X_C1, 4.0 * (fm * X_C0 + fm * X_C1 + (double)X_C0 * X_C1));
        launch_mat<A_MAT_K, B_KCONT, EPI_STORE>(w.dz1, X_C1, e + E_P1, X_C1, w.du, X_C0, M, X_C0, X_C1, s);
    }
    {   // dD1 over the cached x
        ProfScope ps(c, s, "exit_train_dd1", 18.0 * fm * X_C0, (4.0 + act_elt_bytes(b.type)) * fm * X_C0);
        enqueue_cache_reader<true>(b, w.du, w.part, s);
        hipLaunchKernelGGL(exit_colsum_kernel, dim3(9 * X_C0 / 32), dim3(256), 0, s, w.part, n, 9 * X_C0, grad + E_D1);
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The refusal of an exit batch, "" for none; own_ok: the entry's own pointers are there and aligned.
std::string bad_exit(bq_ctx* c, const char* entry, const ExitBatch& b, const void* ws, bool own_ok) {
    const std::string e(entry);
    if (!c) return e + ": null context";
    if (b.n < 1 || b.n > EXIT_MAX_N) return e + ": 1 <= n <= " + std::to_string(EXIT_MAX_N);
    if (b.n_act < 1) return e + ": an empty activation cache";
    if (!aligned(b.params, 16) || !aligned(b.stats, 16) || !aligned(b.acts, 16) || !aligned(b.rows, 8) || !aligned(ws, 256) || !own_ok)
        return e + ": bad argument (null pointer, params, stats, acts or an output not 16-byte, rows not 8-byte or the workspace not 256-byte aligned)";
    return "";
}
std::string bad_exit_grad(bq_ctx* c, const char* entry, const ExitBatch& b, const void* labels, long long step, double rate, const void* ws,
                          const void* grad, const void* loss) {
    const std::string bad = bad_exit(c, entry, b, ws, labels && aligned(grad, 16) && aligned(loss, 4));
    if (!bad.empty()) return bad;
    if (step < 0 || step > 0xffffffffLL || !(rate >= 0.0) || !(rate < 1.0))
        return std::string(entry) + ": a step outside 0 .. 2^32 - 1, or a rate outside [0, 1)";
    return "";
}

// The refusal of a cache descriptor, "" for none: a type and a place of the header's, at least one row, and a mul that is a positive
// finite power of two -- 1 for float32, which is read as it is.
std::string bad_cache(const char* entry, const bq_act_cache* a) {
    const std::string e(entry);
    if (!a) return e + ": null cache descriptor";
    if (a->type != BQ_ACT_F32 && a->type != BQ_ACT_F16 && a->type != BQ_ACT_BF16) return e + ": the cache's type is none of BQ_ACT_F32 / F16 / BF16";
    if (a->where != BQ_ACT_DEVICE && a->where != BQ_ACT_HOST) return e + ": the cache's place is neither BQ_ACT_DEVICE nor BQ_ACT_HOST";
    int ex = 0;
    if (!(a->mul > 0.f) || !std::isfinite(a->mul) || std::frexp(a->mul, &ex) != 0.5f || (a->type == BQ_ACT_F32 && a->mul != 1.f))
        return e + ": the cache's mul is a positive finite power of two, and 1 for a float32 cache";
    return "";
}

// the workspace of a call on cache `a` over up to n rows: the device tier's, and the staging rows behind it for a cache in host memory
size_t exit_ws_bytes(const bq_act_cache& a, int n, bool train) {
    if (n < 1 || n > EXIT_MAX_N) return 0;
    return exit_ws(nullptr, n, train).total + (a.where == BQ_ACT_HOST ? (size_t)n * act_row_bytes(a.type) : 0);
}
// b.stage of a call whose largest batch is n
void* exit_stage(const bq_act_cache& a, void* ws, int n, bool train) {
    return a.where == BQ_ACT_HOST ? (unsigned char*)ws + exit_ws(nullptr, n, train).total : nullptr;
}

// the moving statistics after a step over n tiles, M = 100 n (class exit_train_bnmove)
int enqueue_bn_move(bq_ctx* c, float* moving, const float* batch, int n, hipStream_t s) {
    const double m = (double)n * X_POS;
    ProfScope ps(c, s, "exit_train_bnmove", 3.0 * BN_STATS, 12.0 * BN_STATS);
    hipLaunchKernelGGL(exit_bn_move_kernel, dim3(BN_STATS / 256), dim3(256), 0, s, moving, batch, 0.01 * m / (m - 1.0));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // namespace

extern "C" {

size_t bq_exit_features_workspace_bytes(int n) { return n < 1 || n > EXIT_MAX_N ? 0 : exit_ws(nullptr, n, false).total; }
size_t bq_exit_train_workspace_bytes(int n) { return n < 1 || n > EXIT_MAX_N ? 0 : exit_ws(nullptr, n, true).total; }
size_t bq_exit_features_staged_workspace_bytes(int n, int type) {
    return exit_ws_bytes(bq_act_cache{nullptr, 0, type, 1.f, BQ_ACT_HOST}, type < 0 || type > 2 ? 0 : n, false);
}
size_t bq_exit_staged_workspace_bytes(int n, int type) {
    return exit_ws_bytes(bq_act_cache{nullptr, 0, type, 1.f, BQ_ACT_HOST}, type < 0 || type > 2 ? 0 : n, true);
}

int bq_host_device_pointer(void* host, void** dev) {
    if (!host || !dev) return fail(nullptr, BQ_ERR_ARG, "bq_host_device_pointer: null pointer");
    *dev = nullptr;
    hipPointerAttribute_t at{};
    // asked of the runtime first: hipHostGetDevicePointer is only called on memory it says is host memory it registered
    if (hipPointerGetAttributes(&at, host) != hipSuccess || at.type != hipMemoryTypeHost || hipHostGetDevicePointer(dev, host, 0) != hipSuccess ||
        !*dev) {
        (void)hipGetLastError();       // the refusal is this call's answer, not a pending error of the next launch
        *dev = nullptr;
        return fail(nullptr, BQ_ERR_ARG, "bq_host_device_pointer: not mapped pinned host memory");
    }
    return BQ_OK;
}

int bq_exit_features_c(bq_ctx* c, const float* d_exit_params, const float* d_bn_stats, const bq_act_cache* cache, const int64_t* d_rows, int n,
                       float* d_feat2048, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    std::string bad = bad_cache("bq_exit_features", cache);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    ExitBatch b = exit_batch(d_exit_params, d_bn_stats, *cache, (const long long*)d_rows, n);
    bad = bad_exit(c, "bq_exit_features", b, d_ws, aligned(d_feat2048, 16));
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < exit_ws_bytes(*cache, n, false))
        return fail(c, BQ_ERR_WORKSPACE, std::string("bq_exit_features: workspace below ") +
                    (cache->where == BQ_ACT_HOST ?"bq_exit_features_staged_workspace_bytes(n, type)" : "bq_exit_features_workspace_bytes(n)"));
    DeviceGuard guard(c->device);
    ExitWs w = exit_ws(d_ws, n, false);
    w.f = d_feat2048;
    b.stage = exit_stage(*cache, d_ws, n, false);
    enqueue_exit_forward(c, b, w, "exit_feat_", (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bq_exit_features(bq_ctx* c, const float* d_exit_params, const float* d_bn_stats, const float* d_acts, int64_t n_act, const int64_t* d_rows,
                     int n, float* d_feat2048, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    const bq_act_cache cache{d_acts, n_act, BQ_ACT_F32, 1.f, BQ_ACT_DEVICE};
    return bq_exit_features_c(c, d_exit_params, d_bn_stats, &cache, d_rows, n, d_feat2048, d_ws, ws_bytes, stream);
}

int bq_exit_grad_c(bq_ctx* c, const float* d_params, const float* d_bn_stats, const bq_act_cache* cache, const int64_t* d_rows,
                   const uint8_t* d_labels, int n, int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws,
                   size_t ws_bytes, bq_stream_t stream) {
    std::string bad = bad_cache("bq_exit_grad", cache);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    ExitBatch b = exit_batch(d_params, d_bn_stats, *cache, (const long long*)d_rows, n);
    bad = bad_exit_grad(c, "bq_exit_grad", b, d_labels, (long long)step, rate, d_ws, d_grad, d_loss);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < exit_ws_bytes(*cache, n, true))
        return fail(c, BQ_ERR_WORKSPACE, std::string("bq_exit_grad: workspace below ") +
                    (cache->where == BQ_ACT_HOST ?"bq_exit_staged_workspace_bytes(n, type)" : "bq_exit_train_workspace_bytes(n)"));
    DeviceGuard guard(c->device);
    b.stage = exit_stage(*cache, d_ws, n, true);
    return enqueue_exit_grad(c, b, d_labels, (long long)step, seed, rate, d_ws, d_grad, d_loss, (hipStream_t)stream);
}

int bq_exit_grad(bq_ctx* c, const float* d_params, const float* d_bn_stats, const float* d_acts, int64_t n_act, const int64_t* d_rows,
                 const uint8_t* d_labels, int n, int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws,
                 size_t ws_bytes, bq_stream_t stream) {
    const bq_act_cache cache{d_acts, n_act, BQ_ACT_F32, 1.f, BQ_ACT_DEVICE};
    return bq_exit_grad_c(c, d_params, d_bn_stats, &cache, d_rows, d_labels, n, step, seed, rate, d_grad, d_loss, d_ws, ws_bytes, stream);
}

int bq_adam_n(bq_ctx* c, float* d_params, float* d_m, float* d_v, const float* d_grad, int64_t count, int64_t step, double lr, double b1,
              double b2, double eps, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_adam_n: null context");
    if (count < 1 || count > (int64_t)0xffffffffLL * 256) return fail(c, BQ_ERR_ARG, "bq_adam_n: 1 <= count <= 256 (2^32 - 1)");
    const std::string bad = bad_adam_args("bq_adam_n", d_params, d_m, d_v, d_grad, step, lr, b1, b2, eps);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    DeviceGuard guard(c->device);
    return enqueue_adam(c, d_params, d_m, d_v, d_grad, (long long)step, lr, b1, b2, eps, (hipStream_t)stream, (long long)count, "adam_n");
}

int bq_exit_train_steps_c(bq_ctx* c, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_bn_stats, const bq_act_cache* cache,
                          const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0, uint64_t seed,
                          double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws, size_t ws_bytes,
                          bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_exit_train_steps: null context");
    if (steps < 1 || steps > (1 << 24) || last_n < 1 || last_n > batch || !h_lr)
        return fail(c, BQ_ERR_ARG, "bq_exit_train_steps: 1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step");
    std::string bad = bad_cache("bq_exit_train_steps", cache);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    ExitBatch b = exit_batch(d_params, d_bn_stats, *cache, (const long long*)d_rows, batch);
    bad = bad_exit_grad(c, "bq_exit_train_steps", b, d_labels, (long long)step0, rate, d_ws, d_grad, d_losses);
    if (bad.empty() && step0 + steps > 0x100000000LL) bad = "bq_exit_train_steps: the steps pass 2^32";
    for (int i = 0; bad.empty() && i < steps; ++i) bad = bad_adam_args("bq_exit_train_steps", d_params, d_m, d_v, d_grad, step0 + i, h_lr[i], b1, b2, eps);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < exit_ws_bytes(*cache, batch, true))
        return fail(c, BQ_ERR_WORKSPACE, std::string("bq_exit_train_steps: workspace below ") +
                    (cache->where == BQ_ACT_HOST ? "bq_exit_staged_workspace_bytes(batch, type)" : "bq_exit_train_workspace_bytes(batch)"));
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    b.stage = exit_stage(*cache, d_ws, batch, true);          // behind the largest step's regions: a short last step uses fewer of them
    for (int i = 0; i < steps; ++i) {
        b.rows = (const long long*)d_rows + (size_t)i * batch;
        b.n = i + 1 < steps ? batch : last_n;
        RUN(enqueue_exit_grad(c, b, d_labels + (size_t)i * batch, (long long)step0 + i, seed, rate, d_ws, d_grad, d_losses + i, s));
        RUN(enqueue_adam(c, d_params, d_m, d_v, d_grad, (long long)step0 + i, h_lr[i], b1, b2, eps, s, P_ALL, "exit_train_adam"));
    }
    return BQ_OK;
}

int bq_exit_train_steps(bq_ctx* c, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_bn_stats, const float* d_acts,
                        int64_t n_act, const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0,
                        uint64_t seed, double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws,
                        size_t ws_bytes, bq_stream_t stream) {
    const bq_act_cache cache{d_acts, n_act, BQ_ACT_F32, 1.f, BQ_ACT_DEVICE};
    return bq_exit_train_steps_c(c, d_params, d_m, d_v, d_grad, d_bn_stats, &cache, d_rows, d_labels, steps, batch, last_n, step0, seed, rate,
                                 h_lr, b1, b2, eps, d_losses, d_ws, ws_bytes, stream);
}

// ---- training-mode batch norm: the calls above with the batch's own statistics (enqueue_bn_stats, exit_bn_fix_kernel)
size_t bq_exit_bn_workspace_bytes(int n, int type, int where) {
    if (type < 0 || type > 2 || (where != BQ_ACT_DEVICE && where != BQ_ACT_HOST)) return 0;
    const size_t base = exit_ws_bytes(bq_act_cache{nullptr, 0, type, 1.f, where}, n, true);
    return base ? base + al(BN_STATS * 4) : 0;      // bq_exit_train_steps_bn keeps a step's batch statistics behind the rest
}

int bq_exit_grad_bn(bq_ctx* c, const float* d_params, const bq_act_cache* cache, const int64_t* d_rows, const uint8_t* d_labels, int n,
                    int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, float* d_batch_stats, void* d_ws, size_t ws_bytes,
                    bq_stream_t stream) {
    std::string bad = bad_cache("bq_exit_grad_bn", cache);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    ExitBatch b = exit_batch(d_params, d_batch_stats, *cache, (const long long*)d_rows, n);
    bad = bad_exit_grad(c, "bq_exit_grad_bn", b, d_labels, (long long)step, rate, d_ws, d_grad, d_loss);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < bq_exit_bn_workspace_bytes(n, cache->type, cache->where))
        return fail(c, BQ_ERR_WORKSPACE, "bq_exit_grad_bn: workspace below bq_exit_bn_workspace_bytes(n, type, where)");
    DeviceGuard guard(c->device);
    b.stage = exit_stage(*cache, d_ws, n, true);
    b.bstats = d_batch_stats;
    return enqueue_exit_grad(c, b, d_labels, (long long)step, seed, rate, d_ws, d_grad, d_loss, (hipStream_t)stream);
}

int bq_exit_bn_move(bq_ctx* c, float* d_bn_stats, const float* d_batch_stats, int n, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_exit_bn_move: null context");
    if (n < 1 || n > EXIT_MAX_N) return fail(c, BQ_ERR_ARG, "bq_exit_bn_move: 1 <= n <= " + std::to_string(EXIT_MAX_N));
    if (!aligned(d_bn_stats, 16) || !aligned(d_batch_stats, 16)) return fail(c, BQ_ERR_ARG, "bq_exit_bn_move: null or misaligned statistics");
    DeviceGuard guard(c->device);
    return enqueue_bn_move(c, d_bn_stats, d_batch_stats, n, (hipStream_t)stream);
}

int bq_exit_train_steps_bn(bq_ctx* c, float* d_params, float* d_m, float* d_v, float* d_grad, float* d_bn_stats, const bq_act_cache* cache,
                           const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0, uint64_t seed,
                           double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws, size_t ws_bytes,
                           bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_exit_train_steps_bn: null context");
    if (steps < 1 || steps > (1 << 24) || last_n < 1 || last_n > batch || !h_lr)
        return fail(c, BQ_ERR_ARG, "bq_exit_train_steps_bn: 1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step");
    std::string bad = bad_cache("bq_exit_train_steps_bn", cache);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    ExitBatch b = exit_batch(d_params, d_bn_stats, *cache, (const long long*)d_rows, batch);
    bad = bad_exit_grad(c, "bq_exit_train_steps_bn", b, d_labels, (long long)step0, rate, d_ws, d_grad, d_losses);
    if (bad.empty() && step0 + steps > 0x100000000LL) bad = "bq_exit_train_steps_bn: the steps pass 2^32";
    for (int i = 0; bad.empty() && i < steps; ++i) bad = bad_adam_args("bq_exit_train_steps_bn", d_params, d_m, d_v, d_grad, step0 + i, h_lr[i], b1, b2, eps);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < bq_exit_bn_workspace_bytes(batch, cache->type, cache->where))
        return fail(c, BQ_ERR_WORKSPACE, "bq_exit_train_steps_bn: workspace below bq_exit_bn_workspace_bytes(batch, type, where)");
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    b.stage = exit_stage(*cache, d_ws, batch, true);
    b.bstats = (float*)((unsigned char*)d_ws + exit_ws_bytes(*cache, batch, true));     // behind the largest step's regions and rows
    b.stats = b.bstats;
    for (int i = 0; i < steps; ++i) {
        b.rows = (const long long*)d_rows + (size_t)i * batch;
        b.n = i + 1 < steps ? batch : last_n;
        RUN(enqueue_exit_grad(c, b, d_labels + (size_t)i * batch, (long long)step0 + i, seed, rate, d_ws, d_grad, d_losses + i, s));
        RUN(enqueue_adam(c, d_params, d_m, d_v, d_grad, (long long)step0 + i, h_lr[i], b1, b2, eps, s, P_ALL, "exit_train_adam"));
        RUN(enqueue_bn_move(c, d_bn_stats, b.bstats, b.n, s));
    }
    return BQ_OK;
}

size_t bq_head_train_workspace_bytes(int n) { return n < 1 || n > MAX_N ? 0 : train_ws(nullptr, n).total; }

int bq_head_grad(bq_ctx* c, const float* d_params, const float* d_feats, int64_t n_feat, const int64_t* d_rows, const uint8_t* d_labels, int n,
                 int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    const Batch b{d_params, d_feats, (long long)n_feat, (const long long*)d_rows, d_labels, n, (long long)step, rate, d_ws};
    const std::string bad = bad_grad_args(c, "bq_head_grad", b, d_grad, d_loss);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < bq_head_train_workspace_bytes(n)) return fail(c, BQ_ERR_WORKSPACE, "bq_head_grad: workspace below bq_head_train_workspace_bytes(n)");
    DeviceGuard guard(c->device);
    return enqueue_grad(c, b, drop_of(b, seed), d_grad, d_loss, (hipStream_t)stream);
}

size_t bq_head_validate_workspace_bytes(int n) { return n < 1 || n > VALIDATE_MAX_N ? 0 : validate_ws(nullptr, n).total; }

int bq_head_validate(bq_ctx* c, const float* d_params, const float* d_feats, int64_t n_feat, const int64_t* d_rows, const uint8_t* d_labels,
                     int n, int64_t pass, uint64_t seed, double rate, double* d_stats, double* d_rowloss, uint8_t* d_hit, void* d_ws,
                     size_t ws_bytes, bq_stream_t stream) {
    const Batch b{d_params, d_feats, (long long)n_feat, (const long long*)d_rows, d_labels, n, (long long)pass, rate, d_ws};
    const std::string bad = bad_batch(c, "bq_head_validate", b, VALIDATE_MAX_N, "pass", aligned(d_stats, 8) && !((uintptr_t)d_rowloss & 7),
                                      ": bad argument (null pointer, params or feats not 16-byte, rows, stats or rowloss not 8-byte or the "
                                      "workspace not 256-byte aligned)");
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < bq_head_validate_workspace_bytes(n))
        return fail(c, BQ_ERR_WORKSPACE, "bq_head_validate: workspace below bq_head_validate_workspace_bytes(n)");
    DeviceGuard guard(c->device);
    const Drop d = drop_of(b, seed);
    return rate > 0.0 ? enqueue_validate<true>(c, b, d, d_stats, d_rowloss, d_hit, (hipStream_t)stream)
                      : enqueue_validate<false>(c, b, d, d_stats, d_rowloss, d_hit, (hipStream_t)stream);
}

int bq_head_adam(bq_ctx* c, float* d_params, float* d_m, float* d_v, const float* d_grad, int64_t step, double lr, double b1, double b2,
                 double eps, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_head_adam: null context");
    const std::string bad = bad_adam_args("bq_head_adam", d_params, d_m, d_v, d_grad, step, lr, b1, b2, eps);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    DeviceGuard guard(c->device);
    return enqueue_adam(c, d_params, d_m, d_v, d_grad, (long long)step, lr, b1, b2, eps, (hipStream_t)stream);
}

int bq_head_train_steps(bq_ctx* c, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_feats, int64_t n_feat,
                        const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0, uint64_t seed,
                        double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws, size_t ws_bytes,
                        bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_head_train_steps: null context");
    if (steps < 1 || steps > (1 << 24) || last_n < 1 || last_n > batch || !h_lr)
        return fail(c, BQ_ERR_ARG, "bq_head_train_steps: 1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step");
    Batch b{d_params, d_feats, (long long)n_feat, (const long long*)d_rows, d_labels, batch, (long long)step0, rate, d_ws};
    std::string bad = bad_grad_args(c, "bq_head_train_steps", b, d_grad, d_losses);
    if (bad.empty() && step0 + steps > 0x100000000LL) bad = "bq_head_train_steps: the steps pass 2^32";
    for (int i = 0; bad.empty() && i < steps; ++i) bad = bad_adam_args("bq_head_train_steps", d_params, d_m, d_v, d_grad, step0 + i, h_lr[i], b1, b2, eps);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    if (ws_bytes < bq_head_train_workspace_bytes(batch))
        return fail(c, BQ_ERR_WORKSPACE, "bq_head_train_steps: workspace below bq_head_train_workspace_bytes(batch)");
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < steps; ++i, ++b.step) {
        b.rows = (const long long*)d_rows + (size_t)i * batch;
        b.labels = d_labels + (size_t)i * batch;
        b.n = i + 1 < steps ? batch : last_n;
        RUN(enqueue_grad(c, b, drop_of(b, seed), d_grad, d_losses + i, s));
        RUN(enqueue_adam(c, d_params, d_m, d_v, d_grad, b.step, h_lr[i], b1, b2, eps, s));
    }
    return BQ_OK;
}

}  // extern "C"
