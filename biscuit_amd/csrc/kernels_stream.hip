// Streaming separable-convolution kernels for the big, HBM-bound entry-flow layers (block 2 at 147x147: 64 -> 128,
// 128 -> 128 and the block's fused tail), 16-bit storage, round 4.
//
// The tile kernels these layers ran on (kernels_tile.hip) are one fat workgroup per CU that walks barrier-separated
// phases -- halo registers -> LDS, barrier, depthwise, matrix stage, staged epilogue -- so all 256 CUs load, compute and
// store in lock step and nothing overlaps (3.4-4.2 TB/s).  Here every WAVE is an independent worker and there is no
// workgroup barrier after the weights have been copied to LDS:
//  * a work item is a vertical strip of an image: <= 16 output columns x a band of rows.  The wave walks DOWN the strip
//    one output row per step.
//  * lane = channel pair.  A step fetches ONE new input row of 18 pixels with coalesced `global_load_dword`s (64 lanes x
//    4 B = the 256 contiguous bytes of a 128-channel pixel), one step ahead of its use.  No halo image in LDS, no staging
//    pass, every input row of a strip is read once (18 columns per <= 16 output columns).
//  * depthwise 3x3 as RUNNING PARTIAL SUMS in registers: for every column of the strip a lane keeps sa = the taps of
//    rows y-1 and y already applied, sb = the taps of row y applied for the NEXT output row.  The new row is converted to
//    fp32 once (not once per output row it takes part in) and pushed: out(y) = sa + taps2 . row, sa' = sb + taps1 . row,
//    sb' = taps0 . row -- nine fp32 fmas per output in exactly the order of the tile kernels' tap loop (dy-major, from
//    0.0f), so the results are bit-identical to them; no 3-row window to rotate.
//  * the 16 results of a step, rounded to the storage type, go to a 4 KB wave-private A tile in LDS -- the transposition
//    from (lane = channel pair) to the MFMA operand (lane = pixel, 8 consecutive channels) -- and come back as the B
//    operand of v_mfma_f32_16x16x32 (D[cout][pixel]); the weights (A operand, 16x16x32 fragment order with interleaved
//    fragment pairs: "<layer>/wp16") sit in LDS once per workgroup.
//  * epilogue straight from the accumulators: with the pair interleave a lane holds 8 consecutive channels of its pixel
//    per fragment pair -> folded BN, ReLU, one 16-byte store; a pair's store covers 64 contiguous bytes of 16 pixels.
//  * 12 waves per CU (3 per SIMD, <= 168 registers; the fused tail: 8, its 240 registers spill at 168 and spills in the vmcnt
//    stream cost 2x) drift apart by themselves: one wave's loads and stores run under
//    the others' depthwise and matrix work.
#include "mfma16_common.h"

namespace {
using namespace bqk;

constexpr int STREAM_NW = 12;   // waves per workgroup of the plain streaming kernel (<= 128 output channels)
constexpr int TAIL_NW = 8;      // waves per workgroup of the fused block-2 tail

// first element and length of part s when n elements are cut into ns parts of nearly equal length
__device__ __forceinline__ void strip_span(int s, int n, int ns, int& x0, int& nc) {
    const int base = n / ns, rem = n - base * ns;
    x0 = s * base + (s < rem ? s : rem);
    nc = base + (s < rem ? 1 : 0);
}

// ---- depthwise 3x3 of one strip as running partial sums --------------------------------------------------------------
// NCOL output columns per lane, window columns j = 0 .. NCOL + 1 (column j is output column j - 1's left neighbour).
// push(row): row = the packed input row y + 1, already masked to zero where it lies outside the image.
//   OUT:  out(y)[x] = sa[x] + taps(2, .) . row[x ..]  -> rounded, written to the A tile (one ds_write_b32 per column)
//   then  sa[x] = sb[x] + taps(1, .) . row[x ..],  sb[x] = 0 + taps(0, .) . row[x ..]
// Tap order per output: (0,0) (0,1) (0,2) (1,0) ... (2,2), each `a = fma(tap, v, a)` from 0.0f: the tile kernels' order.
// (The same sums in packed half arithmetic for the f16 instances were measured in round 6 and not adopted: experiments/r06.md.)
template <typename T, int NCOL>
struct DwSums {
    f32x2s sa[NCOL], sb[NCOL];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int x = 0; x < NCOL; ++x) { sa[x] = (f32x2s){0.f, 0.f}; sb[x] = (f32x2s){0.f, 0.f}; }
    }
    template <bool OUT>
    __device__ __forceinline__ void push(const f32x2s (&tap)[9], const unsigned (&row)[NCOL + 2], unsigned char* a_lane, int ast) {
        f32x2s v[NCOL + 2];
#pragma unroll
        for (int j = 0; j < NCOL + 2; ++j) v[j] = unpack2<T>(row[j]);
#pragma unroll
        for (int x = 0; x < NCOL; ++x) {
            if constexpr (OUT) {
                f32x2s o = sa[x];
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) o = __builtin_elementwise_fma(tap[6 + dx], v[x + dx], o);
                *reinterpret_cast<unsigned*>(a_lane + x * ast) = H16<T>::pack2(o.x, o.y);
            }
            f32x2s a = sb[x];
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) a = __builtin_elementwise_fma(tap[3 + dx], v[x + dx], a);
            sa[x] = a;
            f32x2s b = {0.f, 0.f};
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) b = __builtin_elementwise_fma(tap[dx], v[x + dx], b);
            sb[x] = b;
        }
    }
};

// ---- pointwise: D[cout][pixel] = W[cout][k] * A[pixel][k] from the wave's A tile (LDS operations of a wave complete in order)
template <typename T, int KS, int NF>
__device__ __forceinline__ void pointwise(const unsigned char* smem_w, const unsigned char* a_read, int lane, f32x4 (&acc)[NF]) {
    // Written as an explicit pipeline: all B operands first, the weight fragments in groups of four, one group ahead of the
    // MFMAs that use them (LDS returns in order: the wait in front of a group is lgkmcnt(4), the next group stays in flight).
    // Left as `read fragment; mfma` the compiler waits lgkmcnt(0) in front of most MFMAs: an LDS round trip each.
    constexpr int G = 4, NG = KS * NF / G;
    static_assert(NF % G == 0, "fragments per k-step in groups of four");
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    uint4 b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const uint4*>(a_read + ks * 64);
    uint4 w[2][G];
    auto fetch = [&](int grp, uint4 (&dst)[G]) {
#pragma unroll
        for (int i = 0; i < G; ++i)
            dst[i] = *reinterpret_cast<const uint4*>(smem_w + ((grp * G + i) * 64 + lane) * 16);    // (ks * NF + f) = grp * G + i
    };
    fetch(0, w[0]);
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
        if (grp + 1 < NG) fetch(grp + 1, w[(grp + 1) & 1]);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int ks = (grp * G + i) / NF, f = (grp * G + i) % NF;
            acc[f] = mma16<T>(w[grp & 1][i], b[ks], acc[f]);
        }
    }
}

template <typename T>
struct StreamParams {
    const T* in;           // NHWC [n][H][W][CIN]
    const uint4* wp16;     // [CIN/32][COUT/16][64] x 16 B (weights.py: pack_fragments16)
    const float* dw;       // [9][CIN] fp32
    const float* scale;    // [COUT] folded BN
    const float* bias;
    T* out;                // NHWC [n][H][W][COUT]
    int n, H, W;
    int nstrips, nbands;   // strips per row (<= 16 columns each), bands per image
    int items;             // n * nbands * nstrips
    int relu;
};

template <typename T, int CIN, int COUT, bool RELU_IN, int NW>
__global__ void __launch_bounds__(NW * 64) sepconv_stream_kernel(const StreamParams<T> p) {
    if constexpr (H16<T>::F16) bq_f16_saturate();
    constexpr int NT = NW * 64;
    constexpr int KS = CIN / 32, NF = COUT / 16, NQ = COUT / 32;
    constexpr int HALVES = 128 / CIN;           // 1: a lane is a channel pair of all 128; 2: lanes 32-63 take columns 8-15
    constexpr int NCOL = 16 / HALVES;           // output columns per lane
    constexpr int NWIN = NCOL + 2;              // window columns per lane
    constexpr int AST = CIN * 2 + 32;           // A row stride in 16-byte slots = 2 (mod 4): the operand's ds_read_b128 (lane -> row l & 15,
                                                // k-group l >> 4) is conflict-free over its four 16-lane groups; an ODD slot count (round 4)
                                                // leaves one 2-way conflict per group: 27 % of the LDS cycles of the cooperative tail
    constexpr int W_BYTES = KS * NF * 1024;
    constexpr int SB_OFF = W_BYTES;             // scale[COUT] | bias[COUT], fp32
    constexpr int A_OFF = SB_OFF + 2 * COUT * 4;
    constexpr int A_BYTES = 16 * AST;
    static_assert(CIN == 64 || CIN == 128, "lane = channel pair of <= 128 channels");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int i = tid; i < W_BYTES / 16; i += NT) *reinterpret_cast<uint4*>(smem + i * 16) = p.wp16[i];
    for (int i = tid; i < COUT; i += NT) {
        reinterpret_cast<float*>(smem + SB_OFF)[i] = p.scale[i];
        reinterpret_cast<float*>(smem + SB_OFF)[COUT + i] = p.bias[i];
    }
    const int cpair = HALVES == 1 ? lane : (lane & 31);
    const int chalf = HALVES == 1 ? 0 : (lane >> 5);
    f32x2s tap[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tap[t] = *reinterpret_cast<const f32x2s*>(p.dw + t * CIN + 2 * cpair);
    __syncthreads();                            // the only workgroup barrier of the kernel

    unsigned char* const At = smem + A_OFF + wave * A_BYTES;
    const int px = lane & 15, g = lane >> 4;
    unsigned char* const a_lane = At + (chalf * NCOL) * AST + cpair * 4;
    const unsigned char* const a_read = At + px * AST + g * 16;
    const float* const sb = reinterpret_cast<const float*>(smem + SB_OFF) + 8 * g;
    const unsigned lo2 = p.relu ? 0u : 0x80008000u;     // ReLU = packed signed 16-bit max with 0 (0x8000: no-op)
    const int wgx = xcd_tile(blockIdx.x, gridDim.x);
    const int lane_el = chalf * NCOL * CIN + 2 * cpair;  // element offset of this lane's first window column
    // buffer resource of the output tensor (raw buffer, 32-bit byte offsets: launch_stream checks the size)
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.out, 0, (int)((size_t)p.n * p.H * p.W * COUT * sizeof(T)), 0x00020000);

    for (int it = 0;; ++it) {
        const int item = __builtin_amdgcn_readfirstlane((it * (int)gridDim.x + wgx) * NW + wave);
        if (item >= p.items) break;
        const int strip = item % p.nstrips;
        const int t1 = item / p.nstrips;
        const int band = t1 % p.nbands;
        const int img = t1 / p.nbands;
        int x0, nc, y0, nr;
        strip_span(strip, p.W, p.nstrips, x0, nc);
        strip_span(band, p.H, p.nbands, y0, nr);
        const int y1 = y0 + nr;
        // window column j of this lane is image column xl + j; outside [0, W) it reads as zero ('same' padding); columns
        // past the strip's own 16 + 1 are never used for a stored pixel.  Column -1 of an image's first row and the columns
        // behind its last row's end are read (and masked) from the bytes next to the tensor: the workspace is padded.
        const int xl = x0 - 1 + chalf * NCOL;
        unsigned cmask = 0;
#pragma unroll
        for (int j = 0; j < NWIN; ++j) cmask |= ((unsigned)(xl + j) < (unsigned)p.W) ? (1u << j) : 0u;
        const T* const img_in = p.in + ((size_t)img * p.H * p.W + (x0 - 1)) * CIN + lane_el;

        unsigned nx[NWIN], row[NWIN];
        auto load_row = [&](int y) {                       // row clamped into the image: always valid memory
            const int yc = y < 0 ? 0 : (y >= p.H ? p.H - 1 : y);
            const T* rp = img_in + (size_t)yc * p.W * CIN;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) nx[j] = *reinterpret_cast<const unsigned*>(rp + j * CIN);
        };
        auto take_row = [&](int y) {                       // nx (row y) -> row, zero outside the image, ReLU of the layer in front
            const unsigned m = (unsigned)y < (unsigned)p.H ? cmask : 0u;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = RELU_IN ? relu_pk16(nx[j]) : nx[j];
            if (HALVES == 1 && m == (1u << NWIN) - 1u) return;      // (wave-uniform) an inner strip, a row of the image: nothing to mask
            asm volatile("" ::: "memory");                 // keep the branch: 18 selects on every row otherwise
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = ((m >> j) & 1u) ? row[j] : 0u;
        };
        DwSums<T, NCOL> dws;
        dws.clear();
        load_row(y0 - 1); take_row(y0 - 1);
        load_row(y0);
        dws.template push<false>(tap, row, a_lane, AST);   // (only sb of this push is used)
        take_row(y0);
        load_row(y0 + 1);
        dws.template push<false>(tap, row, a_lane, AST);

        // Stores are raw buffer stores: a lane whose pixel lies outside the strip gets an offset beyond the buffer and the
        // hardware drops its store.  Under `if (px < nc)` hipcc cannot count the stores in vmcnt any more and the wait for
        // the next input row becomes a wait for this row's stores as well (vmcnt retires in order).  (+ 64 q must stay
        // below 2^32: the offset sum wraps there: 0xfffff000 + 64 * 7.)
        unsigned ooff = px < nc ? (unsigned)(((((size_t)img * p.H + y0) * p.W + x0 + px) * COUT + 8 * g) * sizeof(T)) : 0xfffff000u;
        const unsigned ostep = px < nc ? (unsigned)((size_t)p.W * COUT * sizeof(T)) : 0u;
        // NQ stores the hardware drops, so that the vector-memory queue looks the same on entry to the loop as on its back
        // edge -- the next row's loads, then a row's stores: the compiler then waits for the LOADS at the top of a step
        // (vmcnt(NQ)); with "loads only" on entry it merged the two into vmcnt(0) and every step waited for the previous
        // step's stores to be acknowledged.
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            __builtin_amdgcn_raw_buffer_store_b128((u32x4s){0u, 0u, 0u, 0u}, orsrc, (int)(0xfffff000u + 16 * q), 0, 0);
        for (int y = y0; y < y1; ++y, ooff += ostep) {
            take_row(y + 1);
            // the row after next, one step ahead of its use (the last step re-reads row y1: an L2 hit, branch-free)
            load_row(y + 2 < y1 ? y + 2 : y1);
            // the loads really are issued here: left to itself hipcc sinks them behind the MFMAs, half a step later
            // (64 -> 128: 0.477 -> 0.440 ms)
            __builtin_amdgcn_sched_barrier(0);
            dws.template push<true>(tap, row, a_lane, AST);
            f32x4 acc[NF];
            pointwise<T, KS, NF>(smem, a_read, lane, acc);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned o[4];
                bn_pair<T>(acc[2 * q], acc[2 * q + 1], sb + 32 * q, COUT, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) asm("v_pk_max_i16 %0, %1, %2" : "=v"(o[i]) : "v"(o[i]), "v"(lo2));
                const u32x4s ov = {o[0], o[1], o[2], o[3]};
                __builtin_amdgcn_raw_buffer_store_b128(ov, orsrc, (int)ooff + 64 * q, 0, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Block tail in one kernel: out = MaxPool3x3/s2 'same'(BN(sepconv2(y1))) + BN(Conv1x1/s2(x)).
//
// The second separable convolution of an entry-flow block is only ever read by the block's max-pool: written and read
// back it is 2 x 1.42 GB of the 4.8 GB that block 2's sepconv2 + pool/shortcut kernel pair move.  On the streaming
// structure the pool is incremental and needs no tile-sized staging (the 16x16-tile form of round 3 lost to its
// serialised phases):
//  * a strip owns <= 7 POOLED columns = 15 convolution columns (window columns 2xo-pl .. 2xo-pl+2 overlap by one, so
//    strips overlap by one column: 16 MFMA pixel slots per 14 new columns), a band owns a run of pooled rows;
//  * a row step produces one convolution row in the accumulator layout (lane = pixel slot px, 8 channels per fragment
//    pair), folded BN, rounded to the storage type -- the rounding point of the tensor that no longer exists;
//  * vertical max: a running packed maximum VM of the rows of the current window (16 registers); horizontal max on the
//    rows that complete a window: the neighbours px-1 / px+1 are the neighbouring LANES of a 16-lane DPP row
//    (row_shr:1 / row_shl:1), columns outside the image count as -inf;
//  * the shortcut of the pooled row: x sampled at (2yo, 2xo) straight from global memory in MFMA operand layout (slot
//    px reads the pixel its own pooled output needs, so the result lands in the lane that holds the pooled maximum),
//    16 more MFMAs per pooled row, folded BN, rounded (the rounding point of the shortcut tensor of the two-kernel
//    path), added in fp32, rounded, stored from the odd slots.
template <typename T>
struct TailParams {
    const T* in;           // sepconv2's input [n][H][W][128]
    const uint4* wp16;     // sepconv2 pointwise weights, 16x16x32 fragment order [4][8][64] x 16 B
    const float* dw;       // [9][128]
    const float* scale;    // [128] folded BN of sepconv2
    const float* bias;
    const T* x;            // the block's input [n][H][W][CX]
    const uint4* wr16;     // shortcut weights [CX/32][8][64] x 16 B
    const float* rscale;   // [128] folded BN of the shortcut
    const float* rbias;
    T* out;                // [n][Ho][Wo][128]
    int n, H, W, Ho, Wo;
    int nstrips, nbands, items;
};

// pooled rows [p0, p0 + np) of band b when Ho rows are cut into nb bands: the first and the last band end at the image
// border (one convolution row fewer than 2 np + 1), so the remainder goes to them first
__device__ __forceinline__ void band_span(int b, int Ho, int nb, int& p0, int& np) {
    const int base = Ho / nb, rem = Ho - base * nb;
    const int lo = (rem + 1) / 2, hi = rem / 2;           // bands [0, lo) and [nb - hi, nb) take one more
    p0 = b * base + (b < lo ? b : lo) + (b > nb - hi ? b - (nb - hi) : 0);
    np = base + ((b < lo || b >= nb - hi) ? 1 : 0);
}

template <typename T, int CX, int NW>
__global__ void __launch_bounds__(NW * 64) block_tail_stream_kernel(const TailParams<T> p) {
    if constexpr (H16<T>::F16) bq_f16_saturate();
    constexpr int NT = NW * 64;
    constexpr int CIN = 128, COUT = 128, KS = CIN / 32, NF = COUT / 16, NQ = COUT / 32, NCOL = 16, NWIN = NCOL + 2;
    constexpr int KR = CX / 32;
    constexpr int AST = CIN * 2 + 32;           // slots per row = 2 (mod 4), see sepconv_stream_kernel
    constexpr int W_BYTES = KS * NF * 1024, WR_BYTES = KR * NF * 1024;
    constexpr int WR_OFF = W_BYTES;
    constexpr int SB_OFF = WR_OFF + WR_BYTES;   // scale | bias | rscale | rbias, fp32 [4][COUT]
    constexpr int A_OFF = SB_OFF + 4 * COUT * 4;
    constexpr int A_BYTES = 16 * AST;
    constexpr unsigned NEG = NegInf<T>::v;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < W_BYTES / 16; i += NT) *reinterpret_cast<uint4*>(smem + i * 16) = p.wp16[i];
    for (int i = tid; i < WR_BYTES / 16; i += NT) *reinterpret_cast<uint4*>(smem + WR_OFF + i * 16) = p.wr16[i];
    for (int i = tid; i < COUT; i += NT) {
        float* sbw = reinterpret_cast<float*>(smem + SB_OFF);
        sbw[i] = p.scale[i]; sbw[COUT + i] = p.bias[i]; sbw[2 * COUT + i] = p.rscale[i]; sbw[3 * COUT + i] = p.rbias[i];
    }
    f32x2s tap[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tap[t] = *reinterpret_cast<const f32x2s*>(p.dw + t * CIN + 2 * lane);
    __syncthreads();

    unsigned char* const At = smem + A_OFF + wave * A_BYTES;
    const int px = lane & 15, g = lane >> 4;
    unsigned char* const a_lane = At + lane * 4;
    const unsigned char* const a_read = At + px * AST + g * 16;
    const float* const sb = reinterpret_cast<const float*>(smem + SB_OFF) + 8 * g;
    const int wgx = xcd_tile(blockIdx.x, gridDim.x);
    const int pt = p.H & 1, pl = p.W & 1;               // TensorFlow 'same' padding of the pool in front: 1 for odd sizes
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.out, 0, (int)((size_t)p.n * p.Ho * p.Wo * COUT * sizeof(T)), 0x00020000);

    for (int it = 0;; ++it) {
        const int item = __builtin_amdgcn_readfirstlane((it * (int)gridDim.x + wgx) * NW + wave);
        if (item >= p.items) break;
        const int strip = item % p.nstrips;
        const int t1 = item / p.nstrips;
        const int band = t1 % p.nbands;
        const int img = t1 / p.nbands;
        int xo_a, npx, p0, npb;
        strip_span(strip, p.Wo, p.nstrips, xo_a, npx);   // pooled columns [xo_a, xo_a + npx), npx <= 7
        band_span(band, p.Ho, p.nbands, p0, npb);        // pooled rows [p0, p0 + npb)
        const int x0 = 2 * xo_a - pl;                    // convolution column of pixel slot 0 (may be -1)
        int ys = 2 * p0 - pt;                            // first and last convolution row of the band
        int ye = 2 * (p0 + npb - 1) - pt + 2;
        ys = ys < 0 ? 0 : ys;
        ye = ye > p.H - 1 ? p.H - 1 : ye;
        const int xl = x0 - 1;
        unsigned cmask = 0;
#pragma unroll
        for (int j = 0; j < NWIN; ++j) cmask |= ((unsigned)(xl + j) < (unsigned)p.W) ? (1u << j) : 0u;
        const T* const img_in = p.in + ((size_t)img * p.H * p.W + (x0 - 1)) * CIN + 2 * lane;
        const bool col_out = (unsigned)(x0 + px) >= (unsigned)p.W;      // this slot's column lies outside the image: -inf for the pool
        const bool any_col_out = x0 < 0 || x0 + 15 >= p.W;              // (wave-uniform)
        // shortcut operand: slot px (odd) needs x at column 2 xo = x0 + px - (1 - pl); even slots read their right neighbour's
        // pixel (same lines, never used); lane = (slot, k-group g)
        int xs = x0 + (px | 1) - (1 - pl);
        xs = xs < 0 ? 0 : (xs > p.W - 1 ? p.W - 1 : xs);
        const T* const xcol = p.x + ((size_t)img * p.H * p.W + xs) * CX + 8 * g;
        // pooled output of this lane: odd slots with (px >> 1) < npx
        const bool lane_out = (px & 1) && (px >> 1) < npx;
        const unsigned obase = (unsigned)((((size_t)img * p.Ho * p.Wo + xo_a + (px >> 1)) * COUT + 8 * g) * sizeof(T));

        unsigned nx[NWIN], row[NWIN];
        auto load_row = [&](int y) {
            const int yc = y < 0 ? 0 : (y >= p.H ? p.H - 1 : y);
            const T* rp = img_in + (size_t)yc * p.W * CIN;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) nx[j] = *reinterpret_cast<const unsigned*>(rp + j * CIN);
        };
        auto take_row = [&](int y) {
            const unsigned m = (unsigned)y < (unsigned)p.H ? cmask : 0u;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = nx[j];
            if (m == (1u << NWIN) - 1u) return;            // (wave-uniform) an inner strip, a row of the image: nothing to mask
            asm volatile("" ::: "memory");                 // keep the branch: 18 selects on every row otherwise
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = ((m >> j) & 1u) ? row[j] : 0u;
        };
        DwSums<T, NCOL> dws;
        dws.clear();
        load_row(ys - 1); take_row(ys - 1);
        load_row(ys);
        dws.template push<false>(tap, row, a_lane, AST);
        take_row(ys);
        load_row(ys + 1);
        dws.template push<false>(tap, row, a_lane, AST);

        unsigned VM[4 * NQ];
#pragma unroll
        for (int i = 0; i < 4 * NQ; ++i) VM[i] = NEG;
        // (dropped stores: the queue on entry looks like the queue on the back edge, see the plain kernel)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            __builtin_amdgcn_raw_buffer_store_b128((u32x4s){0u, 0u, 0u, 0u}, orsrc, (int)(0xfffff000u + 16 * q), 0, 0);

        for (int y = ys; y <= ye; ++y) {
            // the pooled row this convolution row completes (t even) -- or the next one will (t odd)
            const int t = y + pt;
            const bool t_even = (t & 1) == 0;
            int yo = (t - 1) >> 1;
            yo = yo < 0 ? 0 : (yo > p.Ho - 1 ? p.Ho - 1 : yo);
            const bool do_emit = (t_even ? t >= 2 : y == p.H - 1) && yo >= p0 && y <= ye;
            take_row(y + 1);
            // shortcut operand of pooled row yo: x[2 yo][xs][32 ks + 8 g ..].  In FRONT of the next row's loads: vmcnt retires
            // in order, so the wait for these (inside this step) must not be a wait for the row that is needed a step later
            uint4 xb[KR];
            {
                const T* xr = xcol + (size_t)(2 * yo) * p.W * CX;
#pragma unroll
                for (int ks = 0; ks < KR; ++ks) xb[ks] = *reinterpret_cast<const uint4*>(xr + 32 * ks);
            }
            load_row(y + 2 <= ye + 1 ? y + 2 : ye + 1);
            __builtin_amdgcn_sched_barrier(0);             // (as in the plain kernel: the loads are issued here)
            dws.template push<true>(tap, row, a_lane, AST);
            f32x4 acc[NF];
            pointwise<T, KS, NF>(smem, a_read, lane, acc);
            // ---- folded BN (no ReLU: the block's last convolution), rounded; then the running maximum of the window's rows
            unsigned cur[4 * NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned o[4];
                bn_pair<T>(acc[2 * q], acc[2 * q + 1], sb + 32 * q, COUT, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[4 * q + i] = o[i];
            }
            if (any_col_out) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int i = 0; i < 4 * NQ; ++i) cur[i] = col_out ? NEG : cur[i];
            }
#pragma unroll
            for (int i = 0; i < 4 * NQ; ++i) VM[i] = pmax2<T>(VM[i], cur[i]);
            u32x4s po[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) po[q] = (u32x4s){0u, 0u, 0u, 0u};
            if (do_emit) {                                // wave-uniform; no memory operation of the vmcnt stream inside
                asm volatile("" ::: "memory");            // a real branch: left alone hipcc runs all of this on every row and selects
                // shortcut: D[cout][slot] = Wr[cout][k] x[k][slot]
                f32x4 ar[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) ar[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KR; ++ks)
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        const uint4 wf = *reinterpret_cast<const uint4*>(smem + WR_OFF + ((ks * NF + f) * 64 + lane) * 16);
                        ar[f] = mma16<T>(wf, xb[ks], ar[f]);
                    }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    unsigned res[4], o[4];
                    bn_pair<T>(ar[2 * q], ar[2 * q + 1], sb + 2 * COUT + 32 * q, COUT, res);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned c = VM[4 * q + i];
                        // neighbouring pixel slots = neighbouring lanes of the 16-lane DPP row; row ends keep -inf
                        // (the row's end lanes read 0: slots 0 and 15 are never the centre of a stored pooled pixel)
                        const unsigned lft = (unsigned)__builtin_amdgcn_mov_dpp((int)c, 0x111, 0xf, 0xf, true);   // row_shr:1
                        const unsigned rgt = (unsigned)__builtin_amdgcn_mov_dpp((int)c, 0x101, 0xf, 0xf, true);   // row_shl:1
                        o[i] = padd2<T>(pmax2<T>(pmax2<T>(lft, c), rgt), res[i]);
                    }
                    po[q] = (u32x4s){o[0], o[1], o[2], o[3]};
                }
            }
            {
                const unsigned off = (do_emit && lane_out) ? obase + (unsigned)yo * (unsigned)(p.Wo * COUT * sizeof(T)) : 0xfffff000u;
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    __builtin_amdgcn_raw_buffer_store_b128(po[q], orsrc, (int)off + 64 * q, 0, 0);
            }
            if (t_even) {
#pragma unroll
                for (int i = 0; i < 4 * NQ; ++i) VM[i] = cur[i];
            }
        }
    }
}

inline int pick_bands(long long base_items, int rows, int rows_per_band, int min_rows, int waves);

// ------------------------------------------------------------------------------------------------------------------------
// Block tail for 256 channels (block 3 at 74x74): the same fusion, waves COOPERATING on a strip.
//
// K = N = 256 does not fit a wave-private strip: 128 KB of pointwise weights per wave is neither LDS nor registers.  Split
// over the eight waves of a workgroup it fits in REGISTERS: wave w owns output channels [32 w, 32 w + 32) -- one fragment
// pair, 8 k-steps x 2 fragments = 64 registers of sepconv2 weights and 32 of shortcut weights, loaded once per workgroup --
// and the depthwise convolution of input channels [32 w, 32 w + 32) (lane = channel pair x a group of four columns).  One
// strip step:
//   every wave pushes the new row through ITS channels' running sums and writes its 64-byte slice of the 16 pixels' A rows
//   (double-buffered) -> ONE workgroup barrier (LDS only: `s_waitcnt lgkmcnt(0); s_barrier`, the row prefetch stays in
//   flight) -> every wave multiplies the whole A tile (K = 256) by its own 32 columns -> folded BN, running maximum, and on
//   the rows that complete a pool window the horizontal maximum by DPP, the shortcut's 8 MFMAs on x fetched in operand
//   layout, add, 16-byte stores -- all per wave on its own 32 channels: pooling is per channel, nothing crosses waves.
// No weight traffic at all in the loop (the wide kernel streams 128 KB per 148 pixels from L2), no halo image, and the
// 74x74x256 tensor between the convolution and the pool is never written.
template <typename T>
struct CoopParams {
    const T* in;           // sepconv2's input [n][H][W][C]           (C = 256: block 3)
    const uint4* wp16;     // [C / 32][C / 16][64] x 16 B
    const float* dw;       // [9][C]
    const float* scale;    // [C]
    const float* bias;
    const T* x;            // the block's input [n][H][W][C / 2]
    const uint4* wr16;     // [C / 64][C / 16][64] x 16 B
    const float* rscale;
    const float* rbias;
    T* out;                // [n][Ho][Wo][C]
    int n, H, W, Ho, Wo;
    int nstrips, nbands, items;
};

template <typename T, int C, int WGS>
__global__ void __launch_bounds__(C * 2, WGS) block_tail_coop_kernel(const CoopParams<T> p) {
    if constexpr (H16<T>::F16) bq_f16_saturate();
    constexpr int CIN = C, COUT = C, CX = C / 2, KS = CIN / 32, KR = CX / 32, NCOL = 4, NWIN = NCOL + 2;
    constexpr int NT = C * 2, NFR = COUT / 16;          // C / 32 waves of 32 output (and depthwise input) channels; 16-wide fragments
    constexpr int AST = CIN * 2 + 32;           // slots per row = 2 (mod 4), see sepconv_stream_kernel
    constexpr int A_BYTES = 16 * AST;
    constexpr int SB_OFF = 2 * A_BYTES;         // scale | bias | rscale | rbias, fp32 [4][COUT]
    constexpr unsigned NEG = NegInf<T>::v;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < COUT; i += NT) {
        float* sbw = reinterpret_cast<float*>(smem + SB_OFF);
        sbw[i] = p.scale[i]; sbw[COUT + i] = p.bias[i]; sbw[2 * COUT + i] = p.rscale[i]; sbw[3 * COUT + i] = p.rbias[i];
    }
    // this wave's weights: fragments 2 w and 2 w + 1 of every k-step, in registers for the whole kernel
    uint4 wq[KS][2], wrq[KR][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) wq[ks][i] = p.wp16[((size_t)ks * NFR + 2 * wave + i) * 64 + lane];
#pragma unroll
    for (int ks = 0; ks < KR; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) wrq[ks][i] = p.wr16[((size_t)ks * NFR + 2 * wave + i) * 64 + lane];
    const int pair = lane & 15, cg = lane >> 4;                      // depthwise role: channels 32 w + 2 pair (+1), columns 4 cg .. 4 cg + 3
    f32x2s tap[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tap[t] = *reinterpret_cast<const f32x2s*>(p.dw + t * CIN + 32 * wave + 2 * pair);
    __syncthreads();

    const int px = lane & 15, g = lane >> 4;                         // matrix role: pixel slot, channel group
    const float* const sb = reinterpret_cast<const float*>(smem + SB_OFF) + 32 * wave + 8 * g;
    const int wgx = xcd_tile(blockIdx.x, gridDim.x);
    const int pt = p.H & 1, pl = p.W & 1;
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.out, 0, (int)((size_t)p.n * p.Ho * p.Wo * COUT * sizeof(T)), 0x00020000);

    for (int item = wgx; item < p.items; item += (int)gridDim.x) {
        const int strip = item % p.nstrips;
        const int t1 = item / p.nstrips;
        const int band = t1 % p.nbands;
        const int img = t1 / p.nbands;
        int xo_a, npx, p0, npb;
        strip_span(strip, p.Wo, p.nstrips, xo_a, npx);
        band_span(band, p.Ho, p.nbands, p0, npb);
        const int x0 = 2 * xo_a - pl;
        int ys = 2 * p0 - pt;
        int ye = 2 * (p0 + npb - 1) - pt + 2;
        ye = ye > p.H - 1 ? p.H - 1 : ye;                            // (ys = -1 with a padded top row: a ghost step, below)
        const int xl = x0 - 1 + NCOL * cg;                           // image column of this lane's window column 0
        unsigned cmask = 0;
#pragma unroll
        for (int j = 0; j < NWIN; ++j) cmask |= ((unsigned)(xl + j) < (unsigned)p.W) ? (1u << j) : 0u;
        const bool inner = x0 >= 1 && x0 + 16 < p.W;                 // (wave-uniform) no window column outside the image
        const T* const img_in = p.in + ((size_t)img * p.H * p.W + xl) * CIN + 32 * wave + 2 * pair;
        const bool col_out = (unsigned)(x0 + px) >= (unsigned)p.W;
        const bool any_col_out = x0 < 0 || x0 + 15 >= p.W;
        int xs = x0 + (px | 1) - (1 - pl);
        xs = xs < 0 ? 0 : (xs > p.W - 1 ? p.W - 1 : xs);
        const T* const xcol = p.x + ((size_t)img * p.H * p.W + xs) * CX + 8 * g;
        const bool lane_out = (px & 1) && (px >> 1) < npx;
        const unsigned obase = (unsigned)((((size_t)img * p.Ho * p.Wo + xo_a + (px >> 1)) * COUT + 32 * wave + 8 * g) * sizeof(T));

        // two register sets for rows in flight: a step consumes the row loaded TWO steps earlier (a step is ~1 us here, less
        // than an HBM round trip under load: with one set the kernel waited for its loads, 0.57 against 0.40 ms without them)
        unsigned nxA[NWIN], nxB[NWIN], row[NWIN];
        auto load_row = [&](int y, unsigned (&nx)[NWIN]) {
            const int yc = y < 0 ? 0 : (y >= p.H ? p.H - 1 : y);
            const T* rp = img_in + (size_t)yc * p.W * CIN;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) nx[j] = *reinterpret_cast<const unsigned*>(rp + j * CIN);
        };
        auto take_row = [&](int y, const unsigned (&nx)[NWIN]) {
            const unsigned m = (unsigned)y < (unsigned)p.H ? cmask : 0u;
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = nx[j];
            if (inner && (unsigned)y < (unsigned)p.H) return;
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = 0; j < NWIN; ++j) row[j] = ((m >> j) & 1u) ? row[j] : 0u;
        };
        DwSums<T, NCOL> dws;
        dws.clear();
        unsigned char* a_lane0 = smem + (NCOL * cg) * AST + (32 * wave + 2 * pair) * 2;      // buffer 0; buffer 1 at + A_BYTES
        // Software pipeline: a step pushes row y + 2 -- the depthwise output of row y + 1 goes to the OTHER A buffer -- and
        // multiplies row y's A tile, written a step earlier: the vector ALU work of the next row and the matrix work of this
        // one are independent inside a wave (first form, depthwise -> barrier -> matrix on the same row: both waves of a SIMD
        // in the same phase at the same time, 0.61 ms).
        uint4 xb[KR];                                 // shortcut operand x[2 yo][xs][32 ks + 8 g ..] of the next window to complete
        auto load_x = [&](int yo) {
            const T* xr = xcol + (size_t)(2 * yo) * p.W * CX;
#pragma unroll
            for (int ks = 0; ks < KR; ++ks) xb[ks] = *reinterpret_cast<const uint4*>(xr + 32 * ks);
        };
        load_x(p0);       // the first window this band completes; OLDEST in the queue: the first emit must not wait for the rows
        load_row(ys - 1, nxA); load_row(ys, nxB);
        take_row(ys - 1, nxA); load_row(ys + 1, nxA);
        dws.template push<false>(tap, row, a_lane0, AST);
        take_row(ys, nxB); load_row(ys + 2, nxB);
        dws.template push<false>(tap, row, a_lane0, AST);
        take_row(ys + 1, nxA); load_row(ys + 3, nxA);
        dws.template push<true>(tap, row, a_lane0, AST);                 // row ys -> buffer 0
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

        unsigned VM[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) VM[i] = NEG;
        // (queue shape, see the plain kernel: the compiler's wait for a row is the minimum over the paths into the loop of the
        //  operations behind it -- 17 on the back edge; six dropped stores make the way in from here look the same)
#pragma unroll
        for (int i = 0; i < 6; ++i)              // (distinct offsets: identical stores are merged into one)
            __builtin_amdgcn_raw_buffer_store_b128((u32x4s){0u, 0u, 0u, 0u}, orsrc, (int)(0xfffff000u + 16u * i), 0, 0);
        // one strip row: `buf` = the A buffer of row y (0 / 1, static), nx = the register set that holds input row y + 2
        auto step = [&](int y, int buf, unsigned (&nx)[NWIN], auto parity) {
            const int t = y + pt;
            constexpr bool t_even = decltype(parity)::value;                  // static: see the loop below
            int yo = (t - 1) >> 1;
            yo = yo < 0 ? 0 : (yo > p.Ho - 1 ? p.Ho - 1 : yo);
            const bool do_emit = (t_even ? t >= 2 : y == p.H - 1) && yo >= p0 && y <= ye;
            take_row(y + 2, nx);
            load_row(y + 4 <= ye + 2 ? y + 4 : ye + 2, nx);                 // two steps ahead, into the set just consumed
            __builtin_amdgcn_sched_barrier(0);
            // matrix stage of row y (its A tile was completed by the barrier at the end of the previous step) ...
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            {
                const unsigned char* ar = smem + buf * A_BYTES + px * AST + g * 16;
                uint4 b[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const uint4*>(ar + ks * 64);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[i] = mma16<T>(wq[ks][i], b[ks], acc[i]);
            }
            // ... next to the depthwise stage of row y + 1 (-> the other buffer)
            dws.template push<true>(tap, row, a_lane0 + (buf ^ 1) * A_BYTES, AST);
            unsigned cur[4];
            bn_pair<T>(acc[0], acc[1], sb, COUT, cur);
            if (any_col_out || y < 0) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[i] = (col_out || y < 0) ? NEG : cur[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) VM[i] = pmax2<T>(VM[i], cur[i]);
            u32x4s po = {0u, 0u, 0u, 0u};
            if (do_emit) {
                asm volatile("" ::: "memory");
                f32x4 ar[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int ks = 0; ks < KR; ++ks)
#pragma unroll
                    for (int i = 0; i < 2; ++i) ar[i] = mma16<T>(wrq[ks][i], xb[ks], ar[i]);
                unsigned res[4];
                bn_pair<T>(ar[0], ar[1], sb + 2 * COUT, COUT, res);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned c = VM[i];
                    const unsigned lft = (unsigned)__builtin_amdgcn_mov_dpp((int)c, 0x111, 0xf, 0xf, true);
                    const unsigned rgt = (unsigned)__builtin_amdgcn_mov_dpp((int)c, 0x101, 0xf, 0xf, true);
                    po[i] = padd2<T>(pmax2<T>(pmax2<T>(lft, c), rgt), res[i]);
                }
            }
            {
                const unsigned off = (do_emit && lane_out) ? obase + (unsigned)yo * (unsigned)(p.Wo * COUT * sizeof(T)) : 0xfffff000u;
                __builtin_amdgcn_raw_buffer_store_b128(po, orsrc, (int)off, 0, 0);
            }
            // The shortcut operand of the NEXT regular emit (two steps on: windows complete on every other row), behind this
            // step's use of the registers.  vmcnt retires in order: fetched at the top of the emitting step itself, the wait
            // for it was a wait for the row prefetch issued before it and for the previous step's store as well.  (The cut-off
            // window at the image's bottom completes on row H - 1, t odd, ONE step after a regular one: the clamp below makes
            // that step's fetch the cut-off window's operand.  No fetch inside the emit: the compiler would drain the queue.)
            if constexpr (t_even) {
                load_x((t >> 1) > p.Ho - 1 ? p.Ho - 1 : (t >> 1));           // row t + 2 completes window t / 2
#pragma unroll
                for (int i = 0; i < 4; ++i) VM[i] = cur[i];
            }
            // row y + 1's A tile is complete, and row y's is read, when every wave is here: ONE LDS-only barrier per row
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        // (input row y + 2 of the first step sits in set B, of the second in set A: see the prologue)
        // Steps come in pairs with STATIC roles -- A buffer, register set, and the parity of t = y + pt: a band starts on an even
        // t (ys = 2 p0 - pt; -1 when the image's padded top row is in the band: a ghost step whose row counts as -inf) and ends
        // with a ghost step when its row count is odd (y = ye + 1: clamped loads, no emit).  Both matter to the compiler's
        // wait counts, which are a minimum over every path it can see: with `if (y + 1 <= ye) step(...)` there is a path from
        // the first step straight back to the loop head (vmcnt(5..1) at the top of every pair: no prefetch distance left);
        // with a runtime parity, a path "fetch x at the end of one step, use it in the next" (the emit waits for the rows).
        for (int y = ys; y <= ye; y += 2) {
            step(y, 0, nxB, std::true_type{});
            step(y + 1, 1, nxA, std::false_type{});
        }
    }
}

template <typename T, int C, int WGS>
int launch_coop(CoopParams<T> p, int num_cus, hipStream_t s) {
    constexpr size_t lds = 2 * 16 * (C * 2 + 32) + 4 * C * 4;
    auto kern = block_tail_coop_kernel<T, C, WGS>;
    static BqLdsAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(kern), lds)) return e;
    p.Ho = (p.H + 1) / 2; p.Wo = (p.W + 1) / 2;
    p.nstrips = (p.Wo + 6) / 7;
    const long long base_items = (long long)p.n * p.nstrips;
    p.nbands = pick_bands(base_items, p.Ho, p.Ho, 2, num_cus * WGS);  // whole-height strips: 256 images x 6 strips = 6 per workgroup
    p.items = (int)(base_items * p.nbands);
    int grid = p.items < num_cus * WGS ? p.items : num_cus * WGS;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(C * 2), lds, s, p);
    return (int)hipGetLastError();
}

// bands of ~rows_per_band rows; small batches get shorter bands so that every CU still has work
inline int pick_bands(long long base_items, int rows, int rows_per_band, int min_rows, int waves) {
    int nb = (rows + rows_per_band - 1) / rows_per_band;
    if (base_items * nb < waves) {
        nb = (int)((waves + base_items - 1) / base_items);
        if (nb > rows / min_rows) nb = rows / min_rows;
        if (nb < 1) nb = 1;
    }
    return nb;
}

template <typename T, int CIN, int COUT, bool RELU_IN>
int launch_stream(StreamParams<T> p, int num_cus, hipStream_t s) {
    // 256 output channels: 64 accumulator registers, 64 KB of weights -> 8 waves (2 per SIMD, 256 registers)
    constexpr int NW = COUT > 128 ? 8 : STREAM_NW;
    constexpr size_t lds = (size_t)(CIN / 32) * (COUT / 16) * 1024 + 2 * COUT * 4 + (size_t)NW * 16 * (CIN * 2 + 32);
    static_assert(lds <= 160 * 1024, "stream kernel LDS budget");
    auto kern = sepconv_stream_kernel<T, CIN, COUT, RELU_IN, NW>;
    static BqLdsAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(kern), lds)) return e;
    p.nstrips = (p.W + 15) / 16;
    const long long base_items = (long long)p.n * p.nstrips;
    // bands of ~25 rows (2 halo rows per band); the 74 x 74 map: 8 bands, so that 256 images x 5 strips x 8 bands fill the
    // 2 048 waves five times exactly
    p.nbands = p.H <= 80 ? pick_bands(base_items, p.H, 10, 4, num_cus * NW) : pick_bands(base_items, p.H, 25, 4, num_cus * NW);
    p.items = (int)(base_items * p.nbands);
    int grid = (p.items + NW - 1) / NW;
    if (grid > num_cus) grid = num_cus;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, p);
    return (int)hipGetLastError();
}

template <typename T, int CX>
int launch_tail(TailParams<T> p, int num_cus, hipStream_t s) {
    constexpr int NW = TAIL_NW;
    constexpr size_t lds = (size_t)4 * 8 * 1024 + (size_t)(CX / 32) * 8 * 1024 + 4 * 128 * 4 + (size_t)NW * 16 * (128 * 2 + 32);
    static_assert(lds <= 160 * 1024, "tail kernel LDS budget");
    auto kern = block_tail_stream_kernel<T, CX, NW>;
    static BqLdsAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(kern), lds)) return e;
    p.Ho = (p.H + 1) / 2; p.Wo = (p.W + 1) / 2;
    p.nstrips = (p.Wo + 6) / 7;
    const long long base_items = (long long)p.n * p.nstrips;
    p.nbands = pick_bands(base_items, p.Ho, 18, 2, num_cus * NW);    // ~18 pooled rows = ~37 convolution rows (one shared)
    p.items = (int)(base_items * p.nbands);
    int grid = (p.items + NW - 1) / NW;
    if (grid > num_cus) grid = num_cus;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, p);
    return (int)hipGetLastError();
}

template <typename T>
int launch_stream_t(int cin, int cout, bool relu_in, const void* in, const void* wp16, const float* dw, const float* scale,
                    const float* bias, void* out, int n, int H, int W, int relu, int num_cus, hipStream_t s) {
    StreamParams<T> p;
    p.in = reinterpret_cast<const T*>(in);
    p.wp16 = reinterpret_cast<const uint4*>(wp16);
    p.dw = dw; p.scale = scale; p.bias = bias;
    p.out = reinterpret_cast<T*>(out);
    p.n = n; p.H = H; p.W = W; p.relu = relu;
    p.nstrips = p.nbands = p.items = 0;
    if (cin == 64 && cout == 128 && !relu_in) return launch_stream<T, 64, 128, false>(p, num_cus, s);
    if (cin == 128 && cout == 128 && !relu_in) return launch_stream<T, 128, 128, false>(p, num_cus, s);
    if (cin == 128 && cout == 256 && relu_in) return launch_stream<T, 128, 256, true>(p, num_cus, s);
    return (int)hipErrorInvalidValue;
}

}  // namespace

bool stream_supported(int dtype, int cin, int cout, bool relu_in, long long n, int H, int W) {
    const bool b2 = !relu_in && cout == 128 && (cin == 64 || cin == 128);     // block 2 (147 x 147)
    const bool b3 = relu_in && cout == 256 && cin == 128;                       // block3_sepconv1 (74 x 74)
    return dtype != 0 && (b2 || b3) && H >= 4 && W >= 1 &&
           n * H * W * (long long)cout * 2 <= 0xfffff000ll;
}

bool tail_supported(int dtype, int cin, int cout, int cx, long long n, int H, int W) {
    const bool b2 = cin == 128 && cout == 128 && cx == 64;          // block 2: wave-private strips
    const bool b3 = cin == 256 && cout == 256 && cx == 128;         // block 3: eight waves per strip, weights in registers
    return dtype != 0 && (b2 || b3) && H >= 8 && W >= 8 &&
           n * H * W * (long long)cin * 2 <= 0xfffff000ll;
}

// out = maxpool3x3/s2(BN(sepconv2(y1))) + BN(conv1x1/s2(x)); wp16 / wr16: "<sepconv2>/wp16", "<res>/wp16"
int launch_block_tail(int dtype, int cin, int cout, int cx, const void* y1, const void* wp16, const float* dw,
                      const float* scale, const float* bias, const void* x, const void* wr16, const float* rscale,
                      const float* rbias, void* out, int n, int H, int W, int num_cus, hipStream_t s) {
    if (!tail_supported(dtype, cin, cout, cx, n, H, W)) return (int)hipErrorInvalidValue;
    if (cin == 256) {
        auto go3 = [&](auto tag) {
            typedef decltype(tag) T;
            CoopParams<T> p;
            p.in = reinterpret_cast<const T*>(y1); p.wp16 = reinterpret_cast<const uint4*>(wp16); p.dw = dw;
            p.scale = scale; p.bias = bias;
            p.x = reinterpret_cast<const T*>(x); p.wr16 = reinterpret_cast<const uint4*>(wr16); p.rscale = rscale; p.rbias = rbias;
            p.out = reinterpret_cast<T*>(out);
            p.n = n; p.H = H; p.W = W; p.Ho = p.Wo = p.nstrips = p.nbands = p.items = 0;
            return launch_coop<T, 256, 1>(p, num_cus, s);
        };
        return dtype == 2 ? go3(f16_t{}) : go3(bf16_t{});
    }
    auto go = [&](auto tag) {
        typedef decltype(tag) T;
        TailParams<T> p;
        p.in = reinterpret_cast<const T*>(y1); p.wp16 = reinterpret_cast<const uint4*>(wp16); p.dw = dw;
        p.scale = scale; p.bias = bias;
        p.x = reinterpret_cast<const T*>(x); p.wr16 = reinterpret_cast<const uint4*>(wr16); p.rscale = rscale; p.rbias = rbias;
        p.out = reinterpret_cast<T*>(out);
        p.n = n; p.H = H; p.W = W; p.Ho = p.Wo = p.nstrips = p.nbands = p.items = 0;
        return launch_tail<T, 64>(p, num_cus, s);
    };
    return dtype == 2 ? go(f16_t{}) : go(bf16_t{});
}

int launch_sepconv_stream(int dtype, int cin, int cout, bool relu_in, const void* in, const void* wp16, const float* dw,
                          const float* scale, const float* bias, void* out, int n, int H, int W, int relu, int num_cus,
                          hipStream_t s) {
    return dtype == 2 ? launch_stream_t<f16_t>(cin, cout, relu_in, in, wp16, dw, scale, bias, out, n, H, W, relu, num_cus, s)
                      : launch_stream_t<bf16_t>(cin, cout, relu_in, in, wp16, dw, scale, bias, out, n, H, W, relu, num_cus, s);
}
