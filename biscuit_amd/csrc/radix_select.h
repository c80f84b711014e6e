// radix_select.h -- exact order statistics over the float32 values of one tile's pixels, for the percentiles of the stain
// normalisers (kernels_stain.hip: Macenko's extreme angles and concentrations; kernels_reinhard.hip: the 90th percentile of L).
// One workgroup of RS_NT threads; the state lives in the caller's LDS (RadixSel).  A radix select over the order-preserving
// 32-bit key of the value: one pass over a monotone 2 048-bin coarse histogram of the value, then 11 + 11 + 10 key bits
// restricted to the chosen coarse bin (so LDS atomics only collide inside it), then one pass for the successor when it is a
// different value.  Counts are integers: the result does not depend on the order of the atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int RS_NT = 1024;
constexpr int RS_NW = RS_NT / 64;
constexpr int RS_BINS = 2048;

struct RadixSel {
    unsigned hist[2][RS_BINS];
    unsigned wsum[RS_NW];
    unsigned rank[2], bin[2], before[2], cbin[2], key[2], eq[2], succ[2];
    float coff, cscl;                      // coarse bin of a value v: clamp((v + coff) * cscl, 0, RS_BINS - 1)
};

__device__ __forceinline__ unsigned rs_key(float v) {       // order-preserving: a < b  <=>  key(a) < key(b) (-0 < +0)
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rs_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int rs_coarse(const RadixSel& sh, float v) {     // monotone non-decreasing in v; NaN -> 0
    const float x = (v + sh.coff) * sh.cscl;
    return x >= 0.f ? (x < (float)(RS_BINS - 1) ? (int)x : RS_BINS - 1) : 0;
}

// numpy's _lerp: a + (b - a) t, or b - (b - a)(1 - t) when t >= 0.5
__device__ __forceinline__ double rs_lerp(double a, double b, double t) {
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// For both targets t (threads [512 t, 512 t + 512)): the bin of hist[t][0..nb) holding the element of rank sh.rank[t]
// -> sh.bin[t], and the count of the bins below it -> sh.before[t].  nb = 1 024 or 2 048.  A target whose histogram does not
// reach its rank (an empty one) leaves bin and before as they are.
__device__ void rs_find(RadixSel& sh, int nb) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int t = tid >> 9, j = tid & 511, per = nb >> 9;
    unsigned loc = 0;
    for (int q = 0; q < per; ++q) loc += sh.hist[t][j * per + q];
    unsigned x = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh.wsum[wid] = x;
    __syncthreads();
    unsigned acc = x - loc;
    for (int w = t * (RS_NW / 2); w < wid; ++w) acc += sh.wsum[w];
    const unsigned r = sh.rank[t];
    if (r >= acc && r < acc + loc) {
        for (int q = 0; q < per; ++q) {
            const unsigned c = sh.hist[t][j * per + q];
            if (r < acc + c) { sh.bin[t] = j * per + q; sh.before[t] = acc; break; }
            acc += c;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void rs_clear(RadixSel& sh) {
    for (int i = threadIdx.x; i < 2 * RS_BINS; i += RS_NT) (&sh.hist[0][0])[i] = 0u;
}

// Exact order statistics: for t = 0, 1 the element of rank sh.rank[t] among the values v[t] of the pixels with ok[t]
// (VAL(i, v, ok) evaluates pixel i), as its key -> sh.key[t], and the key of the element of rank + 1 -> sh.succ[t].
template <class VAL>
__device__ void rs_select(RadixSel& sh, int npix, const VAL& val) {
    const int tid = threadIdx.x;
    rs_clear(sh);
    __syncthreads();
    for (int i = tid; i < npix; i += RS_NT) {
        float v[2]; bool ok[2];
        val(i, v, ok);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (ok[t]) atomicAdd(&sh.hist[t][rs_coarse(sh, v[t])], 1u);
    }
    __syncthreads();
    rs_find(sh, RS_BINS);
    if (tid < 2) { sh.cbin[tid] = sh.bin[tid]; sh.rank[tid] -= sh.before[tid]; sh.key[tid] = 0u; }
    // three radix passes over the key bits [31:21], [20:10], [9:0] of the elements in the chosen coarse bin
    for (int lv = 0; lv < 3; ++lv) {
        const int nb = lv < 2 ? 2048 : 1024, shift = lv == 0 ? 21 : lv == 1 ? 10 : 0;
        const unsigned above = lv == 0 ? 0u : lv == 1 ? 0xffe00000u : 0xfffffc00u;     // key bits already chosen
        __syncthreads();
        rs_clear(sh);
        __syncthreads();
        const unsigned cb0 = sh.cbin[0], cb1 = sh.cbin[1], pk0 = sh.key[0] & above, pk1 = sh.key[1] & above;
        for (int i = tid; i < npix; i += RS_NT) {
            float v[2]; bool ok[2];
            val(i, v, ok);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned k = rs_key(v[t]);
                if (ok[t] && (unsigned)rs_coarse(sh, v[t]) == (t ? cb1 : cb0) && (k & above) == (t ? pk1 : pk0))
                    atomicAdd(&sh.hist[t][(k >> shift) & (unsigned)(nb - 1)], 1u);
            }
        }
        __syncthreads();
        rs_find(sh, nb);
        if (tid < 2) {
            sh.key[tid] |= sh.bin[tid] << shift;
            sh.rank[tid] -= sh.before[tid];
            if (lv == 2) sh.eq[tid] = sh.hist[tid][sh.bin[tid]];
        }
    }
    __syncthreads();
    // the successor: the same value while elements of that key remain, else the least larger key (min: order-free)
    const bool need0 = sh.rank[0] + 1 >= sh.eq[0], need1 = sh.rank[1] + 1 >= sh.eq[1];
    const unsigned k0 = sh.key[0], k1 = sh.key[1];
    __syncthreads();
    if (tid < 2) sh.succ[tid] = (tid ? need1 : need0) ? 0xffffffffu : sh.key[tid];
    __syncthreads();
    if (need0 || need1) {
        unsigned m0 = 0xffffffffu, m1 = 0xffffffffu;
        for (int i = tid; i < npix; i += RS_NT) {
            float v[2]; bool ok[2];
            val(i, v, ok);
            const unsigned a = rs_key(v[0]), b = rs_key(v[1]);
            if (need0 && ok[0] && a > k0) m0 = min(m0, a);
            if (need1 && ok[1] && b > k1) m1 = min(m1, b);
        }
        if (need0) atomicMin(&sh.succ[0], m0);
        if (need1) atomicMin(&sh.succ[1], m1);
        __syncthreads();
    }
}

}  // namespace
