// Sums over the rows of a table in a fixed order, shared by kernels_calib.hip and kernels_delong.hip: the rows are cut into chunks
// of chunk_rows(n) (a function of n alone); a workgroup of NT threads takes one chunk, keeps its sums in registers, adds them across
// the wave with a shuffle butterfly and across the waves through LDS in wave order, and writes a partial per chunk; a finish kernel
// adds the partials in chunk order.  No atomics and no order that depends on timing: the same bits every call.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int NT = 256;              // threads of every workgroup here
constexpr int NW = NT / 64;          // its waves
constexpr long long CHUNK_MIN = 2048;   // rows of a chunk up to MAX_CHUNKS chunks; beyond that the chunk grows, not their number
constexpr long long MAX_CHUNKS = 2048;

__host__ __device__ inline long long chunk_rows(long long n) {
    long long per = (n + MAX_CHUNKS - 1) / MAX_CHUNKS;
    per = (per + NT - 1) / NT * NT;
    return per < CHUNK_MIN ? CHUNK_MIN : per;
}
__host__ __device__ inline long long num_chunks(long long n) { return (n + chunk_rows(n) - 1) / chunk_rows(n); }

// butterfly: every lane ends with the sum of the wave's 64 values, added in the same order in every run
__device__ inline double wave_sum(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// v[K] of every thread -> lds[K]: the workgroup's sums, waves added in wave order.  lds: (NW + 1) * K doubles.  Ends on a barrier.
template <int K>
__device__ inline double* block_sum(double (&v)[K], double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) lds[wave * K + k] = s;
    }
    __syncthreads();
    double* out = lds + NW * K;
    for (int k = threadIdx.x; k < K; k += NT) {
        double s = lds[k];
        for (int w = 1; w < NW; ++w) s += lds[w * K + k];
        out[k] = s;
    }
    __syncthreads();
    return out;
}

}  // namespace
