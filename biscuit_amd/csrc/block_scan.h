// block_scan.h -- the workgroup scan of the two tile encoders (kernels_jpeg_encode.hip, kernels_png_encode.hip), and what both
// do with it last: the files' lengths -> their offsets in the packed output.
#pragma once
#include <hip/hip_runtime.h>

// Inclusive scan of one value per thread over a workgroup of NT threads; `sh` holds NT values.  All threads call it.
template <int NT, typename V>
__device__ V block_scan(V v, V* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const V a = t >= d ? sh[t - d] : (V)0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const V r = sh[t];
    return r;
}

// file lengths flen(0 .. n - 1) of a round -> off[t0 + 1 .. t0 + n], continuing from off[t0]; one workgroup of NT threads
template <int NT, typename F>
__device__ void offsets_scan(long long* off, long long t0, int n, F flen, long long* sh) {
    long long carry = t0 ? off[t0] : 0;
    if (t0 == 0 && threadIdx.x == 0) off[0] = 0;
    for (int base = 0; base < n; base += NT) {
        const int i = base + (int)threadIdx.x;
        const long long v = i < n ? flen(i) : 0;
        const long long incl = block_scan<NT>(v, sh);
        if (i < n) off[t0 + i + 1] = carry + incl;
        carry += sh[NT - 1];
        __syncthreads();
    }
}
