// Exact k nearest neighbours of the rows of X fp32 [n][D] (DESIGN.md "Feature map (Figure 6)"): idx int32 [n][k] and dist fp32
// [n][k], each row sorted by (distance, index) ascending, the row itself a candidate like any other.  The n x n matrix is never
// stored: three kernels, all of them without atomics, so the bits do not depend on the launch.
//
// knn_norms_kernel: |x|^2 of every row, one 16-lane group per row in the order of umap_device.h's direct form.
//
// knn_candidates_kernel: the pruning pass in the GEMM form |q|^2 + |c|^2 - 2 q.c on the exact fp32 matrix instruction
// (v_mfma_f32_32x32x2f32).  One wave per 32 query rows walks all candidate rows in tiles of 32: the tile's 32 x 32 products
// accumulate over D in a fixed order (8 columns per step: lanes 0-31 bring columns 8t .. 8t+3, lanes 32-63 columns 8t+4 .. 8t+7,
// four instructions), so a pair's value is the same whatever tile it falls in.  The query is the instruction's N side: lane l
// ends up with query l % 32 and the 16 candidates 8 (v / 4) + 4 (l / 32) + v % 4 of the tile.  Each LANE keeps a list of the
// KP = k + K_SLACK smallest (value, index) pairs it has seen, unsorted in LDS ([slot][lane]: no bank conflicts) with the largest
// one's slot in registers; a candidate that is not smaller costs one compare.  A query's candidates are the union of its two
// lanes' lists -- a fixed function of the data: lane half h sees the candidates c with (c / 4) % 2 == h.  The GEMM form loses
// every digit between near-duplicate rows, so it decides nothing but who is looked at again.
//
// knn_rerank_kernel: one workgroup per query.  The direct form sum (x - y)^2 of every candidate (bqumap: a 16-lane group per pair,
// a float4 per lane and step), then a rank sort of the at most 2 KP pairs in LDS by (distance, index); ranks below k are the row.
#include "bq_ctx.h"
#include "umap_device.h"

#include <limits.h>

namespace {

using bqumap::K_MAX;
using bqumap::K_SLACK;
constexpr int KP_MAX = K_MAX + K_SLACK;
constexpr int KN_WAVE = 64;
constexpr int RR_NT = 256, RR_GROUPS = RR_NT / 16;

// the partial sums of the direct form held by a 16-lane group, folded: every lane of the group returns the sum
__device__ __forceinline__ float group_fold(float a0, float a1, float a2, float a3) {
    float g = bqumap::sq_fold4(a0, a1, a2, a3);
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) g = g + __shfl_xor(g, s, 16);
    return g;
}

// sum (x - y)^2 over D by the 16-lane group of `lane16` (y null: sum x^2)
__device__ __forceinline__ float group_sqdist(const float* __restrict__ x, const float* __restrict__ y, int D, int lane16) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int e = 4 * lane16; e < D; e += bqumap::SQ_LANES) {
        const float4 xv = *reinterpret_cast<const float4*>(x + e);
        const float4 yv = y ? *reinterpret_cast<const float4*>(y + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        a0 = bqumap::sq_term(a0, xv.x, yv.x);
        a1 = bqumap::sq_term(a1, xv.y, yv.y);
        a2 = bqumap::sq_term(a2, xv.z, yv.z);
        a3 = bqumap::sq_term(a3, xv.w, yv.w);
    }
    return group_fold(a0, a1, a2, a3);
}

__global__ void __launch_bounds__(RR_NT) knn_norms_kernel(const float* __restrict__ X, int n, int D, float* __restrict__ norms) {
    const long long row = (long long)blockIdx.x * RR_GROUPS + threadIdx.x / 16;
    const int lane16 = threadIdx.x & 15;
    const long long r = row < n ? row : n - 1;      // (whole groups stay in step for the shuffles)
    const float v = group_sqdist(X + (size_t)r * D, nullptr, D, lane16);
    if (row < n && lane16 == 0) norms[row] = v;
}

__global__ void __launch_bounds__(KN_WAVE) knn_candidates_kernel(const float* __restrict__ X, const float* __restrict__ norms, int n, int D,
                                                                 int kp, int* __restrict__ cand) {
    __shared__ float s_val[KP_MAX][KN_WAVE];
    __shared__ int s_idx[KP_MAX][KN_WAVE];
    const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
    const int q = blockIdx.x * 32 + col;
    const int qr = q < n ? q : n - 1;
    for (int s = 0; s < kp; ++s) {
        s_val[s][lane] = INFINITY;
        s_idx[s][lane] = INT_MAX;
    }
    float worst_v = INFINITY;
    int worst_i = INT_MAX, worst_s = 0;
    const float nq = norms[qr];
    const float* qrow = X + (size_t)qr * D + 4 * half;
    for (int c0 = 0; c0 < n; c0 += 32) {
        const int cr = c0 + col < n ? c0 + col : n - 1;
        const float* crow = X + (size_t)cr * D + 4 * half;
        f32x16 acc = {0};
        for (int e = 0; e < D; e += 8) {
            const float4 cv = *reinterpret_cast<const float4*>(crow + e);
            const float4 qv = *reinterpret_cast<const float4*>(qrow + e);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.x, qv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.y, qv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.z, qv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.w, qv.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int c = c0 + 8 * (v / 4) + 4 * half + (v % 4);
            if (c >= n) continue;
            const float val = (nq + norms[c]) - 2.f * acc[v];
            if (!bqumap::before(val, c, worst_v, worst_i)) continue;
            s_val[worst_s][lane] = val;
            s_idx[worst_s][lane] = c;
            worst_v = s_val[0][lane];
            worst_i = s_idx[0][lane];
            worst_s = 0;
            for (int s = 1; s < kp; ++s) {
                const float sv = s_val[s][lane];
                const int si = s_idx[s][lane];
                if (bqumap::before(worst_v, worst_i, sv, si)) {
                    worst_v = sv;
                    worst_i = si;
                    worst_s = s;
                }
            }
        }
    }
    if (q < n) {
        int* out = cand + ((size_t)q * 2 + half) * kp;
        for (int s = 0; s < kp; ++s) {
            const int si = s_idx[s][lane];
            out[s] = si == INT_MAX ? -1 : si;
        }
    }
}

__global__ void __launch_bounds__(RR_NT) knn_rerank_kernel(const float* __restrict__ X, int n, int D, int k, int kp, const int* __restrict__ cand,
                                                           int* __restrict__ idx, float* __restrict__ dist) {
    __shared__ float s_d[2 * KP_MAX];
    __shared__ int s_i[2 * KP_MAX];
    const int tid = threadIdx.x, group = tid / 16, lane16 = tid & 15;
    const int m = 2 * kp;
    for (long long q = blockIdx.x; q < n; q += gridDim.x) {      // (uniform: the barriers below are safe)
        const float* x = X + (size_t)q * D;
        const int* mine = cand + (size_t)q * m;
        for (int c0 = 0; c0 < m; c0 += RR_GROUPS) {      // (uniform too: every group takes every step, the shuffles stay whole)
            const int c = c0 + group;
            const int j = c < m ? mine[c] : -1;
            const bool real = j >= 0 && j < n;
            const float d2 = group_sqdist(x, X + (size_t)(real ? j : 0) * D, D, lane16);
            if (c < m && lane16 == 0) {
                // the order is the DISTANCE's (two sums may share a root); through double the root is the correctly rounded one
                s_d[c] = real ? (float)sqrt((double)d2) : INFINITY;
                s_i[c] = real ? j : INT_MAX;
            }
        }
        __syncthreads();
        if (tid < m && s_i[tid] != INT_MAX) {
            const float d = s_d[tid];
            const int j = s_i[tid];
            int rank = 0;
            for (int u = 0; u < m; ++u) rank += bqumap::before(s_d[u], s_i[u], d, j) ? 1 : 0;
            if (rank < k) {
                idx[(size_t)q * k + rank] = j;
                dist[(size_t)q * k + rank] = d;
            }
        }
        __syncthreads();      // the lists are read: the next query's may land
    }
}

}  // namespace

static size_t knn_norm_bytes(long long n) { return ((size_t)n * sizeof(float) + 255) / 256 * 256; }

extern "C" {

size_t bq_knn_workspace_bytes(int64_t n, int D, int k) {
    if (bqumap::check_knn(n, D, k)) return 0;
    return knn_norm_bytes(n) + (size_t)n * 2 * (k + K_SLACK) * sizeof(int);
}

int bq_knn(bq_ctx* c, const float* d_x, int64_t n, int D, int k, int32_t* d_idx, float* d_dist, void* d_ws, size_t ws_bytes,
           bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_knn: null context");
    if (const char* why = bqumap::check_knn(n, D, k)) return fail(c, BQ_ERR_ARG, std::string("bq_knn: ") + why);
    if (!d_x || !d_idx || !d_dist || !d_ws || ((uintptr_t)d_x & 15) || ((uintptr_t)d_ws & 15))
        return fail(c, BQ_ERR_ARG, "bq_knn: bad argument (null pointer, X or the workspace not 16-byte aligned)");
    if (ws_bytes < bq_knn_workspace_bytes(n, D, k)) return fail(c, BQ_ERR_WORKSPACE, "bq_knn: workspace below bq_knn_workspace_bytes(n, D, k)");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(c->device);
    ProfScope ps(c, s, "knn", 2.0 * (double)n * (double)n * D, (double)n * D * sizeof(float));
    const int kp = k + K_SLACK, N = (int)n;
    float* norms = reinterpret_cast<float*>(d_ws);
    int* cand = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(d_ws) + knn_norm_bytes(n));
    hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((n + RR_GROUPS - 1) / RR_GROUPS)), dim3(RR_NT), 0, s, d_x, N, D, norms);
    hipLaunchKernelGGL(knn_candidates_kernel, dim3((unsigned)((n + 31) / 32)), dim3(KN_WAVE), 0, s, d_x, norms, N, D, kp, cand);
    hipLaunchKernelGGL(knn_rerank_kernel, dim3((unsigned)(n < 65535 * 16 ? n : 65535 * 16)), dim3(RR_NT), 0, s, d_x, N, D, k, kp, cand, d_idx,
                       d_dist);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
