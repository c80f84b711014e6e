// Exact k nearest neighbours of the rows of X fp32 [n][D] (DESIGN.md "Feature map (Figure 6)"): idx int32 [n][k] and dist fp32
// [n][k], each row sorted by (distance, index) ascending, the row itself a candidate like any other -- bqio_knn's table (all n rows
// by the direct form) on every row, bit for bit, by construction: a pruned row is kept only where a certificate proves it.  The
// n x n matrix is never stored: four kernels, all of them without atomics, so the bits do not depend on the launch.
//
// knn_norms_kernel: |x|^2 of every row, one 16-lane group per row in the order of umap_device.h's direct form.
//
// knn_candidates_kernel: the pruning pass in the GEMM form |q|^2 + |c|^2 - 2 q.c on the exact fp32 matrix instruction
// (v_mfma_f32_32x32x2f32).  One wave per 32 query rows walks all candidate rows in tiles of 32: the tile's 32 x 32 products
// accumulate over D in a fixed order (8 columns per step: lanes 0-31 bring columns 8t .. 8t+3, lanes 32-63 columns 8t+4 .. 8t+7,
// four instructions), so a pair's value is the same whatever tile it falls in.  The query is the instruction's N side: lane l
// ends up with query l % 32 and the 16 candidates 8 (v / 4) + 4 (l / 32) + v % 4 of the tile.  Each LANE keeps a list of the
// KP = k + K_SLACK smallest (value, index) pairs it has seen, unsorted in LDS ([slot][lane]: no bank conflicts) with the largest
// one's slot in registers; a candidate that is not smaller costs one compare and the floor below.  A query's candidates are the
// union of its two lanes' lists -- a fixed function of the data: lane half h sees the candidates c with (c / 4) % 2 == h.  The GEMM
// form loses every digit between near-duplicate rows, so it decides nothing but who is looked at again -- and among more than KP
// rows that lie closer together than its rounding error it decides that by noise.  Hence the certificate: every value is off from
// the exact squared distance by at most E(|q|^2, |c|^2, D) (umap_device.h: gemm_form_err, any summation order), and the lane keeps
// its FLOOR, the minimum of value - E over everything it rejected or evicted (for an evicted row E at the largest norm the list
// has held, which is in a register): no row it dropped is nearer than that.  +inf while
// it dropped nothing; -inf once it saw a value that is not finite (an overflow, a NaN: no bound holds).
//
// knn_rerank_kernel: one workgroup per query.  The direct form sum (x - y)^2 of every candidate (bqumap: a 16-lane group per pair,
// a float4 per lane and step), then a rank sort of the at most 2 KP pairs in LDS by (distance, index); ranks below k are the row.
// The row is CERTIFIED where the direct-form d^2 of its k-th neighbour lies strictly below both halves' floors by a margin that
// covers the direct form's own error and the rounded root (bqumap::knn_certified; ties and NaNs are not certified) and every
// candidate's distance is finite; flags[q] = 0 then, else 1.
//
// knn_exhaustive_kernel: the flagged rows again over all n rows by the same direct form, the same root and the same order, so the
// bits are bqio_knn's; the other rows' workgroups return at once.  No host synchronisation between the passes.  It writes every
// place of its rows: idx -1 and dist NaN where a row has fewer than k rows at a finite distance (X not finite: the precondition
// of bq_knn broken).  The flags stay in the workspace's first 4 n bytes for the caller (Engine.knn_exhaustive_rows).
//
// Measured on the MI355X before the certificate (tests/test_gpu_knn.py's tight groups): the pruning alone differed from bqio_knn
// on every row of groups of 96 and 200 near-identical rows, with neighbours at up to 6.8 x the true k-th squared distance.
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
                                                                 int kp, int* __restrict__ cand, float* __restrict__ floors) {
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
    // the certificate: the smallest value - E of everything this lane did not keep (+inf while it kept everything)
    float floor_ = INFINITY, kept_nc = 0.f;
    const float coeff = bqumap::gemm_err_coeff(D);
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
            const float nc = norms[c];
            const float val = (nq + nc) - 2.f * acc[v];
            if (!(fabsf(val) < INFINITY)) floor_ = -INFINITY;      // an overflow or a NaN: the bound does not hold, nothing is certified
            if (!bqumap::before(val, c, worst_v, worst_i)) {
                floor_ = fminf(floor_, val - bqumap::gemm_err_with(nq, nc, coeff));
                continue;
            }
            // the evicted one: E grows with the norm, and no kept row's norm is above kept_nc (no load on this path)
            kept_nc = fmaxf(kept_nc, nc);
            if (worst_i != INT_MAX) floor_ = fminf(floor_, worst_v - bqumap::gemm_err_with(nq, kept_nc, coeff));
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
        floors[(size_t)q * 2 + half] = floor_;
    }
}

// Ranks the candidates; flags[q] = 0 where the table row is proven to be the one over all n rows (bqumap::knn_certified against
// both halves' floors, at least k candidates, every distance finite), else 1: knn_exhaustive_kernel writes that row again.
__global__ void __launch_bounds__(RR_NT) knn_rerank_kernel(const float* __restrict__ X, int n, int D, int k, int kp, const int* __restrict__ cand,
                                                           const float* __restrict__ floors, int* __restrict__ flags, int* __restrict__ idx,
                                                           float* __restrict__ dist) {
    __shared__ float s_d[2 * KP_MAX], s_d2[2 * KP_MAX];
    __shared__ int s_i[2 * KP_MAX];
    __shared__ float s_kth;
    __shared__ int s_bad;
    const int tid = threadIdx.x, group = tid / 16, lane16 = tid & 15;
    const int m = 2 * kp;
    for (long long q = blockIdx.x; q < n; q += gridDim.x) {      // (uniform: the barriers below are safe)
        const float* x = X + (size_t)q * D;
        const int* mine = cand + (size_t)q * m;
        if (tid == 0) {
            s_kth = -1.f;      // (no k-th candidate yet)
            s_bad = 0;
        }
        __syncthreads();
        for (int c0 = 0; c0 < m; c0 += RR_GROUPS) {      // (uniform too: every group takes every step, the shuffles stay whole)
            const int c = c0 + group;
            const int j = c < m ? mine[c] : -1;
            const bool real = j >= 0 && j < n;
            const float d2 = group_sqdist(x, X + (size_t)(real ? j : 0) * D, D, lane16);
            if (c < m && lane16 == 0) {
                // the order is the DISTANCE's (two sums may share a root); through double the root is the correctly rounded one
                s_d[c] = real ? (float)sqrt((double)d2) : INFINITY;
                s_d2[c] = d2;
                s_i[c] = real ? j : INT_MAX;
                if (real && !(d2 < INFINITY)) s_bad = 1;
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
            if (rank == k - 1) s_kth = s_d2[tid];
        }
        __syncthreads();
        if (tid == 0) {
            const float kth = s_kth;
            const bool ok = !s_bad && kth >= 0.f && bqumap::knn_certified(kth, floors[(size_t)q * 2], D) &&
                            bqumap::knn_certified(kth, floors[(size_t)q * 2 + 1], D);
            flags[q] = ok ? 0 : 1;
        }
        __syncthreads();      // the lists are read: the next query's may land
    }
}

// The rows the certificate does not cover, over ALL n rows by the direct form: what bqio_knn does.  One workgroup per flagged query;
// 16-lane group g takes the rows j = g (mod 16) and keeps its k best sorted in LDS, then the 16 lists are merged by a rank sort.
// Rows whose distance is not finite are no candidates; places without one get idx -1 and dist NaN.  Every place of the row is written.
__global__ void __launch_bounds__(RR_NT) knn_exhaustive_kernel(const float* __restrict__ X, int n, int D, int k, const int* __restrict__ flags,
                                                               int* __restrict__ idx, float* __restrict__ dist) {
    __shared__ float s_d[RR_GROUPS][K_MAX];
    __shared__ int s_i[RR_GROUPS][K_MAX];
    __shared__ int s_have[RR_GROUPS];
    const int tid = threadIdx.x, group = tid / 16, lane16 = tid & 15;
    for (long long q = blockIdx.x; q < n; q += gridDim.x) {      // (uniform, and so is the flag)
        if (!flags[q]) continue;
        const float* x = X + (size_t)q * D;
        int have = 0;
        for (int j0 = 0; j0 < n; j0 += RR_GROUPS) {      // (every group takes every step)
            const int j = j0 + group;
            const bool real = j < n;
            const float d2 = group_sqdist(x, X + (size_t)(real ? j : 0) * D, D, lane16);
            const float d = (float)sqrt((double)d2);
            if (real && lane16 == 0 && d < INFINITY && (have < k || bqumap::before(d, j, s_d[group][k - 1], s_i[group][k - 1]))) {
                int at = have < k ? have++ : k - 1;      // (bqio_knn's insertion)
                while (at > 0 && bqumap::before(d, j, s_d[group][at - 1], s_i[group][at - 1])) {
                    s_d[group][at] = s_d[group][at - 1];
                    s_i[group][at] = s_i[group][at - 1];
                    --at;
                }
                s_d[group][at] = d;
                s_i[group][at] = j;
            }
        }
        if (lane16 == 0) {
            s_have[group] = have;
            for (int s = have; s < k; ++s) {
                s_d[group][s] = INFINITY;
                s_i[group][s] = INT_MAX;
            }
        }
        __syncthreads();
        int total = 0;
        for (int g = 0; g < RR_GROUPS; ++g) total += s_have[g];
        for (int e = tid; e < RR_GROUPS * k; e += RR_NT) {
            const float d = s_d[e / k][e % k];
            const int j = s_i[e / k][e % k];
            if (j == INT_MAX) continue;
            int rank = 0;
            for (int g = 0; g < RR_GROUPS; ++g)
                for (int s = 0; s < k; ++s) rank += bqumap::before(s_d[g][s], s_i[g][s], d, j) ? 1 : 0;
            if (rank < k) {
                idx[(size_t)q * k + rank] = j;
                dist[(size_t)q * k + rank] = d;
            }
        }
        for (int r = total + tid; r < k; r += RR_NT) {
            idx[(size_t)q * k + r] = -1;
            dist[(size_t)q * k + r] = NAN;
        }
        __syncthreads();      // the lists are read: the next query's may land
    }
}

}  // namespace

// the workspace: flags int32 [n] | norms fp32 [n] (each padded to 256 bytes) | candidates int32 [n][2][k + 16] | floors fp32 [n][2]
static size_t knn_pad256(long long n) { return ((size_t)n * 4 + 255) / 256 * 256; }

extern "C" {

size_t bq_knn_workspace_bytes(int64_t n, int D, int k) {
    if (bqumap::check_knn(n, D, k)) return 0;
    return 2 * knn_pad256(n) + (size_t)n * 2 * (k + K_SLACK) * sizeof(int) + (size_t)n * 2 * sizeof(float);
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
    unsigned char* ws = reinterpret_cast<unsigned char*>(d_ws);
    int* flags = reinterpret_cast<int*>(ws);
    float* norms = reinterpret_cast<float*>(ws + knn_pad256(n));
    int* cand = reinterpret_cast<int*>(ws + 2 * knn_pad256(n));
    float* floors = reinterpret_cast<float*>(cand + (size_t)n * 2 * kp);
    const dim3 per_query((unsigned)(n < 65535 * 16 ? n : 65535 * 16));
    hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((n + RR_GROUPS - 1) / RR_GROUPS)), dim3(RR_NT), 0, s, d_x, N, D, norms);
    hipLaunchKernelGGL(knn_candidates_kernel, dim3((unsigned)((n + 31) / 32)), dim3(KN_WAVE), 0, s, d_x, norms, N, D, kp, cand, floors);
    hipLaunchKernelGGL(knn_rerank_kernel, per_query, dim3(RR_NT), 0, s, d_x, N, D, k, kp, cand, floors, flags, d_idx, d_dist);
    hipLaunchKernelGGL(knn_exhaustive_kernel, per_query, dim3(RR_NT), 0, s, d_x, N, D, k, flags, d_idx, d_dist);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
