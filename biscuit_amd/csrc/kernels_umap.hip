// The fuzzy graph's rows and the layout's epochs (DESIGN.md "Feature map (Figure 6)"); the arithmetic of a row and of a vertex is
// umap_device.h's, the one the CPU build (bqio_umap_smooth, bqio_umap_epoch) compiles.
//
// umap_mean_kernel: the mean of all n k distances -- the floor of the rows whose rho is 0 -- by ONE workgroup: thread t sums the
// rows t, t + 256, ... in double, then a tree in LDS.  A fixed order, so the same bits every run.
// umap_smooth_kernel: one thread per row (k <= 64 values, 64 bisection steps).
// umap_epoch_kernel: gather form, one launch per epoch, one thread per vertex: it reads the previous epoch's positions, walks
// its own row of the symmetric CSR in order and writes its own position and its own row's sample clocks.  Nothing is shared
// between threads, there is no atomic and no barrier: the bits do not depend on the block size (bq_umap_epoch's `block`).
#include "bq_ctx.h"
#include "umap_device.h"

namespace {

constexpr int UM_NT = 256;

__global__ void __launch_bounds__(UM_NT) umap_mean_kernel(const float* __restrict__ dist, int n, int k, double* __restrict__ mean) {
    __shared__ double s_sum[UM_NT];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long i = tid; i < n; i += UM_NT) {
        const float* row = dist + (size_t)i * k;
        for (int j = 0; j < k; ++j) acc += (double)row[j];
    }
    s_sum[tid] = acc;
    __syncthreads();
    for (int s = UM_NT / 2; s >= 1; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    if (tid == 0) mean[0] = s_sum[0] / ((double)n * (double)k);
}

__global__ void __launch_bounds__(UM_NT) umap_smooth_kernel(const int* __restrict__ idx, const float* __restrict__ dist, int n, int k,
                                                            const double* __restrict__ mean, float* __restrict__ rho, float* __restrict__ sigma,
                                                            float* __restrict__ w) {
    const long long i = (long long)blockIdx.x * UM_NT + threadIdx.x;
    if (i >= n) return;
    float d[bqumap::K_MAX], wr[bqumap::K_MAX];
    int id[bqumap::K_MAX];
    for (int j = 0; j < k; ++j) {
        d[j] = dist[(size_t)i * k + j];
        id[j] = idx[(size_t)i * k + j];
    }
    float r, sg;
    bqumap::smooth_row(d, id, k, (int)i, (float)mean[0], &r, &sg, wr);
    rho[i] = r;
    sigma[i] = sg;
    for (int j = 0; j < k; ++j) w[(size_t)i * k + j] = wr[j];
}

__global__ void umap_epoch_kernel(const float* __restrict__ prev, float* __restrict__ out, int n, const long long* __restrict__ indptr,
                                  const int* __restrict__ nbr, const float* __restrict__ eps, float* __restrict__ next, int epoch, float alpha,
                                  float a, float b, unsigned seed_lo, unsigned seed_hi) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r0 = indptr[i];
    float o[2];
    bqumap::epoch_vertex(prev, n, (int)i, nbr + r0, eps + r0, next + r0, (int)(indptr[i + 1] - r0), epoch, alpha, a, b, seed_lo, seed_hi, o);
    out[2 * (size_t)i] = o[0];
    out[2 * (size_t)i + 1] = o[1];
}

}  // namespace

extern "C" {

size_t bq_umap_smooth_scratch_bytes(int64_t n) { return n > 0 ? 256 : 0; }

int bq_umap_smooth(bq_ctx* c, const int32_t* d_idx, const float* d_dist, int64_t n, int k, float* d_rho, float* d_sigma, float* d_w,
                   void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_umap_smooth: null context");
    if (!d_idx || !d_dist || !d_rho || !d_sigma || !d_w || !d_scratch || ((uintptr_t)d_scratch & 7) || n < 1 || n > 0x7fffffff || k < 1 ||
        k > bqumap::K_MAX)
        return fail(c, BQ_ERR_ARG, "bq_umap_smooth: bad argument (null pointer, scratch not 8-byte aligned, n < 1 or k outside 1 .. 64)");
    if (scratch_bytes < bq_umap_smooth_scratch_bytes(n)) return fail(c, BQ_ERR_WORKSPACE, "bq_umap_smooth: scratch below bq_umap_smooth_scratch_bytes(n)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "umap_smooth", 0.0, (double)n * k * 16);
    double* mean = reinterpret_cast<double*>(d_scratch);
    hipLaunchKernelGGL(umap_mean_kernel, dim3(1), dim3(UM_NT), 0, s, d_dist, (int)n, k, mean);
    hipLaunchKernelGGL(umap_smooth_kernel, dim3((unsigned)((n + UM_NT - 1) / UM_NT)), dim3(UM_NT), 0, s, d_idx, d_dist, (int)n, k, mean, d_rho,
                       d_sigma, d_w);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bq_umap_epoch(bq_ctx* c, const float* d_prev, float* d_out, int64_t n, const int64_t* d_indptr, const int32_t* d_nbr, const float* d_eps,
                  float* d_next, int epoch, float alpha, float a, float b, uint64_t seed, int block, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_umap_epoch: null context");
    if (!d_prev || !d_out || d_prev == d_out || !d_indptr || !d_nbr || !d_eps || !d_next || n < 1 || n > 0x7fffffff || epoch < 1)
        return fail(c, BQ_ERR_ARG, "bq_umap_epoch: bad argument (null pointer, d_out == d_prev, n < 1 or epoch < 1)");
    if (block == 0) block = 64;
    if (block < 64 || block > 1024 || block % 64) return fail(c, BQ_ERR_ARG, "bq_umap_epoch: block must be a multiple of 64 in 64 .. 1024 (0: 64)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "umap_epoch", 0.0, (double)n * 16);
    hipLaunchKernelGGL(umap_epoch_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, s, d_prev, d_out, (int)n,
                       reinterpret_cast<const long long*>(d_indptr), d_nbr, d_eps, d_next, epoch, alpha, a, b, (unsigned)seed,
                       (unsigned)(seed >> 32));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
