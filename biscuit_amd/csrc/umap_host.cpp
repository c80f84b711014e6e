// Host side of the feature map (include/biscuit_io.h: bqio_knn, bqio_umap_smooth, bqio_umap_epoch): the CPU builds of bq_knn,
// bq_umap_smooth and bq_umap_epoch over the per-row arithmetic of umap_device.h -- the one the GPU kernels are compiled from.
// bqio_knn ranks ALL n rows by the direct form (no pruning pass): what the device returns on every row, because bq_knn keeps a
// pruned row only where it proves that no neighbour was lost and ranks all n rows itself elsewhere.  Row by row, pair by pair:
// for tests.
#include "../../include/biscuit_io.h"
#include "umap_device.h"

#include <vector>

extern "C" {

int bqio_knn_gemm_bound(const float* nq, const float* nc, int64_t count, int D, float* out) {
    if (!nq || !nc || !out || count < 0 || D < 1) return BQIO_ERR_ARG;
    for (int64_t e = 0; e < count; ++e) out[e] = bqumap::gemm_form_err(nq[e], nc[e], D);
    return BQIO_OK;
}

int bqio_knn(const float* X, int n, int D, int k, int32_t* idx, float* dist) {
    if (!X || !idx || !dist || bqumap::check_knn(n, D, k)) return BQIO_ERR_ARG;
    for (size_t e = 0; e < (size_t)n * D; ++e)
        if (!(fabsf(X[e]) < INFINITY)) return BQIO_ERR_ARG;
    std::vector<float> bd((size_t)k);
    std::vector<int> bi((size_t)k);
    for (int i = 0; i < n; ++i) {
        int have = 0;
        for (int j = 0; j < n; ++j) {
            const float d = sqrtf(bqumap::sqdist_host(X + (size_t)i * D, X + (size_t)j * D, D));      // (the order is the DISTANCE's: two sums may share a root)
            if (!(d < INFINITY)) continue;      // (a sum that overflowed: no candidate, on the device neither)
            if (have == k && !bqumap::before(d, j, bd[k - 1], bi[k - 1])) continue;
            int at = have < k ? have++ : k - 1;
            while (at > 0 && bqumap::before(d, j, bd[at - 1], bi[at - 1])) {
                bd[at] = bd[at - 1];
                bi[at] = bi[at - 1];
                --at;
            }
            bd[at] = d;
            bi[at] = j;
        }
        for (int j = 0; j < k; ++j) {
            idx[(size_t)i * k + j] = j < have ? bi[j] : -1;
            dist[(size_t)i * k + j] = j < have ? bd[j] : NAN;
        }
    }
    return BQIO_OK;
}

int bqio_umap_smooth(const int32_t* idx, const float* dist, int n, int k, float* rho, float* sigma, float* w) {
    if (!idx || !dist || !rho || !sigma || !w || n < 1 || k < 1 || k > bqumap::K_MAX) return BQIO_ERR_ARG;
    double total = 0.0;
    for (size_t e = 0; e < (size_t)n * k; ++e) total += (double)dist[e];
    const float global_mean = (float)(total / ((double)n * k));
    for (int i = 0; i < n; ++i)
        bqumap::smooth_row(dist + (size_t)i * k, idx + (size_t)i * k, k, i, global_mean, rho + i, sigma + i, w + (size_t)i * k);
    return BQIO_OK;
}

int bqio_umap_epoch(const float* prev, float* out, int n, const int64_t* indptr, const int32_t* nbr, const float* eps, float* next,
                    int epoch, float alpha, float a, float b, uint64_t seed) {
    if (!prev || !out || !indptr || n < 1 || epoch < 1 || indptr[0] != 0) return BQIO_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (indptr[i + 1] < indptr[i] || indptr[i + 1] - indptr[i] > 0x7fffffff) return BQIO_ERR_ARG;
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e)
            if (nbr[e] < 0 || nbr[e] >= n) return BQIO_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) {
        const int64_t r0 = indptr[i];
        bqumap::epoch_vertex(prev, n, i, nbr + r0, eps + r0, next + r0, (int)(indptr[i + 1] - r0), epoch, alpha, a, b, (uint32_t)seed,
                             (uint32_t)(seed >> 32), out + 2 * (size_t)i);
    }
    return BQIO_OK;
}

}  // extern "C"
