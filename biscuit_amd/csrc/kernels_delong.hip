// DeLong's covariance of the AUROCs of k classifiers scored on the same n rows (biscuit/delong.py, fastDeLong; DESIGN.md section 7
// "Prediction metrics"): per classifier the structural component V of every row and the AUROC from the midranks, then the unbiased
// covariance of V over the positives and over the negatives.  Float64 and integers throughout, HBM-bound, no matrix cores.
//
// Per classifier, in scratch reused across classifiers: one ascending radix sort of (score, row index) pairs (rocPRIM), the labels
// gathered in sorted order, one inclusive scan of the positives, and one pass that finds each row's tie run [s, e) -- its neighbours
// first, two binary searches of its own score where they tie --, turns (s, e, cum_pos) into V, scatters it to the row's original
// position (classifiers are paired by row) and adds 2 tz = s + e + 1 of the positives into a 64-bit integer sum (integer addition:
// the order does not matter).  V's numerators are half-integers, exact in float64; each V costs one rounded division (and one
// rounded subtraction for a negative), uncontracted, so it equals the reference's v01 / v10 bit for bit, and so does the AUROC.
//
// The covariance is two passes over V in row order by chunk_sum.h's scheme: class sums -> class means -> centred products, the
// k (k + 1) / 2 sums of each class in registers.  No floating-point atomics: the same bits every call.  Every scratch byte a kernel
// reads was written earlier in the same call (DESIGN.md "Buffer contract").
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bq_ctx.h"
#include "chunk_sum.h"

namespace {

constexpr int MAX_K = 8;
constexpr long long MAX_N = 1LL << 25;      // sum 2 tz <= m (2 n + 1) < 2^53: exact as an integer and as a double

struct U8ToU32 {
    __host__ __device__ unsigned operator()(unsigned char v) const { return v ? 1u : 0u; }
};

// iota[i] = i, the sort's values; the k integer sums start at 0
__global__ void __launch_bounds__(NT) delong_init_kernel(unsigned* __restrict__ iota, long long n, unsigned long long* __restrict__ sum2,
                                                         int k) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) iota[i] = (unsigned)i;
    if (i < k) sum2[i] = 0ull;
}

__global__ void __launch_bounds__(NT) delong_gather_kernel(const unsigned char* __restrict__ label, const unsigned* __restrict__ idx,
                                                           long long n, unsigned char* __restrict__ lab_sorted) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) lab_sorted[i] = label[idx[i]] != 0 ? 1 : 0;
}

// a thread per sorted position: key ascending, idx the row, lab the label there, cum the inclusive count of positives
__global__ void __launch_bounds__(NT) delong_v_kernel(const double* __restrict__ key, const unsigned* __restrict__ idx,
                                                      const unsigned char* __restrict__ lab, const unsigned* __restrict__ cum, long long n,
                                                      double* __restrict__ V, unsigned long long* __restrict__ sum2) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    unsigned long long t2 = 0ull;
    if (i < n) {
        const double x = key[i];
        long long s = i, e = i + 1;
        if (i > 0 && !(key[i - 1] < x)) {           // the run starts earlier: the first j of 0 .. i - 1 with key[j] >= x
            long long lo = 0, hi = i - 1;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (key[mid] < x) lo = mid + 1; else hi = mid;
            }
            s = lo;
        }
        if (i + 1 < n && !(key[i + 1] > x)) {       // the run ends later: the first j of i + 2 .. n with key[j] > x (n: none)
            long long lo = i + 2, hi = n;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;       // < hi <= n
                if (key[mid] > x) hi = mid; else lo = mid + 1;
            }
            e = lo;
        }
        const long long m = cum[n - 1], n0 = n - m;
        const long long below_pos = s > 0 ? (long long)cum[s - 1] : 0, tied_pos = (long long)cum[e - 1] - below_pos;
        const long long below_neg = s - below_pos, tied_neg = (e - s) - tied_pos;
        double v;
        if (lab[i]) {
            v = (0.5 * (double)(2 * below_neg + tied_neg)) / (double)n0;
            t2 = (unsigned long long)(s + e + 1);
        } else {
            const double q = (0.5 * (double)(2 * below_pos + tied_pos)) / (double)m;
            v = 1.0 - q;
        }
        V[idx[i]] = v;
    }
    for (int msk = 1; msk < 64; msk <<= 1) t2 += __shfl_xor(t2, msk);
    if ((threadIdx.x & 63) == 0 && t2) atomicAdd(sum2, t2);
}

// a thread per classifier: out = auc [k], S [k][k] (the last kernel), m, n0
__global__ void delong_auc_kernel(const unsigned long long* __restrict__ sum2, const unsigned* __restrict__ cum, long long n, int k,
                                  double* __restrict__ out) {
#pragma clang fp contract(off)
    const int r = threadIdx.x;
    const double m = (double)cum[n - 1], n0 = (double)(n - (long long)cum[n - 1]);
    if (r < k) {
        const double tz = 0.5 * (double)sum2[r];
        const double a = tz / m / n0, b = ((m + 1.0) / 2.0) / n0;
        out[r] = a - b;
    }
    if (r == 0) { out[k + k * k] = m; out[k + k * k + 1] = n0; }
}

// pass 1 over a chunk -> part1[chunk][2 K]: the sums of V over the chunk's positives [K], then over its negatives [K]
template <int K>
__global__ void __launch_bounds__(NT) delong_sum_kernel(const double* __restrict__ V, const unsigned char* __restrict__ y, long long n,
                                                        long long rows, double* __restrict__ part1) {
    __shared__ double lds[(NW + 1) * 2 * K];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    double s[2 * K];
#pragma unroll
    for (int r = 0; r < 2 * K; ++r) s[r] = 0.0;
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const bool pos = y[i] != 0;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const double v = V[(size_t)r * n + i];
            s[r] += pos ? v : 0.0;
            s[K + r] += pos ? 0.0 : v;
        }
    }
    const double* sum = block_sum<2 * K>(s, lds);
    if (threadIdx.x < 2 * K) part1[(size_t)blockIdx.x * 2 * K + threadIdx.x] = sum[threadIdx.x];
}

// one workgroup: part1 over the chunks in order -> mean[2 k] = the class means, positives then negatives
__global__ void __launch_bounds__(NT) delong_mean_kernel(const double* __restrict__ part1, int chunks, int k, const double* __restrict__ out,
                                                         double* __restrict__ mean) {
    const int t = threadIdx.x;
    if (t >= 2 * k) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part1[(size_t)c * 2 * k + t];
    mean[t] = s / out[k + k * k + (t < k ? 0 : 1)];
}

// pass 2 over a chunk -> part2[chunk][2 NP]: the centred products of the pairs a <= b over the positives [NP], the negatives [NP]
template <int K>
__global__ void __launch_bounds__(NT) delong_prod_kernel(const double* __restrict__ V, const unsigned char* __restrict__ y, long long n,
                                                         long long rows, const double* __restrict__ mean, double* __restrict__ part2) {
    constexpr int NP = K * (K + 1) / 2;
    __shared__ double lds[(NW + 1) * 2 * NP];
    const long long base = (long long)blockIdx.x * rows;
    const long long end = base + rows < n ? base + rows : n;
    double mu[2 * K], acc[2 * NP];
#pragma unroll
    for (int r = 0; r < 2 * K; ++r) mu[r] = mean[r];
#pragma unroll
    for (int p = 0; p < 2 * NP; ++p) acc[p] = 0.0;
    for (long long i = base + threadIdx.x; i < end; i += NT) {
        const bool pos = y[i] != 0;
        double d[K];
#pragma unroll
        for (int r = 0; r < K; ++r) d[r] = V[(size_t)r * n + i] - (pos ? mu[r] : mu[K + r]);
        int p = 0;
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = a; b < K; ++b, ++p) {
                const double pr = d[a] * d[b];
                acc[p] += pos ? pr : 0.0;
                acc[NP + p] += pos ? 0.0 : pr;
            }
    }
    const double* sum = block_sum<2 * NP>(acc, lds);
    if (threadIdx.x < 2 * NP) part2[(size_t)blockIdx.x * 2 * NP + threadIdx.x] = sum[threadIdx.x];
}

// a thread per entry of S: the partials in chunk order -> S = cov(V | positive) / m + cov(V | negative) / n0, the covariances
// unbiased (a class of one row: 0 / 0, NaN, as numpy.cov gives)
__global__ void __launch_bounds__(NT) delong_cov_kernel(const double* __restrict__ part2, int chunks, int k, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= k * k) return;
    const int a = t / k < t % k ? t / k : t % k, b = t / k < t % k ? t % k : t / k;     // a <= b
    const int np = k * (k + 1) / 2, p = a * k - a * (a - 1) / 2 + (b - a);
    double cp = 0.0, cn = 0.0;
    for (int c = 0; c < chunks; ++c) {
        cp += part2[(size_t)c * 2 * np + p];
        cn += part2[(size_t)c * 2 * np + np + p];
    }
    const double m = out[k + k * k], n0 = out[k + k * k + 1];
    out[k + t] = cp / (m - 1.0) / m + cn / (n0 - 1.0) / n0;
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

bool delong_args_ok(int k, long long n) { return k >= 1 && k <= MAX_K && n >= 1 && n <= MAX_N; }

size_t delong_temp_bytes(long long n) {
    size_t sort_b = 0, scan_b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_b, (double*)nullptr, (double*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (size_t)n, 0,
                                    64, (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, scan_b, rocprim::make_transform_iterator((unsigned char*)nullptr, U8ToU32()), (unsigned*)nullptr,
                                  (size_t)n, rocprim::plus<unsigned>(), (hipStream_t)0);
    return sort_b > scan_b ? sort_b : scan_b;
}

// temp | iota u32 [n] | key f64 [n] | idx u32 [n] | lab u8 [n] | cum u32 [n] | V f64 [k][n] | sum2 u64 [k] | part1 [ch][2 k] |
// mean [2 k] | part2 [ch][k (k + 1)]
size_t delong_workspace_bytes(int k, long long n) {
    if (!delong_args_ok(k, n)) return 0;
    const size_t ch = (size_t)num_chunks(n), N = (size_t)n;
    return al(delong_temp_bytes(n)) + al(N * 4) + al(N * 8) + al(N * 4) + al(N) + al(N * 4) + al((size_t)k * N * 8) + al((size_t)k * 8) +
           al(ch * 2 * k * 8) + al((size_t)2 * k * 8) + al(ch * k * (k + 1) * 8);
}

template <int K>
void launch_cov(const double* V, const unsigned char* y, long long n, long long rows, int ch, double* part1, double* mean, double* part2,
                double* out, hipStream_t s) {
    hipLaunchKernelGGL(delong_sum_kernel<K>, dim3(ch), dim3(NT), 0, s, V, y, n, rows, part1);
    hipLaunchKernelGGL(delong_mean_kernel, dim3(1), dim3(NT), 0, s, part1, ch, K, out, mean);
    hipLaunchKernelGGL(delong_prod_kernel<K>, dim3(ch), dim3(NT), 0, s, V, y, n, rows, mean, part2);
    hipLaunchKernelGGL(delong_cov_kernel, dim3(1), dim3(NT), 0, s, part2, ch, K, out);
}

}  // namespace

extern "C" {

int64_t bq_delong_chunk_rows(int64_t n) { return n >= 1 ? (int64_t)chunk_rows((long long)n) : 0; }

size_t bq_delong_workspace_bytes(int k, int64_t n) { return delong_workspace_bytes(k, (long long)n); }

int bq_delong(bq_ctx* c, const double* d_scores, const uint8_t* d_label, int k, int64_t n, void* d_ws, size_t ws_bytes, double* d_out,
              double* d_V, bq_stream_t stream) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_delong: null context");
    if (!delong_args_ok(k, n)) return fail(c, BQ_ERR_ARG, "bq_delong: 1 <= k <= 8 and 1 <= n <= 2^25");
    if (!d_scores || !d_label || !d_out || !d_ws || ((uintptr_t)d_scores & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_V & 7) ||
        ((uintptr_t)d_ws & 255))
        return fail(c, BQ_ERR_ARG, "bq_delong: bad argument (null pointer, scores, out or V not 8-byte or the workspace not 256-byte aligned)");
    if (ws_bytes < delong_workspace_bytes(k, n)) return fail(c, BQ_ERR_WORKSPACE, "bq_delong: workspace below bq_delong_workspace_bytes(k, n)");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(c->device);
    ProfScope ps(c, s, "delong", (double)n * k * (k + 1) * 3.0, (double)n * k * (120.0 + 16.0));
    const long long rows = chunk_rows(n);
    const int ch = (int)num_chunks(n);
    const size_t N = (size_t)n;
    size_t sort_b = 0, scan_b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_b, (double*)nullptr, (double*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, N, 0, 64, s);
    (void)rocprim::inclusive_scan(nullptr, scan_b, rocprim::make_transform_iterator((unsigned char*)nullptr, U8ToU32()), (unsigned*)nullptr,
                                  N, rocprim::plus<unsigned>(), s);
    unsigned char* p = (unsigned char*)d_ws;
    void* d_tmp = p; p += al(sort_b > scan_b ? sort_b : scan_b);
    unsigned* iota = (unsigned*)p; p += al(N * 4);
    double* key = (double*)p; p += al(N * 8);
    unsigned* idx = (unsigned*)p; p += al(N * 4);
    unsigned char* lab = p; p += al(N);
    unsigned* cum = (unsigned*)p; p += al(N * 4);
    double* V = d_V ? d_V : (double*)p; p += al((size_t)k * N * 8);
    unsigned long long* sum2 = (unsigned long long*)p; p += al((size_t)k * 8);
    double* part1 = (double*)p; p += al((size_t)ch * 2 * k * 8);
    double* mean = (double*)p; p += al((size_t)2 * k * 8);
    double* part2 = (double*)p;
    const unsigned grid = (unsigned)((n + NT - 1) / NT);
    hipLaunchKernelGGL(delong_init_kernel, dim3(grid), dim3(NT), 0, s, iota, (long long)n, sum2, k);
    for (int r = 0; r < k; ++r) {
        HIPCHK(c, rocprim::radix_sort_pairs(d_tmp, sort_b, d_scores + (size_t)r * N, key, iota, idx, N, 0, 64, s));
        hipLaunchKernelGGL(delong_gather_kernel, dim3(grid), dim3(NT), 0, s, d_label, idx, (long long)n, lab);
        HIPCHK(c, rocprim::inclusive_scan(d_tmp, scan_b, rocprim::make_transform_iterator(lab, U8ToU32()), cum, N, rocprim::plus<unsigned>(), s));
        hipLaunchKernelGGL(delong_v_kernel, dim3(grid), dim3(NT), 0, s, key, idx, lab, cum, (long long)n, V + (size_t)r * N, sum2 + r);
    }
    hipLaunchKernelGGL(delong_auc_kernel, dim3(1), dim3(64), 0, s, sum2, cum, (long long)n, k, d_out);
    switch (k) {
        case 1: launch_cov<1>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 2: launch_cov<2>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 3: launch_cov<3>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 4: launch_cov<4>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 5: launch_cov<5>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 6: launch_cov<6>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        case 7: launch_cov<7>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
        default: launch_cov<8>(V, d_label, n, rows, ch, part1, mean, part2, d_out, s); break;
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
