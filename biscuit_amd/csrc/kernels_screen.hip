// The f16 range screen ("Range screen"): every tile of a run gets one number, the largest |value| that
// tf.image.per_image_standardization gives it,
//     key = max(hi - mu, mu - lo) / max(sd, 1/sqrt(N))        N = px * px * 3
// (hi, lo: the tile's largest and smallest byte; mu, sd: float64 from the exact integer sums of its bytes, the statistics of
// stage_apply_kernel; FP contraction off, rounded once to float32), and a per-context set of k candidate slots keeps the top k
// tiles of an interval by (key desc, global tile index asc) -- key, index and the tile's bytes -- for the range taps.
//
// Four kernels, all on the caller's stream:
//   range_stats_kernel   kScreenSlices workgroups per tile, the byte walk of stage_stats_kernel (unaligned head, 16-byte body,
//                        tail; v_sad_u8 / v_dot4_u32_u8) plus a packed byte max / min; one partial per workgroup, no atomics
//   range_key_kernel     one lane per tile: the key from its slices' partials (bq_range_key)
//   range_select_kernel  one workgroup: the batch's keys merged with the k slots, survivors keep their slot, newly admitted tiles
//                        take the freed ones in rank order; writes the copy plan
//   range_copy_kernel    the bytes of each newly admitted tile into its slot (blocks of untouched slots return at once)
#include "bq_ctx.h"

namespace {

constexpr int kScreenSlices = 8;
constexpr int kScreenNT = 256;
constexpr int kCopySlices = 16;

struct RangePart {
    unsigned long long s1, s2;   // sum and sum of squares of the slice's bytes
    unsigned hi, lo;             // its largest and smallest byte
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ us2 as_us2(unsigned u) { return __builtin_bit_cast(us2, u); }

__global__ void __launch_bounds__(kScreenNT) range_stats_kernel(const uint8_t* __restrict__ tiles, int px,
                                                                RangePart* __restrict__ parts) {
    const int nbytes = px * px * 3;
    const int tile = blockIdx.x / kScreenSlices, sl = blockIdx.x - tile * kScreenSlices;
    const uint8_t* src = tiles + (size_t)tile * nbytes;
    const int tid = threadIdx.x, nt = blockDim.x;
    // sums as in stage_stats_kernel (a thread's share of a slice is ~130 bytes: 32-bit partials cannot overflow); max / min of the
    // bytes two at a time with v_pk_max_u16 / v_pk_min_u16: the high byte of the largest (smallest) of a set of 16-bit values is the
    // largest (smallest) of their high bytes, so the word itself carries its odd bytes there and the word shifted left by 8 its even
    // ones -- one shift and four packed operations per four bytes
    unsigned p1 = 0, p2 = 0;
    us2 mxe = {0, 0}, mxo = {0, 0}, mne = {0xFFFF, 0xFFFF}, mno = {0xFFFF, 0xFFFF};
    unsigned hi = 0, lo = 255;
    auto word = [&](unsigned u) {
        p1 = __builtin_amdgcn_sad_u8(u, 0u, p1);
        p2 = __builtin_amdgcn_udot4(u, u, p2, false);
        const us2 e = as_us2(u << 8), o = as_us2(u);
        mxe = __builtin_elementwise_max(mxe, e); mxo = __builtin_elementwise_max(mxo, o);
        mne = __builtin_elementwise_min(mne, e); mno = __builtin_elementwise_min(mno, o);
    };
    auto byte = [&](unsigned v) {
        p1 += v; p2 += v * v;
        hi = v > hi ? v : hi; lo = v < lo ? v : lo;
    };
    const int head = (int)((4 - ((uintptr_t)src & 3)) & 3);
    const int body = (nbytes - head) >> 2;
    const int d0 = (int)((long long)body * sl / kScreenSlices), d1 = (int)((long long)body * (sl + 1) / kScreenSlices);
    if (sl == 0 && tid < head) byte(src[tid]);
    const unsigned* w = reinterpret_cast<const unsigned*>(src + head);
    const int nq = (d1 - d0) >> 2;                      // whole groups of four words (16 bytes: dword alignment is all it needs)
#pragma unroll 2
    for (int i = tid; i < nq; i += nt) {
        const uint4 u = *reinterpret_cast<const uint4*>(w + d0 + 4 * i);
        word(u.x); word(u.y); word(u.z); word(u.w);
    }
    for (int i = d0 + 4 * nq + tid; i < d1; i += nt) word(w[i]);
    const int tail0 = head + body * 4;
    if (sl == kScreenSlices - 1 && tid < nbytes - tail0) byte(src[tail0 + tid]);
    {
        const us2 mx = __builtin_elementwise_max(mxe, mxo) >> (unsigned short)8, mn = __builtin_elementwise_min(mne, mno) >> (unsigned short)8;
        const unsigned a = mx.x > mx.y ? mx.x : mx.y, b = mn.x < mn.y ? mn.x : mn.y;
        hi = a > hi ? a : hi; lo = b < lo ? b : lo;
    }
    unsigned long long s1 = p1, s2 = p2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        const unsigned h = __shfl_xor(hi, o), l = __shfl_xor(lo, o);
        hi = h > hi ? h : hi; lo = l < lo ? l : lo;
    }
    __shared__ RangePart red[kScreenNT / 64];
    if ((tid & 63) == 0) red[tid >> 6] = RangePart{s1, s2, hi, lo};
    __syncthreads();
    if (tid == 0) {
        RangePart r = red[0];
        for (int q = 1; q < nt / 64; ++q) {
            r.s1 += red[q].s1; r.s2 += red[q].s2;
            r.hi = red[q].hi > r.hi ? red[q].hi : r.hi; r.lo = red[q].lo < r.lo ? red[q].lo : r.lo;
        }
        parts[blockIdx.x] = r;
    }
}

// the key of one tile from the partials of its slices (float64, no contraction: a numpy float64 restatement gives the same bits)
__device__ float range_key_of(const RangePart* __restrict__ p, int nbytes) {
#pragma clang fp contract(off)
    unsigned long long s1 = 0, s2 = 0;
    unsigned hi = 0, lo = 255;
    for (int q = 0; q < kScreenSlices; ++q) {
        s1 += p[q].s1; s2 += p[q].s2;
        hi = p[q].hi > hi ? p[q].hi : hi; lo = p[q].lo < lo ? p[q].lo : lo;
    }
    const double n = (double)nbytes;
    const double mu = (double)s1 / n;
    double var = (double)s2 / n - mu * mu;
    if (var < 0) var = 0;
    const double sd = sqrt(var), floor_sd = 1.0 / sqrt(n);
    const double den = sd > floor_sd ? sd : floor_sd;
    const double a = (double)hi - mu, b = mu - (double)lo;
    return (float)((a > b ? a : b) / den);
}

__global__ void __launch_bounds__(kScreenNT) range_key_kernel(const RangePart* __restrict__ parts, int n, int px,
                                                              float* __restrict__ key) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = range_key_of(parts + (size_t)i * kScreenSlices, px * px * 3);
}

// element f beats element e: larger key, then smaller global index, then (equal index: the same tile seen twice) the earlier
// position -- the old slots come first -- so that the order is total and the result deterministic
struct Entry { long long idx; float key; int pos; };     // 16 bytes: one LDS read per comparison
__device__ __forceinline__ int beats(const Entry& f, const Entry& e) {      // (bitwise, not short-circuit: no branches in the scan)
    return (int)(f.key > e.key) | ((int)(f.key == e.key) & ((int)(f.idx < e.idx) | ((int)(f.idx == e.idx) & (int)(f.pos < e.pos))));
}

constexpr int kMaxSlots = 64;
constexpr int kSelectNT = 1024;       // one element per lane at batch 256: the rank scans (total reads each) run side by side

__global__ void __launch_bounds__(kSelectNT) range_select_kernel(const RangePart* __restrict__ parts, int n, int px,
                                                                 long long tile_idx0, const long long* __restrict__ tile_idx,
                                                                 float* cand_key, long long* cand_idx, int k, int filled,
                                                                 int* __restrict__ plan) {
    extern __shared__ Entry ent[];          // [filled + n]: the filled slots, then the batch
    const int total = filled + n;
    __shared__ int at_rank[kMaxSlots];      // the element of rank r < k
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nbytes = px * px * 3;
    for (int e = tid; e < total; e += nt) {
        if (e < filled) {
            ent[e] = Entry{cand_idx[e], cand_key[e], e};
        } else {
            const int i = e - filled;
            ent[e] = Entry{tile_idx ? tile_idx[i] : tile_idx0 + i, range_key_of(parts + (size_t)i * kScreenSlices, nbytes), e};
        }
    }
    __syncthreads();
    for (int e = tid; e < total; e += nt) {
        const Entry me = ent[e];
        int r = 0;
#pragma unroll 8
        for (int f = 0; f < total; ++f) r += beats(ent[f], me);
        if (r < k) at_rank[r] = e;          // a total order: ranks 0 .. total-1 are taken once each
    }
    __syncthreads();
    if (tid != 0) return;
    // survivors keep their slot; the freed slots (evicted or empty) go to the newly admitted tiles in rank order, lowest slot first:
    // the filled slots stay a prefix of the slot array
    const int kept = total < k ? total : k;
    unsigned long long taken = 0;           // bit s: slot s holds a survivor or has been given to an admitted tile
    for (int s = 0; s < k; ++s) plan[s] = -1;
    for (int r = 0; r < kept; ++r)
        if (at_rank[r] < filled) taken |= 1ull << at_rank[r];
    int next = 0;
    for (int r = 0; r < kept; ++r) {
        const int e = at_rank[r];
        if (e < filled) continue;
        while ((taken >> next) & 1ull) ++next;
        taken |= 1ull << next;
        cand_key[next] = ent[e].key;
        cand_idx[next] = ent[e].idx;
        plan[next] = e - filled;
    }
}

__global__ void __launch_bounds__(kScreenNT) range_copy_kernel(const uint8_t* __restrict__ tiles, int px,
                                                               const int* __restrict__ plan, uint8_t* __restrict__ slots) {
    const int slot = blockIdx.x / kCopySlices, sl = blockIdx.x - slot * kCopySlices;
    const int row = plan[slot];
    if (row < 0) return;
    const long long nbytes = (long long)px * px * 3;
    const uint8_t* src = tiles + row * nbytes;
    uint8_t* dst = slots + slot * nbytes;
    const long long b0 = nbytes * sl / kCopySlices, b1 = nbytes * (sl + 1) / kCopySlices;
    for (long long b = b0 + threadIdx.x; b < b1; b += blockDim.x) dst[b] = src[b];
}

}  // namespace

static size_t range_ws_bytes(int n) {
    const size_t parts = (size_t)(n > 0 ? n : 0) * kScreenSlices * sizeof(RangePart);
    return ((parts + 255) & ~(size_t)255) + 256;          // + the copy plan (int [kMaxSlots])
}

static int launch_range_key(const uint8_t* tiles, int n, int px, void* ws, float* key, hipStream_t s) {
    if (n <= 0) return 0;
    RangePart* parts = reinterpret_cast<RangePart*>(ws);
    hipLaunchKernelGGL(range_stats_kernel, dim3(n * kScreenSlices), dim3(kScreenNT), 0, s, tiles, px, parts);
    hipLaunchKernelGGL(range_key_kernel, dim3((n + kScreenNT - 1) / kScreenNT), dim3(kScreenNT), 0, s, parts, n, px, key);
    return (int)hipGetLastError();
}

static int launch_range_screen(const uint8_t* tiles, int n, int px, long long tile_idx0, const long long* tile_idx, float* cand_key,
                               long long* cand_idx, uint8_t* cand_tiles, int k, int filled, void* ws, hipStream_t s) {
    if (n <= 0) return 0;
    RangePart* parts = reinterpret_cast<RangePart*>(ws);
    const size_t pb = (size_t)n * kScreenSlices * sizeof(RangePart);
    int* plan = reinterpret_cast<int*>((unsigned char*)ws + ((pb + 255) & ~(size_t)255));
    hipLaunchKernelGGL(range_stats_kernel, dim3(n * kScreenSlices), dim3(kScreenNT), 0, s, tiles, px, parts);
    hipLaunchKernelGGL(range_select_kernel, dim3(1), dim3(kSelectNT), (size_t)(filled + n) * sizeof(Entry), s, parts, n, px, tile_idx0,
                       tile_idx, cand_key, cand_idx, k, filled, plan);
    hipLaunchKernelGGL(range_copy_kernel, dim3(k * kCopySlices), dim3(kScreenNT), 0, s, tiles, px, plan, cand_tiles);
    return (int)hipGetLastError();
}

extern "C" {

size_t bq_range_ws_bytes(int n) { return n < 0 ? 0 : range_ws_bytes(n); }

int bq_range_key(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_key, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || n < 0 || (n > 0 && (!d_tiles || !d_key || !d_ws))) return fail(c, BQ_ERR_ARG, "bq_range_key: bad argument");
    if (ws_bytes < range_ws_bytes(n)) return fail(c, BQ_ERR_ARG, "bq_range_key: scratch smaller than bq_range_ws_bytes(n)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "range_key", 2.0 * n * kStaged, (double)n * kStaged);
    if (launch_range_key(d_tiles, n, 299, d_ws, d_key, s)) return fail(c, BQ_ERR_HIP, "range key launch failed");
    return BQ_OK;
}

int bq_range_screen(bq_ctx* c, const uint8_t* d_tiles, int n, int64_t tile_idx0, const int64_t* d_tile_idx, float* d_cand_key,
                    int64_t* d_cand_idx, uint8_t* d_cand_tiles, int k, int filled, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || n < 0 || n > 2048 || (n > 0 && (!d_tiles || !d_cand_key || !d_cand_idx || !d_cand_tiles || !d_ws)))
        return fail(c, BQ_ERR_ARG, "bq_range_screen: bad argument");
    if (k < 1 || k > kMaxSlots || filled < 0 || filled > k)
        return fail(c, BQ_ERR_ARG, "bq_range_screen: need 1 <= k <= " + std::to_string(kMaxSlots) + " and 0 <= filled <= k");
    if (ws_bytes < range_ws_bytes(n)) return fail(c, BQ_ERR_ARG, "bq_range_screen: scratch smaller than bq_range_ws_bytes(n)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "range_screen", 2.0 * n * kStaged, (double)n * kStaged);
    if (launch_range_screen(d_tiles, n, 299, (long long)tile_idx0, reinterpret_cast<const long long*>(d_tile_idx), d_cand_key,
                            reinterpret_cast<long long*>(d_cand_idx), d_cand_tiles, k, filled, d_ws, s))
        return fail(c, BQ_ERR_HIP, "range screen launch failed");
    return BQ_OK;
}

}  // extern "C"
