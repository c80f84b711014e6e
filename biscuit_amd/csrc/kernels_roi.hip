// The whole-slide heatmap's region-of-interest mask (DESIGN.md "Heatmap input", Region-of-interest mask): polygons -> a uint8
// plane [H][W], 1 where the sample point (xs[x], ys[y]) lies inside any polygon (even-odd per polygon, union across polygons), in
// integers on doubled level-0 coordinates.  The crossing rule is roi_device.h's, the one the CPU build (bqio_roi_plane) compiles.
//
// roi_plane_kernel: one workgroup = RO_NT threads x RO_PPT consecutive pixels of ONE row (blockIdx.y; a plane taller than the
// grid's 65 535 rows wraps around in the kernel's row loop), so the row's sample coordinate is uniform over the workgroup.  The
// edge table goes through LDS in chunks of RO_NT edges: every thread loads one edge (one 16-byte load), tests whether it straddles
// the row, and a wave's 64 answers become one 64-bit ballot in LDS.  After the barrier every wave walks the set bits of the four
// ballots -- scalar code, the words pass through readfirstlane -- so an edge whose y-span misses the row costs no vector
// instruction at all, and only the rest is read back from LDS (one address for all lanes: a broadcast) and put through the two
// 32 x 32 -> 64-bit products of the rule, once per pixel of the thread.
//
// Polygons: a thread keeps RO_PPT parity bits and RO_PPT inside bits.  The walk is in edge order, so when it meets an edge at or
// beyond the current polygon's end it folds the parity into the inside bits, clears it and advances to the polygon that holds the
// edge (starts[] is read at a uniform index); a boundary may fall anywhere in a chunk, and polygons none of whose edges straddle
// the row are stepped over without a fold of their own.  One last fold after the last chunk.
//
// Stores: a thread's four pixels are one ALIGNED dword of the plane -- the pixel groups of a row start at -(address of the row
// & 3), not at 0 -- stored as a dword when all four lie in the row and byte by byte at the row's two ends.  The sample tables and
// the polygon starts are checked on the host before they are uploaded (bq_roi_plane); indices are clamped here all the same.
#include "bq_ctx.h"
#include "roi_device.h"

namespace {

constexpr int RO_NT = 256;      // threads of a workgroup = edges of a chunk
constexpr int RO_PPT = 4;      // pixels of a thread: one dword of the plane
constexpr int RO_WAVE = 64, RO_WAVES = RO_NT / RO_WAVE;

__global__ void __launch_bounds__(RO_NT) roi_plane_kernel(const int4* __restrict__ edges, int E, const int* __restrict__ starts, int P,
                                                          const int* __restrict__ xs, const int* __restrict__ ys, int H, int W,
                                                          uint8_t* __restrict__ plane) {
    __shared__ int4 s_edge[RO_NT];
    __shared__ unsigned s_mask[RO_WAVES][2];
    const int tid = threadIdx.x;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {      // (uniform: the barriers below are safe)
        uint8_t* row = plane + (size_t)y * W;
        // the thread's first pixel: -3 .. -1 in the row's first group when the row does not start on a dword
        const long long x0 = ((long long)blockIdx.x * RO_NT + tid) * RO_PPT - (long long)((uintptr_t)row & 3);
        const int py = ys[y];
        int px[RO_PPT];
#pragma unroll
        for (int k = 0; k < RO_PPT; ++k) px[k] = xs[(int)min(max(x0 + k, 0ll), (long long)W - 1)];
        unsigned par = 0, ins = 0;      // bit k: pixel x0 + k
        int p = 0, pend = starts[1];      // the current polygon and its end
        for (int c0 = 0; c0 < E; c0 += RO_NT) {
            const int e = c0 + tid;
            bool hit = false;
            if (e < E) {
                const int4 v = edges[e];
                s_edge[tid] = v;
                hit = bqroi::straddles(v.y, v.w, py);
            }
            const unsigned long long b = __ballot(hit);
            if ((tid & (RO_WAVE - 1)) == 0) {
                s_mask[tid / RO_WAVE][0] = (unsigned)b;
                s_mask[tid / RO_WAVE][1] = (unsigned)(b >> 32);
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < RO_WAVES; ++w) {
                unsigned long long m = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)s_mask[w][0]) |
                                       ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)s_mask[w][1]) << 32);
                while (m) {      // (uniform over the workgroup)
                    const int j = w * RO_WAVE + __builtin_ctzll(m);
                    m &= m - 1;
                    if (c0 + j >= pend) {
                        ins |= par;
                        par = 0;
                        do {
                            ++p;
                            pend = starts[min(p + 1, P)];
                        } while (c0 + j >= pend && p + 1 < P);
                    }
                    const int4 v = s_edge[j];
#pragma unroll
                    for (int k = 0; k < RO_PPT; ++k) par ^= (bqroi::counts_beyond(v.x, v.y, v.z, v.w, px[k], py) ? 1u : 0u) << k;
                }
            }
            __syncthreads();      // the chunk is read: the next may land
        }
        ins |= par;
        if (x0 >= 0 && x0 + RO_PPT <= W) {
            unsigned v = 0;
#pragma unroll
            for (int k = 0; k < RO_PPT; ++k) v |= ((ins >> k) & 1u) << (8 * k);
            *reinterpret_cast<unsigned*>(row + x0) = v;      // (row + x0 is a multiple of 4)
        } else {
#pragma unroll
            for (int k = 0; k < RO_PPT; ++k)
                if (x0 + k >= 0 && x0 + k < W) row[x0 + k] = (uint8_t)((ins >> k) & 1u);
        }
    }
}

}  // namespace

static int launch_roi_plane(const int* edges, int E, const int* starts, int P, const int* xs, const int* ys, int H, int W, uint8_t* plane,
                            hipStream_t s) {
    if (E < 1 || P < 1 || H < 1 || W < 1 || ((uintptr_t)edges & 15)) return (int)hipErrorInvalidValue;
    const long long groups = ((long long)W + 2 * (RO_PPT - 1)) / RO_PPT;      // ceil((W + 3) / 4): any misalignment
    const long long bx = (groups + RO_NT - 1) / RO_NT;      // (W < 2^31: below 2^21)
    const int by = H < 65535 ? H : 65535;      // (taller planes: the kernel's row loop)
    hipLaunchKernelGGL(roi_plane_kernel, dim3((unsigned)bx, (unsigned)by), dim3(RO_NT), 0, s, reinterpret_cast<const int4*>(edges), E, starts,
                       P, xs, ys, H, W, plane);
    return (int)hipGetLastError();
}

extern "C" {

int bq_roi_plane(bq_ctx* c, const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys, int H,
                 int32_t* d_tables, uint8_t* d_plane, bq_stream_t stream) {
    if (!c || !d_tables || !d_plane || ((uintptr_t)d_tables & 15)) return fail(c, BQ_ERR_ARG, "bq_roi_plane: bad argument");
    if (const char* why = bqroi::check_tables(edges, E, starts, P, xs, W, ys, H)) return fail(c, BQ_ERR_ARG, std::string("bq_roi_plane: ") + why);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "roi_plane", 0.0, (double)H * W);
    int32_t* d_edges = d_tables;                                             // (first: the kernel loads an edge as 16 bytes)
    int32_t* d_starts = d_edges + (size_t)4 * E;
    int32_t* d_xs = d_starts + P + 1;
    int32_t* d_ys = d_xs + W;
    HIPCHK(c, hipMemcpyAsync(d_edges, edges, (size_t)4 * E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_starts, starts, ((size_t)P + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_xs, xs, (size_t)W * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ys, ys, (size_t)H * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_roi_plane(d_edges, E, d_starts, P, d_xs, d_ys, H, W, d_plane, s)) return fail(c, BQ_ERR_HIP, "roi plane launch failed");
    return BQ_OK;
}

}  // extern "C"
