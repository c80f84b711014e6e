// kernels_j2k.hip -- a TIFF page's JPEG 2000 tiles decoded on the device into a slide canvas (bq_j2k_decode_canvas; DESIGN.md
// "Heatmap input", JPEG 2000 tiles).  Tier 2 -- the packet headers -- stays on the host (j2k_host.cpp: bqio_j2k_extract);
// what it packs goes through four launches a round, over the routines of j2k_device.h, which bqio_j2k_decode_canvas runs on
// the CPU and which the result equals byte for byte:
//   j2k_status   a lane per segment: the descriptor's status, or ST_DESC for a descriptor the decoder does not take
//   j2k_t1       a lane per code block: the MQ decoder and the three coding passes.  One dependent chain per block, so the
//                parallelism is across blocks (the precedent: kernels_inflate.hip, a stream per lane).  MQ state in
//                registers, the 19 context bytes and the probability table in LDS, samples and flags in the segment's
//                planes in global scratch.  A row of the block table is checked (block_ok) before anything is indexed by it.
//   j2k_idwt     a workgroup per segment and component: dequantisation, then level by level the row pass (a lane per
//                row) and the column pass (a lane per column) between two planes in global scratch
//   j2k_store    a lane per pixel: inverse RCT / ICT, rounding, level shift, clamp, YCbCr -> RGB for compression 33003, and
//                the write into the canvas inside the clip rectangle; a segment whose status is not 0 writes nothing
// Scratch per segment: two int32 planes of 3 * seg_w * seg_h samples (coefficients; the second holds tier 1's flags first,
// then the transform's intermediate lines).
#include "bq_ctx.h"
#include "j2k_device.h"

namespace {

using namespace bqj2k;

constexpr int T1_NT = 64, JK_NT = 256;

struct J2kParams {
    const Seg* seg;              // the call's descriptors
    const Block* blocks;
    const uint8_t* bytes;
    const int32_t* place;
    int32_t* status;             // the call's status array
    int32_t* plane_a;            // [round segment][3][h][w]
    int32_t* plane_b;
    uint8_t* canvas;
    unsigned long long n_bytes;
    long long n_blocks;
    int n, t0, cnt, w, h, H, W, ycc;
    int32_t clip[4];
};

__global__ __launch_bounds__(JK_NT) void j2k_status_kernel(J2kParams p) {
    const int i = p.t0 + (int)(blockIdx.x * JK_NT + threadIdx.x);
    if (i >= p.t0 + p.cnt) return;
    const Seg s = p.seg[i];
    int st = s.status;
    if (!st && (!seg_ok(s, p.w, p.h) || s.first_block < 0 || s.n_blocks < 0 || (long long)s.first_block + s.n_blocks > p.n_blocks)) st = ST_DESC;
    p.status[i] = st;
}

__global__ __launch_bounds__(T1_NT) void j2k_t1_kernel(J2kParams p) {
    __shared__ uint32_t tab[MQ_STATES];
    __shared__ uint8_t cx[CX_N * T1_NT];
    if (threadIdx.x < MQ_STATES) tab[threadIdx.x] = mq_table_row((int)threadIdx.x);
    __syncthreads();
    const long long q = (long long)blockIdx.x * T1_NT + threadIdx.x;
    if (q >= p.n_blocks) return;
    const Block b = p.blocks[q];
    if (b.seg < p.t0 || b.seg >= p.t0 + p.cnt) return;                          // another round's, or no segment of this call
    if (p.status[b.seg]) return;
    const Seg& s = p.seg[b.seg];
    if (q < s.first_block || q >= (long long)s.first_block + s.n_blocks) return;
    if (!block_ok(b, p.n, p.w, p.h, p.n_bytes)) { atomicOr(&p.status[b.seg], ST_DESC); return; }
    const size_t plane = (size_t)p.w * p.h, at = ((size_t)(b.seg - p.t0) * 3 + b.comp) * plane;
    t1_block(b, p.bytes, p.plane_a + at, reinterpret_cast<uint16_t*>(p.plane_b) + at, p.w, tab, cx + threadIdx.x, T1_NT);
}

__global__ __launch_bounds__(JK_NT) void j2k_idwt_kernel(J2kParams p) {
    const int i = p.t0 + (int)blockIdx.y, c = (int)blockIdx.x;
    if (p.status[i]) return;                                                   // (uniform across the workgroup)
    __shared__ Seg s;                                                          // (half_step is indexed by the sample's sub-band)
    if (threadIdx.x < SEG_I32) reinterpret_cast<int32_t*>(&s)[threadIdx.x] = reinterpret_cast<const int32_t*>(p.seg + i)[threadIdx.x];
    __syncthreads();
    const size_t plane = (size_t)p.w * p.h, at = ((size_t)blockIdx.y * 3 + c) * plane;
    int32_t* A = p.plane_a + at;
    int32_t* B = p.plane_b + at;
    for (int k = threadIdx.x; k < s.w * s.h; k += JK_NT) {
        const int y = k / s.w, x = k - y * s.w;
        A[k] = dequant_sample(A[k], s, x, y);
    }
    for (int r = 1; r <= s.levels; ++r) {
        const int rw = ceil_shift(s.w, s.levels - r), rh = ceil_shift(s.h, s.levels - r);
        __syncthreads();
        for (int y = threadIdx.x; y < rh; y += JK_NT) synth_row(A, B, p.w, rw, y, s.reversible);
        __syncthreads();
        for (int x = threadIdx.x; x < rw; x += JK_NT) synth_col(B, A, p.w, rh, x, s.reversible);
    }
}

__global__ __launch_bounds__(JK_NT) void j2k_store_kernel(J2kParams p) {
    const int i = p.t0 + (int)blockIdx.y;
    if (p.status[i]) return;
    const int k = (int)(blockIdx.x * JK_NT + threadIdx.x);
    if (k >= p.w * p.h) return;
    const int y = k / p.w, x = k - y * p.w;
    const int px = p.place[2 * i], py = p.place[2 * i + 1];
    Window win;
    if (!place_window(px, py, p.w, p.h, p.H, p.W, p.clip, win)) return;
    if (x < win.x0 || x >= win.x1 || y < win.y0 || y >= win.y1) return;
    const size_t plane = (size_t)p.w * p.h;
    const int32_t* A = p.plane_a + (size_t)blockIdx.y * 3 * plane + k;
    uint8_t rgb[3];
    finish_pixel(A[0], A[plane], A[2 * plane], p.seg[i], p.ycc, rgb);
    uint8_t* o = p.canvas + ((size_t)(py + y) * p.W + (size_t)(px + x)) * 3;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// segments a round, by default: 256 tiles of 256 px hold about 19 000 code blocks -- one wave on every CU -- in 403 MB of scratch
constexpr int J2K_ROUND = 256;

size_t seg_scratch_bytes(int w, int h) { return (size_t)w * h * 3 * 4 * 2; }

size_t j2k_canvas_scratch_bytes(int n, int w, int h) {
    if (n <= 0 || w <= 0 || h <= 0) return 0;
    return round_cap(n, J2K_ROUND) * seg_scratch_bytes(w, h);
}

}  // namespace

extern "C" {

size_t bq_j2k_canvas_scratch_bytes(int n, int seg_w, int seg_h) { return j2k_canvas_scratch_bytes(n, seg_w, seg_h); }

int bq_j2k_decode_canvas(bq_ctx* c, const void* d_seg, int n, const void* d_blocks, int64_t n_blocks, const uint8_t* d_bytes, size_t n_bytes,
                         int seg_w, int seg_h, int ycc, const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0,
                         int clip_x1, int clip_y1, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || n_blocks < 0 || n_blocks > (1ll << 30) || seg_w <= 0 || seg_w > MAX_SIDE || seg_h <= 0 || seg_h > MAX_SIDE ||
        !bqcanvas::canvas_args_ok(H, W))
        return fail(c, BQ_ERR_ARG, "bq_j2k_decode_canvas: bad argument (need 0 < seg_w, seg_h <= 512 and 0 < H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_seg || (n_blocks && (!d_blocks || !d_bytes)) || !d_place || !d_canvas || !d_status || !d_scratch || ((uintptr_t)d_seg & 3) ||
        ((uintptr_t)d_blocks & 3) || ((uintptr_t)d_place & 3) || ((uintptr_t)d_scratch & 3))
        return fail(c, BQ_ERR_ARG, "bq_j2k_decode_canvas: bad argument");
    const size_t per = seg_scratch_bytes(seg_w, seg_h);
    const size_t m = round_items(scratch_bytes, per, 1);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_j2k_decode_canvas: scratch smaller than one segment's (bq_j2k_canvas_scratch_bytes(1, seg_w, seg_h))");
    hipStream_t s = (hipStream_t)stream;
    J2kParams p;
    p.seg = reinterpret_cast<const Seg*>(d_seg); p.blocks = reinterpret_cast<const Block*>(d_blocks); p.bytes = d_bytes;
    p.place = d_place; p.status = d_status; p.canvas = d_canvas;
    p.n_bytes = n_bytes; p.n_blocks = n_blocks; p.n = n; p.w = seg_w; p.h = seg_h; p.H = H; p.W = W; p.ycc = ycc ? 1 : 0;
    p.clip[0] = clip_x0; p.clip[1] = clip_y0; p.clip[2] = clip_x1; p.clip[3] = clip_y1;
    const double px = (double)seg_w * seg_h * 3.0;
    for (long long t0 = 0; t0 < n; t0 += (long long)m) {
        const int cnt = (int)(n - t0 < (long long)m ? n - t0 : (long long)m);
        p.t0 = (int)t0; p.cnt = cnt;
        p.plane_a = reinterpret_cast<int32_t*>(d_scratch);
        p.plane_b = p.plane_a + (size_t)cnt * 3 * seg_w * seg_h;
        {
            ProfScope ps(c, s, "j2k_t1", 0.0, (double)cnt * px * 6.0);
            HIPCHK(c, hipMemsetAsync(d_scratch, 0, (size_t)cnt * per, s));
            hipLaunchKernelGGL(j2k_status_kernel, dim3((cnt + JK_NT - 1) / JK_NT), dim3(JK_NT), 0, s, p);
            if (n_blocks) hipLaunchKernelGGL(j2k_t1_kernel, dim3((unsigned)((n_blocks + T1_NT - 1) / T1_NT)), dim3(T1_NT), 0, s, p);
        }
        {
            ProfScope ps(c, s, "j2k_idwt", 0.0, (double)cnt * px * 8.0);
            hipLaunchKernelGGL(j2k_idwt_kernel, dim3(3, cnt), dim3(JK_NT), 0, s, p);
        }
        {
            ProfScope ps(c, s, "j2k_store", 0.0, (double)cnt * px * 5.0);
            hipLaunchKernelGGL(j2k_store_kernel, dim3((seg_w * seg_h + JK_NT - 1) / JK_NT, cnt), dim3(JK_NT), 0, s, p);
        }
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
