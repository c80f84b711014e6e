// kernels_lzw.hip -- a TIFF page's LZW tiles (compression 5) decoded on the device into a slide canvas (bq_lzw_decode_canvas;
// DESIGN.md "Heatmap input", LZW tiles).  The host only packs the segments (numpy: each at a multiple of 16, zeros behind it);
// the stream is the statement of lzw_device.h, which bqio_lzw_decode_canvas runs on the CPU and which the result equals byte
// for byte and status for status.  Two launches a round:
//   lzw_decode   a wave per segment.  The code chain is one dependent sequence, parsed wave-uniformly by next(); what the wave
//                shares is the EMISSION: a string is a run of bytes already in the segment's output (scratch), copied 64 bytes a
//                step, lane k byte k.  The table -- one start offset per entry, 16 388 bytes -- is in LDS, private to the wave.
//                A copy may read bytes other lanes stored for an earlier code: a workgroup barrier with its release / acquire
//                fences stands between such stores and the read (`dirty`); within one copy every source byte is older than the
//                copy, except the last byte of a KwKwK string, which is the first byte the copy writes and is read from there.
//                The unpredicted bytes go to scratch; the status is written last.
//   lzw_place    a wave per segment row: predictor 2 undone -- the per-sample running sum modulo 256, four pixels a lane, a
//                wave scan of the lanes' sums, a carry between chunks of 256 pixels -- and the window place_window gives stored
//                into the canvas in the groups of four flat canvas pixels bq_jpeg_decode_canvas documents (three aligned dword
//                stores inside the row's run, byte stores at its ends).  Reads d_status: a refused segment writes nothing, and
//                only bytes lzw_decode wrote for a status-0 segment are read.
// Scratch per segment: seg_w * seg_h * 3 bytes rounded up to 16.
#include "bq_ctx.h"
#include "lzw_device.h"

namespace {

using namespace bqlzw;

constexpr int LZ_NT = 64;            // one wave

struct LzwParams {
    const uint8_t* data;
    const Desc* desc;                // the call's descriptors
    const int32_t* place;
    int32_t* status;                 // the call's status array
    uint8_t* scratch;                // [round segment][per]
    uint8_t* canvas;
    size_t per;
    uint32_t need;
    int t0, w, h, H, W, predictor;
    int32_t clip[4];
};

// The stream as a wave reads it: 256 bytes in the wave's registers, lane k the big-endian dword at byte base + 4 k, refilled with
// one load whenever a code reaches into the last dword; a code is cut out of two neighbouring dwords, fetched from their lanes
// (the index is wave-uniform).  A dword is loaded only if it begins inside the segment's length rounded up to 16 -- the bytes
// the packing guarantees -- and a code's bits lie inside len (next() has checked), so what stands behind len never shows.
struct WaveSource {
    const uint8_t* raw; uint32_t len, lane;
    uint32_t base = 0xFFFFFFFFu;     // byte offset of lane 0's dword (a multiple of 4); none loaded yet
    uint32_t word = 0;
    __device__ uint32_t get(uint32_t bit, int w) {
        uint32_t k = (bit >> 5) - (base >> 2);                       // (wraps to something large while nothing is loaded)
        if (base == 0xFFFFFFFFu || k >= LZ_NT - 1) {
            base = bit >> 5 << 2;
            const uint32_t at = base + 4 * lane;
            word = at < ((len + 15u) & ~15u) ? __builtin_bswap32(*reinterpret_cast<const uint32_t*>(raw + at)) : 0u;
            k = 0;
        }
        const uint64_t v = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)word, (int)k) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane((int)word, (int)k + 1);
        return (uint32_t)(v >> (64 - (int)(bit & 31) - w)) & ((1u << w) - 1);
    }
};

__global__ __launch_bounds__(LZ_NT) void lzw_decode_kernel(LzwParams p) {
    __shared__ uint32_t start[TABLE + 1];
    const int i = p.t0 + (int)blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const Desc d = p.desc[i];
    int st = ST_DESC;
    if (desc_ok(d)) {
        const uint8_t* raw = p.data + d.off;
        uint8_t* out = p.scratch + (size_t)blockIdx.x * p.per;
        st = head_status(raw, d.len);
        if (!st) {
            State s;
            Step e;
            WaveSource src{raw, d.len, lane};
            bool dirty = false;      // stores since the last barrier (wave-uniform, like everything next() decides)
            while (next(s, src, d.len, p.need, start, e)) {
                if (e.kind == LITERAL) {
                    if (lane == 0) out[e.dst] = e.lit;
                } else {
                    if (dirty) __syncthreads();
                    for (uint32_t k = lane; k < e.cnt; k += LZ_NT)
                        out[e.dst + k] = out[e.kind == KWKWK && k == e.len - 1 ? e.src : e.src + k];
                }
                dirty = true;
            }
            st = s.status;
        }
    }
    if (lane == 0) p.status[i] = st;
}

// The group of four flat pixels that starts at pixel a, b[12] their bytes, to o: three dword stores where the whole group lies in
// the row's run [P0, P1) (`all`) and o is aligned, otherwise byte stores of the pixels that do lie in it.
__device__ __forceinline__ void store_group(uint8_t* o, const uint8_t (&b)[12], bool all, long long a, long long P0, long long P1) {
    if (all && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long P = a + j;
            if (P >= P0 && P < P1) { o[3 * j] = b[3 * j]; o[3 * j + 1] = b[3 * j + 1]; o[3 * j + 2] = b[3 * j + 2]; }
        }
    }
}

// inclusive scan across the wave
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < LZ_NT; d <<= 1) {
        const int a = __shfl_up(v, d, LZ_NT);
        if (lane >= d) v += a;
    }
    return v;
}

// blockIdx.x = the row of the segment's window, blockIdx.y = the segment of the round
__global__ __launch_bounds__(LZ_NT) void lzw_place_kernel(LzwParams p) {
    const int i = p.t0 + (int)blockIdx.y;
    if (p.status[i]) return;
    const int sx = p.place[2 * i], sy = p.place[2 * i + 1];
    Window win;
    if (!place_window(sx, sy, p.w, p.h, p.H, p.W, p.clip, win)) return;
    const int y = win.y0 + (int)blockIdx.x;
    if (y >= win.y1) return;
    const int lane = threadIdx.x;
    const uint8_t* row = p.scratch + (size_t)blockIdx.y * p.per + (size_t)y * p.w * 3;
    // flat canvas pixel of the row's segment pixel 0 (negative only left of the canvas's first pixel), and the window's run
    const long long base = (long long)(sy + y) * p.W + sx;
    const long long P0 = base + win.x0, P1 = base + win.x1;
    // groups of four flat canvas pixels from the one that holds segment pixel 0 (predictor 2 sums from there) or the window's first
    const long long first = p.predictor == 2 ? base : P0;
    const long long q0 = (first >= 0 ? first : first - 3) / 4;
    int carry[3] = {0, 0, 0};
    for (long long q = q0 + lane; 4 * (q - lane) < P1; q += LZ_NT) {
        const long long a = 4 * q;
        int v[4][3];
        int sum[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long x = a + j - base;
            const bool in = x >= (p.predictor == 2 ? 0 : win.x0) && x < win.x1;       // (what lies right of the window is not needed)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[j][c] = in ? (int)row[3 * x + c] : 0;
                sum[c] += v[j][c];
                if (p.predictor == 2) v[j][c] = sum[c];
            }
        }
        if (p.predictor == 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int incl = wave_scan(sum[c], lane);
                const int before = carry[c] + incl - sum[c];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j][c] += before;
                carry[c] += __shfl(incl, LZ_NT - 1, LZ_NT);
            }
        }
        uint8_t b[12];
        bool all = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            all &= a + j >= P0 && a + j < P1;
#pragma unroll
            for (int c = 0; c < 3; ++c) b[3 * j + c] = (uint8_t)(v[j][c] & 255);
        }
        if (a + 4 > P0 && a < P1) store_group(p.canvas + 3 * a, b, all, a, P0, P1);
    }
}

constexpr int LZW_ROUND = 1024;      // segments a round, by default: 201 MB of scratch at 256 x 256

size_t seg_scratch_bytes(int w, int h) { return ((size_t)w * h * 3 + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

size_t bq_lzw_canvas_scratch_bytes(int n, int seg_w, int seg_h) {
    if (n <= 0 || !geom_ok(seg_h, seg_w)) return 0;
    return round_cap(n, LZW_ROUND) * seg_scratch_bytes(seg_w, seg_h);
}

int bq_lzw_decode_canvas(bq_ctx* c, const uint8_t* d_data, const void* d_desc, int n, int seg_w, int seg_h, int predictor,
                         const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0, int clip_x1, int clip_y1,
                         int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || !geom_ok(seg_h, seg_w) || (predictor != 1 && predictor != 2) || !bqcanvas::canvas_args_ok(H, W))
        return fail(c, BQ_ERR_ARG, "bq_lzw_decode_canvas: bad argument (need 0 < seg_w, seg_h <= 1024, predictor 1 or 2 and 0 < H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_data || !d_desc || !d_place || !d_canvas || !d_status || !d_scratch || ((uintptr_t)d_data & 15) || ((uintptr_t)d_desc & 3) ||
        ((uintptr_t)d_place & 3) || ((uintptr_t)d_status & 3))
        return fail(c, BQ_ERR_ARG, "bq_lzw_decode_canvas: bad argument (null pointer, d_data not 16-byte aligned)");
    const size_t per = seg_scratch_bytes(seg_w, seg_h);
    const size_t m = round_items(scratch_bytes, per, 1);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_lzw_decode_canvas: scratch smaller than one segment's (bq_lzw_canvas_scratch_bytes(1, seg_w, seg_h))");
    hipStream_t s = (hipStream_t)stream;
    LzwParams p;
    p.data = d_data; p.desc = reinterpret_cast<const Desc*>(d_desc); p.place = d_place; p.status = d_status;
    p.scratch = reinterpret_cast<uint8_t*>(d_scratch); p.canvas = d_canvas; p.per = per;
    p.need = (uint32_t)seg_w * (uint32_t)seg_h * 3u;
    p.w = seg_w; p.h = seg_h; p.H = H; p.W = W; p.predictor = predictor;
    p.clip[0] = clip_x0; p.clip[1] = clip_y0; p.clip[2] = clip_x1; p.clip[3] = clip_y1;
    const double px = (double)seg_w * seg_h * 3.0;
    for (long long t0 = 0; t0 < n; t0 += (long long)m) {
        const int cnt = (int)(n - t0 < (long long)m ? n - t0 : (long long)m);
        p.t0 = (int)t0;
        {
            ProfScope ps(c, s, "lzw_decode", 0.0, (double)cnt * px * 2.0);
            hipLaunchKernelGGL(lzw_decode_kernel, dim3(cnt), dim3(LZ_NT), 0, s, p);
        }
        {
            ProfScope ps(c, s, "lzw_place", 0.0, (double)cnt * px * 2.0);
            hipLaunchKernelGGL(lzw_place_kernel, dim3(seg_h, cnt), dim3(LZ_NT), 0, s, p);
        }
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

}  // extern "C"
