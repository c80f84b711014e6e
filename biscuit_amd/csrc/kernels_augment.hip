// kernels_augment.hip -- the training augmentation 'xyrjb' on the device (bq_augment): the routines of augment_device.h, which
// libbiscuit_io runs unchanged on the CPU (bqio_augment), behind four stages of kernels.  A tile's four parameter bytes live on the
// device, so which stages a tile takes is decided there: the grids cover every tile of the round, and the workgroups of a tile
// that skips a stage leave at once (the choice is the same for a whole workgroup: blockIdx.y is the tile).
//
//   jpeg     quality > 0: one thread per 8 x 8 block of the scan (MCU order, dummy blocks skipped): the encoder's coefficients
//            (colour, edges, 4:2:0, fDCT, quantisation), times the quantiser, the islow IDCT, 64 samples to the decoder's plane
//            layout in scratch.  The tile's two quantiser tables are made from its quality in LDS (quant_entry).
//   place    four output pixels per thread over the flattened NHWC output, three dword stores: the inverse dihedral map, then
//            pixel_rgb over the planes (fancy upsampling, colour) or the input tile's pixel.  Every tile is written here.
//   blur_h   blur > 0: one thread per pixel, the row pass over the placed tile in d_out -> uint16 [px][px][3] in scratch.
//   blur_v   blur > 0: one thread per pixel, the column pass over those -> d_out.
//
// A tile costs tile_scratch_bytes(px) of scratch (the planes, 554 496 bytes at 299 px, and the row pass, 536 416); a call works in
// rounds of as many tiles as the caller's scratch holds.  The weight tables (128 bytes) and the base quantisers (128 bytes) are
// kernel arguments: nothing is allocated or copied, and nothing waits for the device.  No atomics: the one status bit a kernel
// sets is stored, and every thread that stores it stores the same word.
#include "augment_device.h"
#include "bq_ctx.h"

namespace {

constexpr int NT = 256;
constexpr int AUG_ROUND = 256;           // tiles per round that bq_augment_scratch_bytes asks scratch for

struct AugParams {
    int px;
    bqje::Geom Ge;
    bqjd::Geom Gd;
    const uint8_t* tiles;                // of the CALL's first tile
    const uint8_t* params;               // the CALL's [n][4]
    uint8_t* out;                        // of the CALL's first tile
    int* status;                         // the CALL's [n]
    uint8_t* planes;  size_t plane_stride;       // [m][plane_stride] bytes
    uint16_t* rows;   size_t row_stride;         // [m][row_stride] uint16
    long long t0;                        // the round's first tile within the call
    int n;                               // tiles of this round
    long long p0, p1;                    // the round's pixels within the call's flattened output
};

__device__ __forceinline__ size_t tile_bytes(const AugParams& p) { return (size_t)p.px * p.px * 3; }

__global__ void __launch_bounds__(NT) augment_jpeg_kernel(const AugParams p, const bqaug::QuantBase QB) {
    __shared__ uint16_t sq[2][64];
    const int i = blockIdx.y;
    const uint8_t* prm = p.params + 4 * (size_t)(p.t0 + i);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !bqaug::valid_params(prm)) p.status[p.t0 + i] = bqaug::ST_PARAM;
    const bqaug::Params a = bqaug::params_of(prm);
    if (a.quality == 0) return;
    if (threadIdx.x < 128) sq[threadIdx.x >> 6][threadIdx.x & 63] = bqaug::quant_entry(QB.b[threadIdx.x >> 6][threadIdx.x & 63], a.quality);
    __syncthreads();
    const uint32_t b = blockIdx.x * NT + threadIdx.x;
    if (b >= p.Ge.nblk) return;
    const bqje::BlockPos P = bqje::block_pos(p.Ge, b);
    if (P.dummy) return;
    const uint8_t* tile = p.tiles + (size_t)(p.t0 + i) * tile_bytes(p);
    if (!bqaug::jpeg_block(tile, p.Ge, p.Gd, P, sq[P.comp ? 1 : 0], p.planes + (size_t)i * p.plane_stride))
        p.status[p.t0 + i] = bqaug::ST_RANGE;
}

// The group of four flat pixels that starts at pixel a = 4 q, b[12] their bytes, to o = base + 12 q: three dword stores where
// the whole group lies in [P0, P1) (`all`) and o is aligned, otherwise byte stores of the pixels that do lie in it.
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

__global__ void __launch_bounds__(NT) augment_place_kernel(const AugParams p) {
    const long long q = p.p0 / 4 + (long long)blockIdx.x * NT + threadIdx.x;        // group of four pixels of the call's output
    const long long a = q * 4;
    if (a >= p.p1) return;
    const int px = p.px;
    const long long ppt = (long long)px * px;
    long long tile = a / ppt;
    const int rem = (int)(a - tile * ppt);
    int y = rem / px, x = rem - y * px;
    uint8_t b[12];
    bool all = true;
    long long cur = -1;
    bqaug::Params prm{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long P = a + j;
        const bool valid = P >= p.p0 && P < p.p1;
        all &= valid;
        b[3 * j] = b[3 * j + 1] = b[3 * j + 2] = 0;
        if (valid) {
            if (tile != cur) {
                cur = tile;
                prm = bqaug::params_of(p.params + 4 * (size_t)tile);
            }
            bqaug::placed_pixel(p.tiles + (size_t)tile * tile_bytes(p), p.planes + (size_t)(tile - p.t0) * p.plane_stride, p.Gd, px, prm,
                                y, x, b + 3 * j);
        }
        if (++x == px) { x = 0; if (++y == px) { y = 0; ++tile; } }
    }
    store_group(p.out + 12 * q, b, all, a, p.p0, p.p1);
}

__global__ void __launch_bounds__(NT) augment_blur_h_kernel(const AugParams p, const bqaug::BlurTables BT) {
    const int i = blockIdx.y;
    const bqaug::Params a = bqaug::params_of(p.params + 4 * (size_t)(p.t0 + i));
    if (a.blur == 0) return;
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= p.px * p.px) return;
    const int y = idx / p.px, x = idx - y * p.px;
    uint16_t h[3];
    bqaug::blur_row_at(p.out + (size_t)(p.t0 + i) * tile_bytes(p), p.px, y, x, BT.w[a.blur - 1], BT.r[a.blur - 1], h);
    uint16_t* o = p.rows + (size_t)i * p.row_stride + (size_t)idx * 3;
    o[0] = h[0]; o[1] = h[1]; o[2] = h[2];
}

__global__ void __launch_bounds__(NT) augment_blur_v_kernel(const AugParams p, const bqaug::BlurTables BT) {
    const int i = blockIdx.y;
    const bqaug::Params a = bqaug::params_of(p.params + 4 * (size_t)(p.t0 + i));
    if (a.blur == 0) return;
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= p.px * p.px) return;
    const int y = idx / p.px, x = idx - y * p.px;
    uint8_t v[3];
    bqaug::blur_col_at(p.rows + (size_t)i * p.row_stride, p.px, y, x, BT.w[a.blur - 1], BT.r[a.blur - 1], v);
    uint8_t* o = p.out + (size_t)(p.t0 + i) * tile_bytes(p) + (size_t)idx * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

}  // namespace

static size_t augment_scratch_bytes(int n, int px) {
    if (n <= 0 || !bqaug::valid_px(px)) return 0;
    return round_cap(n, AUG_ROUND) * bqaug::tile_scratch_bytes(px);
}

enum { AUG_JPEG = 0, AUG_PLACE = 1, AUG_BLUR_H = 2, AUG_BLUR_V = 3, AUG_STAGES = 4 };
// One stage of one round, so that bq_augment can time each: tiles [t0, t0 + cnt) of the call, in a scratch laid out for m tiles (cnt <= m).
static int launch_augment_stage(int stage, const uint8_t* d_tiles, long long t0, int cnt, int m, int px, const uint8_t* d_params,
                                uint8_t* d_out, int* d_status, void* d_scratch, hipStream_t s) {
    AugParams p;
    p.px = px; p.Ge = bqaug::encode_geom(px); p.Gd = bqaug::decode_geom(px);
    p.tiles = d_tiles; p.params = d_params; p.out = d_out; p.status = d_status;
    p.planes = reinterpret_cast<uint8_t*>(d_scratch);
    p.plane_stride = bqaug::plane_bytes(px);
    p.rows = reinterpret_cast<uint16_t*>(p.planes + (size_t)m * p.plane_stride);
    p.row_stride = bqaug::row_bytes(px) / 2;
    p.t0 = t0; p.n = cnt;
    const long long ppt = (long long)px * px;
    p.p0 = t0 * ppt; p.p1 = (t0 + cnt) * ppt;
    const dim3 per_pixel((unsigned)((ppt + NT - 1) / NT), cnt);
    switch (stage) {
        case AUG_JPEG:
            if (const hipError_t e = hipMemsetAsync(d_status + t0, 0, (size_t)cnt * sizeof(int), s)) return (int)e;
            hipLaunchKernelGGL(augment_jpeg_kernel, dim3((p.Ge.nblk + NT - 1) / NT, cnt), dim3(NT), 0, s, p, bqaug::quant_base());
            break;
        case AUG_PLACE: {
            const long long groups = (p.p1 + 3) / 4 - p.p0 / 4;
            hipLaunchKernelGGL(augment_place_kernel, dim3((unsigned)((groups + NT - 1) / NT)), dim3(NT), 0, s, p);
            break;
        }
        case AUG_BLUR_H:
        case AUG_BLUR_V: {
            bqaug::BlurTables BT;
            bqaug::build_blur_tables(BT);
            if (stage == AUG_BLUR_H) hipLaunchKernelGGL(augment_blur_h_kernel, per_pixel, dim3(NT), 0, s, p, BT);
            else hipLaunchKernelGGL(augment_blur_v_kernel, per_pixel, dim3(NT), 0, s, p, BT);
            break;
        }
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" {

size_t bq_augment_scratch_bytes(int n, int px) { return augment_scratch_bytes(n, px); }

int bq_augment(bq_ctx* c, const uint8_t* d_tiles, int n, int px, const uint8_t* d_params, uint8_t* d_out, int32_t* d_status,
               void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0) return fail(c, BQ_ERR_ARG, "bq_augment: bad argument");
    if (!bqaug::valid_px(px)) return fail(c, BQ_ERR_ARG, "bq_augment: need 8 <= px <= 4096");
    if (n == 0) return BQ_OK;
    if (!d_tiles || !d_params || !d_out || !d_status || !d_scratch || ((uintptr_t)d_status & 3) || ((uintptr_t)d_scratch & 15))
        return fail(c, BQ_ERR_ARG, "bq_augment: bad argument (null pointer, d_status not 4-byte or d_scratch not 16-byte aligned)");
    const uintptr_t total = (uintptr_t)n * px * px * 3, in0 = (uintptr_t)d_tiles, out0 = (uintptr_t)d_out;
    if (out0 < in0 + total && in0 < out0 + total) return fail(c, BQ_ERR_ARG, "bq_augment: d_out overlaps d_tiles");
    const int m = (int)round_items(scratch_bytes, bqaug::tile_scratch_bytes(px), 1);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_augment: scratch smaller than one tile's (bq_augment_scratch_bytes(1, px))");
    hipStream_t s = (hipStream_t)stream;
    static const char* const kStage[AUG_STAGES] = {"augment_jpeg", "augment_place", "augment_blur_h", "augment_blur_v"};
    for (long long t0 = 0; t0 < n; t0 += m) {
        const int cnt = (int)(n - t0 < m ? n - t0 : m);
        for (int stage = 0; stage < AUG_STAGES; ++stage) {
            ProfScope ps(c, s, kStage[stage], 0.0, (double)cnt * px * px * 3.0 * 2.0);
            const int e = launch_augment_stage(stage, d_tiles, t0, cnt, m, px, d_params, d_out, d_status, d_scratch, s);
            if (e) return fail(c, BQ_ERR_HIP, std::string("augment launch: ") + hipGetErrorString((hipError_t)e));
        }
    }
    return BQ_OK;
}

}  // extern "C"
