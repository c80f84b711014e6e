// kernels_jpeg_encode.hip -- tiles encoded as baseline JPEG on the device (bq_jpeg_encode): the routines of jpeg_encode_device.h,
// which libbiscuit_io runs unchanged on the CPU (bqio_jpeg_encode), behind four stages of kernels.
//
//   pixel   one thread per 8 x 8 block of the scan (MCU order): colour conversion, edge replication and -- for a chroma block at
//           4:2:0 -- the 2 x 2 average straight from the tile, the islow fDCT in registers, quantisation, 64 int16 coefficients
//           in zigzag order to scratch.  Every block reads its own samples: a component's conversions are done exactly once
//           (a luma thread converts 64 pixels to Y only, a chroma thread 256 pixels to its one component), so staging an MCU row
//           in LDS would save loads that hit the cache, not arithmetic (DESIGN.md "Tile extraction"; profiles/extract.txt for its share).
//   size    one thread per block: the bit length of its code from its coefficients and the DC of the previous block of its
//           component (prev_block / dummy_src of the header: a neighbour, not a walk); then one workgroup per tile turns the
//           lengths into bit offsets (exclusive scan) and leaves the tile's unstuffed length.
//   pack    one thread per block: its bits at its offset into the tile's zeroed unstuffed buffer, 32-bit words in the stream's
//           byte order; a word shared with a neighbouring block is merged with atomicOr, a word a block fills alone is stored.
//           The scan's last block pads the last byte with ones.
//   stuff   one workgroup per tile counts the 0xFF bytes per 32-byte chunk and scans the counts (each chunk's shift, the file's
//           exact length); one workgroup scans the lengths into d_off behind the previous round's last offset; a copy kernel
//           writes header + stuffed segment + EOI at d_off[i], or sets status bit 1 when the file would end beyond `cap`.
//
// A tile costs Layout::per_tile() bytes of scratch (889 KB at 299 px / 4:2:0, of which 536 KB are the worst-case unstuffed code); a call
// works in rounds of as many tiles as the caller's scratch holds.  The tables (2.4 KB) and the header (623 bytes) are kernel
// arguments: nothing is allocated or copied, and nothing waits for the device.
#include "block_scan.h"
#include "bq_ctx.h"
#include "jpeg_encode_device.h"

namespace {

constexpr int NT = 256;
constexpr int ENC_ROUND = 256;           // tiles per round that bq_jpeg_encode_scratch_bytes asks scratch for
constexpr int COPY_BLOCKS = 256;         // most workgroups per tile of the copy kernel (it strides over the chunks)

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Scratch of a round of m tiles: five arrays, each [m][its per-tile size], every per-tile size a multiple of 16 bytes.
struct Layout {
    size_t coef, bits, ubuf, ffpre, meta;            // per tile, bytes
    size_t per_tile() const { return coef + bits + ubuf + ffpre + meta; }
};

Layout layout_of(const bqje::Geom& G) {
    Layout L;
    L.coef = (size_t)G.nblk * 128;
    L.bits = align16(((size_t)G.nblk + 1) * 4);
    L.ubuf = (bqje::unstuffed_bytes(G) + 31) & ~(size_t)31;        // whole chunks: the 0xFF count reads words
    L.ffpre = align16((L.ubuf / bqje::STUFF_CHUNK) * 4);
    L.meta = 16;                                                   // uint32 unstuffed length, int64 file length
    return L;
}

struct EncParams {
    bqje::Geom G;
    const uint8_t* tiles;                // of the round's first tile
    int16_t* coef;
    uint32_t* bits;  size_t bits_stride; // in words
    uint8_t* ubuf;   size_t ubuf_stride; // in bytes
    uint32_t* ffpre; size_t ffpre_stride;
    uint8_t* meta;                       // [m][16]
    int n;                               // tiles of this round
    long long t0;                        // the round's first tile within the call
    uint8_t* out;
    long long cap;
    long long* off;                      // the CALL's [n + 1]
    int* status;                         // of the round's first tile
};

__device__ uint32_t& meta_ulen(const EncParams& p, int i) { return *reinterpret_cast<uint32_t*>(p.meta + (size_t)i * 16); }
__device__ long long& meta_flen(const EncParams& p, int i) { return *reinterpret_cast<long long*>(p.meta + (size_t)i * 16 + 8); }

__global__ void __launch_bounds__(NT) jenc_pixel_kernel(const EncParams p, const bqje::Tables T) {
    // Both quantiser tables in LDS: which one a thread divides by depends on its block, and 64 + 64 entries held in SGPRs for a
    // per-lane choice do not fit beside the rest (they spilled).
    __shared__ uint16_t sq[2][64];
    if (threadIdx.x < 64) reinterpret_cast<uint32_t*>(&sq[0][0])[threadIdx.x] = reinterpret_cast<const uint32_t*>(&T.q[0][0])[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.y;
    const uint32_t b = blockIdx.x * NT + threadIdx.x;
    if (b >= p.G.nblk) return;
    const bqje::BlockPos P = bqje::block_pos(p.G, b);
    const uint8_t* tile = p.tiles + (size_t)i * p.G.px * p.G.px * 3;
    bqje::block_coefs(tile, p.G, P, sq[P.comp ? 1 : 0], p.coef + ((size_t)i * p.G.nblk + b) * 64);
}

__global__ void __launch_bounds__(NT) jenc_size_kernel(const EncParams p, const bqje::Tables T) {
    const int i = blockIdx.y;
    const uint32_t b = blockIdx.x * NT + threadIdx.x;
    if (b >= p.G.nblk) return;
    p.bits[(size_t)i * p.bits_stride + b] = bqje::block_bits(p.coef + (size_t)i * p.G.nblk * 64, p.G, T, b);
}

// lengths -> bit offsets, in place; one workgroup per tile
__global__ void __launch_bounds__(NT) jenc_scan_kernel(const EncParams p) {
    __shared__ uint32_t sh[NT];
    const int i = blockIdx.x;
    uint32_t* bits = p.bits + (size_t)i * p.bits_stride;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < p.G.nblk; base += NT) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < p.G.nblk ? bits[b] : 0;
        const uint32_t incl = block_scan<NT>(v, sh);
        if (b < p.G.nblk) bits[b] = carry + incl - v;
        carry += sh[NT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) meta_ulen(p, i) = (carry + 7) / 8;
}

__global__ void __launch_bounds__(NT) jenc_pack_kernel(const EncParams p, const bqje::Tables T) {
    const int i = blockIdx.y;
    const uint32_t b = blockIdx.x * NT + threadIdx.x;
    if (b >= p.G.nblk) return;
    bqje::block_pack(p.coef + (size_t)i * p.G.nblk * 64, p.G, T, b, p.bits[(size_t)i * p.bits_stride + b],
                     reinterpret_cast<uint32_t*>(p.ubuf + (size_t)i * p.ubuf_stride));
}

__device__ uint32_t ff_in_word(uint32_t w) {
    return (uint32_t)((w & 0xFF) == 0xFF) + (uint32_t)((w & 0xFF00) == 0xFF00) + (uint32_t)((w & 0xFF0000) == 0xFF0000) + (uint32_t)(w >= 0xFF000000u);
}

// per chunk: the 0xFF bytes in front of it; per tile: the file's length.  Bytes behind the unstuffed length are zero (the buffer
// was zeroed and nothing is packed there), so whole chunks are counted.
__global__ void __launch_bounds__(NT) jenc_ff_kernel(const EncParams p) {
    __shared__ uint32_t sh[NT];
    const int i = blockIdx.x;
    const uint32_t ulen = meta_ulen(p, i);
    const uint32_t nch = (ulen + bqje::STUFF_CHUNK - 1) / bqje::STUFF_CHUNK;       // <= ubuf_stride / STUFF_CHUNK
    const uint4* u = reinterpret_cast<const uint4*>(p.ubuf + (size_t)i * p.ubuf_stride);
    uint32_t* pre = p.ffpre + (size_t)i * p.ffpre_stride;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nch; base += NT) {
        const uint32_t c = base + threadIdx.x;
        uint32_t v = 0;
        if (c < nch) {
            const uint4 a = u[2 * (size_t)c], d = u[2 * (size_t)c + 1];
            v = ff_in_word(a.x) + ff_in_word(a.y) + ff_in_word(a.z) + ff_in_word(a.w) + ff_in_word(d.x) + ff_in_word(d.y) +
                ff_in_word(d.z) + ff_in_word(d.w);
        }
        const uint32_t incl = block_scan<NT>(v, sh);
        if (c < nch) pre[c] = carry + incl - v;
        carry += sh[NT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) meta_flen(p, i) = (long long)bqje::HEADER_BYTES + ulen + carry + 2;
}

// file lengths -> d_off[t0 + 1 .. t0 + n], continuing from d_off[t0]; one workgroup
__global__ void __launch_bounds__(NT) jenc_offsets_kernel(const EncParams p) {
    __shared__ long long sh[NT];
    offsets_scan<NT>(p.off, p.t0, p.n, [&](int i) { return meta_flen(p, i); }, sh);
}

// header + stuffed segment + EOI of tile i at out + off[i], when it ends inside `cap`
__global__ void __launch_bounds__(NT) jenc_copy_kernel(const EncParams p, const bqje::Header H) {
    const int i = blockIdx.y;
    const long long start = p.off[p.t0 + i], end = p.off[p.t0 + i + 1];
    const bool fits = end <= p.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.status[i] = fits ? bqje::ST_OK : bqje::ST_CAP;
    if (!fits) return;
    uint8_t* o = p.out + start;
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < bqje::HEADER_BYTES; k += NT) o[k] = H.b[k];
        if (threadIdx.x == 0) { p.out[end - 2] = 0xFF; p.out[end - 1] = 0xD9; }
    }
    const uint32_t ulen = meta_ulen(p, i);
    const uint32_t nch = (ulen + bqje::STUFF_CHUNK - 1) / bqje::STUFF_CHUNK;
    const uint8_t* u = p.ubuf + (size_t)i * p.ubuf_stride;
    const uint32_t* pre = p.ffpre + (size_t)i * p.ffpre_stride;
    for (uint32_t c = blockIdx.x * NT + threadIdx.x; c < nch; c += gridDim.x * NT) {
        const uint32_t lo = c * bqje::STUFF_CHUNK, hi = lo + bqje::STUFF_CHUNK < ulen ? lo + bqje::STUFF_CHUNK : ulen;
        bqje::copy_stuffed(u, lo, hi, o + bqje::HEADER_BYTES + lo + pre[c]);
    }
}

}  // namespace

static size_t jpeg_encode_scratch_bytes(int n, int px, int sub) {
    if (n <= 0 || !bqje::valid_args(px, 1, sub)) return 0;
    return round_cap(n, ENC_ROUND) * layout_of(bqje::geom_of(px, sub)).per_tile();
}

enum { JPEG_ENC_PIXEL = 0, JPEG_ENC_SIZE = 1, JPEG_ENC_PACK = 2, JPEG_ENC_STUFF = 3, JPEG_ENC_STAGES = 4 };
// One stage of one round, so that bq_jpeg_encode can time each: tiles [t0, t0 + cnt) of the call, in a scratch laid out for m tiles (cnt <= m).
static int launch_jpeg_encode_stage(int stage, const uint8_t* d_tiles, long long t0, int cnt, int m, int px, int quality, int sub, void* d_scratch,
                                    uint8_t* d_out, long long cap, long long* d_off, int* d_status, hipStream_t s) {
    bqje::Tables T;
    bqje::Header H;
    bqje::build_tables(px, quality, sub, T, H);
    const bqje::Geom G = bqje::geom_of(px, sub);
    const Layout L = layout_of(G);
    EncParams p;
    p.G = G;
    p.tiles = d_tiles + (size_t)t0 * px * px * 3;
    uint8_t* base = reinterpret_cast<uint8_t*>(d_scratch);
    p.coef = reinterpret_cast<int16_t*>(base);                     base += (size_t)m * L.coef;
    p.bits = reinterpret_cast<uint32_t*>(base);                    base += (size_t)m * L.bits;
    p.ubuf = base;                                                 base += (size_t)m * L.ubuf;
    p.ffpre = reinterpret_cast<uint32_t*>(base);                   base += (size_t)m * L.ffpre;
    p.meta = base;
    p.bits_stride = L.bits / 4; p.ubuf_stride = L.ubuf; p.ffpre_stride = L.ffpre / 4;
    p.n = cnt; p.t0 = t0; p.out = d_out; p.cap = cap; p.off = d_off; p.status = d_status + t0;
    const dim3 per_block((G.nblk + NT - 1) / NT, cnt);
    switch (stage) {
        case JPEG_ENC_PIXEL:
            hipLaunchKernelGGL(jenc_pixel_kernel, per_block, dim3(NT), 0, s, p, T);
            break;
        case JPEG_ENC_SIZE:
            hipLaunchKernelGGL(jenc_size_kernel, per_block, dim3(NT), 0, s, p, T);
            hipLaunchKernelGGL(jenc_scan_kernel, dim3(cnt), dim3(NT), 0, s, p);
            break;
        case JPEG_ENC_PACK:
            if (const hipError_t e = hipMemsetAsync(p.ubuf, 0, (size_t)cnt * L.ubuf, s)) return (int)e;
            hipLaunchKernelGGL(jenc_pack_kernel, per_block, dim3(NT), 0, s, p, T);
            break;
        case JPEG_ENC_STUFF: {
            hipLaunchKernelGGL(jenc_ff_kernel, dim3(cnt), dim3(NT), 0, s, p);
            hipLaunchKernelGGL(jenc_offsets_kernel, dim3(1), dim3(NT), 0, s, p);
            size_t blocks = (L.ubuf / bqje::STUFF_CHUNK + NT - 1) / NT;
            if (blocks > COPY_BLOCKS) blocks = COPY_BLOCKS;
            hipLaunchKernelGGL(jenc_copy_kernel, dim3((unsigned)blocks, cnt), dim3(NT), 0, s, p, H);
            break;
        }
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" {

size_t bq_jpeg_encode_scratch_bytes(int n, int px, int subsampling) { return jpeg_encode_scratch_bytes(n, px, subsampling); }

int bq_jpeg_encode(bq_ctx* c, const uint8_t* d_tiles, int n, int px, int quality, int subsampling, uint8_t* d_out, int64_t cap,
                   int64_t* d_off, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || cap < 0) return fail(c, BQ_ERR_ARG, "bq_jpeg_encode: bad argument");
    if (px < 1 || px > 4096 || quality < 1 || quality > 100 || (subsampling != 0 && subsampling != 2))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_encode: outside the encoder's subset (need 1 <= px <= 4096, 1 <= quality <= 100, subsampling 0 = 4:4:4 or 2 = 4:2:0)");
    if (n == 0) return BQ_OK;
    const std::string bad = bad_encode_args("bq_jpeg_encode", d_tiles, d_out, cap, d_off, d_status, d_scratch);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    const int m = (int)round_items(scratch_bytes, layout_of(bqje::geom_of(px, subsampling)).per_tile(), 1);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_encode: scratch smaller than one tile's (bq_jpeg_encode_scratch_bytes(1, px, subsampling))");
    hipStream_t s = (hipStream_t)stream;
    static const char* const kStage[JPEG_ENC_STAGES] = {"jpeg_encode_pixel", "jpeg_encode_size", "jpeg_encode_pack", "jpeg_encode_stuff"};
    const double blocks = (double)jpeg_encode_scratch_bytes(1, px, subsampling) / 344.0;       // (for the profile's byte column only: about the blocks of a tile)
    for (long long t0 = 0; t0 < n; t0 += m) {
        const int cnt = (int)(n - t0 < m ? n - t0 : m);
        for (int stage = 0; stage < JPEG_ENC_STAGES; ++stage) {
            ProfScope ps(c, s, kStage[stage], 0.0, stage == JPEG_ENC_PIXEL ? (double)cnt * px * px * 3.0 : (double)cnt * blocks * 128.0);
            const int e = launch_jpeg_encode_stage(stage, d_tiles, t0, cnt, m, px, quality, subsampling, d_scratch, d_out, (long long)cap,
                                                   (long long*)d_off, d_status, s);
            if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg encode launch: ") + hipGetErrorString((hipError_t)e));
        }
    }
    return BQ_OK;
}

}  // extern "C"
