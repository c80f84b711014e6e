// kernels_png_encode.hip -- tiles encoded as PNG on the device (bq_png_encode): the routines of png_encode_device.h, which
// libbiscuit_io runs unchanged on the CPU (bqio_png_encode), behind four stages of kernels.
//
//   filter  one wave per row, lanes strided over its 3 px bytes: the four candidates' scores by wave reduction, the choice, the
//           1 + 3 px filtered bytes to scratch, and the row's two Adler sums.
//   match   one wave per block of 16 384 filtered bytes, staged in LDS: groups of 64 positions against the hash table the
//           earlier groups left (LDS, atomicMax per hash after the group), the greedy walk over the group by lane broadcast,
//           tokens and the block's histogram to scratch.
//   code    one wave per block: both codes' lengths (rank sort across the lanes, the rest on lane 0 in LDS), the dynamic header,
//           the three sizes and the choice; then one wave per tile combines the Adler sums and walks the blocks' bit offsets
//           (a stored block starts on a byte boundary, so the walk is serial: nb steps).
//   pack    one wave per block: the header, every token's bits at its own offset (a scan of the code lengths per 64 tokens),
//           all through atomicOr into the tile's zeroed deflate buffer -- in the representation chosen only, so a block writes
//           at most its stored size; file lengths scanned into d_off; zlib bytes copied out behind the `cap` check into IDAT
//           chunks of 8 192, one wave per chunk for its length, type and CRC-32 (64 slices, combined).
//
// A tile costs Layout::per_tile() bytes of scratch (1.71 MB at 299 px, of which 1.11 MB are the tokens' worst case); a call works
// in rounds of as many tiles as the caller's scratch holds.  Nothing is allocated or copied, and nothing waits for the device.
#include "block_scan.h"
#include "bq_ctx.h"
#include "png_encode_device.h"

namespace {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int ENC_ROUND = 128;           // tiles per round that bq_png_encode_scratch_bytes asks scratch for
constexpr int COPY_BLOCKS = 64;          // most workgroups per tile of the copy kernel (it strides over the bytes)

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Scratch of a round of m tiles: arrays [m][per-tile size], every per-tile size a multiple of 16 bytes.
struct Layout {
    size_t filt, rows, toks, hist, codes, hdr, info, dbuf, meta;           // per tile, bytes
    size_t per_tile() const { return filt + rows + toks + hist + codes + hdr + info + dbuf + meta; }
};

Layout layout_of(const bqpe::Geom& G) {
    Layout L;
    L.filt = align16((size_t)G.L + 4);                             // (the match kernel stages whole words)
    L.rows = align16((size_t)G.px * 8);
    L.toks = (size_t)G.nb * bqpe::BLOCK * 4;
    L.hist = (size_t)G.nb * bqpe::NCODE * 4;
    L.codes = (size_t)G.nb * bqpe::NCODE * 4;
    L.hdr = (size_t)G.nb * bqpe::HDR_WORDS * 4;
    L.info = (size_t)G.nb * sizeof(bqpe::BlockInfo);
    L.dbuf = bqpe::deflate_bytes(G);
    L.meta = 32;                                                   // uint64 deflate bytes, int64 file bytes, uint32 adler
    return L;
}
static_assert(sizeof(bqpe::BlockInfo) == 32, "BlockInfo is 32 bytes");

struct EncParams {
    bqpe::Geom G;
    const uint8_t* tiles;                // of the round's first tile
    uint8_t* filt;    size_t filt_stride;   // bytes
    uint32_t* rows;   size_t rows_stride;   // words: [px][2]
    uint32_t* toks;                      // [m][nb][BLOCK]
    uint32_t* hist;                      // [m][nb][NCODE]
    uint32_t* codes;                     // [m][nb][NCODE]
    uint32_t* hdr;                       // [m][nb][HDR_WORDS]
    bqpe::BlockInfo* info;               // [m][nb]
    uint8_t* dbuf;    size_t dbuf_stride;   // bytes
    uint8_t* meta;                       // [m][32]
    int n;                               // tiles of this round
    long long t0;                        // the round's first tile within the call
    uint8_t* out;
    long long cap;
    long long* off;                      // the CALL's [n + 1]
    int* status;                         // of the round's first tile
};

__device__ unsigned long long& meta_dlen(const EncParams& p, int i) { return *reinterpret_cast<unsigned long long*>(p.meta + (size_t)i * 32); }
__device__ long long& meta_flen(const EncParams& p, int i) { return *reinterpret_cast<long long*>(p.meta + (size_t)i * 32 + 8); }
__device__ uint32_t& meta_adler(const EncParams& p, int i) { return *reinterpret_cast<uint32_t*>(p.meta + (size_t)i * 32 + 16); }

__device__ uint32_t wave_sum(uint32_t v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}
// inclusive scan over the wave
__device__ uint32_t wave_scan(uint32_t v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t a = __shfl_up(v, d, WAVE);
        if (lane >= d) v += a;
    }
    return v;
}

// ---- filter: one wave per row -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) penc_filter_kernel(const EncParams p) {
    const int i = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const uint32_t y = blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE;
    if (y >= (uint32_t)p.G.px) return;                               // (a whole wave leaves)
    const uint32_t rb = p.G.rl - 1;
    const uint8_t* cur = p.tiles + ((size_t)i * p.G.px + y) * rb;
    const uint8_t* prev = y ? cur - rb : nullptr;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t k = lane; k < rb; k += WAVE) {
        const bqpe::Cand c = bqpe::candidates(cur, prev, k);
        s0 += bqpe::abs8(c.none); s1 += bqpe::abs8(c.sub); s2 += bqpe::abs8(c.up); s3 += bqpe::abs8(c.pae);
    }
    const int f = bqpe::choose_filter(wave_sum(s0), wave_sum(s1), wave_sum(s2), wave_sum(s3));
    uint8_t* row = p.filt + (size_t)i * p.filt_stride + (size_t)y * p.G.rl;
    uint32_t A = 0, B = 0;                                           // per lane: at most 193 bytes, B <= 193 * 12289 * 255 < 2^32
    if (lane == 0) { row[0] = (uint8_t)f; A = (uint32_t)f; B = p.G.rl * (uint32_t)f; }
    for (uint32_t k = lane; k < rb; k += WAVE) {
        const uint32_t v = (uint32_t)bqpe::pick(bqpe::candidates(cur, prev, k), f);
        row[1 + k] = (uint8_t)v;
        A += v; B += (p.G.rl - 1 - k) * v;
    }
    A = wave_sum(A % bqpe::ADLER) % bqpe::ADLER;
    B = wave_sum(B % bqpe::ADLER) % bqpe::ADLER;
    if (lane == 0) {
        uint32_t* r = p.rows + (size_t)i * p.rows_stride + 2 * (size_t)y;
        r[0] = A; r[1] = B;
    }
}

// ---- match: one wave per block ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) penc_match_kernel(const EncParams p) {
    __shared__ uint32_t sbw[bqpe::BLOCK / 4 + 1];
    __shared__ uint32_t table[bqpe::HASH_SIZE];
    __shared__ uint32_t hist[bqpe::NCODE];
    const int i = blockIdx.y, lane = threadIdx.x;
    const uint32_t b = blockIdx.x, n = bqpe::block_len(p.G, b);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.filt + (size_t)i * p.filt_stride + (size_t)b * bqpe::BLOCK);
    for (uint32_t k = lane; k < (n + 3) / 4; k += WAVE) sbw[k] = src[k];      // (up to 3 bytes beyond n: inside the tile's padded array, never compared)
    for (uint32_t k = lane; k < bqpe::HASH_SIZE; k += WAVE) table[k] = 0;
    for (uint32_t k = lane; k < (uint32_t)bqpe::NCODE; k += WAVE) hist[k] = 0;
    __syncthreads();
    const uint8_t* base = reinterpret_cast<const uint8_t*>(sbw);
    uint32_t* toks = p.toks + ((size_t)i * p.G.nb + b) * bqpe::BLOCK;
    uint32_t q = 0, ntok = 0;                                        // the same in every lane
    for (uint32_t p0 = 0; p0 < n; p0 += bqpe::GROUP) {
        const uint32_t pos = p0 + lane;
        uint32_t len = 0, dist = 0, h = bqpe::HASH_SIZE;
        if (pos + bqpe::HASH_BYTES <= n) {
            h = bqpe::hash3(base + pos);
            const uint32_t c = table[h];
            if (c && pos >= q) {
                const uint32_t room = n - pos;
                len = bqpe::match_len(base, c - 1, pos, room < bqpe::MAX_MATCH ? room : bqpe::MAX_MATCH);
                dist = pos - (c - 1);
            }
        }
        __syncthreads();                                             // every lane has read the table of the earlier groups
        if (h < bqpe::HASH_SIZE) atomicMax(&table[h], pos + 1);
        __syncthreads();
        const uint32_t lim = n - p0 < bqpe::GROUP ? n - p0 : bqpe::GROUP;
        // The greedy walk, uniform across the wave.  Between the current position and the next lane that holds a match every
        // position is a literal, so the walk goes from match to match: one broadcast per match taken, not one per position.
        const unsigned long long matches = __ballot(len >= bqpe::TAKE_MATCH);      // (such a lane is below lim: it hashed 3 bytes)
        uint32_t j = q - p0;
        bool start = false;
        while (j < lim) {
            const unsigned long long rest = matches >> j;
            const uint32_t nxt = rest ? j + (uint32_t)__builtin_ctzll(rest) : bqpe::GROUP;
            if ((uint32_t)lane >= j && (uint32_t)lane < (nxt < lim ? nxt : lim)) start = true;      // literals
            if (nxt >= lim) { j = lim; break; }
            if ((uint32_t)lane == nxt) start = true;
            j = nxt + __shfl(len, (int)nxt, WAVE);
        }
        q = p0 + j;
        const unsigned long long mask = __ballot(start);
        if (start) {
            const uint32_t idx = ntok + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            if (len >= bqpe::TAKE_MATCH) {
                toks[idx] = bqpe::match_token(len, dist);
                atomicAdd(&hist[bqpe::length_sym(len).sym], 1u);
                atomicAdd(&hist[bqpe::DIST0 + bqpe::dist_sym(dist).sym], 1u);
            } else {
                toks[idx] = base[pos];
                atomicAdd(&hist[base[pos]], 1u);
            }
        }
        ntok += (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (lane == 0) { hist[256] = 1; p.info[(size_t)i * p.G.nb + b].ntok = ntok; }
    __syncthreads();
    uint32_t* gh = p.hist + ((size_t)i * p.G.nb + b) * bqpe::NCODE;
    for (uint32_t k = lane; k < (uint32_t)bqpe::NCODE; k += WAVE) gh[k] = hist[k];
}

// ---- code: one wave per block -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) penc_code_kernel(const EncParams p) {
    __shared__ bqpe::CodeWork W;
    const int i = blockIdx.y, lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const size_t blk = (size_t)i * p.G.nb + b;
    const uint32_t* gh = p.hist + blk * bqpe::NCODE;
    for (int k = lane; k < bqpe::NCODE; k += WAVE) { W.hist[k] = gh[k]; W.lens[k] = 0; W.codes[k] = 0; }
    __syncthreads();
    bqpe::huff_keys(W.hist, bqpe::NLL, W.key, lane, WAVE);
    __syncthreads();
    bqpe::rank_sort(W.key, bqpe::NLL, W.sorted, lane, WAVE);
    __syncthreads();
    if (lane == 0) bqpe::huff_from_sorted(W.sorted, bqpe::NLL, 15, W.lens, W.A, W.cnt);
    __syncthreads();
    bqpe::huff_keys(W.hist + bqpe::DIST0, bqpe::NDIST, W.key, lane, WAVE);
    __syncthreads();
    bqpe::rank_sort(W.key, bqpe::NDIST, W.sorted, lane, WAVE);
    __syncthreads();
    if (lane == 0) {
        bqpe::huff_from_sorted(W.sorted, bqpe::NDIST, 15, W.lens + bqpe::DIST0, W.A, W.cnt);
        bqpe::BlockInfo I = bqpe::finish_block(W, p.info[blk].ntok, bqpe::block_len(p.G, b), b + 1 == p.G.nb);
        p.info[blk] = I;
    }
    __syncthreads();
    uint32_t* gc = p.codes + blk * bqpe::NCODE;
    for (int k = lane; k < bqpe::NCODE; k += WAVE) gc[k] = W.codes[k];
    uint32_t* ghd = p.hdr + blk * bqpe::HDR_WORDS;
    for (int k = lane; k < bqpe::HDR_WORDS; k += WAVE) ghd[k] = W.hdr[k];
}

// per tile: Adler-32 from the rows' sums, the blocks' bit offsets, the deflate and the file length
__global__ void __launch_bounds__(WAVE) penc_tile_kernel(const EncParams p) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint32_t* rows = p.rows + (size_t)i * p.rows_stride;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t y = lane; y < (uint32_t)p.G.px; y += WAVE) {
        s1 = (s1 + rows[2 * y]) % bqpe::ADLER;
        s2 = (s2 + bqpe::adler_row_term(p.G, y, rows[2 * y], rows[2 * y + 1])) % bqpe::ADLER;
    }
    s1 = (wave_sum(s1) + 1) % bqpe::ADLER;
    s2 = (wave_sum(s2) + p.G.L % bqpe::ADLER) % bqpe::ADLER;
    if (lane != 0) return;
    bqpe::BlockInfo* info = p.info + (size_t)i * p.G.nb;
    uint64_t pos = 0;
    for (uint32_t b = 0; b < p.G.nb; ++b) {
        info[b].start = pos;
        pos = bqpe::block_end(info[b], pos, bqpe::block_len(p.G, b));
    }
    uint64_t dlen = (pos + 7) / 8;                                   // <= deflate_bytes(G) - 16: every block is at most its stored size
    if (dlen > p.dbuf_stride - 16) dlen = p.dbuf_stride - 16;       // (the copy kernel reads this many bytes)
    meta_dlen(p, i) = dlen;
    meta_flen(p, i) = (long long)bqpe::file_bytes(dlen);
    meta_adler(p, i) = s1 | (s2 << 16);
}

// ---- pack: one wave per block -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) penc_pack_kernel(const EncParams p) {
    __shared__ uint32_t codes[bqpe::NCODE];
    const int i = blockIdx.y, lane = threadIdx.x;
    const uint32_t b = blockIdx.x, n = bqpe::block_len(p.G, b);
    const size_t blk = (size_t)i * p.G.nb + b;
    const bqpe::BlockInfo I = p.info[blk];
    const bool bfinal = b + 1 == p.G.nb;
    uint32_t* dbuf = reinterpret_cast<uint32_t*>(p.dbuf + (size_t)i * p.dbuf_stride);
    // Every size here was computed from the very tokens that are packed, so the stream ends inside the buffer; the limit makes
    // that hold whatever the sizes say: no write of this kernel depends on data for its bounds.
    const uint64_t limit = 8 * (uint64_t)(p.dbuf_stride - 16);
    uint64_t pos = I.start;
    if (bqpe::block_end(I, pos, n) > limit) return;
    if (I.kind == bqpe::KIND_STORED) {
        const uint8_t* src = p.filt + (size_t)i * p.filt_stride + (size_t)b * bqpe::BLOCK;
        if (lane == 0) bqpe::put_bits<true>(dbuf, pos, bfinal ? 1u : 0u, 3);
        pos = (pos + 3 + 7) & ~(uint64_t)7;
        if (lane == 0) bqpe::put_bits<true>(dbuf, pos, (uint64_t)n | ((uint64_t)(~n & 0xFFFF) << 16), 32);
        pos += 32;
        for (uint32_t k = 4 * lane; k < n; k += 4 * WAVE) {
            const uint32_t m = n - k < 4 ? n - k : 4;
            uint32_t v = 0;
            for (uint32_t t = 0; t < m; ++t) v |= (uint32_t)src[k + t] << (8 * t);
            bqpe::put_bits<true>(dbuf, pos + 8 * (uint64_t)k, v, 8 * m);
        }
        return;
    }
    const uint32_t* gc = p.codes + blk * bqpe::NCODE;
    for (int k = lane; k < bqpe::NCODE; k += WAVE) codes[k] = gc[k];
    __syncthreads();
    if (I.kind == bqpe::KIND_FIXED) {
        if (lane == 0) bqpe::put_bits<true>(dbuf, pos, (bfinal ? 1u : 0u) | (1u << 1), 3);
    } else {
        const uint32_t* ghd = p.hdr + blk * bqpe::HDR_WORDS;
        for (uint32_t k = lane; 32 * k < I.hdr_bits; k += WAVE) bqpe::put_bits<true>(dbuf, pos + 32 * (uint64_t)k, ghd[k], 32);
    }
    pos += I.hdr_bits;
    const uint32_t* toks = p.toks + blk * bqpe::BLOCK;
    for (uint32_t t0 = 0; t0 < I.ntok; t0 += WAVE) {
        const uint32_t t = t0 + lane;
        uint64_t v = 0;
        uint32_t nb = 0;
        if (t < I.ntok) bqpe::token_bits(toks[t], codes, v, nb);
        const uint32_t incl = wave_scan(nb, lane);
        if (pos + incl <= limit) bqpe::put_bits<true>(dbuf, pos + incl - nb, v, nb);
        pos += __shfl(incl, WAVE - 1, WAVE);
    }
    if (lane == 0 && pos + (codes[256] >> 16) <= limit) bqpe::put_bits<true>(dbuf, pos, codes[256] & 0xFFFF, codes[256] >> 16);
}

// file lengths -> d_off[t0 + 1 .. t0 + n], continuing from d_off[t0]; one workgroup
__global__ void __launch_bounds__(NT) penc_offsets_kernel(const EncParams p) {
    __shared__ long long sh[NT];
    offsets_scan<NT>(p.off, p.t0, p.n, [&](int i) { return meta_flen(p, i); }, sh);
}

// signature + IHDR, the zlib bytes at their places between the chunk frames, IEND of tile i at out + off[i], when it ends inside `cap`
__global__ void __launch_bounds__(NT) penc_copy_kernel(const EncParams p, const bqpe::Header H) {
    const int i = blockIdx.y;
    const long long start = p.off[p.t0 + i], end = p.off[p.t0 + i + 1];
    const bool fits = end <= p.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.status[i] = fits ? bqpe::ST_OK : bqpe::ST_CAP;
    if (!fits) return;
    uint8_t* o = p.out + start;
    if (blockIdx.x == 0) {
        if (threadIdx.x < bqpe::FILE_HEAD) o[threadIdx.x] = H.b[threadIdx.x];
        if (threadIdx.x < 12) p.out[end - 12 + threadIdx.x] = H.b[bqpe::FILE_HEAD + threadIdx.x];
    }
    const uint64_t dlen = meta_dlen(p, i), zlen = bqpe::zlib_bytes(dlen);
    const uint32_t adler = meta_adler(p, i);
    const uint8_t* d = p.dbuf + (size_t)i * p.dbuf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x; k < zlen; k += (uint64_t)gridDim.x * NT)
        o[bqpe::zbyte_at(k)] = (uint8_t)bqpe::zbyte(d, dlen, adler, k);
}

// one wave per IDAT chunk: every lane the CRC-32 share of its slice of the chunk (read from scratch, not from the output), the
// shares XORed across the wave, lane 0 writes the chunk's length and type in front and its CRC behind
__global__ void __launch_bounds__(WAVE) penc_crc_kernel(const EncParams p) {
    static_assert(bqpe::CRC_LANES == WAVE, "one slice per lane");
    __shared__ uint32_t table[256];
    for (uint32_t k = threadIdx.x; k < 256; k += WAVE) table[k] = bqpe::crc_entry(k);
    __syncthreads();
    const int i = blockIdx.y;
    if (p.off[p.t0 + i + 1] > p.cap) return;
    const uint64_t dlen = meta_dlen(p, i), zlen = bqpe::zlib_bytes(dlen);
    const uint64_t c = blockIdx.x;
    if (c >= bqpe::idat_chunks(zlen)) return;
    uint32_t crc = bqpe::chunk_crc_share(table, p.dbuf + (size_t)i * p.dbuf_stride, dlen, meta_adler(p, i), c, threadIdx.x);
    for (int d = WAVE / 2; d > 0; d >>= 1) crc ^= __shfl_xor(crc, d, WAVE);
    if (threadIdx.x == 0) bqpe::write_chunk_frame(p.out + p.off[p.t0 + i], zlen, c, crc);
}

}  // namespace

static size_t png_encode_scratch_bytes(int n, int px) {
    if (n <= 0 || !bqpe::valid_px(px)) return 0;
    return round_cap(n, ENC_ROUND) * layout_of(bqpe::geom_of(px)).per_tile();
}

enum { PNG_ENC_FILTER = 0, PNG_ENC_MATCH = 1, PNG_ENC_CODE = 2, PNG_ENC_PACK = 3, PNG_ENC_STAGES = 4 };
// One stage of one round, so that bq_png_encode can time each: tiles [t0, t0 + cnt) of the call, in a scratch laid out for m tiles (cnt <= m).
static int launch_png_encode_stage(int stage, const uint8_t* d_tiles, long long t0, int cnt, int m, int px, void* d_scratch, uint8_t* d_out,
                                   long long cap, long long* d_off, int* d_status, hipStream_t s) {
    const bqpe::Geom G = bqpe::geom_of(px);
    const Layout L = layout_of(G);
    EncParams p;
    p.G = G;
    p.tiles = d_tiles + (size_t)t0 * px * px * 3;
    uint8_t* base = reinterpret_cast<uint8_t*>(d_scratch);
    p.filt = base;                                                 base += (size_t)m * L.filt;
    p.rows = reinterpret_cast<uint32_t*>(base);                    base += (size_t)m * L.rows;
    p.toks = reinterpret_cast<uint32_t*>(base);                    base += (size_t)m * L.toks;
    p.hist = reinterpret_cast<uint32_t*>(base);                    base += (size_t)m * L.hist;
    p.codes = reinterpret_cast<uint32_t*>(base);                   base += (size_t)m * L.codes;
    p.hdr = reinterpret_cast<uint32_t*>(base);                     base += (size_t)m * L.hdr;
    p.info = reinterpret_cast<bqpe::BlockInfo*>(base);             base += (size_t)m * L.info;
    p.dbuf = base;                                                 base += (size_t)m * L.dbuf;
    p.meta = base;
    p.filt_stride = L.filt; p.rows_stride = L.rows / 4; p.dbuf_stride = L.dbuf;
    p.n = cnt; p.t0 = t0; p.out = d_out; p.cap = cap; p.off = d_off; p.status = d_status + t0;
    const dim3 per_block(G.nb, cnt);
    switch (stage) {
        case PNG_ENC_FILTER:
            hipLaunchKernelGGL(penc_filter_kernel, dim3((px + NT / WAVE - 1) / (NT / WAVE), cnt), dim3(NT), 0, s, p);
            break;
        case PNG_ENC_MATCH:
            hipLaunchKernelGGL(penc_match_kernel, per_block, dim3(WAVE), 0, s, p);
            break;
        case PNG_ENC_CODE:
            hipLaunchKernelGGL(penc_code_kernel, per_block, dim3(WAVE), 0, s, p);
            hipLaunchKernelGGL(penc_tile_kernel, dim3(cnt), dim3(WAVE), 0, s, p);
            break;
        case PNG_ENC_PACK: {
            if (const hipError_t e = hipMemsetAsync(p.dbuf, 0, (size_t)cnt * L.dbuf, s)) return (int)e;
            hipLaunchKernelGGL(penc_pack_kernel, per_block, dim3(WAVE), 0, s, p);
            hipLaunchKernelGGL(penc_offsets_kernel, dim3(1), dim3(NT), 0, s, p);
            bqpe::Header H;
            bqpe::build_header(px, H);
            const size_t zmax = bqpe::zlib_bytes(L.dbuf);
            size_t blocks = (zmax + NT - 1) / NT;
            if (blocks > COPY_BLOCKS) blocks = COPY_BLOCKS;
            hipLaunchKernelGGL(penc_copy_kernel, dim3((unsigned)blocks, cnt), dim3(NT), 0, s, p, H);
            const size_t chunks = (size_t)bqpe::idat_chunks(zmax);
            hipLaunchKernelGGL(penc_crc_kernel, dim3((unsigned)chunks, cnt), dim3(WAVE), 0, s, p);
            break;
        }
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" {

size_t bq_png_encode_scratch_bytes(int n, int px) { return png_encode_scratch_bytes(n, px); }

int bq_png_encode(bq_ctx* c, const uint8_t* d_tiles, int n, int px, uint8_t* d_out, int64_t cap, int64_t* d_off, int32_t* d_status,
                  void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || cap < 0) return fail(c, BQ_ERR_ARG, "bq_png_encode: bad argument");
    if (!bqpe::valid_px(px)) return fail(c, BQ_ERR_ARG, "bq_png_encode: outside the encoder's subset (need 1 <= px <= 4096)");
    if (n == 0) return BQ_OK;
    const std::string bad = bad_encode_args("bq_png_encode", d_tiles, d_out, cap, d_off, d_status, d_scratch);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, bad);
    const int m = (int)round_items(scratch_bytes, layout_of(bqpe::geom_of(px)).per_tile(), 1);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_png_encode: scratch smaller than one tile's (bq_png_encode_scratch_bytes(1, px))");
    hipStream_t s = (hipStream_t)stream;
    static const char* const kStage[PNG_ENC_STAGES] = {"png_encode_filter", "png_encode_match", "png_encode_code", "png_encode_pack"};
    const double stream_bytes = (double)bqpe::geom_of(px).L;         // (for the profile's byte column only: the filtered stream of a tile)
    for (long long t0 = 0; t0 < n; t0 += m) {
        const int cnt = (int)(n - t0 < m ? n - t0 : m);
        for (int stage = 0; stage < PNG_ENC_STAGES; ++stage) {
            ProfScope ps(c, s, kStage[stage], 0.0, (double)cnt * stream_bytes * 2.0);
            const int e = launch_png_encode_stage(stage, d_tiles, t0, cnt, m, px, d_scratch, d_out, (long long)cap, (long long*)d_off, d_status, s);
            if (e) return fail(c, BQ_ERR_HIP, std::string("png encode launch: ") + hipGetErrorString((hipError_t)e));
        }
    }
    return BQ_OK;
}

}  // extern "C"
