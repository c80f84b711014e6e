// Host side of the JPEG encoder (include/biscuit_io.h: bqio_jpeg_encode, bqio_jpeg_encode_header): the CPU build of
// bq_jpeg_encode, over the routines of jpeg_encode_device.h -- the ones the GPU kernels are compiled from -- in the same four
// steps: coefficients, code lengths and their scan, packing at bit offsets, stuffing.  Tile by tile, block by block: for tests.
#include "../../include/biscuit_io.h"
#include "jpeg_encode_device.h"

#include <string>
#include <vector>

namespace {
thread_local std::string g_encode_error;
int refuse(const char* what) { g_encode_error = what; return BQIO_ERR_ARG; }
const char* const kSubset = "outside the encoder's subset: need 1 <= px <= 4096, 1 <= quality <= 100, subsampling 0 (4:4:4) or 2 (4:2:0)";
}  // namespace

extern "C" {

const char* bqio_jpeg_encode_last_error(void) { return g_encode_error.c_str(); }

size_t bqio_jpeg_encode_header_bytes(void) { return bqje::HEADER_BYTES; }

int bqio_jpeg_encode_header(int px, int quality, int subsampling, uint8_t* out) {
    if (!bqje::valid_args(px, quality, subsampling)) return refuse(kSubset);
    if (!out) return refuse("bqio_jpeg_encode_header: out is null");
    bqje::Tables T;
    bqje::Header H;
    bqje::build_tables(px, quality, subsampling, T, H);
    memcpy(out, H.b, bqje::HEADER_BYTES);
    return BQIO_OK;
}

int bqio_jpeg_encode(const uint8_t* tiles, int64_t n, int px, int quality, int subsampling, uint8_t* out, size_t cap, int64_t* off,
                     int32_t* status) {
    if (!bqje::valid_args(px, quality, subsampling)) return refuse(kSubset);
    if (n < 0 || !off || (n > 0 && (!tiles || !status || (!out && cap)))) return refuse("bqio_jpeg_encode: bad argument");
    bqje::Tables T;
    bqje::Header H;
    bqje::build_tables(px, quality, subsampling, T, H);
    const bqje::Geom G = bqje::geom_of(px, subsampling);
    std::vector<int16_t> coef((size_t)G.nblk * 64);
    std::vector<uint64_t> pos((size_t)G.nblk + 1);
    std::vector<uint32_t> ubuf;
    off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* tile = tiles + (size_t)i * px * px * 3;
        for (uint32_t b = 0; b < G.nblk; ++b) {
            const bqje::BlockPos P = bqje::block_pos(G, b);
            bqje::block_coefs(tile, G, P, T.q[P.comp ? 1 : 0], coef.data() + (size_t)b * 64);
        }
        pos[0] = 0;
        for (uint32_t b = 0; b < G.nblk; ++b) pos[b + 1] = pos[b] + bqje::block_bits(coef.data(), G, T, b);
        const uint32_t ulen = (uint32_t)((pos[G.nblk] + 7) / 8);
        ubuf.assign((size_t)ulen / 4 + 2, 0);
        for (uint32_t b = 0; b < G.nblk; ++b) bqje::block_pack(coef.data(), G, T, b, pos[b], ubuf.data());
        const uint8_t* u = reinterpret_cast<const uint8_t*>(ubuf.data());
        const int64_t len = (int64_t)bqje::HEADER_BYTES + ulen + bqje::count_ff(u, 0, ulen) + 2;
        off[i + 1] = off[i] + len;
        if ((uint64_t)off[i + 1] > (uint64_t)cap) { status[i] = bqje::ST_CAP; continue; }
        status[i] = bqje::ST_OK;
        uint8_t* o = out + off[i];
        memcpy(o, H.b, bqje::HEADER_BYTES);
        o += bqje::HEADER_BYTES;
        o += bqje::copy_stuffed(u, 0, ulen, o);
        o[0] = 0xFF; o[1] = 0xD9;
    }
    return BQIO_OK;
}

}  // extern "C"
