// Host side of the training augmentation (include/biscuit_io.h: bqio_augment, bqio_augment_blur_weights): the CPU build of
// bq_augment, over the routines of augment_device.h -- the ones the GPU kernels are compiled from -- in the same stages: the JPEG
// round trip's blocks, the dihedral placement, the row and the column pass of the blur.  Tile by tile on `threads` host threads:
// for the tests, and the baseline the device entry is timed against (tools/bench_augment.py).
#include "../../include/biscuit_io.h"
#include "augment_device.h"

#include <atomic>
#include <string>
#include <thread>
#include <vector>

namespace {
thread_local std::string g_augment_error;
int refuse(const char* what) { g_augment_error = what; return BQIO_ERR_ARG; }

struct Job {
    const uint8_t* tiles; const uint8_t* params; uint8_t* out; int32_t* status;
    int64_t n; int px;
    bqaug::QuantBase QB; bqaug::BlurTables BT;
};

void augment_tile(const Job& J, int64_t i, std::vector<uint8_t>& planes, std::vector<uint16_t>& rows) {
    const int px = J.px;
    const size_t tile_bytes = (size_t)px * px * 3;
    const uint8_t* tile = J.tiles + (size_t)i * tile_bytes;
    uint8_t* out = J.out + (size_t)i * tile_bytes;
    const bqaug::Params a = bqaug::params_of(J.params + 4 * (size_t)i);
    const bqjd::Geom Gd = bqaug::decode_geom(px);
    int32_t st = bqaug::ST_OK;
    if (a.quality) {
        const bqje::Geom Ge = bqaug::encode_geom(px);
        uint16_t q[2][64];
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) q[t][k] = bqaug::quant_entry(J.QB.b[t][k], a.quality);
        planes.resize(bqaug::plane_bytes(px));
        for (uint32_t b = 0; b < Ge.nblk; ++b) {
            const bqje::BlockPos P = bqje::block_pos(Ge, b);
            if (P.dummy) continue;
            if (!bqaug::jpeg_block(tile, Ge, Gd, P, q[P.comp ? 1 : 0], planes.data())) st |= bqaug::ST_RANGE;
        }
    }
    for (int y = 0; y < px; ++y)
        for (int x = 0; x < px; ++x) bqaug::placed_pixel(tile, planes.data(), Gd, px, a, y, x, out + ((size_t)y * px + x) * 3);
    if (a.blur) {
        const uint16_t* w = J.BT.w[a.blur - 1];
        const int r = J.BT.r[a.blur - 1];
        rows.resize((size_t)px * px * 3);
        for (int y = 0; y < px; ++y)
            for (int x = 0; x < px; ++x) bqaug::blur_row_at(out, px, y, x, w, r, rows.data() + ((size_t)y * px + x) * 3);
        for (int y = 0; y < px; ++y)
            for (int x = 0; x < px; ++x) bqaug::blur_col_at(rows.data(), px, y, x, w, r, out + ((size_t)y * px + x) * 3);
    }
    J.status[i] = st;
}
}  // namespace

extern "C" {

const char* bqio_augment_last_error(void) { return g_augment_error.c_str(); }

int bqio_augment_blur_weights(int blur, uint16_t* out) {
    if (blur < 1 || blur > bqaug::MAX_BLUR || !out) return refuse("bqio_augment_blur_weights: blur outside 1..4 or out is null");
    bqaug::BlurTables B;
    bqaug::build_blur_tables(B);
    for (int i = 0; i < bqaug::MAX_TAPS; ++i) out[i] = B.w[blur - 1][i];
    return B.r[blur - 1];
}

int bqio_augment(const uint8_t* tiles, int64_t n, int px, const uint8_t* params, uint8_t* out, int32_t* status, int threads) {
    if (!bqaug::valid_px(px)) return refuse("bqio_augment: need 8 <= px <= 4096");
    if (n < 0 || (n > 0 && (!tiles || !params || !out || !status))) return refuse("bqio_augment: bad argument (n < 0 or a null pointer)");
    const uintptr_t total = (uintptr_t)n * px * px * 3, in0 = (uintptr_t)tiles, out0 = (uintptr_t)out;
    if (n > 0 && out0 < in0 + total && in0 < out0 + total) return refuse("bqio_augment: out overlaps tiles");
    for (int64_t i = 0; i < n; ++i)
        if (!bqaug::valid_params(params + 4 * (size_t)i))
            return refuse("bqio_augment: a parameter row outside k 0..3, flips 0..3, quality 0..100, blur 0..4");
    Job J{tiles, params, out, status, n, px, bqaug::quant_base(), {}};
    bqaug::build_blur_tables(J.BT);
    int nt = threads < 1 ? 1 : threads > 64 ? 64 : threads;
    if ((int64_t)nt > n) nt = (int)n;
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        std::vector<uint8_t> planes;
        std::vector<uint16_t> rows;
        for (int64_t i; (i = next.fetch_add(1)) < n;) augment_tile(J, i, planes, rows);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    if (n > 0) work();
    for (auto& t : pool) t.join();
    return BQIO_OK;
}

}  // extern "C"
