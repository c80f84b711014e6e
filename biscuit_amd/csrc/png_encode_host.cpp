// Host side of the PNG encoder (include/biscuit_io.h: bqio_png_encode): the CPU build of bq_png_encode, over the routines of
// png_encode_device.h -- the ones the GPU kernels are compiled from -- in the same four steps: filter, match, code, pack.
// Tile by tile, block by block, group by group: for tests.
#include "../../include/biscuit_io.h"
#include "png_encode_device.h"

#include <string>
#include <vector>

namespace {
thread_local std::string g_png_encode_error;
int refuse(const char* what) { g_png_encode_error = what; return BQIO_ERR_ARG; }
}  // namespace

extern "C" {

const char* bqio_png_encode_last_error(void) { return g_png_encode_error.c_str(); }

int bqio_png_encode(const uint8_t* tiles, int64_t n, int px, uint8_t* out, size_t cap, int64_t* off, int32_t* status) {
    if (!bqpe::valid_px(px)) return refuse("outside the encoder's subset: need 1 <= px <= 4096");
    if (n < 0 || !off || (n > 0 && (!tiles || !status || (!out && cap)))) return refuse("bqio_png_encode: bad argument");
    std::vector<uint8_t> file;
    off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        bqpe::serial_encode(tiles + (size_t)i * px * px * 3, px, file);
        off[i + 1] = off[i] + (int64_t)file.size();
        if ((uint64_t)off[i + 1] > (uint64_t)cap) { status[i] = bqpe::ST_CAP; continue; }
        status[i] = bqpe::ST_OK;
        memcpy(out + off[i], file.data(), file.size());
    }
    return BQIO_OK;
}

}  // extern "C"
