// Host side of the region-of-interest mask (include/biscuit_io.h: bqio_roi_plane): the CPU build of bq_roi_plane, over the crossing
// rule and the table checks of roi_device.h -- the ones the GPU kernel and its entry are compiled from.  Edge by edge, pixel by
// pixel: for tests.
#include "../../include/biscuit_io.h"
#include "roi_device.h"

#include <vector>

extern "C" {

int bqio_roi_plane(const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys, int H,
                   uint8_t* plane) {
    if (!plane || bqroi::check_tables(edges, E, starts, P, xs, W, ys, H)) return BQIO_ERR_ARG;
    std::vector<uint8_t> parity((size_t)W);
    for (int y = 0; y < H; ++y) {
        uint8_t* row = plane + (size_t)y * W;
        const int py = ys[y];
        for (int x = 0; x < W; ++x) row[x] = 0;
        for (int p = 0; p < P; ++p) {
            bool any = false;
            for (int e = starts[p]; e < starts[p + 1]; ++e) {
                const int32_t* v = edges + (size_t)4 * e;
                if (!bqroi::straddles(v[1], v[3], py)) continue;
                if (!any) parity.assign((size_t)W, 0);
                any = true;
                for (int x = 0; x < W; ++x) parity[x] ^= bqroi::counts_beyond(v[0], v[1], v[2], v[3], xs[x], py) ? 1 : 0;
            }
            if (any)
                for (int x = 0; x < W; ++x) row[x] |= parity[x];
        }
    }
    return BQIO_OK;
}

}  // extern "C"
