// lzw_host.cpp -- the host half of libbiscuit_io for TIFF pages with LZW compression (include/biscuit_io.h): the slide reader's
// segment decoder (bqio_lzw_decode) and the CPU statement of the device decoder (bqio_lzw_decode_canvas), both over the one
// statement of the stream in lzw_device.h.
#include <atomic>
#include <string.h>
#include <thread>
#include <vector>

#include "../../include/biscuit_io.h"
#include "lzw_device.h"

namespace {

using namespace bqlzw;

template <class F> void run_threads(int n, int n_threads, F&& body) {
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n) n_threads = n ? n : 1;
    std::atomic<int> next(0);
    auto work = [&]() { for (;;) { const int i = next.fetch_add(1); if (i >= n) return; body(i); } };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}

// rows x seg_w pixels of one segment into out (need bytes), the predictor undone: -> the status; out is no image unless 0
int decode_segment(const uint8_t* raw, uint32_t len, int rows, int seg_w, int predictor, uint8_t* out, uint32_t* start) {
    const uint32_t need = (uint32_t)rows * (uint32_t)seg_w * 3u;
    const int st = decode_serial(raw, len, need, out, start);
    if (!st && predictor == 2)
        for (int y = 0; y < rows; ++y) unpredict_row(out + (size_t)y * seg_w * 3, seg_w);
    return st;
}

}  // namespace

extern "C" {

int bqio_lzw_max_side(void) { return MAX_SIDE; }

int bqio_lzw_decode(const uint8_t* raw, size_t len, int rows, int seg_w, int predictor, uint8_t* out) {
    // (the reader's segments may be larger than the device takes: a strip is as wide as its page)
    if ((!raw && len) || !out || rows <= 0 || seg_w <= 0 || rows > (1 << 15) || seg_w > (1 << 20) || (uint64_t)rows * seg_w * 3 > (1u << 30) ||
        (predictor != 1 && predictor != 2))
        return BQIO_ERR_ARG;
    if (len > MAX_LEN) return ST_DESC;
    std::vector<uint32_t> start(TABLE + 1);
    return decode_segment(raw, (uint32_t)len, rows, seg_w, predictor, out, start.data());
}

int bqio_lzw_decode_canvas(const uint8_t* data, const uint32_t* desc, int n, int seg_w, int seg_h, int predictor, const int32_t* place,
                           uint8_t* canvas, int H, int W, const int32_t* clip, int32_t* status, int n_threads) {
    if (n < 0 || !geom_ok(seg_h, seg_w) || (predictor != 1 && predictor != 2) || !bqcanvas::canvas_args_ok(H, W) || !canvas || !clip ||
        (n && (!data || !desc || !place || !status)))
        return BQIO_ERR_ARG;
    const size_t need = (size_t)seg_w * seg_h * 3;
    run_threads(n, n_threads, [&](int i) {
        const Desc d{desc[2 * i], desc[2 * i + 1]};
        if (!desc_ok(d)) { status[i] = ST_DESC; return; }
        std::vector<uint8_t> px(need);
        std::vector<uint32_t> start(TABLE + 1);
        status[i] = decode_segment(data + d.off, d.len, seg_h, seg_w, predictor, px.data(), start.data());
        if (status[i]) return;
        const int sx = place[2 * i], sy = place[2 * i + 1];
        Window w;
        if (!place_window(sx, sy, seg_w, seg_h, H, W, clip, w)) return;
        for (int y = w.y0; y < w.y1; ++y)
            memcpy(canvas + ((size_t)(sy + y) * W + (size_t)(sx + w.x0)) * 3, px.data() + ((size_t)y * seg_w + w.x0) * 3, (size_t)(w.x1 - w.x0) * 3);
    });
    return BQIO_OK;
}

}  // extern "C"
