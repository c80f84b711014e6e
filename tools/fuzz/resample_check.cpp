// bqio_resample_taps / bqio_tile_resample (csrc/resample_host.cpp over csrc/resample_device.h -- the routines the GPU kernel is
// compiled from) under AddressSanitizer + UndefinedBehaviorSanitizer: every case file holds a canvas, tile origins (inside the
// canvas, partly and wholly outside) and the bytes Pillow gave; canvas, origins, tables and output live in heap buffers of
// EXACTLY their sizes, so a read or write past an end is a report.  Usage: resample_check CASE...   (tests/test_sanitizers_resample.py
// writes the cases: int32 H, W, n, src_px, px; canvas [H][W][3]; origin int32 [n][2]; expected [n][px][px][3])
#include "../../biscuit_amd/csrc/resample_host.cpp"

#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <memory>

int main(int argc, char** argv) {
    long long mismatches = 0, tiles = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        int32_t hd[5];
        if (raw.size() < sizeof hd) { fprintf(stderr, "%s: short file\n", argv[a]); return 2; }
        memcpy(hd, raw.data(), sizeof hd);
        const int H = hd[0], W = hd[1], n = hd[2], src = hd[3], px = hd[4];
        const size_t nc = (size_t)H * W * 3, no = (size_t)n * 2 * 4, ne = (size_t)n * px * px * 3;
        if (raw.size() != sizeof hd + nc + no + ne) { fprintf(stderr, "%s: size mismatch\n", argv[a]); return 2; }
        std::unique_ptr<uint8_t[]> canvas(new uint8_t[nc]), out(new uint8_t[ne]);
        std::unique_ptr<int32_t[]> origin(new int32_t[(size_t)n * 2]);
        memcpy(canvas.get(), raw.data() + sizeof hd, nc);
        memcpy(origin.get(), raw.data() + sizeof hd + nc, no);
        const uint8_t* want = reinterpret_cast<const uint8_t*>(raw.data()) + sizeof hd + nc + no;
        const int k = bqio_resample_ksize(src, px);
        if (k <= 0) { fprintf(stderr, "%s: ksize %d\n", argv[a], k); return 2; }
        std::unique_ptr<int32_t[]> bounds(new int32_t[(size_t)px * 2]), coef(new int32_t[(size_t)px * k]);
        if (bqio_resample_taps(src, px, bounds.get(), coef.get(), k) != k) { fprintf(stderr, "%s: taps failed\n", argv[a]); return 2; }
        if (bqio_resample_taps(src, px, bounds.get(), coef.get(), k - 1) >= 0) { fprintf(stderr, "short table accepted\n"); return 2; }
        memset(out.get(), 0x5a, ne);
        if (bqio_tile_resample(canvas.get(), H, W, origin.get(), n, src, px, out.get()) != BQIO_OK) { fprintf(stderr, "%s: resample failed\n", argv[a]); return 2; }
        for (int t = 0; t < n; ++t) {
            ++tiles;
            if (memcmp(out.get() + (size_t)t * px * px * 3, want + (size_t)t * px * px * 3, (size_t)px * px * 3) != 0) {
                ++mismatches;
                fprintf(stderr, "%s: tile %d differs from Pillow\n", argv[a], t);
            }
        }
        // refusals leave the output alone
        if (bqio_tile_resample(canvas.get(), H, W, origin.get(), -1, src, px, out.get()) >= 0 ||
            bqio_tile_resample(canvas.get(), H, W, origin.get(), n, 9 * px, px, out.get()) >= 0 ||
            bqio_tile_resample(canvas.get(), H, W, origin.get(), n, src, 0, out.get()) >= 0) { fprintf(stderr, "a refusal was accepted\n"); return 2; }
    }
    printf("tiles %lld mismatches %lld\n", tiles, mismatches);
    return mismatches ? 1 : 0;
}
