// A program of its own over csrc/png_encode_device.h, for a build with -fsanitize=address,undefined (tests/test_png_encode.py
// builds and runs it): flats, an LCG noise tile and a ramp at 1, 5, 74 and 299 px through the header's serial encoder; every
// file's chunks are walked (CRC-32 through zlib's crc32), the IDAT payloads inflated with zlib and un-filtered back to the tile.
// And the round rule the encoder's entry point shares with the other codecs (csrc/bq_rounds.h) against the expression it replaced.
#include "bq_rounds.h"
#include "png_encode_device.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fail(const char* what, int px, int kind) {
    std::printf("FAILED: %s (px %d, content %d)\n", what, px, kind);
    return 1;
}

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static int check(const std::vector<uint8_t>& tile, int px, int kind) {
    std::vector<uint8_t> file;
    bqpe::serial_encode(tile.data(), px, file);
    const bqpe::Geom G = bqpe::geom_of(px);
    if (file.size() > (size_t)G.L + G.L / 256 + 128) return fail("larger than L + L / 256 + 128", px, kind);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (file.size() < 8 || memcmp(file.data(), sig, 8)) return fail("signature", px, kind);
    std::vector<uint8_t> z;
    size_t p = 8;
    int nchunk = 0;
    bool end = false;
    while (p + 12 <= file.size()) {
        const uint32_t n = be32(&file[p]);
        if (p + 12 + n > file.size()) return fail("chunk runs beyond the file", px, kind);
        if ((uint32_t)crc32(0, &file[p + 4], n + 4) != be32(&file[p + 8 + n])) return fail("chunk CRC", px, kind);
        if (nchunk == 0 && (memcmp(&file[p + 4], "IHDR", 4) || n != 13 || be32(&file[p + 8]) != (uint32_t)px)) return fail("IHDR", px, kind);
        if (!memcmp(&file[p + 4], "IDAT", 4)) z.insert(z.end(), &file[p + 8], &file[p + 8] + n);
        end = !memcmp(&file[p + 4], "IEND", 4);
        p += 12 + n;
        ++nchunk;
    }
    if (p != file.size() || !end) return fail("chunk walk", px, kind);
    std::vector<uint8_t> rows(G.L);
    uLongf got = G.L;
    if (uncompress(rows.data(), &got, z.data(), (uLong)z.size()) != Z_OK || got != G.L) return fail("zlib refuses the stream", px, kind);
    std::vector<uint8_t> back((size_t)px * px * 3);
    const uint32_t rb = 3 * (uint32_t)px;
    for (int y = 0; y < px; ++y) {
        const uint8_t* r = &rows[(size_t)y * G.rl];
        uint8_t* cur = &back[(size_t)y * rb];
        const uint8_t* prev = y ? cur - rb : nullptr;
        for (uint32_t i = 0; i < rb; ++i) {
            const int a = i >= 3 ? cur[i - 3] : 0, b = prev ? prev[i] : 0, c = (prev && i >= 3) ? prev[i - 3] : 0;
            int pred;
            switch (r[0]) {
                case 0: pred = 0; break;
                case 1: pred = a; break;
                case 2: pred = b; break;
                case 4: pred = bqpe::paeth(a, b, c); break;
                default: return fail("filter type", px, kind);
            }
            cur[i] = (uint8_t)(r[1 + i] + pred);
        }
    }
    if (back != tile) return fail("pixels", px, kind);
    return 0;
}

// round_items over scratch sizes around one item, around `align` items and beyond the cap, for the aligns and per-item sizes in use
static int check_rounds() {
    for (size_t per : {(size_t)1, (size_t)7, (size_t)393216})
        for (size_t align : {(size_t)1, (size_t)64})
            for (size_t s : {(size_t)0, per - 1, per, 63 * per, 64 * per, 100 * per, 40000 * per}) {
                size_t m = s / per;
                if (m > 32768) m = 32768;
                if (m >= align) m &= ~(align - 1);
                if (round_items(s, per, align) != m) {
                    std::printf("FAILED: round_items(%zu, %zu, %zu) = %zu, not %zu\n", s, per, align, round_items(s, per, align), m);
                    return 1;
                }
            }
    return round_cap(3, 256) == 3 && round_cap(256, 256) == 256 && round_cap(300, 256) == 256 ? 0 : 1;
}

int main() {
    const int sizes[4] = {1, 5, 74, 299};
    int bad = check_rounds(), files = 0;
    for (int px : sizes) {
        std::vector<uint8_t> t((size_t)px * px * 3);
        for (int kind = 0; kind < 5; ++kind) {
            uint32_t lcg = 12345u + (uint32_t)px;
            for (size_t k = 0; k < t.size(); ++k) {
                const size_t pixel = k / 3, x = pixel % (size_t)px, y = pixel / (size_t)px;
                switch (kind) {
                    case 0: t[k] = 0; break;
                    case 1: t[k] = 128; break;
                    case 2: t[k] = 255; break;
                    case 3: lcg = lcg * 1664525u + 1013904223u; t[k] = (uint8_t)(lcg >> 24); break;
                    default: t[k] = (uint8_t)((x + 2 * y + 40 * (k % 3)) * 255 / (3 * (size_t)px + 80)); break;
                }
            }
            bad += check(t, px, kind);
            ++files;
        }
    }
    if (bad) return 1;
    std::printf("ok: %d files\n", files);
    return 0;
}
