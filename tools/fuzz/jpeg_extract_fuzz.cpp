// Sanitizer fuzz of the device JPEG decoder's host half and of its shared routines (CPU only):
//   g++ -O1 -g -fsanitize=address,undefined jpeg_extract_fuzz.cpp -o jpeg_extract_fuzz -lz -lpthread
//   ./jpeg_extract_fuzz ITERS file.jpg [file.jpg ...]          (tools/fuzz/make_jpeg_corpus.py writes the files)
// Mutates valid JPEG files as jpeg_fuzz.cpp does (byte flips, splices, truncations, marker injections, the scan cut to a few
// bytes in front of a valid EOI), writes them as the records of a TFRecord file, and takes each through bqio_extract_jpeg into
// heap buffers of EXACTLY the sizes it asks for, then through bqio_jpeg_decode_extracted -- the routines of
// csrc/jpeg_device.h, the ones the GPU kernels are compiled from -- with a coefficient space, an output and a status of exactly
// their sizes.  The pair may accept, refuse or answer with a status; it may never read or write outside those buffers, and it
// must come back.  Agreement of accepted streams with libjpeg is what tests/test_jpeg_extract.py checks.
#include "../../biscuit_amd/csrc/tfrecord_reader.cpp"

#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>

static void put_varint(std::vector<uint8_t>& o, uint64_t v) {
    while (v >= 0x80) { o.push_back((uint8_t)(v | 0x80)); v >>= 7; }
    o.push_back((uint8_t)v);
}
static void put_bytes(std::vector<uint8_t>& o, int field, const std::vector<uint8_t>& b) {
    put_varint(o, (uint64_t)(field << 3 | 2));
    put_varint(o, b.size());
    o.insert(o.end(), b.begin(), b.end());
}
// tf.train.Example { features { feature { key: "image_raw" value { bytes_list { value: image } } } } }
static std::vector<uint8_t> example_of(const std::vector<uint8_t>& image) {
    std::vector<uint8_t> bl, feat, entry, feats, ex;
    put_bytes(bl, 1, image);
    put_bytes(feat, 1, bl);
    const char* k = "image_raw";
    put_bytes(entry, 1, std::vector<uint8_t>(k, k + 9));
    put_bytes(entry, 2, feat);
    put_bytes(feats, 1, entry);
    put_bytes(ex, 1, feats);
    return ex;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: jpeg_extract_fuzz ITERS file.jpg ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    srand(4242);
    std::vector<std::vector<uint8_t>> files;
    std::vector<int> px;
    for (int a = 2; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        files.emplace_back((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const auto& d = files.back();
        int w = 0;
        for (size_t i = 2; i + 9 < d.size(); ++i)
            if (d[i] == 0xFF && (d[i + 1] == 0xC0 || d[i + 1] == 0xC1 || d[i + 1] == 0xC2)) { w = (d[i + 7] << 8) | d[i + 8]; break; }
        px.push_back(w);
    }
    char path[] = "/tmp/bq_jpeg_extract_fuzz_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { perror("mkstemp"); return 2; }
    close(fd);
    long ok = 0, status = 0, refused = 0, wrong = 0;
    const int BATCH = 32;
    for (int it0 = 0; it0 < iters; it0 += BATCH) {
        const int nb = iters - it0 < BATCH ? iters - it0 : BATCH;
        std::vector<int> tile_px;
        {
            std::ofstream out(path, std::ios::binary | std::ios::trunc);
            for (int it = it0; it < it0 + nb; ++it) {
                const size_t fi = (size_t)it % files.size();
                std::vector<uint8_t> d = files[fi];
                const int kind = rand() % 10;
                if (kind < 4) {
                    for (int k = rand() % 4 + 1; k > 0; --k) d[(size_t)rand() % d.size()] = (uint8_t)rand();
                } else if (kind == 4) {
                    d.resize((size_t)rand() % d.size() + 1);
                } else if (kind == 5) {                       // splice a stretch of the file over another place
                    const size_t n = (size_t)rand() % 64 + 1, a = (size_t)rand() % (d.size() - n), b = (size_t)rand() % (d.size() - n);
                    memmove(d.data() + a, d.data() + b, n);
                } else if (kind == 8 || kind == 9) {          // the scan cut down (8: to a few bytes), the EOI kept
                    size_t sos = 0;
                    for (size_t i = 2; i + 3 < d.size(); ++i) if (d[i] == 0xFF && d[i + 1] == 0xDA) { sos = i; break; }
                    if (sos) {
                        const size_t hdr = sos + 2 + ((d[sos + 2] << 8) | d[sos + 3]);
                        if (hdr < d.size()) {
                            const size_t keep = kind == 8 ? (size_t)rand() % 40 : (size_t)rand() % (d.size() - hdr);
                            std::vector<uint8_t> e(d.begin(), d.begin() + (hdr + keep < d.size() ? hdr + keep : hdr));
                            for (size_t i = hdr; i < e.size(); ++i) if (e[i] == 0xFF) e[i] = 0x7F;  // no markers inside what is kept
                            e.push_back(0xFF); e.push_back(0xD9);
                            d.swap(e);
                        }
                    }
                } else if (kind == 6) {                       // a marker where there was data
                    const size_t a = (size_t)rand() % (d.size() - 1);
                    d[a] = 0xFF; d[a + 1] = (uint8_t)(0xC0 + rand() % 64);
                } else {                                      // header fields: sizes, sampling, table ids, table bytes
                    const size_t a = 2 + (size_t)rand() % (d.size() < 700 ? d.size() - 2 : 700);
                    d[a] = (uint8_t)rand();
                }
                const std::vector<uint8_t> ex = example_of(d);
                const uint64_t len = ex.size();
                const uint32_t zero = 0;                      // (the reader is opened without CRC verification)
                out.write((const char*)&len, 8); out.write((const char*)&zero, 4);
                out.write((const char*)ex.data(), (std::streamsize)ex.size()); out.write((const char*)&zero, 4);
                tile_px.push_back(px[fi]);
            }
        }
        bqio_reader* r = bqio_open(path, BQIO_VERIFY_NONE);
        if (!r || bqio_count(r) != nb) { fprintf(stderr, "cannot read the batch back\n"); return 2; }
        for (int i = 0; i < nb; ++i) {
            const int p = tile_px[(size_t)i];
            size_t used = 0;
            int nt = 0;
            int64_t bad = -1;
            int e = bqio_extract_jpeg(r, i, 1, p, nullptr, 0, nullptr, nullptr, 0, &nt, nullptr, &used, 1 + i % 3, &bad);
            if (e == BQIO_ERR_FORMAT) { ++wrong; continue; }
            if (e != BQIO_OK) { ++refused; continue; }
            // exact-size heap buffers: any overrun is the sanitizer's
            std::unique_ptr<uint8_t[]> scan(new uint8_t[used]), tables(new uint8_t[(size_t)nt * bqio_jpeg_table_bytes()]);
            uint32_t desc[4];
            e = bqio_extract_jpeg(r, i, 1, p, scan.get(), used, desc, tables.get(), nt, &nt, nullptr, &used, 1, &bad);
            if (e != BQIO_OK || desc[0] + (size_t)desc[1] + bqio_jpeg_ecs_pad() > used) { fprintf(stderr, "second pass differs\n"); return 1; }
            std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)p * p * 3]);
            int32_t st = -1;
            if (bqio_jpeg_decode_extracted(scan.get(), desc, tables.get(), nt, 1, p, out.get(), &st, 1) != BQIO_OK) return 1;
            if (st == 0) ++ok; else ++status;
        }
        bqio_close(r);
    }
    unlink(path);
    printf("%d mutated files: %ld decoded, %ld with a status, %ld refused, %ld of another size\n", iters, ok, status, refused, wrong);
    return 0;
}
