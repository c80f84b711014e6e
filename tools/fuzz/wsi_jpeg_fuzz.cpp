// Sanitizer run of the slide-segment extractor and the CPU canvas decode (CPU only):
//   g++ -O1 -g -fsanitize=address,undefined wsi_jpeg_fuzz.cpp -o wsi_jpeg_fuzz -lz -lpthread
//   ./wsi_jpeg_fuzz ITERS case.bqsg [case.bqsg ...]          (tools/fuzz/make_wsi_jpeg_corpus.py writes the files and their format)
// First every case as it is: a page that decodes goes through bqio_extract_jpeg_segments and bqio_jpeg_decode_canvas into a canvas
// 10 pixels larger than the page on every side and must give Pillow's page (the case file holds it) inside and white around it; a
// page with a segment outside the subset must be refused with that segment's index.  Then ITERS mutations: byte flips and
// truncations of a segment or of the tables, places that push segments partly and wholly outside the canvas, clip rectangles of
// any kind, canvases of any small size.  Heap buffers of EXACTLY the sizes asked for; the canvas stands between guard rows.  The
// pair may accept, refuse or answer with a status; it may never touch a guard row or a pixel outside the clip rectangle, and it
// must come back.
#include "../../biscuit_amd/csrc/tfrecord_reader.cpp"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>

struct Case {
    uint32_t seg_w, seg_h, page_w, page_h, across, n, expect_bad;
    std::vector<uint8_t> tables;
    std::vector<std::vector<uint8_t>> segs;
    std::vector<uint8_t> page;
};

static bool load(const char* path, Case& c) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (d.size() < 36 || memcmp(d.data(), "BQSG", 4) != 0) return false;
    uint32_t h[8];
    memcpy(h, d.data() + 4, 32);
    c.seg_w = h[0]; c.seg_h = h[1]; c.page_w = h[2]; c.page_h = h[3]; c.across = h[4]; c.n = h[5]; c.expect_bad = h[7];
    size_t at = 36;
    if (c.n > 4096 || d.size() < at + 4 * (size_t)c.n) return false;
    std::vector<uint32_t> len(c.n);
    if (c.n) memcpy(len.data(), d.data() + at, 4 * (size_t)c.n);
    at += 4 * (size_t)c.n;
    if (d.size() < at + h[6]) return false;
    c.tables.assign(d.begin() + (long)at, d.begin() + (long)(at + h[6]));
    at += h[6];
    for (uint32_t i = 0; i < c.n; ++i) {
        if (d.size() < at + len[i]) return false;
        c.segs.emplace_back(d.begin() + (long)at, d.begin() + (long)(at + len[i]));
        at += len[i];
    }
    if (c.expect_bad == 0xFFFFFFFFu) {
        const size_t need = (size_t)c.page_w * c.page_h * 3;
        if (d.size() != at + need) return false;
        c.page.assign(d.begin() + (long)at, d.end());
    }
    return true;
}

struct Packed {
    std::unique_ptr<uint8_t[]> scan, tables;
    std::vector<uint32_t> desc;
    int nt = 0;
};

// BQIO_OK with exact-size buffers filled, or the extractor's error (*bad = the segment)
static int extract(const std::vector<uint8_t>& tables, const std::vector<std::vector<uint8_t>>& segs, int seg_w, int seg_h, int threads,
                   Packed& P, int64_t* bad) {
    size_t total = 0;
    for (auto& s : segs) total += s.size();
    std::unique_ptr<uint8_t[]> data(new uint8_t[total ? total : 1]);
    std::vector<uint64_t> off(segs.size()), len(segs.size());
    size_t at = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        off[i] = at; len[i] = segs[i].size();
        if (len[i]) memcpy(data.get() + at, segs[i].data(), len[i]);
        at += len[i];
    }
    std::unique_ptr<uint8_t[]> tb(new uint8_t[tables.size() ? tables.size() : 1]);
    if (!tables.empty()) memcpy(tb.get(), tables.data(), tables.size());
    size_t used = 0;
    int nt = 0;
    int e = bqio_extract_jpeg_segments(data.get(), total, off.data(), len.data(), (int64_t)segs.size(), tables.empty() ? nullptr : tb.get(),
                                       tables.size(), seg_w, seg_h, nullptr, 0, nullptr, nullptr, 0, &nt, &used, threads, bad);
    if (e != BQIO_OK) return e;
    P.scan.reset(new uint8_t[used ? used : 1]);
    P.tables.reset(new uint8_t[(size_t)(nt ? nt : 1) * bqio_jpeg_table_bytes()]);
    P.desc.assign(4 * segs.size(), 0);
    size_t used2 = 0;
    e = bqio_extract_jpeg_segments(data.get(), total, off.data(), len.data(), (int64_t)segs.size(), tables.empty() ? nullptr : tb.get(),
                                   tables.size(), seg_w, seg_h, P.scan.get(), used, P.desc.data(), P.tables.get(), nt, &P.nt, &used2, 1, bad);
    if (e != BQIO_OK || used2 != used || P.nt != nt) { fprintf(stderr, "second pass differs\n"); exit(1); }
    for (size_t i = 0; i < segs.size(); ++i)
        if (P.desc[4 * i] + (size_t)P.desc[4 * i + 1] + bqio_jpeg_ecs_pad() > used) { fprintf(stderr, "descriptor outside the scan\n"); exit(1); }
    return BQIO_OK;
}

constexpr int GUARD = 3;                 // rows in front of and behind the canvas
constexpr uint8_t GUARD_BYTE = 0xA5;

// canvas H x W between guard rows, decoded into; exits on a touched guard or a pixel changed outside canvas-and-clip
static void decode_checked(const Packed& P, int n, int seg_w, int seg_h, const std::vector<int32_t>& place, int H, int W, const int32_t* clip,
                           int threads, std::vector<uint8_t>& canvas, std::vector<int32_t>& status) {
    const size_t row = (size_t)W * 3;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)(H + 2 * GUARD) * row]);
    memset(buf.get(), GUARD_BYTE, (size_t)GUARD * row);
    memset(buf.get() + (size_t)GUARD * row, 255, (size_t)H * row);
    memset(buf.get() + (size_t)(GUARD + H) * row, GUARD_BYTE, (size_t)GUARD * row);
    std::unique_ptr<int32_t[]> st(new int32_t[n ? n : 1]);
    std::unique_ptr<int32_t[]> pl(new int32_t[n ? 2 * n : 1]);
    if (n) memcpy(pl.get(), place.data(), sizeof(int32_t) * 2 * (size_t)n);
    if (bqio_jpeg_decode_canvas(P.scan.get(), P.desc.data(), P.tables.get(), P.nt, n, seg_w, seg_h, pl.get(), buf.get() + (size_t)GUARD * row, H, W,
                                clip, st.get(), threads) != BQIO_OK) { fprintf(stderr, "canvas decode refused its arguments\n"); exit(1); }
    for (size_t i = 0; i < (size_t)GUARD * row; ++i)
        if (buf[i] != GUARD_BYTE || buf[(size_t)(GUARD + H) * row + i] != GUARD_BYTE) { fprintf(stderr, "guard row touched\n"); exit(1); }
    const uint8_t* cv = buf.get() + (size_t)GUARD * row;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if (x >= clip[0] && x < clip[2] && y >= clip[1] && y < clip[3]) continue;
            const uint8_t* p = cv + (size_t)y * row + 3 * (size_t)x;
            if (p[0] != 255 || p[1] != 255 || p[2] != 255) { fprintf(stderr, "pixel (%d, %d) outside the clip rectangle written\n", x, y); exit(1); }
        }
    canvas.assign(cv, cv + (size_t)H * row);
    status.assign(st.get(), st.get() + n);
}

static int32_t wild() {
    switch (rand() % 6) {
        case 0: return INT_MIN + rand() % 3;
        case 1: return INT_MAX - rand() % 3;
        case 2: return -(rand() % 100000);
        case 3: return rand() % 100000;
        default: return rand() % 700 - 350;
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: wsi_jpeg_fuzz ITERS case.bqsg ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    srand(777);
    std::vector<Case> cases(argc - 2);
    for (int a = 2; a < argc; ++a)
        if (!load(argv[a], cases[(size_t)a - 2])) { fprintf(stderr, "%s: not a case file\n", argv[a]); return 2; }
    // ---- every case as it is
    long pages = 0, refusals = 0;
    std::vector<size_t> good;
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case& c = cases[ci];
        Packed P;
        int64_t bad = -1;
        const int e = extract(c.tables, c.segs, (int)c.seg_w, (int)c.seg_h, 3, P, &bad);
        if (c.expect_bad != 0xFFFFFFFFu) {
            if ((e != BQIO_ERR_UNSUPPORTED && e != BQIO_ERR_FORMAT) || bad != (int64_t)c.expect_bad) {
                fprintf(stderr, "%s: error %d at segment %lld, refusal of segment %u expected\n", argv[2 + ci], e, (long long)bad, c.expect_bad);
                return 1;
            }
            ++refusals;
            continue;
        }
        if (e != BQIO_OK) { fprintf(stderr, "%s: refused (%d, segment %lld)\n", argv[2 + ci], e, (long long)bad); return 1; }
        const int M = 10, H = (int)c.page_h + 2 * M, W = (int)c.page_w + 2 * M;
        std::vector<int32_t> place;
        for (uint32_t i = 0; i < c.n; ++i) {
            place.push_back((int32_t)((i % c.across) * c.seg_w) + M);
            place.push_back((int32_t)((i / c.across) * c.seg_h) + M);
        }
        const int32_t clip[4] = {M, M, M + (int)c.page_w, M + (int)c.page_h};
        std::vector<uint8_t> canvas;
        std::vector<int32_t> status;
        decode_checked(P, (int)c.n, (int)c.seg_w, (int)c.seg_h, place, H, W, clip, 3, canvas, status);
        for (int32_t s : status)
            if (s) { fprintf(stderr, "%s: a segment answered with status %d\n", argv[2 + ci], s); return 1; }
        for (int y = 0; y < (int)c.page_h; ++y)
            if (memcmp(canvas.data() + ((size_t)(y + M) * W + M) * 3, c.page.data() + (size_t)y * c.page_w * 3, (size_t)c.page_w * 3) != 0) {
                fprintf(stderr, "%s: row %d differs from the page in the case file\n", argv[2 + ci], y);
                return 1;
            }
        ++pages;
        good.push_back(ci);
    }
    if (good.empty()) { fprintf(stderr, "no case that decodes\n"); return 2; }
    // ---- mutations
    long ok = 0, with_status = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        const Case& c = cases[good[(size_t)it % good.size()]];
        std::vector<std::vector<uint8_t>> segs;
        std::vector<int32_t> place;
        const int n = 1 + rand() % 3;
        for (int k = 0; k < n; ++k) {
            const uint32_t i = (uint32_t)rand() % c.n;
            segs.push_back(c.segs[i]);
            place.push_back((int32_t)((i % c.across) * c.seg_w));
            place.push_back((int32_t)((i / c.across) * c.seg_h));
        }
        std::vector<uint8_t> tables = c.tables;
        const int kind = rand() % 8;
        std::vector<uint8_t>& victim = (kind == 7 && !tables.empty()) ? tables : segs[(size_t)rand() % segs.size()];
        if (kind < 3 || kind == 7) {
            for (int k = rand() % 4 + 1; k > 0; --k) victim[(size_t)rand() % victim.size()] = (uint8_t)rand();
        } else if (kind == 3) {
            victim.resize((size_t)rand() % victim.size() + 1);
        } else if (kind == 4) {                               // a header field: sizes, sampling, table ids
            victim[2 + (size_t)rand() % (victim.size() < 200 ? victim.size() - 2 : 200)] = (uint8_t)rand();
        }                                                     // (5, 6: the streams as they are, only the geometry below)
        int H = 1 + rand() % (3 * (int)c.seg_h), W = 1 + rand() % (3 * (int)c.seg_w);
        for (auto& v : place)
            if (rand() % 3 == 0) v = rand() % 2 ? wild() : v + rand() % (2 * (int)c.seg_w) - (int)c.seg_w;
        int32_t clip[4] = {0, 0, W, H};
        for (int k = 0; k < 4; ++k)
            if (rand() % 3 == 0) clip[k] = rand() % 2 ? wild() : rand() % (W + H) - 8;
        Packed P;
        int64_t bad = -1;
        const int e = extract(tables, segs, (int)c.seg_w, (int)c.seg_h, 1 + it % 3, P, &bad);
        if (e != BQIO_OK) {
            if (bad < 0 || bad >= n) { fprintf(stderr, "refusal %d without a segment index\n", e); return 1; }
            ++refused;
            continue;
        }
        std::vector<uint8_t> canvas;
        std::vector<int32_t> status;
        decode_checked(P, n, (int)c.seg_w, (int)c.seg_h, place, H, W, clip, 1, canvas, status);   // (places may overlap: one thread)
        bool any = false;
        for (int32_t s : status) any |= s != 0;
        if (any) ++with_status; else ++ok;
    }
    printf("%ld pages equal to the case files, %ld refusals as expected; %d mutations: %ld decoded, %ld with a status, %ld refused\n", pages,
           refusals, iters, ok, with_status, refused);
    return 0;
}
