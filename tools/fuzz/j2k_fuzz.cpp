// Sanitizer run of the JPEG 2000 extractor (tier 2) and the CPU statement of the device decoder (CPU only):
//   g++ -O1 -g -fsanitize=address,undefined -ffp-contract=off -DBQK_CONTRACT_OFF j2k_fuzz.cpp -o j2k_fuzz -lpthread
// (the two last flags matter where the target has a fused multiply-add; csrc/j2k_device.h refuses such a build without them)
//   ./j2k_fuzz ITERS case.bqjk [case.bqjk ...]          (tools/fuzz/make_j2k_corpus.py writes the files and their format)
// First every case as it is: its segments go through bqio_j2k_extract and bqio_j2k_decode_canvas side by side into a canvas 10
// pixels larger on every side; every segment must have the status the case file states, a decoded one must give Pillow's pixels
// (equal, or within one level for an irreversible stream), a refused one and the margin must stay white.  Then ITERS mutations:
// byte flips in the headers and in the packets, truncations, changed fields of the packed descriptors and block rows, places
// that push segments partly and wholly outside the canvas, clip rectangles of any kind, canvases of any small size.  Heap
// buffers of EXACTLY the sizes asked for; the canvas stands between guard rows.  The pair may decode, answer with a status or
// refuse; it may never touch a guard row or a pixel outside the clip rectangle, and it must come back.
#include "../../biscuit_amd/csrc/j2k_host.cpp"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <memory>

struct Case {
    uint32_t w, h, n, ycc, exact;
    std::vector<std::vector<uint8_t>> segs;
    std::vector<uint32_t> status;
    std::vector<uint8_t> pixels;
};

static bool load(const char* path, Case& c) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (d.size() < 24 || memcmp(d.data(), "BQJK", 4) != 0) return false;
    uint32_t h[5];
    memcpy(h, d.data() + 4, 20);
    c.w = h[0]; c.h = h[1]; c.n = h[2]; c.ycc = h[3]; c.exact = h[4];
    size_t at = 24;
    if (c.n < 1 || c.n > 64 || d.size() < at + 8 * (size_t)c.n) return false;
    std::vector<uint32_t> len(c.n);
    c.status.resize(c.n);
    memcpy(len.data(), d.data() + at, 4 * (size_t)c.n);
    memcpy(c.status.data(), d.data() + at + 4 * (size_t)c.n, 4 * (size_t)c.n);
    at += 8 * (size_t)c.n;
    for (uint32_t i = 0; i < c.n; ++i) {
        if (d.size() < at + len[i]) return false;
        c.segs.emplace_back(d.begin() + (long)at, d.begin() + (long)(at + len[i]));
        at += len[i];
    }
    if (d.size() != at + (size_t)c.n * c.w * c.h * 3) return false;
    c.pixels.assign(d.begin() + (long)at, d.end());
    return true;
}

struct Packed {
    std::vector<int32_t> desc;
    std::unique_ptr<int32_t[]> blocks;
    std::unique_ptr<uint8_t[]> bytes;
    int64_t nb = 0;
    size_t nbytes = 0;
};

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(1); }

// exact-size buffers filled by a probe and a second call
static void extract(const std::vector<std::vector<uint8_t>>& segs, int seg_w, int seg_h, int threads, Packed& P) {
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
    P.desc.assign(segs.size() * bqj2k::SEG_I32, 0);
    if (bqio_j2k_extract(data.get(), total, off.data(), len.data(), (int64_t)segs.size(), seg_w, seg_h, P.desc.data(), nullptr, 0, nullptr, 0,
                         &P.nb, &P.nbytes, threads) != BQIO_OK) die("the probe refused its arguments");
    P.blocks.reset(new int32_t[(size_t)(P.nb ? P.nb : 1) * bqj2k::BLOCK_I32]);
    P.bytes.reset(new uint8_t[P.nbytes ? P.nbytes : 1]);
    int64_t nb2 = 0;
    size_t by2 = 0;
    std::vector<int32_t> first = P.desc;
    if (P.nb && (bqio_j2k_extract(data.get(), total, off.data(), len.data(), (int64_t)segs.size(), seg_w, seg_h, P.desc.data(), P.blocks.get(), P.nb,
                                  P.bytes.get(), P.nbytes, &nb2, &by2, 1) != BQIO_OK || nb2 != P.nb || by2 != P.nbytes || first != P.desc))
        die("second pass differs");
}

constexpr int GUARD = 3;                 // rows in front of and behind the canvas
constexpr uint8_t GUARD_BYTE = 0xA5;

// canvas H x W between guard rows, decoded into; exits on a touched guard or a pixel changed outside canvas-and-clip
static void decode_checked(const Packed& P, int n, int seg_w, int seg_h, int ycc, const std::vector<int32_t>& place, int H, int W,
                           const int32_t* clip, int threads, std::vector<uint8_t>& canvas, std::vector<int32_t>& status) {
    const size_t row = (size_t)W * 3;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)(H + 2 * GUARD) * row]);
    memset(buf.get(), GUARD_BYTE, (size_t)GUARD * row);
    memset(buf.get() + (size_t)GUARD * row, 255, (size_t)H * row);
    memset(buf.get() + (size_t)(GUARD + H) * row, GUARD_BYTE, (size_t)GUARD * row);
    std::unique_ptr<int32_t[]> st(new int32_t[n ? n : 1]);
    std::unique_ptr<int32_t[]> pl(new int32_t[n ? 2 * n : 1]);
    if (n) memcpy(pl.get(), place.data(), sizeof(int32_t) * 2 * (size_t)n);
    if (bqio_j2k_decode_canvas(P.desc.data(), n, P.blocks.get(), P.nb, P.bytes.get(), P.nbytes, seg_w, seg_h, ycc, pl.get(),
                               buf.get() + (size_t)GUARD * row, H, W, clip, st.get(), nullptr, threads) != BQIO_OK)
        die("canvas decode refused its arguments");
    for (size_t i = 0; i < (size_t)GUARD * row; ++i)
        if (buf[i] != GUARD_BYTE || buf[(size_t)(GUARD + H) * row + i] != GUARD_BYTE) die("guard row touched");
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
    if (argc < 3) { fprintf(stderr, "usage: j2k_fuzz ITERS case.bqjk ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    srand(777);
    std::vector<Case> cases(argc - 2);
    for (int a = 2; a < argc; ++a)
        if (!load(argv[a], cases[(size_t)a - 2])) { fprintf(stderr, "%s: not a case file\n", argv[a]); return 2; }
    // ---- every case as it is
    long decoded = 0, refusals = 0;
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case& c = cases[ci];
        Packed P;
        extract(c.segs, (int)c.w, (int)c.h, 3, P);
        const int M = 10, H = (int)c.h + 2 * M, W = (int)(c.n * c.w) + 2 * M;
        std::vector<int32_t> place;
        for (uint32_t i = 0; i < c.n; ++i) { place.push_back((int32_t)(i * c.w) + M); place.push_back(M); }
        const int32_t clip[4] = {M, M, W - M, H - M};
        std::vector<uint8_t> canvas;
        std::vector<int32_t> status;
        decode_checked(P, (int)c.n, (int)c.w, (int)c.h, (int)c.ycc, place, H, W, clip, 3, canvas, status);
        for (uint32_t i = 0; i < c.n; ++i) {
            if (status[i] != (int32_t)c.status[i] || P.desc[(size_t)i * bqj2k::SEG_I32] != (int32_t)c.status[i]) {
                fprintf(stderr, "%s: segment %u has status %d, %u expected\n", argv[2 + ci], i, status[i], c.status[i]);
                return 1;
            }
            for (uint32_t y = 0; y < c.h; ++y)
                for (uint32_t x = 0; x < 3 * c.w; ++x) {
                    const int got = canvas[((size_t)(y + M) * W + M + (size_t)i * c.w) * 3 + x];
                    const int want = c.pixels[((size_t)i * c.h + y) * c.w * 3 + x];
                    if (abs(got - want) > (c.exact ? 0 : 1)) {
                        fprintf(stderr, "%s: segment %u, row %u, byte %u: %d, the case file says %d\n", argv[2 + ci], i, y, x, got, want);
                        return 1;
                    }
                }
            if (c.status[i]) ++refusals; else ++decoded;
        }
    }
    // ---- mutations
    long ok = 0, with_status = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        const Case& c = cases[(size_t)it % cases.size()];
        std::vector<std::vector<uint8_t>> segs;
        std::vector<int32_t> place;
        const int n = 1 + rand() % 3;
        for (int k = 0; k < n; ++k) {
            const uint32_t i = (uint32_t)rand() % c.n;
            segs.push_back(c.segs[i]);
            place.push_back((int32_t)(k * c.w));
            place.push_back(0);
        }
        const int kind = rand() % 10;
        std::vector<uint8_t>& victim = segs[(size_t)rand() % segs.size()];
        if (kind < 3) {                                        // anywhere: mostly packet bytes
            for (int k = rand() % 4 + 1; k > 0; --k) victim[(size_t)rand() % victim.size()] = (uint8_t)rand();
        } else if (kind == 3) {
            victim.resize((size_t)rand() % victim.size() + 1);
        } else if (kind < 6) {                                 // a header field: sizes, COD, QCD, the tile part
            victim[2 + (size_t)rand() % (victim.size() < 140 ? victim.size() - 2 : 140)] = (uint8_t)rand();
        }                                                      // (6..9: the streams as they are; the tables or the geometry below)
        int H = 1 + rand() % (3 * (int)c.h), W = 1 + rand() % (3 * (int)c.w);
        for (auto& v : place)
            if (rand() % 3 == 0) v = rand() % 2 ? wild() : v + rand() % (2 * (int)c.w) - (int)c.w;
        int32_t clip[4] = {0, 0, W, H};
        for (int k = 0; k < 4; ++k)
            if (rand() % 3 == 0) clip[k] = rand() % 2 ? wild() : rand() % (W + H) - 8;
        Packed P;
        extract(segs, (int)c.w, (int)c.h, 1 + it % 3, P);
        bool all_refused = true;
        for (int k = 0; k < n; ++k) all_refused &= P.desc[(size_t)k * bqj2k::SEG_I32] != 0;
        if (kind == 6 && P.nb) {                               // a row of the block table
            P.blocks[(size_t)(rand() % P.nb) * bqj2k::BLOCK_I32 + (size_t)rand() % bqj2k::BLOCK_I32] = rand() % 2 ? wild() : rand() % 70;
        } else if (kind == 7) {                                // a descriptor
            P.desc[(size_t)(rand() % n) * bqj2k::SEG_I32 + 1 + (size_t)rand() % 7] = rand() % 2 ? wild() : rand() % 8;
        }
        std::vector<uint8_t> canvas;
        std::vector<int32_t> status;
        decode_checked(P, n, (int)c.w, (int)c.h, (int)c.ycc, place, H, W, clip, 1, canvas, status);   // (places may overlap: one thread)
        bool any = false;
        for (int32_t s : status) any |= s != 0;
        if (all_refused) ++refused; else if (any) ++with_status; else ++ok;
    }
    printf("%ld segments equal to the case files, %ld refusals as expected; %d mutations: %ld decoded, %ld with a status, %ld refused\n", decoded,
           refusals, iters, ok, with_status, refused);
    return 0;
}
