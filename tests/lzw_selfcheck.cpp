// lzw_selfcheck.cpp -- csrc/lzw_device.h as a host program of its own, for AddressSanitizer and UBSan (tests/test_lzw.py builds
// and runs it): valid streams from a built-in encoder must come back byte for byte; seeded mutations and truncations of them
// must end in a status or in `need` bytes, whatever they hold -- every buffer is an exact-size heap allocation (the stream `len`
// bytes, the output `need` bytes, the table 4097 words), so one byte read or written outside them stops the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "lzw_device.h"

using namespace bqlzw;

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Bits {
    std::vector<uint8_t> out; uint64_t acc = 0; int n = 0;
    void put(uint32_t code, int w) {
        acc = acc << w | code; n += w;
        while (n >= 8) { n -= 8; out.push_back((uint8_t)(acc >> n)); }
        acc &= (1ull << n) - 1;
    }
    std::vector<uint8_t> done() { if (n) out.push_back((uint8_t)(acc << (8 - n))); return out; }
};

// TIFF LZW as the header reads it; clear_at: the next free index at which a ClearCode goes out (0: never)
std::vector<uint8_t> encode(const std::vector<uint8_t>& data, int clear_at, bool eoi) {
    Bits b;
    std::map<std::pair<int, int>, int> table;
    int enc_n = FIRST, dec_n = FIRST, w = -1;
    bool fresh = true;
    auto emit = [&](int code) {
        b.put((uint32_t)code, width_for(dec_n));
        if (code == CLEAR) { dec_n = FIRST; fresh = true; }
        else if (fresh) fresh = false;
        else ++dec_n;
    };
    emit(CLEAR);
    for (uint8_t c : data) {
        if (w < 0) { w = c; continue; }
        auto it = table.find({w, c});
        if (it != table.end()) { w = it->second; continue; }
        emit(w);
        if (enc_n < TABLE) table[{w, c}] = enc_n;
        ++enc_n;
        w = c;
        if (clear_at && enc_n >= clear_at) { emit(CLEAR); table.clear(); enc_n = FIRST; }
    }
    if (w >= 0) emit(w);
    if (eoi) emit(EOI);
    return b.done();
}

std::vector<uint8_t> content(int kind, size_t n, Rng& r) {
    std::vector<uint8_t> d(n);
    for (size_t i = 0; i < n; ++i)
        d[i] = kind == 0 ? (uint8_t)r.next() : kind == 1 ? (uint8_t)200 : kind == 2 ? (uint8_t)(i / 7 + (r.next() & 3)) : (uint8_t)(i % 3 ? 9 : r.below(4));
    return d;
}

// one run in exact-size heap buffers: -> the status; *out_copy receives the output when the status is 0
int run(const std::vector<uint8_t>& stream, size_t len, uint32_t need, std::vector<uint8_t>* out_copy) {
    std::unique_ptr<uint8_t[]> raw(new uint8_t[len ? len : 1]);
    if (len) memcpy(raw.get(), stream.data(), len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[need]);
    std::unique_ptr<uint32_t[]> start(new uint32_t[TABLE + 1]);
    // (len == 0: a one-byte allocation of which nothing may be read)
    const int st = decode_serial(raw.get(), (uint32_t)len, need, out.get(), start.get());
    if (!st && out_copy) out_copy->assign(out.get(), out.get() + need);
    return st;
}

int fails = 0;
void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) { printf("FAIL %s (%ld, %ld)\n", what, a, b); ++fails; }
}

}  // namespace

int main() {
    Rng r{12345};
    long runs = 0, decoded = 0, by_status[32] = {0};
    // widths
    expect(width_for(258) == 9 && width_for(510) == 9 && width_for(511) == 10 && width_for(1022) == 10 && width_for(1023) == 11 &&
           width_for(2046) == 11 && width_for(2047) == 12 && width_for(5000) == 12, "width_for");
    const size_t sizes[] = {1, 2, 3, 64, 65, 700 * 3, 96 * 80 * 3};
    const int clears[] = {4094, 0, 300, 4096};
    for (int kind = 0; kind < 4; ++kind)
        for (size_t n : sizes)
            for (int clear_at : clears)
                for (int eoi = 0; eoi < 2; ++eoi) {
                    const std::vector<uint8_t> data = content(kind, n, r);
                    const std::vector<uint8_t> good = encode(data, clear_at, eoi != 0);
                    std::vector<uint8_t> back;
                    int st = run(good, good.size(), (uint32_t)n, &back);
                    ++runs;
                    // without a ClearCode the table may run to its end first: then, and only then, the refusal is ST_FULL
                    if (st == ST_FULL) expect(clear_at == 0 && n > 4000, "ST_FULL on a stream that clears", kind, (long)n);
                    else expect(st == 0 && back == data, "round trip", kind, (long)n);
                    // a shorter need: the last string is cut
                    if (n > 1) {
                        st = run(good, good.size(), (uint32_t)(n - 1), &back);
                        ++runs;
                        if (st != ST_FULL) expect(st == 0 && !memcmp(back.data(), data.data(), n - 1), "cut at need", kind, (long)n);
                    }
                    // a longer need: the data ends first
                    st = run(good, good.size(), (uint32_t)(n + 1), nullptr);
                    ++runs;
                    expect(st == ST_SHORT || st == ST_FULL, "longer need", st, (long)n);
                    // mutations and truncations
                    const int rounds = n > 5000 ? 300 : 100;
                    for (int m = 0; m < rounds; ++m) {
                        std::vector<uint8_t> bad = good;
                        const int flips = 1 + (int)r.below(3);
                        for (int f = 0; f < flips; ++f) bad[r.below((uint32_t)bad.size())] ^= (uint8_t)(1 + r.below(255));
                        const size_t len = m % 3 == 0 ? r.below((uint32_t)bad.size() + 1) : bad.size();
                        const uint32_t need = m % 5 == 0 ? 1 + r.below((uint32_t)(2 * n)) : (uint32_t)n;
                        st = run(bad, len, need, nullptr);
                        ++runs;
                        expect(st >= 0 && st < 32 && (st & (st - 1)) == 0, "status is one bit or zero", st);
                        if (st >= 0 && st < 32) ++by_status[st];
                        decoded += st == 0;
                    }
                }
    expect(by_status[ST_HEAD] > 0 && by_status[ST_CODE] > 0 && by_status[ST_SHORT] > 0 && decoded > 0, "every refusal seen");
    // unpredict_row: the running sum modulo 256, against its definition
    {
        const int w = 700;
        std::unique_ptr<uint8_t[]> row(new uint8_t[3 * w]);
        std::vector<uint8_t> want(3 * w);
        for (int i = 0; i < 3 * w; ++i) row[i] = (uint8_t)r.next();
        for (int i = 0; i < 3 * w; ++i) want[i] = (uint8_t)(row[i] + (i >= 3 ? want[i - 3] : 0));
        unpredict_row(row.get(), w);
        expect(!memcmp(row.get(), want.data(), 3 * w), "unpredict_row");
    }
    printf("%ld runs, %ld decoded, head %ld code %ld short %ld full %ld\n", runs, decoded, by_status[ST_HEAD], by_status[ST_CODE],
           by_status[ST_SHORT], by_status[ST_FULL]);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
