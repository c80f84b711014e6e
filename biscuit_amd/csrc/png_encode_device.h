// png_encode_device.h -- the PNG ENCODER (row filters + a deflate compressor), stated once for the host and the device.
// One header, two users: the kernels of kernels_png_encode.hip (bq_png_encode) and the host entry bqio_png_encode
// (png_encode_host.cpp: the very same routines on the CPU, for the tests).
//
// A tile uint8 [px][px][3] becomes one complete file: signature, IHDR (8-bit, colour type 2, no interlace), IDAT chunks of
// IDAT_PAYLOAD bytes (the last one shorter) that together hold one zlib stream, IEND; no ancillary chunk.  The contract has
// two halves (DESIGN.md "Tile extraction"):
//
//   rows      The filtered scanlines are Pillow's, byte for byte.  Per row the candidates None (0), Up (2), Sub (1), Paeth (4) in
//             that order, score = sum of |byte read as int8|, a candidate replaces the choice only when strictly smaller; the
//             row above row 0 is zeros; Average is never chosen.
//   deflate   The stream is OURS, defined by the sequential semantics below so that the device (parallel) and the host (loops)
//             write the same bytes.  The filtered stream of L = px (1 + 3 px) bytes is cut into blocks of BLOCK input bytes that
//             share nothing (no window across blocks).
//               match  a block is walked in groups of GROUP positions.  Position p hashes its 3 bytes (hash3) and looks up the
//                      table AS THE EARLIER GROUPS LEFT IT: the most recent earlier-group position with that hash.  The match is
//                      extended byte by byte to at most MAX_MATCH and the block's end.  After the group the table takes, per
//                      hash, the group's highest position.  A greedy walk picks tokens: at the current position a match of at
//                      least TAKE_MATCH is taken (and skipped over, possibly into later groups), otherwise a literal.
//               code   per block: histograms of the 286 literal/length and 30 distance symbols, length-limited (15) Huffman
//                      lengths (sort by (count, symbol), the in-place minimum-redundancy lengths of Moffat & Katajainen, too-long
//                      codes folded to the limit and the Kraft sum repaired from the longest codes), at least two distance and
//                      code-length codes so that every code is complete; the code-length code (19 symbols, limit 7) over the
//                      run-length symbols 16 / 17 / 18.  Three sizes in bits: dynamic, fixed, stored (counted with its worst
//                      padding: 42 + 8 n).  Stored when stored <= both others, else fixed when fixed <= dynamic, else dynamic.
//               pack   blocks follow one another bit by bit (a stored block pads to a byte after its 3 header bits); the last
//                      carries BFINAL.  Every token's bits are ORed in at its own bit offset (put_bits: LSB first).
//   zlib      0x78 0x01, the blocks, Adler-32 of the filtered stream (combined from per-row partial sums).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQP_HD __host__ __device__ inline
#else
#define BQP_HD inline
#endif

namespace bqpe {

enum { ST_OK = 0, ST_CAP = 1 };          // status bit 1: the file would end beyond the output buffer; nothing was written
enum { KIND_STORED = 0, KIND_FIXED = 1, KIND_DYNAMIC = 2 };

constexpr int MAX_PX = 4096;
constexpr uint32_t BLOCK = 16384;        // input bytes per deflate block
constexpr uint32_t GROUP = 64;           // positions matched against one state of the table
constexpr int HASH_BITS = 12;
constexpr uint32_t HASH_SIZE = 1u << HASH_BITS;
constexpr uint32_t HASH_BYTES = 3;       // bytes a position is hashed over: no shorter match is found
constexpr uint32_t TAKE_MATCH = 5;       // the walk takes a match from this length on (3 and 4 cost more than their literals)
constexpr uint32_t MAX_MATCH = 258;
constexpr uint32_t IDAT_PAYLOAD = 8192;  // zlib bytes per IDAT chunk
constexpr int NLL = 286, NDIST = 30, DIST0 = 288, NCODE = 320, NCL = 19;    // code tables: [0, 288) literal/length, [288, 318) distance
constexpr int HDR_WORDS = 144;           // a dynamic header is at most 17 + 57 + 316 * 14 = 4498 bits
constexpr int FILE_HEAD = 33;            // signature + IHDR chunk
constexpr uint32_t ADLER = 65521;

BQP_HD bool valid_px(int px) { return px >= 1 && px <= MAX_PX; }

struct Geom {
    int px;
    uint32_t rl;                         // bytes of a filtered row: 1 + 3 px
    uint32_t L;                          // of the filtered stream
    uint32_t nb;                         // deflate blocks
};

BQP_HD Geom geom_of(int px) {
    Geom G;
    G.px = px; G.rl = 1u + 3u * (uint32_t)px; G.L = (uint32_t)px * G.rl; G.nb = (G.L + BLOCK - 1) / BLOCK;
    return G;
}
BQP_HD uint32_t block_len(const Geom& G, uint32_t b) { const uint32_t r = G.L - b * BLOCK; return r < BLOCK ? r : BLOCK; }
// bytes that hold any tile's deflate stream: a block costs at most its stored form, 8 n + 42 bits
BQP_HD size_t deflate_bytes(const Geom& G) { return ((size_t)G.L + 6 * (size_t)G.nb + 16 + 15) & ~(size_t)15; }

struct BlockInfo {                       // what the stages hand on per block (32 bytes)
    uint32_t ntok, kind, hdr_bits, pad;
    uint64_t bits;                       // of the block in its chosen form (stored: without the padding, which depends on start)
    uint64_t start;                      // bit offset in the tile's deflate stream
};

// ---- row filters ------------------------------------------------------------------------------------------------------------
BQP_HD int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
BQP_HD uint32_t abs8(int v) { v &= 255; return (uint32_t)(v < 128 ? v : 256 - v); }

// byte i (0 <= i < 3 px) of a row under the four candidates; prev: the row above, null for row 0 (zeros)
struct Cand { int none, sub, up, pae; };
BQP_HD Cand candidates(const uint8_t* cur, const uint8_t* prev, uint32_t i) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = prev ? prev[i] : 0, c = (prev && i >= 3) ? prev[i - 3] : 0;
    Cand r;
    r.none = x; r.sub = (x - a) & 255; r.up = (x - b) & 255; r.pae = (x - paeth(a, b, c)) & 255;
    return r;
}
// the filter type from the four scores: None, Up, Sub, Paeth in that order, strictly smaller only
BQP_HD int choose_filter(uint32_t none, uint32_t sub, uint32_t up, uint32_t pae) {
    int f = 0;
    uint32_t best = none;
    if (up < best) { best = up; f = 2; }
    if (sub < best) { best = sub; f = 1; }
    if (pae < best) { best = pae; f = 4; }
    return f;
}
BQP_HD int pick(const Cand& c, int f) { return f == 0 ? c.none : f == 1 ? c.sub : f == 2 ? c.up : c.pae; }

// Adler-32 of the stream from per-row sums: A_r = sum of the row's bytes, B_r = sum of (rl - j) * byte j, both mod 65521.
// s1 = 1 + sum A_r; s2 = L + sum (B_r + (bytes behind row r) * A_r).  One row's term of s2:
BQP_HD uint32_t adler_row_term(const Geom& G, uint32_t y, uint32_t A, uint32_t B) {
    const uint64_t behind = (uint64_t)((uint32_t)G.px - 1 - y) * G.rl % ADLER;
    return (uint32_t)((B + behind * A) % ADLER);
}

// ---- matching ---------------------------------------------------------------------------------------------------------------
BQP_HD uint32_t hash3(const uint8_t* p) {
    return (((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) * 0x9E3779B1u) >> (32 - HASH_BITS);
}
BQP_HD uint32_t match_len(const uint8_t* base, uint32_t cand, uint32_t p, uint32_t maxl) {
    uint32_t l = 0;
    while (l < maxl && base[cand + l] == base[p + l]) ++l;
    return l;
}
// tokens: a literal is its byte; a match is bit 31 | (distance - 1) << 9 | length
BQP_HD uint32_t match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((dist - 1) << 9) | len; }

struct Sym { uint32_t sym, eb, ex; };    // symbol, number of extra bits, their value
BQP_HD Sym length_sym(uint32_t len) {    // 3..258 -> 257..285
    const uint32_t l = len - 3;
    Sym s;
    if (l < 8) { s.sym = 257 + l; s.eb = 0; s.ex = 0; }
    else if (l == 255) { s.sym = 285; s.eb = 0; s.ex = 0; }
    else {
        const uint32_t msb = 31 - (uint32_t)__builtin_clz(l);
        s.eb = msb - 2; s.sym = 257 + 4 * s.eb + 4 + ((l >> s.eb) & 3); s.ex = l & ((1u << s.eb) - 1);
    }
    return s;
}
BQP_HD Sym dist_sym(uint32_t dist) {     // 1..32768 -> 0..29
    const uint32_t d = dist - 1;
    Sym s;
    if (d < 4) { s.sym = d; s.eb = 0; s.ex = 0; }
    else {
        const uint32_t msb = 31 - (uint32_t)__builtin_clz(d);
        s.eb = msb - 1; s.sym = 2 * msb + ((d >> s.eb) & 1); s.ex = d & ((1u << s.eb) - 1);
    }
    return s;
}
BQP_HD uint32_t length_extra_bits(uint32_t ls) { return (ls < 4 || ls == 28) ? 0 : (ls >> 2) - 1; }    // ls = symbol - 257
BQP_HD uint32_t dist_extra_bits(uint32_t ds) { return ds < 2 ? 0 : (ds >> 1) - 1; }

// ---- bits -------------------------------------------------------------------------------------------------------------------
// ORs the n <= 48 bits of v in at bit `pos` of a zeroed buffer of 32-bit words, least significant bit first.  On the device every
// word goes through an atomic OR (neighbours share words); ATOMIC = false is for a buffer one thread owns.
template <bool ATOMIC>
BQP_HD void or_word(uint32_t* w, uint32_t v) {
    if (!v) return;
#if defined(__HIP_DEVICE_COMPILE__)
    if (ATOMIC) atomicOr(w, v); else *w |= v;
#else
    *w |= v;
#endif
}
template <bool ATOMIC>
BQP_HD void put_bits(uint32_t* buf, uint64_t pos, uint64_t v, uint32_t n) {
    if (n == 0) return;
    uint32_t* w = buf + (pos >> 5);
    const uint32_t s = (uint32_t)(pos & 31);
    const uint64_t lo = v << s;
    or_word<ATOMIC>(w, (uint32_t)lo);
    or_word<ATOMIC>(w + 1, (uint32_t)(lo >> 32));
    if (s && s + n > 64) or_word<ATOMIC>(w + 2, (uint32_t)(v >> (64 - s)));
}

// the bits of one token under the block's codes ((length << 16) | code, code already bit-reversed)
BQP_HD void token_bits(uint32_t tok, const uint32_t* codes, uint64_t& v, uint32_t& n) {
    if (!(tok & 0x80000000u)) {
        const uint32_t e = codes[tok & 255];
        v = e & 0xFFFF; n = e >> 16;
        return;
    }
    const Sym ls = length_sym(tok & 0x1FF), ds = dist_sym(((tok >> 9) & 0x7FFF) + 1);
    uint32_t e = codes[ls.sym];
    v = e & 0xFFFF; n = e >> 16;
    v |= (uint64_t)ls.ex << n; n += ls.eb;
    e = codes[DIST0 + ds.sym];
    v |= (uint64_t)(e & 0xFFFF) << n; n += e >> 16;
    v |= (uint64_t)ds.ex << n; n += ds.eb;
}

// ---- Huffman codes ----------------------------------------------------------------------------------------------------------
// Work space of one block's code construction: LDS on the device, the stack on the host.
struct CodeWork {
    uint32_t hist[NCODE];                // counts: [0, 286) literal/length (256 = end of block, once), [288, 318) distance
    uint32_t key[NCODE], sorted[NCODE], A[NCODE];
    uint32_t lens[NCODE];                // dynamic code lengths
    uint32_t codes[NCODE];               // the chosen form's codes
    uint32_t seq[NCODE];                 // code-length sequence: symbol | extra << 8
    uint32_t hdr[HDR_WORDS];             // the dynamic header's bits
    uint32_t clfreq[NCL], cllens[NCL], clcodes[NCL];
    uint32_t cnt[17], next[17];
    uint32_t nseq, hlit, hdist;
};

// key[s] = count << 9 | s: unique, so the order is total.  Lanes lane, lane + nl, ... of nl.
BQP_HD void huff_keys(const uint32_t* freq, int n, uint32_t* key, int lane, int nl) {
    for (int s = lane; s < n; s += nl) key[s] = (freq[s] << 9) | (uint32_t)s;
}
// ascending sort by rank: every key is placed at the number of smaller keys
BQP_HD void rank_sort(const uint32_t* key, int n, uint32_t* sorted, int lane, int nl) {
    for (int i = lane; i < n; i += nl) {
        const uint32_t k = key[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += key[j] < k;
        sorted[r] = k;
    }
}
// lengths (<= limit) of the n symbols from their sorted keys.  Fewer than two used symbols: symbols 0 / 1 join with length 1.
BQP_HD void huff_from_sorted(const uint32_t* sorted, int n, int limit, uint32_t* lens, uint32_t* A, uint32_t* cnt) {
    for (int s = 0; s < n; ++s) lens[s] = 0;
    int z = 0;
    while (z < n && (sorted[z] >> 9) == 0) ++z;
    const int m = n - z;
    if (m == 0) { lens[0] = lens[1] = 1; return; }
    if (m == 1) { const uint32_t s = sorted[z] & 511; lens[s] = 1; lens[s ? 0 : 1] = 1; return; }
    for (int i = 0; i < m; ++i) A[i] = sorted[z + i] >> 9;
    // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": A ascending -> code lengths
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int nx = 1; nx < m - 1; ++nx) {
        if (leaf >= m || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (uint32_t)nx; } else A[nx] = A[leaf++];
        if (leaf >= m || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (uint32_t)nx; } else A[nx] += A[leaf++];
    }
    A[m - 2] = 0;
    for (int nx = m - 3; nx >= 0; --nx) A[nx] = A[A[nx]] + 1;
    int avbl = 1, used = 0, nx = m - 1;
    uint32_t depth = 0;
    root = m - 2;
    while (avbl > 0) {
        while (root >= 0 && A[root] == depth) { ++used; --root; }
        while (avbl > used) { A[nx--] = depth; --avbl; }
        avbl = 2 * used; ++depth; used = 0;
    }
    // fold to the limit, repair the Kraft sum from the longest codes
    for (int l = 0; l <= limit; ++l) cnt[l] = 0;
    for (int i = 0; i < m; ++i) { const uint32_t l = A[i]; ++cnt[l > (uint32_t)limit ? (uint32_t)limit : l]; }
    uint32_t total = 0;
    for (int l = limit; l >= 1; --l) total += cnt[l] << (limit - l);
    while (total != (1u << limit)) {
        --cnt[limit];
        for (int l = limit - 1; l >= 1; --l)
            if (cnt[l]) { --cnt[l]; cnt[l + 1] += 2; break; }
        --total;
    }
    int j = m;                            // the shortest codes to the most frequent symbols
    for (int l = 1; l <= limit; ++l)
        for (uint32_t k = cnt[l]; k > 0; --k) lens[sorted[z + --j] & 511] = (uint32_t)l;
}
BQP_HD uint32_t reverse_bits(uint32_t x, uint32_t l) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < l; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}
// canonical codes (RFC 1951 3.2.2) of n symbols, bit-reversed for an LSB-first stream: (length << 16) | code, 0 = unused
BQP_HD void canonical(const uint32_t* lens, int n, int maxbits, uint32_t* codes, uint32_t* cnt, uint32_t* next) {
    for (int l = 0; l <= maxbits; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) ++cnt[lens[s]];
    cnt[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l <= maxbits; ++l) { code = (code + cnt[l - 1]) << 1; next[l] = code; }
    for (int s = 0; s < n; ++s) {
        const uint32_t l = lens[s];
        codes[s] = l ? (l << 16) | reverse_bits(next[l]++, l) : 0;
    }
}
BQP_HD uint32_t fixed_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

BQP_HD void seq_emit(CodeWork& W, uint32_t sym, uint32_t extra) { W.seq[W.nseq++] = sym | (extra << 8); ++W.clfreq[sym]; }

// After W.lens holds the dynamic lengths of both codes: the code-length code, the dynamic header, the three sizes, the choice,
// W.codes for the chosen form.  One thread.  n: the block's input bytes; bfinal: the tile's last block.
BQP_HD BlockInfo finish_block(CodeWork& W, uint32_t ntok, uint32_t n, bool bfinal) {
    constexpr uint8_t ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    W.hlit = NLL;
    while (W.hlit > 257 && W.lens[W.hlit - 1] == 0) --W.hlit;
    W.hdist = NDIST;
    while (W.hdist > 1 && W.lens[DIST0 + W.hdist - 1] == 0) --W.hdist;
    const uint32_t total = W.hlit + W.hdist;
    W.nseq = 0;
    for (int i = 0; i < NCL; ++i) W.clfreq[i] = 0;
    auto at = [&](uint32_t k) { return k < W.hlit ? W.lens[k] : W.lens[DIST0 + k - W.hlit]; };
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = at(i);
        uint32_t run = 1;
        while (i + run < total && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const uint32_t r = run < 138 ? run : 138; seq_emit(W, 18, r - 11); run -= r; }
            if (run >= 3) { seq_emit(W, 17, run - 3); run = 0; }
            for (; run; --run) seq_emit(W, 0, 0);
        } else {
            seq_emit(W, v, 0); --run;
            while (run >= 3) { const uint32_t r = run < 6 ? run : 6; seq_emit(W, 16, r - 3); run -= r; }
            for (; run; --run) seq_emit(W, v, 0);
        }
    }
    huff_keys(W.clfreq, NCL, W.key, 0, 1);
    rank_sort(W.key, NCL, W.sorted, 0, 1);
    huff_from_sorted(W.sorted, NCL, 7, W.cllens, W.A, W.cnt);
    canonical(W.cllens, NCL, 7, W.clcodes, W.cnt, W.next);
    uint32_t hclen = NCL;
    while (hclen > 4 && W.cllens[ORDER[hclen - 1]] == 0) --hclen;
    // the header
    for (int k = 0; k < HDR_WORDS; ++k) W.hdr[k] = 0;
    uint64_t pos = 0;
    put_bits<false>(W.hdr, pos, (bfinal ? 1u : 0u) | (2u << 1), 3); pos += 3;
    put_bits<false>(W.hdr, pos, W.hlit - 257, 5); pos += 5;
    put_bits<false>(W.hdr, pos, W.hdist - 1, 5); pos += 5;
    put_bits<false>(W.hdr, pos, hclen - 4, 4); pos += 4;
    for (uint32_t k = 0; k < hclen; ++k) { put_bits<false>(W.hdr, pos, W.cllens[ORDER[k]], 3); pos += 3; }
    for (uint32_t k = 0; k < W.nseq; ++k) {
        const uint32_t sym = W.seq[k] & 255, ex = W.seq[k] >> 8, e = W.clcodes[sym];
        put_bits<false>(W.hdr, pos, e & 0xFFFF, e >> 16); pos += e >> 16;
        const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        put_bits<false>(W.hdr, pos, ex, eb); pos += eb;
    }
    // the sizes
    uint64_t extra = 0, dyn = pos, fix = 3;
    for (uint32_t s = 0; s < (uint32_t)NLL; ++s) { dyn += (uint64_t)W.hist[s] * W.lens[s]; fix += (uint64_t)W.hist[s] * fixed_len(s); }
    for (uint32_t s = 0; s < (uint32_t)NDIST; ++s) { dyn += (uint64_t)W.hist[DIST0 + s] * W.lens[DIST0 + s]; fix += (uint64_t)W.hist[DIST0 + s] * 5; }
    for (uint32_t ls = 0; ls < 29; ++ls) extra += (uint64_t)W.hist[257 + ls] * length_extra_bits(ls);
    for (uint32_t ds = 0; ds < (uint32_t)NDIST; ++ds) extra += (uint64_t)W.hist[DIST0 + ds] * dist_extra_bits(ds);
    dyn += extra; fix += extra;
    const uint64_t stored = 42 + 8 * (uint64_t)n;
    BlockInfo I;
    I.ntok = ntok; I.pad = 0; I.start = 0;
    if (stored <= dyn && stored <= fix) { I.kind = KIND_STORED; I.hdr_bits = 3; I.bits = 35 + 8 * (uint64_t)n; }
    else if (fix <= dyn) { I.kind = KIND_FIXED; I.hdr_bits = 3; I.bits = fix; }
    else { I.kind = KIND_DYNAMIC; I.hdr_bits = (uint32_t)pos; I.bits = dyn; }
    if (I.kind == KIND_FIXED) {
        for (uint32_t s = 0; s < 288; ++s) W.lens[s] = fixed_len(s);
        for (uint32_t s = 0; s < (uint32_t)NDIST; ++s) W.lens[DIST0 + s] = 5;
        canonical(W.lens, 288, 9, W.codes, W.cnt, W.next);
        canonical(W.lens + DIST0, NDIST, 5, W.codes + DIST0, W.cnt, W.next);
    } else if (I.kind == KIND_DYNAMIC) {
        canonical(W.lens, NLL, 15, W.codes, W.cnt, W.next);
        canonical(W.lens + DIST0, NDIST, 15, W.codes + DIST0, W.cnt, W.next);
    }
    return I;
}

// where a block's successor starts
BQP_HD uint64_t block_end(const BlockInfo& I, uint64_t start, uint32_t n) {
    if (I.kind == KIND_STORED) return ((start + 3 + 7) & ~(uint64_t)7) + 32 + 8 * (uint64_t)n;
    return start + I.bits;
}

// ---- the file ---------------------------------------------------------------------------------------------------------------
BQP_HD uint32_t crc_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
BQP_HD uint32_t crc_step(const uint32_t* table, uint32_t crc, uint32_t byte) { return table[(crc ^ byte) & 255] ^ (crc >> 8); }

BQP_HD uint64_t zlib_bytes(uint64_t dlen) { return 2 + dlen + 4; }
BQP_HD uint64_t idat_chunks(uint64_t zlen) { return (zlen + IDAT_PAYLOAD - 1) / IDAT_PAYLOAD; }
BQP_HD uint64_t file_bytes(uint64_t dlen) { const uint64_t z = zlib_bytes(dlen); return FILE_HEAD + 12 * idat_chunks(z) + z + 12; }
// byte k of the zlib stream: CMF / FLG (32 KB window, check bits), the deflate stream, Adler-32 big-endian
BQP_HD uint32_t zbyte(const uint8_t* dbuf, uint64_t dlen, uint32_t adler, uint64_t k) {
    if (k < 2) return k ? 0x01 : 0x78;
    if (k < 2 + dlen) return dbuf[k - 2];
    return (adler >> (8 * (3 - (uint32_t)(k - 2 - dlen)))) & 255;
}
// where byte k of the zlib stream stands in the file
BQP_HD uint64_t zbyte_at(uint64_t k) { return FILE_HEAD + 12 * (k / IDAT_PAYLOAD) + 8 + k; }
// CRC-32 of a chunk in CRC_LANES slices.  Polynomials mod the CRC-32 polynomial with bit 31 = x^0 (the register's own order):
// the CRC of A || B is crc(A) * x^(8 |B|) + crc(B), so a slice's CRC times x^(8 * bytes behind it) is its share of the whole, and
// the shares add up (XOR) in any order.
constexpr uint32_t CRC_LANES = 64;
BQP_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;           // times x
    }
    return p;
}
BQP_HD uint32_t crc_shift(uint32_t crc, uint32_t nbytes) {       // crc * x^(8 nbytes), by squaring
    uint32_t r = 0x80000000u, base = 0x00800000u;                // x^0, x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) r = gf_mul(r, base);
        base = gf_mul(base, base);
    }
    return gf_mul(r, crc);
}
BQP_HD uint32_t chunk_payload(uint64_t zlen, uint64_t c) {
    const uint64_t k0 = c * IDAT_PAYLOAD;
    return (uint32_t)(zlen - k0 < IDAT_PAYLOAD ? zlen - k0 : IDAT_PAYLOAD);
}
// slice `lane` of CRC_LANES of IDAT chunk c (its type and its payload): that slice's share of the chunk's CRC-32
BQP_HD uint32_t chunk_crc_share(const uint32_t* table, const uint8_t* dbuf, uint64_t dlen, uint32_t adler, uint64_t c, uint32_t lane) {
    const uint64_t k0 = c * IDAT_PAYLOAD;
    const uint32_t T = 4 + chunk_payload(zlib_bytes(dlen), c), S = (T + CRC_LANES - 1) / CRC_LANES;
    const uint32_t lo = lane * S, hi = lo + S < T ? lo + S : T;
    if (lo >= T) return 0;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t byte = k < 4 ? (k == 0 ? 'I' : k == 1 ? 'D' : k == 2 ? 'A' : 'T') : zbyte(dbuf, dlen, adler, k0 + k - 4);
        crc = crc_step(table, crc, byte);
    }
    return crc_shift(~crc, T - hi);
}
// the 12 bytes around IDAT chunk c: length and type in front of it, CRC behind it
BQP_HD void write_chunk_frame(uint8_t* file, uint64_t zlen, uint64_t c, uint32_t crc) {
    const uint32_t n = chunk_payload(zlen, c);
    uint8_t* o = file + FILE_HEAD + c * (IDAT_PAYLOAD + 12);
    o[0] = (uint8_t)(n >> 24); o[1] = (uint8_t)(n >> 16); o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)n;
    o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
    o += 8 + n;
    o[0] = (uint8_t)(crc >> 24); o[1] = (uint8_t)(crc >> 16); o[2] = (uint8_t)(crc >> 8); o[3] = (uint8_t)crc;
}

struct Header { uint8_t b[FILE_HEAD + 12 + 3]; };          // signature + IHDR, then IEND

// Host only; the device gets it as a kernel argument.
inline void build_header(int px, Header& H) {
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = crc_entry(i);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    uint8_t* o = H.b;
    memcpy(o, sig, 8); o += 8;
    auto put4 = [&](uint32_t v) { *o++ = (uint8_t)(v >> 24); *o++ = (uint8_t)(v >> 16); *o++ = (uint8_t)(v >> 8); *o++ = (uint8_t)v; };
    auto crc_of = [&](const uint8_t* p, int n) { uint32_t c = 0xFFFFFFFFu; for (int i = 0; i < n; ++i) c = crc_step(table, c, p[i]); return ~c; };
    put4(13);
    uint8_t* t = o;
    memcpy(o, "IHDR", 4); o += 4;
    put4((uint32_t)px); put4((uint32_t)px);
    *o++ = 8; *o++ = 2; *o++ = 0; *o++ = 0; *o++ = 0;
    put4(crc_of(t, 17));
    put4(0);
    t = o;
    memcpy(o, "IEND", 4); o += 4;
    put4(crc_of(t, 4));
    while (o < H.b + sizeof(H.b)) *o++ = 0;
}

}  // namespace bqpe

#if !defined(__HIPCC__)
// ---- the steps one after the other, on the CPU (bqio_png_encode; tests/png_encode_selfcheck.cpp) ------------------------------
#include <vector>

namespace bqpe {

// filter: the filtered stream and its Adler-32 through the per-row sums
inline uint32_t serial_filter(const uint8_t* tile, const Geom& G, uint8_t* filt) {
    uint64_t s1 = 1, s2 = G.L % ADLER;
    for (uint32_t y = 0; y < (uint32_t)G.px; ++y) {
        const uint8_t* cur = tile + (size_t)y * 3 * G.px;
        const uint8_t* prev = y ? cur - (size_t)3 * G.px : nullptr;
        uint32_t sc[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < G.rl - 1; ++i) {
            const Cand c = candidates(cur, prev, i);
            sc[0] += abs8(c.none); sc[1] += abs8(c.sub); sc[2] += abs8(c.up); sc[3] += abs8(c.pae);
        }
        const int f = choose_filter(sc[0], sc[1], sc[2], sc[3]);
        uint8_t* row = filt + (size_t)y * G.rl;
        row[0] = (uint8_t)f;
        uint64_t A = (uint64_t)f, B = (uint64_t)G.rl * (uint64_t)f;
        for (uint32_t i = 0; i < G.rl - 1; ++i) {
            const uint32_t v = (uint32_t)pick(candidates(cur, prev, i), f);
            row[1 + i] = (uint8_t)v;
            A += v; B += (uint64_t)(G.rl - 1 - i) * v;
        }
        s1 += A % ADLER;
        s2 += adler_row_term(G, y, (uint32_t)(A % ADLER), (uint32_t)(B % ADLER));
    }
    return (uint32_t)(s1 % ADLER) | ((uint32_t)(s2 % ADLER) << 16);
}

// match: one block's tokens and histogram, group by group
inline uint32_t serial_match(const uint8_t* base, uint32_t n, uint32_t* toks, uint32_t* hist, uint32_t* table) {
    for (uint32_t h = 0; h < HASH_SIZE; ++h) table[h] = 0;
    for (int s = 0; s < NCODE; ++s) hist[s] = 0;
    uint32_t q = 0, ntok = 0;
    for (uint32_t p0 = 0; p0 < n; p0 += GROUP) {
        uint32_t len[GROUP], dist[GROUP], hsh[GROUP];
        for (uint32_t j = 0; j < GROUP; ++j) {
            const uint32_t p = p0 + j;
            len[j] = dist[j] = 0; hsh[j] = HASH_SIZE;
            if (p + HASH_BYTES > n) continue;
            hsh[j] = hash3(base + p);
            const uint32_t c = table[hsh[j]];
            if (c && p >= q) {
                const uint32_t room = n - p;
                len[j] = match_len(base, c - 1, p, room < MAX_MATCH ? room : MAX_MATCH);
                dist[j] = p - (c - 1);
            }
        }
        for (uint32_t j = 0; j < GROUP; ++j)
            if (hsh[j] < HASH_SIZE) table[hsh[j]] = p0 + j + 1;                    // ascending: the highest position stays
        const uint32_t lim = n - p0 < GROUP ? n - p0 : GROUP;
        uint32_t j = q - p0;
        while (j < lim) {
            if (len[j] >= TAKE_MATCH) {
                toks[ntok++] = match_token(len[j], dist[j]);
                ++hist[length_sym(len[j]).sym]; ++hist[DIST0 + dist_sym(dist[j]).sym];
                j += len[j];
            } else {
                toks[ntok++] = base[p0 + j];
                ++hist[base[p0 + j]];
                ++j;
            }
        }
        q = p0 + j;
    }
    hist[256] = 1;
    return ntok;
}

// code: lengths of both codes, then finish_block
inline BlockInfo serial_code(CodeWork& W, uint32_t ntok, uint32_t n, bool bfinal) {
    huff_keys(W.hist, NLL, W.key, 0, 1);
    rank_sort(W.key, NLL, W.sorted, 0, 1);
    huff_from_sorted(W.sorted, NLL, 15, W.lens, W.A, W.cnt);
    for (int s = NLL; s < DIST0; ++s) W.lens[s] = 0;
    huff_keys(W.hist + DIST0, NDIST, W.key, 0, 1);
    rank_sort(W.key, NDIST, W.sorted, 0, 1);
    huff_from_sorted(W.sorted, NDIST, 15, W.lens + DIST0, W.A, W.cnt);
    return finish_block(W, ntok, n, bfinal);
}

// pack: one block's bits into the tile's zeroed deflate buffer
inline void serial_pack(const BlockInfo& I, const CodeWork& W, const uint32_t* toks, const uint8_t* base, uint32_t n, bool bfinal, uint32_t* dbuf) {
    uint64_t pos = I.start;
    if (I.kind == KIND_STORED) {
        put_bits<true>(dbuf, pos, bfinal ? 1u : 0u, 3);
        pos = (pos + 3 + 7) & ~(uint64_t)7;
        put_bits<true>(dbuf, pos, (uint64_t)n | ((uint64_t)(~n & 0xFFFF) << 16), 32);
        pos += 32;
        for (uint32_t k = 0; k < n; ++k) put_bits<true>(dbuf, pos + 8 * (uint64_t)k, base[k], 8);
        return;
    }
    if (I.kind == KIND_FIXED) put_bits<true>(dbuf, pos, (bfinal ? 1u : 0u) | (1u << 1), 3);
    else
        for (uint32_t k = 0; 32 * k < I.hdr_bits; ++k) put_bits<true>(dbuf, pos + 32 * (uint64_t)k, W.hdr[k], 32);
    pos += I.hdr_bits;
    for (uint32_t t = 0; t < I.ntok; ++t) {
        uint64_t v; uint32_t nb;
        token_bits(toks[t], W.codes, v, nb);
        put_bits<true>(dbuf, pos, v, nb);
        pos += nb;
    }
    put_bits<true>(dbuf, pos, W.codes[256] & 0xFFFF, W.codes[256] >> 16);
}

// one tile -> its file
inline void serial_encode(const uint8_t* tile, int px, std::vector<uint8_t>& file) {
    const Geom G = geom_of(px);
    std::vector<uint8_t> filt((size_t)G.L + 4);
    const uint32_t adler = serial_filter(tile, G, filt.data());
    std::vector<uint32_t> toks((size_t)G.nb * BLOCK), table(HASH_SIZE);
    std::vector<CodeWork> W(G.nb);
    std::vector<BlockInfo> info(G.nb);
    for (uint32_t b = 0; b < G.nb; ++b) {
        const uint32_t n = block_len(G, b);
        const uint32_t ntok = serial_match(filt.data() + (size_t)b * BLOCK, n, toks.data() + (size_t)b * BLOCK, W[b].hist, table.data());
        info[b] = serial_code(W[b], ntok, n, b + 1 == G.nb);
    }
    uint64_t pos = 0;
    for (uint32_t b = 0; b < G.nb; ++b) { info[b].start = pos; pos = block_end(info[b], pos, block_len(G, b)); }
    const uint64_t dlen = (pos + 7) / 8;
    std::vector<uint32_t> dbuf(deflate_bytes(G) / 4, 0);
    for (uint32_t b = 0; b < G.nb; ++b)
        serial_pack(info[b], W[b], toks.data() + (size_t)b * BLOCK, filt.data() + (size_t)b * BLOCK, block_len(G, b), b + 1 == G.nb, dbuf.data());
    const uint8_t* d = reinterpret_cast<const uint8_t*>(dbuf.data());
    Header H;
    build_header(px, H);
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = crc_entry(i);
    file.assign((size_t)file_bytes(dlen), 0);
    memcpy(file.data(), H.b, FILE_HEAD);
    const uint64_t zlen = zlib_bytes(dlen);
    for (uint64_t k = 0; k < zlen; ++k) file[(size_t)zbyte_at(k)] = (uint8_t)zbyte(d, dlen, adler, k);
    for (uint64_t c = 0; c < idat_chunks(zlen); ++c) {
        uint32_t crc = 0;
        for (uint32_t lane = 0; lane < CRC_LANES; ++lane) crc ^= chunk_crc_share(crc_table, d, dlen, adler, c, lane);
        write_chunk_frame(file.data(), zlen, c, crc);
    }
    memcpy(file.data() + file.size() - 12, H.b + FILE_HEAD, 12);
}

}  // namespace bqpe
#endif
