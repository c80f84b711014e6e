// lzw_device.h -- TIFF LZW (compression 5) as libtiff writes and reads it, stated once in plain __host__ __device__ C++.  Three
// users: the kernels of kernels_lzw.hip, the host entries bqio_lzw_decode / bqio_lzw_decode_canvas (lzw_host.cpp) and
// tests/lzw_selfcheck.cpp (ASan / UBSan over seeded mutations).
//
// The stream.  Codes are packed MSB first.  ClearCode 256, EndOfInformation 257, first free entry 258.  The width of the next
// code follows from the table's next free index n after each code: 9 bits while n < 511, 10 while n < 1023, 11 while n < 2047,
// else 12 ("early change").  ClearCode resets n to 258 (and the width to 9); the code after it (after the last of several) must
// be a byte, which is emitted and adds no entry.  Every later code c names an existing entry (emit it; add prev + first(entry))
// or equals n (emit and add prev + first(prev): KwKwK).  Decoding stops as soon as need = rows * seg_w * 3 bytes are out; a
// last string that overruns need is cut.  EndOfInformation, or the end of the data, before that is a refusal.  The segment
// must begin with ClearCode (byte 0 = 0x80, top bit of byte 1 = 0): old-style (pre-6.0, bit-reversed) streams are refused.
//
// A table that fills without a ClearCode: libtiff (4.7.1, through Pillow -- tests/test_lzw.py holds every case against it) goes
// on reading 12-bit codes and counting entries that no 12-bit code can name, up to index 5118 (its table has 1024 spare rows
// for old-style files); the code after that, unless it is ClearCode, is refused.  So does next() below: entries from 4096 on
// are counted, not kept.
//
// The table holds no strings.  An entry past 257 is a contiguous run of bytes ALREADY IN THE OUTPUT -- the previous code's
// string and the first byte of the one after it -- and every code but ClearCode adds exactly one entry, so entry k starts
// where the string before its last byte was emitted and entry k + 1 starts where entry k's last byte lies:
//     entry k = out[start[k] .. start[k + 1]]   (both ends included),   length = start[k + 1] - start[k] + 1
// with start[n] = where the previous code's string began.  One uint32 per entry: 4097 words, 16 388 bytes.
//
// Bounds.  A source reads byte i of the stream only for i < len (the wave's: inside the padding the packing guarantees).
// next() hands out a Step only with dst + cnt <= need and src + len <= dst for a copy (the bytes exist), and reads
// start[code], start[code + 1] only for 258 <= code < min(n, 4096).
#pragma once
#include <stdint.h>

#include "canvas_place.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQL_HD __host__ __device__ inline
#else
#define BQL_HD inline
#endif
// A value every lane of the wave holds alike, said so to the compiler (the kernel parses wave-uniformly: the table's words come
// out of LDS, which it takes for lane-dependent, and everything computed from them would leave the scalar unit).
#if defined(__HIP_DEVICE_COMPILE__)
#define BQL_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define BQL_UNIFORM(x) (x)
#endif

namespace bqlzw {

using bqcanvas::Window;
using bqcanvas::place_window;

constexpr int CLEAR = 256, EOI = 257, FIRST = 258;
constexpr int TABLE = 4096;          // entries a 12-bit code can name
constexpr int TABLE_END = 5119;      // libtiff's CSIZE: the next free index at which it takes no further string
constexpr int MAX_SIDE = 1024;       // the longest segment side the decoder takes: need <= 3 MiB
constexpr uint32_t MAX_LEN = 1u << 28;   // bytes of one segment's stream: a bit position stays inside 32 bits

// status of one segment: 0 = decoded, otherwise bits (mirrored in tfrecord_native.py)
enum { ST_OK = 0,
       ST_HEAD = 1,        // the first code is not ClearCode (old-style or damaged)
       ST_CODE = 2,        // a code beyond the next free index, or no byte after a ClearCode
       ST_SHORT = 4,       // the data ends, or EndOfInformation arrives, before `need` bytes are out
       ST_FULL = 8,        // the table ran to its end without a ClearCode
       ST_DESC = 16 };     // a descriptor that fails the decoder's own bounds checks

struct Desc { uint32_t off, len; };  // a segment of the packed stream buffer: off a multiple of 16

BQL_HD bool desc_ok(const Desc& d) { return (d.off & 15u) == 0 && d.len <= MAX_LEN; }
BQL_HD bool geom_ok(int rows, int seg_w) { return rows > 0 && seg_w > 0 && rows <= MAX_SIDE && seg_w <= MAX_SIDE; }

BQL_HD int width_for(int n) { return n < 511 ? 9 : n < 1023 ? 10 : n < 2047 ? 11 : 12; }

BQL_HD int head_status(const uint8_t* raw, uint32_t len) {
    if (len < 2) return ST_SHORT;
    return raw[0] == 0x80 && !(raw[1] & 0x80) ? ST_OK : ST_HEAD;
}

// Where the codes come from: get(bit, w) = the w bits at bit position `bit` (w <= 12); next() has checked bit + w <= 8 * len.
// ByteSource reads the (at most three) bytes that hold them, each only if it lies inside len: the CPU's source, and the
// definition.  kernels_lzw.hip has a second one that keeps 256 bytes of the stream in a wave's registers; the bits are the same.
struct ByteSource {
    const uint8_t* raw; uint32_t len;
    BQL_HD uint32_t get(uint32_t bit, int w) const {
        const uint32_t b = bit >> 3;
        uint32_t v = 0;
        for (uint32_t k = 0; k < 3; ++k) v = v << 8 | (b + k < len ? (uint32_t)raw[b + k] : 0u);
        return v >> (24 - (int)(bit & 7) - w) & ((1u << w) - 1);
    }
};

struct State {
    uint32_t bit = 0;                // position in the stream
    uint32_t pos = 0;                // bytes out
    uint32_t prev_pos = 0, prev_len = 0;   // the previous code's string: where it began, its whole length
    int n = FIRST;                   // the table's next free index
    int status = ST_OK;
    bool fresh = true;               // no string since the last ClearCode (or since the start)
};

// what one code emits: cnt bytes at dst -- the byte `lit` (LITERAL), or out[src .. src + cnt) (COPY), or the same with byte
// len - 1 of the string = out[src], which the copy itself writes at dst (KWKWK)
enum { LITERAL = 0, COPY = 1, KWKWK = 2 };
struct Step { int kind; uint32_t dst, cnt, src, len; uint8_t lit; };

// The next code that emits, parsed: true with `e` set, false when the segment is over (s.status says how).  `start` is the
// table above, 4097 words; it needs no initialisation.
template <class Source>
BQL_HD bool next(State& s, Source& src, uint32_t len, uint32_t need, uint32_t* start, Step& e) {
    for (;;) {
        if (s.pos >= need) return false;
        const int w = width_for(s.n);
        if ((uint64_t)s.bit + (uint32_t)w > (uint64_t)len * 8) { s.status = ST_SHORT; return false; }
        const int code = (int)src.get(s.bit, w);
        s.bit += (uint32_t)w;
        if (code == EOI) { s.status = ST_SHORT; return false; }
        if (code == CLEAR) { s.n = FIRST; s.fresh = true; continue; }
        e.dst = s.pos; e.cnt = 1; e.src = 0; e.len = 1; e.lit = (uint8_t)code; e.kind = LITERAL;
        if (s.fresh) {
            if (code > 255) { s.status = ST_CODE; return false; }
            s.fresh = false;
            start[FIRST] = s.pos;
        } else {
            if (s.n >= TABLE_END) { s.status = ST_FULL; return false; }
            if (code >= FIRST) {
                if (code < s.n) { e.kind = COPY; e.src = BQL_UNIFORM(start[code]); e.len = BQL_UNIFORM(start[code + 1]) - e.src + 1; }
                else if (code == s.n) { e.kind = KWKWK; e.src = s.prev_pos; e.len = s.prev_len + 1; }
                else { s.status = ST_CODE; return false; }
                e.cnt = e.len < need - s.pos ? e.len : need - s.pos;
            }
            if (++s.n <= TABLE) start[s.n] = s.pos;
        }
        s.prev_pos = s.pos; s.prev_len = e.len;
        s.pos += e.cnt;
        return true;
    }
}

// One segment decoded serially into out[need] (the CPU's emission; the kernel copies with a wave): -> its status.
BQL_HD int decode_serial(const uint8_t* raw, uint32_t len, uint32_t need, uint8_t* out, uint32_t* start) {
    int st = head_status(raw, len);
    if (st) return st;
    State s;
    Step e;
    ByteSource src{raw, len};
    while (next(s, src, len, need, start, e)) {
        if (e.kind == LITERAL) { out[e.dst] = e.lit; continue; }
        for (uint32_t k = 0; k < e.cnt; ++k) out[e.dst + k] = out[e.kind == KWKWK && k == e.len - 1 ? e.src : e.src + k];
    }
    return s.status;
}

// TIFF predictor 2 undone along one row of w pixels: the running sum per sample modulo 256
BQL_HD void unpredict_row(uint8_t* row, int w) {
    for (int x = 1; x < w; ++x)
        for (int c = 0; c < 3; ++c) row[3 * x + c] = (uint8_t)(row[3 * x + c] + row[3 * x - 3 + c]);
}

}  // namespace bqlzw
