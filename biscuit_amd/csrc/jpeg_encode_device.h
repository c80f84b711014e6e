// jpeg_encode_device.h -- the baseline-JPEG ENCODER, stated once for the host and the device: the reverse of jpeg_device.h.
// One header, two users: the kernels of kernels_jpeg_encode.hip (bq_jpeg_encode) and the host entry bqio_jpeg_encode
// (jpeg_encode_host.cpp: the very same routines on the CPU, for the tests).
//
// The target is the complete file Pillow writes for `Image.fromarray(tile).save(buf, 'JPEG', quality=q, subsampling=s)` with
// libjpeg(-turbo)'s defaults, s = 4:2:0 or 4:4:4 -- integer arithmetic end to end, so it is held to Pillow's BYTES
// (tests/test_jpeg_encode.py), not to a tolerance.  The stages, as they are computed here (DESIGN.md "Tile extraction" records
// where they differ from a first recollection of libjpeg):
//
//   header    SOI, JFIF APP0 (1.01, density 1:1, no unit), DQT 0, DQT 1, SOF0, DHT DC0 / AC0 / DC1 / AC1 (Annex K.3 - K.6), SOS:
//             623 bytes that depend on (px, q, s) only.  Quantisers: scale = q < 50 ? 5000 / q : 200 - 2 q, entry = clamp((base *
//             scale + 50) / 100, 1, 255), written in zigzag order.
//   colour    BT.601 in 16-bit fixed point: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb, Cr carry 128 << 16 and the
//             rounding term 32767.
//   edges     A component's samples beyond the image repeat its last column and last row.  At 4:2:0 the full-size chroma is
//             widened by its last COLUMN before the 2 x 2 average, padded by its last ROW to an even height only, and the rows
//             below that repeat the last DOWNSAMPLED row (for an even height that is not the average of the last row with
//             itself).
//   4:2:0     (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... along a chroma row.
//   fDCT      samples - 128 through libjpeg's jfdctint (LL&M, 13-bit constants, 2 extra bits between the passes): output scaled
//             by 8.
//   quantise  on the magnitude: (|c| + (8 Q >> 1)) / (8 Q), sign restored.
//   dummies   At 4:2:0 an MCU holds 2 x 2 luma blocks although the luma plane is only ceil(px / 8) blocks wide and high.  A block
//             beyond the last block column has zero AC and the DC of the block to its left; a block beyond the last block row has
//             zero AC and the DC of the MCU's upper right block (itself a copy of the upper left one when that column is beyond
//             the plane too).  Either way its DC difference is zero.
//   entropy   per block in MCU order: DC difference against the previous block of the same component as category + bits, AC as
//             (run, size) with ZRL for runs of 16, EOB unless coefficient 63 is non-zero; the last byte padded with 1 bits,
//             0x00 stuffed after every 0xFF, then EOI.
//
// The decomposition is the device's: (1) every block's quantised coefficients, zigzag order, from the pixels alone; (2) every
// block's code length, from its coefficients and ONE neighbour's DC (prev_block / dummy_src: no serial walk); (3) after a scan
// of the lengths every block writes its bits at its own bit offset into an unstuffed buffer (BitSink: 32-bit words, big-endian
// bit order, words shared with a neighbour merged with an atomic OR on the device); (4) the 0xFF bytes are counted per chunk,
// scanned, and the file is copied out.  The host runs the same four steps one after the other.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQE_HD __host__ __device__ inline
#else
#define BQE_HD inline
#endif
#if defined(__clang__)
#define BQE_UNROLL _Pragma("unroll")
#else
#define BQE_UNROLL
#endif

namespace bqje {

enum { SUB_444 = 0, SUB_420 = 2 };       // Pillow's own numbering of `subsampling`
enum { ST_OK = 0, ST_CAP = 1 };          // status bit 1: the file would end beyond the output buffer; nothing was written

constexpr int HEADER_BYTES = 623;
constexpr int MAX_PX = 4096;
// Upper bound of one block's code: a DC code of at most 11 bits + 15 value bits, 63 AC symbols of at most 16 + 15 bits (a
// coefficient of an 8-bit image needs 10; the bound holds for anything an int16 can be).
constexpr uint32_t BLOCK_BITS_MAX = 26 + 63 * 31;
constexpr int STUFF_CHUNK = 32;          // bytes of unstuffed data per 0xFF count

BQE_HD bool valid_args(int px, int quality, int sub) {
    return px >= 1 && px <= MAX_PX && quality >= 1 && quality <= 100 && (sub == SUB_444 || sub == SUB_420);
}

// 8 x 8 natural index of zigzag position k (the table of jpeg_baseline.h; repeated so that unrolled loops see constants)
BQE_HD int zigzag(int k) {
    constexpr uint8_t Z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return Z[k];
}

// ---- geometry -----------------------------------------------------------------------------------------------------------
struct Geom {
    int px, hs;                          // hs = 2 at 4:2:0 (2 x 2 luma blocks per MCU), 1 at 4:4:4
    int mcux, mcuy, bpm;                 // MCUs per row / column, blocks per MCU (6 or 3)
    int wb, hb;                          // luma blocks that exist: ceil(px / 8) each way
    int ch;                              // chroma rows that exist: ceil(px / hs)
    uint32_t nblk;                       // blocks of the scan: mcux * mcuy * bpm
};

BQE_HD Geom geom_of(int px, int sub) {
    Geom G;
    G.px = px; G.hs = sub == SUB_420 ? 2 : 1;
    G.mcux = G.mcuy = (px + 8 * G.hs - 1) / (8 * G.hs);
    G.bpm = G.hs * G.hs + 2;
    G.wb = G.hb = (px + 7) / 8;
    G.ch = (px + G.hs - 1) / G.hs;
    G.nblk = (uint32_t)G.mcux * (uint32_t)G.mcuy * (uint32_t)G.bpm;
    return G;
}

// Bytes of the unstuffed buffer that hold any tile of this geometry (a multiple of 16).
BQE_HD size_t unstuffed_bytes(const Geom& G) { return (((size_t)G.nblk * BLOCK_BITS_MAX + 7) / 8 + 8 + 15) & ~(size_t)15; }
BQE_HD size_t stuff_chunks(const Geom& G) { return unstuffed_bytes(G) / STUFF_CHUNK + 1; }

struct BlockPos {
    int comp;                            // 0 = Y, 1 = Cb, 2 = Cr
    int bx, by;                          // block column / row in the component's plane
    int mcu, k;                          // MCU index, block within the MCU
    bool dummy;                          // beyond the component's own blocks (luma at 4:2:0 only)
};

BQE_HD BlockPos block_pos(const Geom& G, uint32_t b) {
    BlockPos P;
    P.mcu = (int)(b / (uint32_t)G.bpm); P.k = (int)(b - (uint32_t)P.mcu * (uint32_t)G.bpm);
    const int mx = P.mcu % G.mcux, my = P.mcu / G.mcux;
    const int nl = G.hs * G.hs;
    if (P.k < nl) {
        P.comp = 0;
        P.bx = mx * G.hs + (P.k % G.hs); P.by = my * G.hs + (P.k / G.hs);
        P.dummy = P.bx >= G.wb || P.by >= G.hb;
    } else {
        P.comp = 1 + (P.k - nl);
        P.bx = mx; P.by = my;
        P.dummy = false;
    }
    return P;
}

// The block whose DC the DC of block b is coded against: the previous block of the same component in scan order; -1: none (0).
BQE_HD int64_t prev_block(const Geom& G, const BlockPos& P, uint32_t b) {
    if (P.comp == 0 && P.k > 0) return (int64_t)b - 1;
    if (P.mcu == 0) return -1;
    return (int64_t)b - G.bpm + (P.comp == 0 ? G.hs * G.hs - 1 : 0);
}

// The REAL block whose DC a dummy block repeats (see "dummies" above); b itself for a block that exists.
BQE_HD uint32_t dummy_src(const Geom& G, const BlockPos& P, uint32_t b) {
    if (!P.dummy) return b;
    const uint32_t first = b - (uint32_t)P.k;                      // the MCU's upper left block: always real
    if (P.by < G.hb) return b - 1;                                 // right of the plane, in a row that exists
    return (P.bx | 1) < G.wb ? first + 1 : first;                  // below the plane: the upper right block, or what that one copies
}

// ---- tables -------------------------------------------------------------------------------------------------------------
struct Tables {
    uint16_t q[2][64];                   // quantisers, zigzag order: [0] luma, [1] chroma
    uint32_t dc[2][16];                  // (length << 16) | code by category; 0 = no such code
    uint32_t ac[2][256];                 // by (run << 4) | size
};

struct Header { uint8_t b[HEADER_BYTES + 1]; };

// ITU-T T.81 Annex K
static const uint8_t K_LUMA_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                     81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72,  92,  95,  98,  112, 100, 103, 99};
static const uint8_t K_CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                       99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const uint8_t K_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t K_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t K_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t K_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Canonical codes (T.81 Annex C) of one table into the (length << 16) | code form, indexed by symbol.
inline void build_codes(const uint8_t bits[16], const uint8_t* vals, uint32_t* out, int nout) {
    for (int i = 0; i < nout; ++i) out[i] = 0;
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++p, ++code)
            if (vals[p] < nout) out[vals[p]] = ((uint32_t)l << 16) | code;
        code <<= 1;
    }
}

// The quantisers and codes of (quality, sub) and the 623 header bytes of (px, quality, sub).  Host only; the device gets both
// as kernel arguments.
inline void build_tables(int px, int quality, int sub, Tables& T, Header& H) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t) {
        const uint8_t* base = t ? K_CHROMA_Q : K_LUMA_Q;
        for (int k = 0; k < 64; ++k) {
            int v = (base[zigzag(k)] * scale + 50) / 100;
            T.q[t][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
        build_codes(K_DC_BITS[t], K_DC_VALS, T.dc[t], 16);
        build_codes(K_AC_BITS[t], K_AC_VALS[t], T.ac[t], 256);
    }
    uint8_t* o = H.b;
    auto put = [&](int v) { *o++ = (uint8_t)v; };
    auto put2 = [&](int v) { put(v >> 8); put(v & 255); };
    put2(0xFFD8);
    put2(0xFFE0); put2(16); put('J'); put('F'); put('I'); put('F'); put(0); put2(0x0101); put(0); put2(1); put2(1); put(0); put(0);
    for (int t = 0; t < 2; ++t) {
        put2(0xFFDB); put2(67); put(t);
        for (int k = 0; k < 64; ++k) put(T.q[t][k]);
    }
    const int samp = sub == SUB_420 ? 0x22 : 0x11;
    put2(0xFFC0); put2(17); put(8); put2(px); put2(px); put(3);
    put(1); put(samp); put(0); put(2); put(0x11); put(1); put(3); put(0x11); put(1);
    for (int t = 0; t < 2; ++t) {
        put2(0xFFC4); put2(31); put(t);
        for (int i = 0; i < 16; ++i) put(K_DC_BITS[t][i]);
        for (int i = 0; i < 12; ++i) put(K_DC_VALS[i]);
        put2(0xFFC4); put2(181); put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(K_AC_BITS[t][i]);
        for (int i = 0; i < 162; ++i) put(K_AC_VALS[t][i]);
    }
    put2(0xFFDA); put2(12); put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(63); put(0);
    H.b[HEADER_BYTES] = 0;
}

// ---- pixels -> samples ----------------------------------------------------------------------------------------------------
// One component of BT.601 as a dot product: sample = (cr R + cg G + cb B + add) >> 16.
struct Ycc { int32_t cr, cg, cb, add; };

BQE_HD Ycc ycc_of(int comp) {
    if (comp == 0) return Ycc{19595, 38470, 7471, 32768};
    if (comp == 1) return Ycc{-11059, -21709, 32768, (128 << 16) + 32767};
    return Ycc{32768, -27439, -5329, (128 << 16) + 32767};
}

BQE_HD int ycc(const Ycc& k, const uint8_t* p) { return (k.cr * p[0] + k.cg * p[1] + k.cb * p[2] + k.add) >> 16; }

// ---- forward DCT (IJG jfdctint "islow") + quantisation ------------------------------------------------------------------
constexpr int CB = 13, P1 = 2;
constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633,
                  F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// One 1-D pass over the 8 values d[0], d[S], ..., d[7 S], in place.  FIRST: the row pass (results kept with P1 extra bits).
template <bool FIRST, int S>
BQE_HD void fdct_1d(int32_t* d) {
    const int32_t t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int32_t t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SH = FIRST ? CB - P1 : CB + P1;
    constexpr int32_t R = 1 << (SH - 1);
    if (FIRST) {
        d[0] = (t10 + t11) * (1 << P1);
        d[4 * S] = (t10 - t11) * (1 << P1);
    } else {
        d[0] = (t10 + t11 + (1 << (P1 - 1))) >> P1;
        d[4 * S] = (t10 - t11 + (1 << (P1 - 1))) >> P1;
    }
    int32_t z1 = (t12 + t13) * F_0_541;
    d[2 * S] = (z1 + t13 * F_0_765 + R) >> SH;
    d[6 * S] = (z1 - t12 * F_1_847 + R) >> SH;
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * F_1_175;
    const int32_t a4 = t4 * F_0_298, a5 = t5 * F_2_053, a6 = t6 * F_3_072, a7 = t7 * F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    d[7 * S] = (a4 + z1 + z3 + R) >> SH;
    d[5 * S] = (a5 + z2 + z4 + R) >> SH;
    d[3 * S] = (a6 + z2 + z3 + R) >> SH;
    d[S] = (a7 + z1 + z4 + R) >> SH;
}

// The quantised coefficients of block P of a tile (uint8 [px][px][3]), zigzag order; q: the component's quantisers, zigzag order.
// A dummy block is all zero here; its DC is dummy_src's (block_dc).  Samples beyond the image: see "edges" at the top.
BQE_HD void block_coefs(const uint8_t* tile, const Geom& G, const BlockPos& P, const uint16_t* q, int16_t* out) {
    if (P.dummy) {
        BQE_UNROLL
        for (int k = 0; k < 64; ++k) out[k] = 0;
        return;
    }
    const int px = G.px, last = px - 1;
    const Ycc K = ycc_of(P.comp);
    int32_t d[64];
    if (P.comp == 0 || G.hs == 1) {
        BQE_UNROLL
        for (int r = 0; r < 8; ++r) {
            const int y = P.by * 8 + r;
            const uint8_t* row = tile + (size_t)(y < last ? y : last) * px * 3;
            BQE_UNROLL
            for (int c = 0; c < 8; ++c) {
                const int x = P.bx * 8 + c;
                d[8 * r + c] = ycc(K, row + 3 * (x < last ? x : last)) - 128;
            }
            fdct_1d<true, 1>(d + 8 * r);
        }
    } else {
        BQE_UNROLL
        for (int r = 0; r < 8; ++r) {
            const int y = P.by * 8 + r, cy = y < G.ch ? y : G.ch - 1;              // 2 cy <= last always
            const uint8_t *r0 = tile + (size_t)(2 * cy) * px * 3, *r1 = tile + (size_t)(2 * cy + 1 < last ? 2 * cy + 1 : last) * px * 3;
            BQE_UNROLL
            for (int c = 0; c < 8; ++c) {
                const int x = 2 * (P.bx * 8 + c), x0 = 3 * (x < last ? x : last), x1 = 3 * (x + 1 < last ? x + 1 : last);
                const int sum = ycc(K, r0 + x0) + ycc(K, r0 + x1) + ycc(K, r1 + x0) + ycc(K, r1 + x1);
                d[8 * r + c] = ((sum + 1 + (c & 1)) >> 2) - 128;
            }
            fdct_1d<true, 1>(d + 8 * r);
        }
    }
    BQE_UNROLL
    for (int c = 0; c < 8; ++c) fdct_1d<false, 8>(d + c);
    BQE_UNROLL
    for (int k = 0; k < 64; ++k) {
        const int32_t v = d[zigzag(k)], q8 = (int32_t)q[k] * 8;
        const int32_t m = ((v < 0 ? -v : v) + (q8 >> 1)) / q8;
        out[k] = (int16_t)(v < 0 ? -m : m);
    }
}

// ---- entropy coding -------------------------------------------------------------------------------------------------------
BQE_HD int bit_size(int v) {             // number of bits of |v|, 0 for 0
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// One block's symbols into `sink.put(bits, count)` (count <= 16 per call).  zz: zigzag coefficients whose [0] is ignored;
// diff: the DC difference; t: 0 luma / 1 chroma tables.
template <typename Sink>
BQE_HD void encode_block(const int16_t* zz, int diff, const Tables& T, int t, Sink& sink) {
    int s = bit_size(diff) & 15;
    uint32_t e = T.dc[t][s];
    sink.put(e & 0xFFFF, (int)(e >> 16));
    if (s) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { e = T.ac[t][0xF0]; sink.put(e & 0xFFFF, (int)(e >> 16)); run -= 16; }
        s = bit_size(v) & 15;
        e = T.ac[t][(run << 4) | s];
        sink.put(e & 0xFFFF, (int)(e >> 16));
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
        run = 0;
    }
    if (run) { e = T.ac[t][0]; sink.put(e & 0xFFFF, (int)(e >> 16)); }
}

struct CountSink {
    uint32_t bits = 0;
    BQE_HD void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// Writes bits from bit position `pos` of a zeroed buffer of 32-bit words, most significant bit of byte 0 first.  A word this
// writer fills alone is stored; the word it starts in (when `pos` is inside it) and the one it ends in may hold a neighbour's
// bits too and are merged: an atomic OR on the device, a plain OR on the (serial) host.
struct BitSink {
    uint32_t* words;
    uint64_t w;                          // current word
    uint32_t acc;                        // its bits so far, big-endian bit order
    int fill;                            // bits of the word behind us (ours or a neighbour's)
    bool shared;                         // a neighbour wrote into the current word
    BQE_HD void open(uint32_t* buf, uint64_t pos) { words = buf; w = pos >> 5; acc = 0; fill = (int)(pos & 31); shared = fill != 0; }
    BQE_HD void merge(uint32_t v) {
        v = __builtin_bswap32(v);
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(words + w, v);
#else
        words[w] |= v;
#endif
    }
    BQE_HD void flush() {                // the current word is full
        if (shared) merge(acc); else words[w] = __builtin_bswap32(acc);
        ++w; acc = 0; fill = 0; shared = false;
    }
    BQE_HD void put(uint32_t bits, int n) {      // 0 <= n <= 16, bits < 2^n
        if (n == 0) return;
        const int room = 32 - fill;
        if (n < room) { acc |= bits << (room - n); fill += n; return; }
        acc |= bits >> (n - room);
        const int rest = n - room;
        flush();
        if (rest) { acc = bits << (32 - rest); fill = rest; }
    }
    BQE_HD void close() { if (fill && acc) merge(acc); }
};

// The effective DC of block b: its own, or the one a dummy block repeats.  coef: the tile's [nblk][64] coefficients.
BQE_HD int block_dc(const int16_t* coef, const Geom& G, const BlockPos& P, uint32_t b) { return coef[(size_t)dummy_src(G, P, b) * 64]; }

BQE_HD int dc_diff(const int16_t* coef, const Geom& G, const BlockPos& P, uint32_t b) {
    const int64_t pb = prev_block(G, P, b);
    int pred = 0;
    if (pb >= 0) pred = block_dc(coef, G, block_pos(G, (uint32_t)pb), (uint32_t)pb);
    return block_dc(coef, G, P, b) - pred;
}

BQE_HD uint32_t block_bits(const int16_t* coef, const Geom& G, const Tables& T, uint32_t b) {
    const BlockPos P = block_pos(G, b);
    CountSink s;
    encode_block(coef + (size_t)b * 64, dc_diff(coef, G, P, b), T, P.comp ? 1 : 0, s);
    return s.bits;
}

// Block b's bits at bit offset `pos` of the tile's unstuffed buffer; the scan's last block also pads the last byte with ones.
BQE_HD void block_pack(const int16_t* coef, const Geom& G, const Tables& T, uint32_t b, uint64_t pos, uint32_t* ubuf) {
    const BlockPos P = block_pos(G, b);
    BitSink s;
    s.open(ubuf, pos);
    encode_block(coef + (size_t)b * 64, dc_diff(coef, G, P, b), T, P.comp ? 1 : 0, s);
    if (b + 1 == G.nblk) {
        const int used = (int)(((s.w << 5) + (uint64_t)s.fill) & 7);
        if (used) s.put((1u << (8 - used)) - 1, 8 - used);
    }
    s.close();
}

// 0xFF bytes among u[lo, hi)
BQE_HD uint32_t count_ff(const uint8_t* u, uint32_t lo, uint32_t hi) {
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c += u[i] == 0xFF;
    return c;
}

// u[lo, hi) to dst with 0x00 behind every 0xFF; returns the bytes written
BQE_HD uint32_t copy_stuffed(const uint8_t* u, uint32_t lo, uint32_t hi, uint8_t* dst) {
    uint32_t o = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint8_t v = u[i];
        dst[o++] = v;
        if (v == 0xFF) dst[o++] = 0;
    }
    return o;
}

}  // namespace bqje
