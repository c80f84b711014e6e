// j2k_host.cpp -- tier 2 of the JPEG 2000 tile decoder, on the host (include/biscuit_io.h: bqio_j2k_extract), and the CPU
// statement of the device decoder over the routines of j2k_device.h (bqio_j2k_decode_canvas).
//
// bqio_j2k_extract parses every segment's main header (SOC SIZ COD QCD) and tile-part headers, then walks the packets in
// the stream's progression order: inclusion and zero-bit-plane tag trees, the number of coding passes, Lblock and the
// segment lengths.  What it leaves is a descriptor per segment, a row per code block that has at least one pass, and the
// blocks' codewords -- a block's contributions from all layers one after the other -- in one packed buffer.  Every length is
// held against the bytes that are left before it is used; a stream outside the device's subset or a damaged one gets a
// status in its descriptor and no blocks.
#include <algorithm>
#include <atomic>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/biscuit_io.h"
#include "j2k_device.h"

namespace {

using namespace bqj2k;

struct Refuse { int status; };

struct Bytes {
    const uint8_t* p; size_t n, pos = 0;
    Bytes(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
    void need(size_t k) const { if (k > n - pos) throw Refuse{ST_DAMAGED}; }
    uint32_t u8() { need(1); return p[pos++]; }
    uint32_t u16() { need(2); const uint32_t v = (uint32_t)p[pos] << 8 | p[pos + 1]; pos += 2; return v; }
    uint32_t u32() { const uint32_t h = u16(); return h << 16 | u16(); }
};

// the packet headers' bit reader: a byte after FF carries 7 bits
struct Bits {
    const uint8_t* p; size_t n, pos; uint32_t cur = 0; int ct = 0;
    Bits(const uint8_t* p_, size_t n_, size_t pos_) : p(p_), n(n_), pos(pos_) {}
    void load() {
        if (pos >= n) throw Refuse{ST_DAMAGED};
        const uint32_t prev = cur;
        cur = p[pos++];
        ct = prev == 0xFF ? 7 : 8;
    }
    int bit() { if (!ct) load(); return (int)(cur >> --ct & 1); }
    uint32_t bits(int k) { uint32_t v = 0; while (k-- > 0) v = v << 1 | (uint32_t)bit(); return v; }
    void align() { if (cur == 0xFF) load(); ct = 0; cur = 0; }
};

struct TagTree {
    std::vector<int> off, lw, val, low;
    void init(int w, int h) {
        off.clear(); lw.clear();
        int total = 0;
        for (;;) {
            off.push_back(total); lw.push_back(w);
            total += w * h;
            if (w <= 1 && h <= 1) break;
            w = (w + 1) >> 1; h = (h + 1) >> 1;
        }
        val.assign(total, 1 << 30); low.assign(total, 0);
    }
    // is the leaf's value below `threshold`?  (reads what that takes)
    bool below(Bits& b, int x, int y, int threshold) {
        int lo = 0, node = 0;
        for (int k = (int)off.size() - 1; k >= 0; --k) {
            node = off[k] + (y >> k) * lw[k] + (x >> k);
            if (lo > low[node]) low[node] = lo; else lo = low[node];
            while (lo < threshold && lo < val[node]) {
                if (b.bit()) val[node] = lo; else ++lo;
            }
            low[node] = lo;
        }
        return val[node] < threshold;
    }
};

struct Cblk {
    int x0, y0, w, h;                    // in the plane
    bool included = false;
    int zbp = 0, lblock = 3, passes = 0;
    std::vector<std::pair<uint32_t, uint32_t>> pieces;   // (offset in the packet bytes, length)
    uint32_t len = 0;
};

struct PBand { int band, orient, res, mb, ncw = 0, nch = 0, first = 0; TagTree incl, zbps; };

struct Precinct { int r, c; int64_t x, y; std::vector<PBand> bands; };

struct Parsed {
    Seg seg;
    std::vector<Block> blocks;
    std::vector<uint8_t> bytes;
};

void parse_segment(const uint8_t* d, size_t n, int seg_w, int seg_h, Parsed& out) {
    Seg& S = out.seg;
    memset(&S, 0, sizeof(S));
    Bytes in(d, n);
    if (in.u16() != 0xFF4F) throw Refuse{ST_DAMAGED};
    bool have_siz = false, have_cod = false, have_qcd = false;
    int xcb = 0, ycb = 0, pp[MAX_LEVELS + 1][2], qstyle = 0, expn[MAX_BANDS] = {0}, mant[MAX_BANDS] = {0}, nq = 0;
    std::vector<uint8_t> body;
    // ---- main header ----
    for (;;) {
        const uint32_t m = in.u16();
        if (m == 0xFF90) break;
        if (m < 0xFF00) throw Refuse{ST_DAMAGED};
        const size_t at = in.pos;
        const uint32_t L = in.u16();
        if (L < 2) throw Refuse{ST_DAMAGED};
        in.need(L - 2);
        if (m == 0xFF51) {
            if (have_siz || L < 38) throw Refuse{ST_DAMAGED};
            in.u16();
            const uint32_t X = in.u32(), Y = in.u32(), XO = in.u32(), YO = in.u32(), XT = in.u32(), YT = in.u32(), XTO = in.u32(), YTO = in.u32();
            const uint32_t C = in.u16();
            if (L != 38 + 3 * C) throw Refuse{ST_DAMAGED};
            if (C != 3 || XO || YO || XTO || YTO || X < 1 || Y < 1 || X > (uint32_t)MAX_SIDE || Y > (uint32_t)MAX_SIDE || XT < X || YT < Y)
                throw Refuse{ST_SUBSET};
            for (int c = 0; c < 3; ++c)
                if (in.u8() != 7 || in.u8() != 1 || in.u8() != 1) throw Refuse{ST_SUBSET};
            if ((int)X != seg_w || (int)Y != seg_h) throw Refuse{ST_SUBSET};
            S.w = (int)X; S.h = (int)Y;
            have_siz = true;
        } else if (m == 0xFF52) {
            if (!have_siz || have_cod || L < 12) throw Refuse{ST_DAMAGED};
            const uint32_t scod = in.u8();
            S.progression = (int)in.u8(); S.layers = (int)in.u16(); S.mct = (int)in.u8(); S.levels = (int)in.u8();
            xcb = (int)in.u8() + 2; ycb = (int)in.u8() + 2;
            const uint32_t style = in.u8(), xform = in.u8();
            if ((scod & ~1u) || style || S.progression > 4 || S.layers < 1 || S.mct > 1 || S.levels > MAX_LEVELS || xcb > 6 || ycb > 6 || xform > 1)
                throw Refuse{ST_SUBSET};
            S.reversible = (int)xform;
            if (L != 12u + ((scod & 1) ? S.levels + 1 : 0)) throw Refuse{ST_DAMAGED};
            for (int r = 0; r <= S.levels; ++r) {
                const uint32_t v = (scod & 1) ? in.u8() : 0xFF;
                pp[r][0] = (int)(v & 15); pp[r][1] = (int)(v >> 4);
                if (r > 0 && (pp[r][0] == 0 || pp[r][1] == 0)) throw Refuse{ST_DAMAGED};
            }
            have_cod = true;
        } else if (m == 0xFF5C) {
            if (!have_cod || have_qcd || L < 4) throw Refuse{ST_DAMAGED};
            const uint32_t sq = in.u8();
            qstyle = (int)(sq & 31); S.guard = (int)(sq >> 5);
            if (qstyle != 0 && qstyle != 2) throw Refuse{ST_SUBSET};
            nq = (int)(L - 3) / (qstyle ? 2 : 1);
            if (nq < 3 * S.levels + 1) throw Refuse{ST_DAMAGED};
            for (int b = 0; b < 3 * S.levels + 1; ++b) {
                if (qstyle) { const uint32_t v = in.u16(); expn[b] = (int)(v >> 11); mant[b] = (int)(v & 2047); }
                else expn[b] = (int)(in.u8() >> 3);
            }
            have_qcd = true;
        } else if (m == 0xFF64 || m == 0xFF55 || m == 0xFF57 || m == 0xFF63) {
            // COM, TLM, PLM, CRG: nothing the decoder needs
        } else if (m == 0xFF53 || m == 0xFF5D || m == 0xFF5E || m == 0xFF5F || m == 0xFF60 || m == 0xFF61) {
            throw Refuse{ST_SUBSET};                         // COC, QCC, RGN, POC, PPM, PPT
        } else {
            throw Refuse{ST_DAMAGED};
        }
        in.pos = at + L;
    }
    if (!have_siz || !have_cod || !have_qcd) throw Refuse{ST_DAMAGED};
    if ((qstyle == 0) != (S.reversible == 1)) throw Refuse{ST_SUBSET};
    // ---- tile parts: their bodies one after the other ----
    for (;;) {                                               // in.pos is behind an SOT marker
        const size_t sot = in.pos - 2;
        if (in.u16() != 10) throw Refuse{ST_DAMAGED};
        if (in.u16() != 0) throw Refuse{ST_SUBSET};
        const uint32_t psot = in.u32();
        in.u8(); in.u8();
        size_t end = n;
        if (psot) {
            if (psot < 14 || psot > n - sot) throw Refuse{ST_DAMAGED};
            end = sot + psot;
        }
        for (;;) {
            const uint32_t m = in.u16();
            if (m == 0xFF93) break;
            const size_t at = in.pos;
            const uint32_t L = in.u16();
            if (L < 2) throw Refuse{ST_DAMAGED};
            in.need(L - 2);
            if (m != 0xFF64 && m != 0xFF58) throw Refuse{(m == 0xFF52 || m == 0xFF53 || m == 0xFF5C || m == 0xFF5D || m == 0xFF5E || m == 0xFF5F || m == 0xFF61) ? ST_SUBSET : ST_DAMAGED};
            in.pos = at + L;
        }
        if (in.pos > end) throw Refuse{ST_DAMAGED};
        if (!psot && end >= in.pos + 2 && d[end - 2] == 0xFF && d[end - 1] == 0xD9) end -= 2;
        body.insert(body.end(), d + in.pos, d + end);
        in.pos = end;
        if (in.n - in.pos < 2) break;
        const uint32_t m = in.u16();
        if (m == 0xFFD9) break;
        if (m != 0xFF90) throw Refuse{ST_DAMAGED};
    }
    // ---- geometry: precincts, their sub-bands and code blocks ----
    const int NL = S.levels;
    std::vector<Cblk> cb;
    std::vector<Precinct> prec;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r <= NL; ++r) {
            const int rw = ceil_shift(S.w, NL - r), rh = ceil_shift(S.h, NL - r);
            const int ppx = pp[r][0], ppy = pp[r][1];
            const int npx = ceil_shift(rw, ppx), npy = ceil_shift(rh, ppy);
            const int lw = r ? ceil_shift(S.w, NL - r + 1) : 0, lh = r ? ceil_shift(S.h, NL - r + 1) : 0;   // the resolution below
            for (int py = 0; py < npy; ++py)
                for (int px = 0; px < npx; ++px) {
                    Precinct P;
                    P.r = r; P.c = c;
                    P.x = (int64_t)px << (ppx + NL - r); P.y = (int64_t)py << (ppy + NL - r);
                    for (int o = r ? 1 : 0; o <= (r ? 3 : 0); ++o) {
                        PBand B;
                        B.orient = o; B.res = r; B.band = r ? 3 * (r - 1) + o : 0;
                        B.mb = expn[B.band] + S.guard - 1;
                        const int bw = r ? ((o & 1) ? rw - lw : lw) : rw, bh = r ? ((o & 2) ? rh - lh : lh) : rh;
                        const int bx = (r && (o & 1)) ? lw : 0, by = (r && (o & 2)) ? lh : 0;
                        const int sx = r ? ppx - 1 : ppx, sy = r ? ppy - 1 : ppy;
                        const int cx = std::min(xcb, sx), cy = std::min(ycb, sy);
                        const int x0 = std::min<int64_t>((int64_t)px << sx, bw), x1 = (int)std::min<int64_t>((int64_t)(px + 1) << sx, bw);
                        const int y0 = std::min<int64_t>((int64_t)py << sy, bh), y1 = (int)std::min<int64_t>((int64_t)(py + 1) << sy, bh);
                        B.first = (int)cb.size();
                        if (x1 > x0 && y1 > y0) {
                            const int gx0 = x0 >> cx, gx1 = ceil_shift(x1, cx), gy0 = y0 >> cy, gy1 = ceil_shift(y1, cy);
                            B.ncw = gx1 - gx0; B.nch = gy1 - gy0;
                            if ((int64_t)cb.size() + (int64_t)B.ncw * B.nch > 3 * 65536) throw Refuse{ST_SUBSET};
                            for (int j = gy0; j < gy1; ++j)
                                for (int i = gx0; i < gx1; ++i) {
                                    Cblk k;
                                    const int ax0 = std::max(i << cx, x0), ax1 = std::min((i + 1) << cx, x1);
                                    const int ay0 = std::max(j << cy, y0), ay1 = std::min((j + 1) << cy, y1);
                                    k.x0 = bx + ax0; k.y0 = by + ay0; k.w = ax1 - ax0; k.h = ay1 - ay0;
                                    cb.push_back(k);
                                }
                            B.incl.init(B.ncw, B.nch); B.zbps.init(B.ncw, B.nch);
                        }
                        P.bands.push_back(std::move(B));
                    }
                    prec.push_back(std::move(P));
                }
        }
    // ---- the order of the packets ----
    std::vector<std::pair<int, int>> order;                   // (precinct, layer)
    std::vector<int> idx(prec.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    auto key = [&](int i) {
        const Precinct& P = prec[i];
        switch (S.progression) {
            case 2: return std::make_tuple((int64_t)P.r, P.y, P.x, (int64_t)P.c, (int64_t)0);          // RPCL
            case 3: return std::make_tuple(P.y, P.x, (int64_t)P.c, (int64_t)P.r, (int64_t)0);          // PCRL
            case 4: return std::make_tuple((int64_t)P.c, P.y, P.x, (int64_t)P.r, (int64_t)0);          // CPRL
            default: return std::make_tuple((int64_t)P.r, (int64_t)P.c, P.y, P.x, (int64_t)0);         // LRCP, RLCP
        }
    };
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return key(a) < key(b); });
    if ((int64_t)idx.size() * S.layers > (1 << 22)) throw Refuse{ST_SUBSET};
    if (S.progression == 0) {
        for (int l = 0; l < S.layers; ++l)
            for (int i : idx) order.emplace_back(i, l);
    } else if (S.progression == 1) {
        for (int r = 0; r <= NL; ++r)
            for (int l = 0; l < S.layers; ++l)
                for (int i : idx) if (prec[i].r == r) order.emplace_back(i, l);
    } else {
        for (int i : idx)
            for (int l = 0; l < S.layers; ++l) order.emplace_back(i, l);
    }
    // ---- the packets ----
    size_t pos = 0;
    std::vector<std::pair<int, uint32_t>> got;                // (code block, bytes) of the packet at hand
    for (const auto& pl : order) {
        Precinct& P = prec[pl.first];
        const int layer = pl.second;
        Bits b(body.data(), body.size(), pos);
        got.clear();
        if (b.bit()) {
            for (PBand& B : P.bands)
                for (int j = 0; j < B.nch; ++j)
                    for (int i = 0; i < B.ncw; ++i) {
                        const int ci = B.first + j * B.ncw + i;
                        Cblk& k = cb[ci];
                        bool inc;
                        if (!k.included) inc = B.incl.below(b, i, j, layer + 1);
                        else inc = b.bit() != 0;
                        if (!inc) continue;
                        if (!k.included) {
                            int z = 0;
                            while (!B.zbps.below(b, i, j, z + 1)) if (++z > 64) throw Refuse{ST_DAMAGED};
                            k.zbp = z; k.included = true;
                            if (B.mb - z < 1) throw Refuse{ST_DAMAGED};
                            if (B.mb - z > MAX_BPS) throw Refuse{ST_SUBSET};
                        }
                        int np;
                        if (!b.bit()) np = 1;
                        else if (!b.bit()) np = 2;
                        else {
                            uint32_t v = b.bits(2);
                            if (v < 3) np = 3 + (int)v;
                            else { v = b.bits(5); if (v < 31) np = 6 + (int)v; else np = 37 + (int)b.bits(7); }
                        }
                        while (b.bit()) if (++k.lblock > 24) throw Refuse{ST_DAMAGED};
                        int lg = 0;
                        while ((np >> (lg + 1)) > 0) ++lg;
                        const uint32_t len = b.bits(k.lblock + lg);
                        k.passes += np;
                        if (k.passes > 3 * (B.mb - k.zbp) - 2) throw Refuse{ST_DAMAGED};
                        got.emplace_back(ci, len);
                    }
        }
        b.align();
        pos = b.pos;
        for (const auto& g : got) {
            if (g.second > body.size() - pos) throw Refuse{ST_DAMAGED};
            Cblk& k = cb[g.first];
            if (g.second) k.pieces.emplace_back((uint32_t)pos, g.second);
            k.len += g.second;
            pos += g.second;
        }
    }
    // ---- the block table and the codewords ----
    for (const Precinct& P : prec)
        for (const PBand& B : P.bands)
            for (int q = 0; q < B.ncw * B.nch; ++q) {
                const Cblk& k = cb[B.first + q];
                if (!k.included || k.passes < 1) continue;
                Block o;
                o.seg = 0; o.comp = P.c; o.band = B.band | B.orient << 8 | B.res << 16;
                o.x0 = k.x0; o.y0 = k.y0; o.w = k.w; o.h = k.h; o.mb = B.mb; o.zbp = k.zbp; o.passes = k.passes;
                o.off = (uint32_t)out.bytes.size(); o.len = k.len;
                for (const auto& pc : k.pieces) out.bytes.insert(out.bytes.end(), body.begin() + pc.first, body.begin() + pc.first + pc.second);
                out.bytes.insert(out.bytes.end(), CW_PAD, 0xFF);
                while (out.bytes.size() % CW_ALIGN) out.bytes.push_back(0xFF);
                out.blocks.push_back(o);
            }
    for (int bnd = 0; bnd < 3 * NL + 1; ++bnd)
        S.half_step[bnd] = S.reversible ? 0.5f : 0.5f * (float)((1.0 + mant[bnd] / 2048.0) * ldexp(1.0, 8 - expn[bnd]));
    S.n_blocks = (int)out.blocks.size();
}

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

}  // namespace

extern "C" {

size_t bqio_j2k_seg_bytes(void) { return sizeof(bqj2k::Seg); }
size_t bqio_j2k_block_bytes(void) { return sizeof(bqj2k::Block); }

int bqio_j2k_extract(const uint8_t* data, size_t data_len, const uint64_t* off, const uint64_t* len, int64_t n, int seg_w, int seg_h,
                     int32_t* seg_desc, int32_t* blocks, int64_t blocks_cap, uint8_t* bytes, size_t bytes_cap, int64_t* n_blocks,
                     size_t* n_bytes, int n_threads) {
    if (n < 0 || n > (1 << 24) || seg_w <= 0 || seg_h <= 0 || !seg_desc || !n_blocks || !n_bytes || (n && (!data || !off || !len)))
        return BQIO_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (off[i] > data_len || len[i] > data_len - off[i]) return BQIO_ERR_ARG;
    std::vector<Parsed> P((size_t)n);
    run_threads((int)n, n_threads, [&](int i) {
        Parsed& o = P[(size_t)i];
        try {
            parse_segment(data + off[i], (size_t)len[i], seg_w, seg_h, o);
        } catch (const Refuse& r) {
            const int w = o.seg.w, h = o.seg.h;
            memset(&o.seg, 0, sizeof(o.seg));
            o.seg.status = r.status; o.seg.w = w; o.seg.h = h;
            o.blocks.clear(); o.bytes.clear();
        }
    });
    int64_t nb = 0;
    uint64_t by = 0;
    for (int64_t i = 0; i < n; ++i) {
        P[(size_t)i].seg.first_block = (int32_t)nb;
        nb += (int64_t)P[(size_t)i].blocks.size();
        by += P[(size_t)i].bytes.size();
        if (nb > (1ll << 30) || by > (1ull << 31)) return BQIO_ERR_ARG;
    }
    *n_blocks = nb; *n_bytes = (size_t)by;
    for (int64_t i = 0; i < n; ++i) memcpy(seg_desc + (size_t)i * SEG_I32, &P[(size_t)i].seg, sizeof(Seg));
    if (!blocks && !bytes) return BQIO_OK;                   // a probe: the sizes and the descriptors
    if (!blocks || !bytes || blocks_cap < nb || bytes_cap < by) return BQIO_ERR_ARG;
    uint64_t at = 0;
    int64_t bi = 0;
    for (int64_t i = 0; i < n; ++i) {
        Parsed& o = P[(size_t)i];
        for (Block b : o.blocks) {
            b.seg = (int32_t)i; b.off += (uint32_t)at;
            memcpy(blocks + (size_t)bi++ * BLOCK_I32, &b, sizeof(b));
        }
        if (!o.bytes.empty()) memcpy(bytes + at, o.bytes.data(), o.bytes.size());
        at += o.bytes.size();
    }
    return BQIO_OK;
}

int bqio_j2k_decode_canvas(const int32_t* seg_desc, int n, const int32_t* blocks, int64_t n_blocks, const uint8_t* bytes, size_t n_bytes,
                           int seg_w, int seg_h, int ycc, const int32_t* place, uint8_t* canvas, int H, int W, const int32_t* clip,
                           int32_t* status, int32_t* t1_out, int n_threads) {
    if (n < 0 || n_blocks < 0 || seg_w <= 0 || seg_h <= 0 || seg_w > MAX_SIDE || seg_h > MAX_SIDE || !bqcanvas::canvas_args_ok(H, W) ||
        !canvas || !clip || (n && (!seg_desc || !place || !status)) || (n_blocks && (!blocks || !bytes)))
        return BQIO_ERR_ARG;
    const size_t plane = (size_t)seg_w * seg_h;
    run_threads(n, n_threads, [&](int i) {
        Seg s;
        memcpy(&s, seg_desc + (size_t)i * SEG_I32, sizeof(s));
        if (t1_out) memset(t1_out + (size_t)i * 3 * plane, 0, 3 * plane * 4);
        if (s.status) { status[i] = s.status; return; }
        if (!seg_ok(s, seg_w, seg_h) || s.first_block < 0 || s.n_blocks < 0 || (int64_t)s.first_block + s.n_blocks > n_blocks) { status[i] = ST_DESC; return; }
        // a row of the segment's own range that names it and fails block_ok marks it, as the device does; rows that name
        // another segment are nobody's
        for (int q = s.first_block; q < s.first_block + s.n_blocks; ++q) {
            Block b;
            memcpy(&b, blocks + (size_t)q * BLOCK_I32, sizeof(b));
            if (b.seg == i && !block_ok(b, n, seg_w, seg_h, n_bytes)) { status[i] = ST_DESC; return; }
        }
        std::vector<int32_t> a(3 * plane, 0), bq(3 * plane, 0);
        std::vector<uint16_t> fl(3 * plane, 0);
        uint32_t tab[MQ_STATES];
        uint8_t cx[CX_N];
        for (int k = 0; k < MQ_STATES; ++k) tab[k] = mq_table_row(k);
        for (int q = s.first_block; q < s.first_block + s.n_blocks; ++q) {
            Block b;
            memcpy(&b, blocks + (size_t)q * BLOCK_I32, sizeof(b));
            if (b.seg != i) continue;
            t1_block(b, bytes, a.data() + b.comp * plane, fl.data() + b.comp * plane, seg_w, tab, cx, 1);
        }
        if (t1_out) memcpy(t1_out + (size_t)i * 3 * plane, a.data(), 3 * plane * 4);
        for (int c = 0; c < 3; ++c) {
            int32_t* A = a.data() + c * plane;
            int32_t* B = bq.data() + c * plane;
            for (int y = 0; y < s.h; ++y)
                for (int x = 0; x < s.w; ++x) A[(size_t)y * seg_w + x] = dequant_sample(A[(size_t)y * seg_w + x], s, x, y);
            for (int r = 1; r <= s.levels; ++r) {
                const int rw = ceil_shift(s.w, s.levels - r), rh = ceil_shift(s.h, s.levels - r);
                for (int y = 0; y < rh; ++y) synth_row(A, B, seg_w, rw, y, s.reversible);
                for (int x = 0; x < rw; ++x) synth_col(B, A, seg_w, rh, x, s.reversible);
            }
        }
        Window w;
        if (place_window(place[2 * i], place[2 * i + 1], s.w, s.h, H, W, clip, w))
            for (int y = w.y0; y < w.y1; ++y)
                for (int x = w.x0; x < w.x1; ++x) {
                    const size_t p = (size_t)y * seg_w + x;
                    finish_pixel(a[p], a[plane + p], a[2 * plane + p], s, ycc,
                                 canvas + ((size_t)(place[2 * i + 1] + y) * W + (size_t)(place[2 * i] + x)) * 3);
                }
        status[i] = ST_OK;
    });
    return BQIO_OK;
}

void bqio_ycc_to_rgb(const uint8_t* ycc, uint8_t* rgb, size_t pixels) {
    for (size_t i = 0; i < pixels; ++i) bqycc::ycc_to_rgb(ycc[3 * i], ycc[3 * i + 1], ycc[3 * i + 2], rgb + 3 * i);
}

}  // extern "C"
