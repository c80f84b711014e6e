// The network side of libbiscuit_hip.so's C ABI (include/biscuit_hip.h): the context (create, destroy, errors, options, masked
// streams, tile indices), the BQW1 weight blob, the Xception launch schedule and its walker (backbone, MC-dropout head, bq_mc_infer,
// the debug taps, bq_describe_schedule) and event-based per-kernel timing.  A tool's entry point stands beside its kernel, in
// kernels_*.hip; bq_ctx.h is what they share with this file.
#include "bq_ctx.h"

#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <string.h>

namespace {

std::string g_create_error;

constexpr int pad16(int c) { return (c + 15) / 16 * 16; }

// ---- the matrix layers of Xception, in network order ---------------------------------------------------------------
// What is fixed about each: bq_load_weights registers from this table, the backbone walks it, choose_route decides from it.
enum LayerFlags : int {
    F_RES = 1,         // adds the block's input (the third separable convolution of a middle-flow block)
    F_DWTMP = 2,       // the walker has scratch for the depthwise kernel's output (two-kernel form)
    F_SPLIT_TMP = 4,   // ... and for the partial sums of split-K
    F_POOLED = 8       // feeds the global average pool
};

struct Layer {
    const char* name;       // blob prefix; the debug-tap name of its output, except:
    const char* out_name;   // the block output this layer completes ("blockN_out": shortcut rows, F_RES rows), or null
    int cin, cout;          // true channels
    int ldi, ldo;           // padded channels: the row strides of its input and output (elements)
    int kpad;               // padded contraction length
    int prod;               // BqProducer; PROD_DW*: has depthwise taps
    int Hi, H;              // input / output map (square)
    int relu;               // ReLU behind it
    int flags;
};

#define SEP(name, out, cin, cout, prod, hw, relu, flags) {name, out, cin, cout, pad16(cin), pad16(cout), pad16(cin), prod, hw, hw, relu, flags}
#define SHORTCUT(b, cin, cout, hi) {"block" #b "_res", "block" #b "_out", cin, cout, pad16(cin), pad16(cout), pad16(cin), PROD_S2, hi, (hi + 1) / 2, 0, 0}
#define ENTRY(b, cin, cout, prod1, hw)                                                 \
    SEP("block" #b "_sepconv1", nullptr, cin, cout, prod1, hw, 1, 0),                   \
    SEP("block" #b "_sepconv2", nullptr, cout, cout, PROD_DW, hw, 0, 0),                \
    SHORTCUT(b, cin, cout, hw)
#define MIDDLE(b)                                                                      \
    SEP("block" #b "_sepconv1", nullptr, 728, 728, PROD_DW_RELU, 19, 1, F_DWTMP),       \
    SEP("block" #b "_sepconv2", nullptr, 728, 728, PROD_DW, 19, 1, F_DWTMP),            \
    SEP("block" #b "_sepconv3", "block" #b "_out", 728, 728, PROD_DW, 19, 0, F_DWTMP | F_RES)
const Layer kLayers[] = {
    {"block1_conv2", nullptr, 32, 64, 32, 64, 288, PROD_IM2COL, 149, 147, 1, 0},
    ENTRY(2, 64, 128, PROD_DW, 147),
    ENTRY(3, 128, 256, PROD_DW_RELU, 74),
    ENTRY(4, 256, 728, PROD_DW_RELU, 37),
    MIDDLE(5), MIDDLE(6), MIDDLE(7), MIDDLE(8), MIDDLE(9), MIDDLE(10), MIDDLE(11), MIDDLE(12),
    SEP("block13_sepconv1", nullptr, 728, 728, PROD_DW_RELU, 19, 1, 0),
    SEP("block13_sepconv2", nullptr, 728, 1024, PROD_DW, 19, 0, 0),
    SHORTCUT(13, 728, 1024, 19),
    SEP("block14_sepconv1", nullptr, 1024, 1536, PROD_DW, 10, 1, F_DWTMP | F_SPLIT_TMP),
    SEP("block14_sepconv2", nullptr, 1536, 2048, PROD_DW, 10, 1, F_DWTMP | F_SPLIT_TMP | F_POOLED),
};
#undef SEP
#undef SHORTCUT
#undef ENTRY
#undef MIDDLE
static_assert(sizeof kLayers / sizeof kLayers[0] == kNumLayers, "bq_ctx.h sizes bq_ctx::layers by kNumLayers");
// first rows of the blocks the walker names: three rows per block up to block 13 (a strided block's third is its shortcut)
constexpr int kConv2 = 0, kBlock2 = 1, kBlock5 = 10, kBlock13 = 34, kBlock14 = 37;

}  // namespace

int fail(bq_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

int prof_class(bq_ctx* c, const std::string& name, double flops, double bytes) {
    int k = -1;
    for (size_t i = 0; i < c->prof_names.size(); ++i)
        if (c->prof_names[i] == name) { k = (int)i; break; }
    if (k < 0) {
        c->prof_names.push_back(name);
        c->prof_flops.push_back(0.0);
        c->prof_bytes.push_back(0.0);
        c->prof_launches.push_back(0);
        c->prof_ms.push_back(0.0);
        k = (int)c->prof_names.size() - 1;
    }
    c->prof_flops[k] += flops;
    c->prof_bytes[k] += bytes;
    return k;
}

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr long long kMaxAct = 147LL * 147 * 128;
constexpr long long kMaxRes = 74LL * 74 * 128;

struct WsLayout {
    size_t a, b, c, r, staged, feat, h0, h1, state, rmax, total;
};

WsLayout ws_layout(const bq_ctx* c, int n, int mc) {
    const size_t es = esize(c);
    WsLayout L{};
    // The streaming and tail kernels (kernels_stream.hip, kernels_front.hip) read -- and mask -- a few pixels OUTSIDE the tensor
    // they walk: the 16-bit pixel in front of an image's first row (window column -1) and up to three pixels (<= 768 B) behind
    // the last row of the last image.  Every activation buffer therefore has kActPad bytes of the workspace on both sides: the
    // pad in front of A, and a pad behind each of A, B, C and R (which is also the front pad of the next one).  run_conv hands
    // these kernels workspace buffers only.
    constexpr size_t kActPad = 4096;
    size_t off = kActPad;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
    L.a = take((size_t)n * kMaxAct * es + kActPad);
    L.b = take((size_t)n * kMaxAct * es + kActPad);
    L.c = take((size_t)n * kMaxAct * es + kActPad);
    L.r = take((size_t)n * kMaxRes * es + kActPad);
    L.staged = take((size_t)n * kStaged * es);
    L.feat = take((size_t)n * 2048 * 4);
    const size_t rows = (size_t)n * (mc > 0 ? mc : 1);
    L.h0 = take(rows * 1024 * 4);
    L.h1 = take(rows * 1024 * 4);
    L.state = take((size_t)n * 5 * 4);
    L.rmax = take(rows * 2 * 4);            // max |hidden_0| per row and column half (kernels_head.hip)
    L.total = off;
    return L;
}

// ---- routes: which kernel family runs a layer ------------------------------------------
int pick_shape(const bq_ctx* c, int prod, int nfp) {
    if (prod == PROD_IM2COL) return SHAPE_A;
    if (is16(c->cfg.dtype)) {
        // 64-row tiles halve the staging tile: four workgroups per CU instead of two for N = 256
        // (128->256 @37x37: 0.161 -> 0.111 ms); for N = 128 they measured slower (0.194 -> 0.234 ms)
        if (prod == PROD_S2 && nfp == 8) return SHAPE_K;
        switch (nfp) {
            case 4: return SHAPE_B;
            case 8: return SHAPE_C;
            case 24: return SHAPE_D;
            case 32: return SHAPE_E;
            case 48: return SHAPE_F;
            case 64: return SHAPE_G;
        }
        return -1;
    }
    if (nfp == 4) return SHAPE_B;
    if (nfp == 8) return SHAPE_C;
    return SHAPE_H;
}

enum RouteKind : int {
    R_ERROR,
    R_FRONT,               // uint8 tiles: staging + block1_conv1 + block1_conv2 in one kernel (kernels_front.hip)
    R_STREAM,              // kernels_stream.hip
    R_TILE,                // kernels_tile.hip: block1_conv2 of the float entry ("TILE kind=0")
    R_DW_THEN_EXIT,        // depthwise kernel (kernels_split.hip), then kernels_exit.hip
    R_S2_TILED_GEMM,       // the 128 x 128-tile GEMM (kernels_split.hip) over the even pixels of the input map
    R_WIDE,                // kernels_wide.hip
    R_FUSED_GEMM,          // kernels_gemm.hip, `nsplit` launches over slices of K: the one fallback below the routes above
    // the end of a block with a strided shortcut (asked of its shortcut row):
    R_BLOCK_TAIL,          // sepconv2 + max-pool + shortcut + add in one kernel (kernels_stream.hip); sepconv2 is not launched
    R_POOL_GEMM,           // the shortcut as the tiled GEMM with the pooling pass as its store pass
    R_CONV_THEN_POOL       // the shortcut by its own route `conv`, then the pool + add kernel (kernels_misc.hip)
};
const char* const kRouteNames[] = {"ERROR", "FRONT", "STREAM", "TILE", "DW_THEN_EXIT", "S2_TILED_GEMM", "WIDE",
                                   "FUSED_GEMM", "BLOCK_TAIL", "POOL_GEMM", "CONV_THEN_POOL"};

struct Route {
    RouteKind kind = R_ERROR;
    RouteKind conv = R_ERROR;   // the convolution's own route: `kind` itself unless kind == R_CONV_THEN_POOL
    int nsplit = 1, shape = -1; // R_FUSED_GEMM
    bool gap = false;           // R_DW_THEN_EXIT: the global average pool is the GEMM's epilogue (GAP_EPILOGUE), the tensor is not written
    int err = BQ_OK;            // R_ERROR: the code, its text in *why
};

// was one of these tensors, which a fusion does not write, asked for by a debug tap?
bool wants(const char* tap, const char* a, const char* b = nullptr) {
    return tap && (strcmp(tap, a) == 0 || (b && strcmp(tap, b) == 0));
}

bool has_front(const bq_ctx* c) { return is16(c->cfg.dtype) && c->front_ws16 && c->front_wc16 && c->layers[kConv2].wp; }

// THE schedule: the route of layer `li` for a batch of n tiles.  `from_u8`: the walk starts from the uint8 tiles (block1_conv2
// only); `tap`: the debug tap of this walk, or null.  Decides only: nothing is launched or allocated.  The order of the tests is
// the specification -- the first route whose conditions hold wins.
Route choose_route(const bq_ctx* c, int li, int n, bool from_u8, const char* tap, std::string* why) {
    const Layer& L = kLayers[li];
    const GemmLayer& G = c->layers[li];
    const int dtype = c->cfg.dtype;
    Route r;
    auto error = [&](int code, const std::string& msg) { r.kind = r.conv = R_ERROR; r.err = code; *why = msg; return r; };
    auto conv = [&](RouteKind k) { r.conv = k; if (r.kind != R_CONV_THEN_POOL) r.kind = k; return r; };
    if (!G.wp) return error(BQ_ERR_WEIGHTS, std::string("layer not loaded: ") + L.name);
    if (li == kConv2 && from_u8) {
        if (!has_front(c)) return error(BQ_ERR_ARG, "the fused front kernel needs a 16-bit context with its weights loaded");
        if (wants(tap, "staged", "block1_conv1"))
            return error(BQ_ERR_ARG, "the fused front kernel does not materialise the staged tile or block1_conv1");
        if (front_supported(dtype, n)) return conv(R_FRONT);
        // a batch beyond the front kernel's 32-bit offsets: the walker stages the tiles and block1_conv2 takes the float entry's route
    }
    if (L.prod == PROD_S2) {   // a block's end
        const Layer& L2 = kLayers[li - 1];   // the block's last separable convolution is the row in front of its shortcut
        const GemmLayer& G2 = c->layers[li - 1];
        if (!wants(tap, L2.name, L.name) && G2.wp16 && G.wp16 && L2.cout == L.ldo && L.cin == L.ldi &&
            tail_supported(dtype, L.ldo, L.ldo, L.ldi, n, L.Hi, L.Hi))
            return conv(R_BLOCK_TAIL);
        const bool want_res = wants(tap, L.name);
        // blocks 3, 4 and 13 (K = 128 / 256 / 736): the shortcut tensor never goes to HBM, one launch instead of two
        // (block 2, K = 64, lives in the fused tail)
        if (is16(dtype) && !want_res && L.kpad >= 128 && G.nfp % 4 == 0) return conv(R_POOL_GEMM);
        r.kind = R_CONV_THEN_POOL;
    }
    const bool residual = L.flags & F_RES, dwp = L.prod == PROD_DW || L.prod == PROD_DW_RELU, same = L.H == L.Hi;
    const int vec = is16(dtype) ? 8 : 4, M = n * L.H * L.H;
    r.shape = pick_shape(c, L.prod, G.nfp);
    if (r.shape < 0) return error(BQ_ERR_ARG, std::string("no kernel shape for ") + L.name);
    while (gemm_lds_bytes(dtype, r.shape, L.kpad / r.nsplit) > 160 * 1024) {
        r.nsplit *= 2;
        if ((L.kpad / r.nsplit) % (2 * vec) != 0 || r.nsplit > 8) return error(BQ_ERR_ARG, std::string("cannot split K for ") + L.name);
    }
    const int nsplit = r.nsplit;
    if (nsplit > 1 && (residual || !(L.flags & F_SPLIT_TMP)))
        return error(BQ_ERR_ARG, std::string("split-K needs a temp and no residual: ") + L.name);
    // the 147x147 separable convolutions of block 2 and block3_sepconv1 on the streaming kernel
    if (dwp && G.wp16 && !residual && nsplit == 1 && same && L.ldi == L.kpad && L.ldo == L.cout &&
        stream_supported(dtype, L.kpad, L.cout, L.prod == PROD_DW_RELU, n, L.H, L.H))
        return conv(R_STREAM);
    if (is16(dtype) && L.prod == PROD_IM2COL && L.cin == 32 && L.cout == 64) return conv(R_TILE);
    // Two-kernel form (depthwise kernel + GEMM) for the wide exit-flow layers (K >= 1024: the fused kernel can only hold 32-64 rows
    // of A in LDS there and re-streams the 3-6 MB weight matrix per 32-64 rows): one image's pixels x 256 channels per workgroup on
    // 16x16x32 fragments, block 14.  No STREAM or TILE layer is that wide.
    if (L.kpad >= 1024 && is16(dtype) && dwp && G.nfp % 4 == 0 && (L.flags & F_DWTMP) && nsplit == 1 && G.wp16 && !residual &&
        L.ldi == L.kpad && L.ldo == L.cout && exit_supported(dtype, L.kpad, L.cout, L.H * L.H, n)) {
        // the pool as the epilogue (one workgroup owns an image's pixels) unless the convolution's own output was asked for
        r.gap = (L.flags & F_POOLED) && !wants(tap, L.name) && L.H * L.H <= 128;
        return conv(R_DW_THEN_EXIT);
    }
    // strided shortcut convolutions with many channels (blocks 4 and 13: K = 256 / 736): a plain GEMM whose A rows are the even
    // pixels of the input map (block 13: 0.13 -> 0.085 ms against the fused-producer form; block 4: the same 0.09 ms)
    if (L.prod == PROD_S2 && is16(dtype) && L.kpad >= 256 && G.nfp % 4 == 0 && nsplit == 1 && !residual) return conv(R_S2_TILED_GEMM);
    if (nsplit == 1 && G.wp16 && same && wide_supported(dtype, L.prod, G.nfp, L.H, L.H, L.kpad, L.ldo, L.ldi, L.ldo, M, residual))
        return conv(R_WIDE);
    return conv(R_FUSED_GEMM);
}

std::string route_text(const Route& r) {
    std::string t = kRouteNames[r.kind];
    if (r.kind == R_CONV_THEN_POOL) t += std::string(" ") + kRouteNames[r.conv];
    if (r.conv == R_TILE) t += " kind=0";
    if (r.conv == R_FUSED_GEMM) t += " nsplit=" + std::to_string(r.nsplit);
    if (r.conv == R_DW_THEN_EXIT) t += r.gap ? " GAP_EPILOGUE=yes" : " GAP_EPILOGUE=no";
    return t;
}

// ---- one walk of the backbone ----------------------------------------------------------
struct Tap {
    const char* want = nullptr;   // requested activation name (null: none)
    float* out = nullptr;
    void* out16 = nullptr;        // in the place of out: the tensor as it is stored, 16-bit and compact (bq_trunk_u8_packed)
    size_t out_elems = 0;
    int64_t written = -1;
};

struct Walk {
    bq_ctx* c; int n; hipStream_t s; Tap* tap;
    std::string* plan;   // bq_describe_schedule: "<layer or tensor> <route>\n" per step instead of its launches
    const char* want() const { return tap ? tap->want : nullptr; }
    bool tapped() const { return tap && tap->written >= 0; }
    void note(const char* what, const std::string& route) const { *plan += std::string(what) + " " + route + "\n"; }
};

// the route of layer li, or the failure; RUN-able
int route_for(const Walk& w, int li, bool from_u8, Route* r) {
    std::string why;
    *r = choose_route(w.c, li, w.n, from_u8, w.want(), &why);
    return r->kind == R_ERROR ? fail(w.c, r->err, why) : BQ_OK;
}

int launch_failed(bq_ctx* c, const char* what, const char* layer, int e) {
    return fail(c, BQ_ERR_HIP, std::string(what) + layer + ": " + hipGetErrorString((hipError_t)e));
}

// returns 1 if the tap asks for this tensor (the walk stops), 0 otherwise, <0 on error
int tap_nhwc(const Walk& w, const char* name, const void* buf, int H, int C, int ld) {
    Tap* t = w.tap;
    if (!wants(w.want(), name)) return 0;
    const long long rows = (long long)w.n * H * H;
    if (w.plan) { t->written = 0; return 1; }
    if ((size_t)(rows * C) > t->out_elems) return fail(w.c, BQ_ERR_ARG, "debug output too small");
    const int e = t->out16 ? launch_copy16_nhwc(buf, rows, C, ld, t->out16, w.s) : launch_to_f32_nhwc(buf, rows, C, ld, t->out, w.c->cfg.dtype, w.s);
    if (e) return fail(w.c, BQ_ERR_HIP, "debug copy failed");
    t->written = rows * C;
    return 1;
}

#define TAP_AT(name, buf, H, C, ld) \
    do { int _t = tap_nhwc(w, name, buf, H, C, ld); if (_t) return _t < 0 ? _t : BQ_OK; } while (0)
// row li's output under `name`: the row's own, or that of the block output it completes
#define TAP(name, li, buf) TAP_AT(name, buf, kLayers[li].H, kLayers[li].cout, kLayers[li].ldo)

GemmParams gemm_params(const bq_ctx* c, int li, int n, const void* in, const void* residual, void* out) {
    const Layer& L = kLayers[li];
    const GemmLayer& G = c->layers[li];
    GemmParams p{};
    p.in = in; p.wp = G.wp; p.dw = G.dw; p.scale = G.scale; p.bias = G.bias; p.residual = residual; p.out = out;
    p.M = n * L.H * L.H;
    p.K = L.kpad; p.KBtot = L.kpad / (is16(c->cfg.dtype) ? 16 : 8); p.kb0 = 0; p.k_off = 0;
    p.NFp = G.nfp; p.Nstore = L.ldo; p.ldo = L.ldo; p.ldi = L.ldi;
    p.H = L.H; p.W = L.H; p.Hi = L.Hi; p.Wi = L.Hi; p.relu = L.relu;
    return p;
}

// What the walker has for a convolution; the row's flags say which of the optional ones it takes.
struct ConvBufs {
    const void* in; void* out;
    const void* residual = nullptr;   // F_RES
    void* split_tmp = nullptr;        // F_SPLIT_TMP: partial sums of split-K
    void* dwtmp = nullptr;            // F_DWTMP: the depthwise kernel's output, >= n*H*W*ldi elements
    float* gap_out = nullptr;         // F_POOLED: fp32 [n][ldo] of the pooling epilogue; `out` is not written then
};

int launch_conv(const Walk& w, int li, const Route& rt, const ConvBufs& b) {
    bq_ctx* c = w.c;
    const Layer& L = kLayers[li];
    const GemmLayer& G = c->layers[li];
    if (w.plan) { w.note(L.prod == PROD_S2 ? L.out_name : L.name, route_text(rt)); return BQ_OK; }
    const int dtype = c->cfg.dtype, n = w.n, vec = is16(dtype) ? 8 : 4;
    hipStream_t s = w.s;
    const void* residual = (L.flags & F_RES) ? b.residual : nullptr;
    void* dwtmp = (L.flags & F_DWTMP) ? b.dwtmp : nullptr;
    void* split_tmp = (L.flags & F_SPLIT_TMP) ? b.split_tmp : nullptr;
    GemmParams p = gemm_params(c, li, n, b.in, residual, b.out);
    const double es = (double)esize(c);
    const double M = (double)p.M;
    const bool dwp = L.prod == PROD_DW || L.prod == PROD_DW_RELU;
    const double flops = 2.0 * M * L.cin * L.cout + (dwp ? 18.0 * M * L.cin : 0.0);
    const double in_rows = (double)n * L.Hi * L.Hi;
    const double kin = L.prod == PROD_IM2COL ? (double)L.ldi : (double)L.cin;
    const double bytes = es * (in_rows * kin * (L.prod == PROD_S2 ? 0.25 : 1.0) + M * L.cout * (residual ? 2.0 : 1.0)) +
                         es * (double)L.cin * L.cout;
    char cls[96];
    snprintf(cls, sizeof cls, "%s_k%d_n%d_%dx%d",
             L.prod == PROD_S2 ? "res1x1s2" : (L.prod == PROD_IM2COL ? "conv3x3" : "sepconv"), L.cin, L.cout, L.H, L.H);
    const bool two = rt.conv == R_DW_THEN_EXIT;   // its two kernels have scopes of their own
    ProfScope ps(c, s, two ? std::string("split_") + cls : std::string(cls), two ? 0.0 : flops, two ? 0.0 : bytes);
    const char* what = "launch ";
    int e = 0;
    switch (rt.conv) {
    case R_STREAM:
        what = "launch(stream) ";
        e = launch_sepconv_stream(dtype, L.kpad, L.cout, L.prod == PROD_DW_RELU, b.in, G.wp16, G.dw, G.scale, G.bias, b.out, n, L.H, L.H,
                                  L.relu, c->num_cus, s);
        break;
    case R_TILE:
        what = "launch(tile) ";
        e = launch_tile_conv(dtype, b.in, G.wp, G.scale, G.bias, b.out, n, L.H, L.H, L.Hi, L.Hi, L.relu, c->num_cus, s);
        break;
    case R_DW_THEN_EXIT: {
        const bool gap = rt.gap;
        {
            ProfScope pd(c, s, std::string("dw3x3_") + cls, 18.0 * M * L.cin, 2.0 * es * M * L.cin);
            what = "launch(dw3x3) ";
            e = launch_dw3x3(dtype, b.in, G.dw, dwtmp, n, L.H, L.H, L.ldi, L.prod == PROD_DW_RELU, s);
        }
        if (e) break;
        ProfScope pg(c, s, std::string(gap ? "gemm_gap_" : "gemm_") + cls, 2.0 * M * L.cin * L.cout + (gap ? M * L.cout : 0.0),
                     gap ? es * M * L.cin + 4.0 * n * L.cout : es * (M * L.cin + M * L.cout * (residual ? 2.0 : 1.0)));
        what = "launch(exit_gemm) ";
        e = launch_exit_gemm(dtype, dwtmp, G.wp16, G.scale, G.bias, b.out, gap ? b.gap_out : nullptr, n, L.H * L.H, L.kpad, L.cout, L.relu,
                             c->feat_mul, s);
        break;
    }
    case R_S2_TILED_GEMM:
        what = "launch(gemm_tile s2) ";
        e = launch_gemm_tile(dtype, p, s, false);
        break;
    case R_WIDE:
        what = "launch(wide) ";
        e = launch_sepconv_wide(dtype, L.prod, p, G.wp16, c->num_cus, s);
        break;
    case R_FUSED_GEMM:
        for (int sp = 0; sp < rt.nsplit && e == 0; ++sp) {
            const bool last = sp == rt.nsplit - 1;
            p.K = L.kpad / rt.nsplit;
            p.k_off = sp * p.K;
            p.kb0 = sp * (p.K / (2 * vec));
            p.bias = last ? G.bias : nullptr;
            p.relu = last ? L.relu : 0;
            p.residual = last ? (rt.nsplit > 1 ? split_tmp : residual) : (sp > 0 ? split_tmp : nullptr);
            p.out = last ? b.out : split_tmp;
            e = launch_gemm(dtype, L.prod, rt.shape, p, s);
        }
        break;
    default:
        return fail(c, BQ_ERR_ARG, std::string("not a convolution's route: ") + L.name);
    }
    return e != 0 ? launch_failed(c, what, L.name, e) : BQ_OK;
}

// *gap: the layer's route pooled its output into b.gap_out
int run_conv(const Walk& w, int li, const ConvBufs& b, bool* gap = nullptr) {
    Route rt;
    RUN(route_for(w, li, false, &rt));
    if (gap) *gap = rt.gap;
    return launch_conv(w, li, rt, b);
}

// uint8 tiles -> block1_conv2 (R_FRONT): the tiles' statistics, then staging + block1_conv1 + block1_conv2 as one kernel
int launch_front_route(const Walk& w, const uint8_t* u8, void* out) {
    bq_ctx* c = w.c;
    const int n = w.n;
    const GemmLayer& G = c->layers[kConv2];
    if (w.plan) { w.note(kLayers[kConv2].name, kRouteNames[R_FRONT]); return BQ_OK; }
    {
        ProfScope ps(c, w.s, "stage_stats", 2.0 * n * kStaged, (double)n * kStaged);
        if (launch_stage_stats(u8, n, 299, c->d_stage_stats, w.s)) return fail(c, BQ_ERR_HIP, "stage stats launch failed");
    }
    const double p1 = (double)n * 149 * 149, p2 = (double)n * 147 * 147;
    ProfScope ps(c, w.s, "front_stage_stem_conv2", 2.0 * p1 * 27 * 32 + 2.0 * p2 * 288 * 64 + 4.0 * n * kStaged,
                 (double)n * kStaged + (double)esize(c) * p2 * 64);
    const int e = launch_front(c->cfg.dtype, u8, reinterpret_cast<const unsigned long long*>(c->d_stage_stats), c->front_ws16, c->stem_s,
                               c->stem_b, c->front_wc16, G.scale, G.bias, out, n, c->num_cus, w.s);
    return e ? launch_failed(c, "launch(front)", "", e) : BQ_OK;
}

// End of a block with a strided shortcut (row li), by route rt: out = maxpool3x3/s2(sepconv2) + BN(conv1x1/s2(x)).  y: sepconv2's
// output -- R_BLOCK_TAIL: sepconv1's, the tail runs sepconv2 itself.  R_CONV_THEN_POOL puts the shortcut into `out` first (where
// a tap finds it) and the pooling pass adds to it in place.  x and out must not overlap.
int launch_block_end(const Walk& w, int li, const Route& rt, const void* x, const void* y, void* out) {
    bq_ctx* c = w.c;
    const Layer& L = kLayers[li];
    const GemmLayer& G = c->layers[li];
    const GemmLayer& G2 = c->layers[li - 1];
    const int dtype = c->cfg.dtype, n = w.n, ci = L.ldi, co = L.ldo;
    hipStream_t s = w.s;
    const double es = (double)esize(c), M = (double)n * L.Hi * L.Hi, Mo = (double)n * L.H * L.H;
    if (rt.kind == R_CONV_THEN_POOL) {
        RUN(launch_conv(w, li, rt, {x, out}));
        TAP(L.name, li, out);
        if (w.plan) return BQ_OK;
        char cls[64];
        snprintf(cls, sizeof cls, "maxpool_add_%d_c%d", L.Hi, L.cout);
        ProfScope ps(c, s, cls, 9.0 * Mo * co, es * ((double)n * L.Hi * L.Hi * co + 2.0 * Mo * co));
        if (launch_pool_add(y, out, out, n, L.Hi, L.Hi, co, dtype, s)) return fail(c, BQ_ERR_HIP, "pool_add launch failed");
        return BQ_OK;
    }
    if (w.plan) { w.note(L.out_name, route_text(rt)); return BQ_OK; }
    if (rt.kind == R_BLOCK_TAIL) {
        char cls[64];
        snprintf(cls, sizeof cls, "blocktail_%d_c%d", L.Hi, L.cout);
        ProfScope ps(c, s, cls, 2.0 * M * co * co + 18.0 * M * co + 2.0 * Mo * ci * co + 9.0 * Mo * co,
                     es * (M * co + Mo * ci + Mo * co) + es * ((double)co * co + (double)ci * co));
        const int e = launch_block_tail(dtype, co, co, ci, y, G2.wp16, G2.dw, G2.scale, G2.bias, x, G.wp16, G.scale, G.bias, out, n,
                                        L.Hi, L.Hi, c->num_cus, s);
        return e ? launch_failed(c, "launch(block tail) ", kLayers[li - 1].name, e) : BQ_OK;
    }
    ProfScope ps(c, s, std::string("respool_") + std::to_string(L.Hi) + "_c" + std::to_string(L.cout),
                 2.0 * Mo * L.cin * L.cout + 9.0 * Mo * co, es * ((double)n * L.Hi * L.Hi * co + Mo * co + Mo * ci) + es * (double)L.cin * L.cout);
    const int e = launch_gemm_tile(dtype, gemm_params(c, li, n, x, y, out), s, true);   // R_POOL_GEMM
    return e ? launch_failed(c, "launch(gemm_tile pool) ", L.name, e) : BQ_OK;
}

// One block with a strided shortcut: rows s1 (first separable convolution), s1 + 1, s1 + 2 (shortcut).  x -> out; t1, t2: scratch.
int strided_block(const Walk& w, int s1, const void* x, void* t1, void* t2, void* out) {
    RUN(run_conv(w, s1, {x, t1}));
    TAP(kLayers[s1].name, s1, t1);
    Route end;
    RUN(route_for(w, s1 + 2, false, &end));
    if (end.kind != R_BLOCK_TAIL) {
        RUN(run_conv(w, s1 + 1, {t1, t2}));
        TAP(kLayers[s1 + 1].name, s1 + 1, t2);
    }
    RUN(launch_block_end(w, s1 + 2, end, x, end.kind == R_BLOCK_TAIL ? t1 : t2, out));
    if (w.tapped()) return BQ_OK;
    TAP(kLayers[s1 + 2].out_name, s1 + 2, out);
    return BQ_OK;
}

// The backbone of w.n tiles, walking kLayers in order: in_nchw (the staged planar tensor) or, u8 != nullptr, the uint8 tiles
// themselves -> feat.  Stops behind the tensor w.tap asks for.
int backbone_impl(const Walk& w, const void* in_nchw, float* feat, unsigned char* ws, const uint8_t* u8 = nullptr) {
    bq_ctx* c = w.c;
    const int n = w.n, dt = c->cfg.dtype;
    hipStream_t s = w.s;
    const WsLayout L = ws_layout(c, n, 1);
    auto at = [&](size_t off) { return reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(ws) + off); };   // (ws is null under w.plan)
    void* A = at(L.a); void* B = at(L.b); void* C = at(L.c); void* R = at(L.r);
    const double es = (double)esize(c);
    Route front;
    RUN(route_for(w, kConv2, u8 != nullptr, &front));
    if (front.kind == R_FRONT) {
        RUN(launch_front_route(w, u8, B));
    } else {
        if (u8) {   // the uint8 entry past the front kernel's limit: stage the tiles, go on as the float entry does
            in_nchw = at(L.staged);
            if (!w.plan) RUN(bq_stage(c, u8, n, at(L.staged), (bq_stream_t)s));
        }
        if (wants(w.want(), "staged")) {
            if (w.plan) { w.tap->written = 0; return BQ_OK; }
            if ((size_t)n * kStaged > w.tap->out_elems) return fail(c, BQ_ERR_ARG, "debug output too small");
            if (launch_nchw_to_f32_nhwc(in_nchw, n, 3, 299 * 299, w.tap->out, dt, s)) return fail(c, BQ_ERR_HIP, "debug copy failed");
            w.tap->written = (int64_t)n * kStaged;
            return BQ_OK;
        }
        if (!w.plan) {   // block1_conv1 + bn + relu  (vector ALU)
            const double px = (double)n * 149 * 149;
            ProfScope ps(c, s, "stem_conv1_3x3s2", 2.0 * px * 27 * 32, es * ((double)n * kStaged + px * 32));
            if (launch_stem1(in_nchw, n, c->stem_w, c->stem_s, c->stem_b, A, dt, s)) return fail(c, BQ_ERR_HIP, "stem1 launch failed");
        }
        TAP_AT("block1_conv1", A, 149, 32, 32);   // (not a matrix layer: no row)
        RUN(launch_conv(w, kConv2, front, {A, B}));
    }
    TAP(kLayers[kConv2].name, kConv2, B);
    // entry flow, blocks 2-4: input and output alternate between B and R, A and C are scratch.  Block 4 reads B and writes R.
    void* X = B; void* Y = R;
    for (int s1 = kBlock2; s1 < kBlock5; s1 += 3) {
        RUN(strided_block(w, s1, X, A, C, Y));
        if (w.tapped()) return BQ_OK;
        void* t = X; X = Y; Y = t;
    }
    // middle flow, blocks 5-12 at 19x19x728 (stride 736): B is the scratch buffer S of the middle and exit flow
    void* S = B; Y = A;
    for (int s1 = kBlock5; s1 < kBlock13; s1 += 3) {
        RUN(run_conv(w, s1, {X, Y, nullptr, nullptr, S}));
        TAP(kLayers[s1].name, s1, Y);
        RUN(run_conv(w, s1 + 1, {Y, C, nullptr, nullptr, S}));
        TAP(kLayers[s1 + 1].name, s1 + 1, C);
        RUN(run_conv(w, s1 + 2, {C, Y, X, nullptr, S}));
        void* t = X; X = Y; Y = t;
        TAP(kLayers[s1 + 2].out_name, s1 + 2, X);
    }
    // exit flow: block 13's output goes to S (X is its input); X is scratch from there on
    RUN(strided_block(w, kBlock13, X, Y, C, S));
    if (w.tapped()) return BQ_OK;
    RUN(run_conv(w, kBlock14, {S, Y, nullptr, C, X}));
    TAP(kLayers[kBlock14].name, kBlock14, Y);
    bool pooled = false;
    RUN(run_conv(w, kBlock14 + 1, {Y, C, nullptr, S, X, feat}, &pooled));
    if (!pooled) {
        TAP(kLayers[kBlock14 + 1].name, kBlock14 + 1, C);
        if (w.plan) {
            w.note("global_avg_pool", "GAP_KERNEL");
        } else {
            ProfScope ps(c, s, "global_avg_pool", (double)n * 100 * 2048, es * (double)n * 100 * 2048 + 4.0 * n * 2048);
            if (launch_gap(C, n, 100, 2048, 2048, feat, c->feat_mul, dt, s)) return fail(c, BQ_ERR_HIP, "gap launch failed");
        }
    }
    if (w.want()) return fail(c, BQ_ERR_ARG, std::string("unknown activation: ") + w.want());
    return BQ_OK;
}

int head_impl(bq_ctx* c, const float* feat, int n, int64_t tile0, int mc_n, int pass0, uint64_t seed,
              int init, int finalize, float* state, float* mean2, float* std2, unsigned char* ws,
              hipStream_t s) {
    const WsLayout L = ws_layout(c, n, mc_n);
    float* h0 = (float*)(ws + L.h0);
    float* h1 = (float*)(ws + L.h1);
    float* rmax = (float*)(ws + L.rmax);
    const unsigned thresh = c->drop_thresh;
    const float dscale = c->drop_scale;
    const int rows = n * mc_n;
    for (int layer = 0; layer < 2; ++layer) {
        const HeadLayer& G = c->head[layer];
        if (!G.wh) return fail(c, BQ_ERR_WEIGHTS, "head weights not loaded");
        const int K = G.k;                       // 2048 / 1024
        // three f16 MFMAs per fp32 product (kernels_head.hip): 6 x the nominal FLOPs of the layer
        ProfScope ps(c, s, layer == 0 ? "mc_head_dense0" : "mc_head_dense1", 2.0 * rows * (double)K * 1024,
                     4.0 * ((layer == 0 ? (double)n : (double)rows) * K + (double)rows * 1024 + (double)K * 1024));
        const int e = launch_head_dense(layer == 0 ? feat : h0, G.wh, G.wl, G.bias, G.wexp, layer == 0 ? h0 : h1, rmax, rows, K,
                                        mc_n, pass0, layer == 0 ? 1 : 0, layer, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
                                        thresh, dscale, tile0, c->d_tile0, c->d_tile_idx, s);
        if (e) return fail(c, BQ_ERR_HIP, std::string("head dense launch: ") + hipGetErrorString((hipError_t)e));
    }
    {
        ProfScope ps(c, s, "mc_head_softmax_welford", 2.0 * rows * 1024 * 2, 4.0 * rows * 1024);
        if (launch_head_final(h1, n, mc_n, pass0, tile0, c->d_tile0, c->d_tile_idx, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
                              thresh, dscale, c->logits_w, c->logits_b, init, finalize, state, mean2, std2, s))
            return fail(c, BQ_ERR_HIP, "head_final launch failed");
    }
    return BQ_OK;
}

// The dropout contract of oracle/philox.py for `rate` (checked by the callers: 0 <= rate < 1).
void set_dropout(bq_ctx* c, double rate) {
    const double t = floor(rate * 4294967296.0);
    c->drop_thresh = t > 4294967295.0 ? 4294967295u : (unsigned)t;
    c->drop_scale = (float)(1.0 / (1.0 - rate));
}

const float* entry_f32(bq_ctx* c, const std::string& name) {
    auto it = c->entries.find(name);
    return it == c->entries.end() ? nullptr : reinterpret_cast<const float*>(it->second.p);
}

// row li of kLayers from the blob's entries
int register_gemm_layer(bq_ctx* c, int li, int vec, int elt) {
    const std::string name = kLayers[li].name;
    const int cout = kLayers[li].cout, kpad = kLayers[li].kpad;
    const bool has_dw = kLayers[li].prod == PROD_DW || kLayers[li].prod == PROD_DW_RELU;
    GemmLayer L;
    auto w = c->entries.find(name + "/wp");
    if (w == c->entries.end()) return fail(c, BQ_ERR_WEIGHTS, "missing " + name + "/wp");
    const size_t per_nf = (size_t)(kpad / (2 * vec)) * 64 * vec * elt;
    if (per_nf == 0 || w->second.n % per_nf) return fail(c, BQ_ERR_WEIGHTS, "bad size for " + name + "/wp");
    L.nfp = (int)(w->second.n / per_nf);
    if (L.nfp * 32 < cout) return fail(c, BQ_ERR_WEIGHTS, "too few output fragments in " + name);
    L.wp = w->second.p;
    auto w16 = c->entries.find(name + "/wp16");
    if (w16 != c->entries.end()) {
        if (kpad % 32 || w16->second.n != (size_t)(kpad / 32) * ((size_t)L.nfp * 2) * 1024)
            return fail(c, BQ_ERR_WEIGHTS, "bad size for " + name + "/wp16");
        L.wp16 = w16->second.p;
    }
    L.scale = entry_f32(c, name + "/scale");
    L.bias = entry_f32(c, name + "/bias");
    if (!L.scale || !L.bias) return fail(c, BQ_ERR_WEIGHTS, "missing scale/bias for " + name);
    if (c->entries[name + "/scale"].n < (size_t)cout * 4 || c->entries[name + "/bias"].n < (size_t)cout * 4)
        return fail(c, BQ_ERR_WEIGHTS, "scale/bias of " + name + " shorter than its output channels");
    if (has_dw) {
        L.dw = entry_f32(c, name + "/dw");
        if (!L.dw) return fail(c, BQ_ERR_WEIGHTS, "missing " + name + "/dw");
        if (c->entries[name + "/dw"].n < (size_t)9 * kpad * 4)
            return fail(c, BQ_ERR_WEIGHTS, "depthwise taps of " + name + " shorter than 9 x its padded input channels");
    }
    c->layers[li] = L;
    return BQ_OK;
}

// Behind a network call's own argument check: the weights are loaded and the workspace holds n tiles x mc passes.  *L: its layout.
int ready(bq_ctx* c, int n, int mc, size_t ws_bytes, WsLayout* L) {
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    *L = ws_layout(c, n, mc);
    if (ws_bytes < L->total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
    return BQ_OK;
}

// bq_debug_activation (d_in: the staged tensor) and bq_debug_activation_u8 (d_tiles), behind their argument checks
int64_t debug_tap(bq_ctx* c, const char* name, const void* d_in, const uint8_t* d_tiles, int n, void* d_ws, size_t ws_bytes, float* d_out,
                  size_t out_elems, bq_stream_t stream) {
    WsLayout L;
    RUN(ready(c, n, 1, ws_bytes, &L));
    Tap t; t.want = name; t.out = d_out; t.out_elems = out_elems;
    unsigned char* ws = (unsigned char*)d_ws;
    const int r = backbone_impl({c, n, (hipStream_t)stream, &t, nullptr}, d_in, (float*)(ws + L.feat), ws, d_tiles);
    return r != BQ_OK ? r : t.written;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

bq_ctx* bq_create(int device_id, const bq_config* cfg) {
    if (!cfg) { g_create_error = "cfg is null"; return nullptr; }
    if (cfg->tile_px != 299 || cfg->n_classes != 2 ||
        (cfg->dtype != BQ_DTYPE_F32 && cfg->dtype != BQ_DTYPE_BF16 && cfg->dtype != BQ_DTYPE_F16) ||
        !(cfg->dropout >= 0.f) || !(cfg->dropout < 1.f)) {
        g_create_error = "unsupported config (need tile_px=299, n_classes=2, dtype f32|bf16|f16, 0<=dropout<1)";
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
        g_create_error = "no such HIP device";
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("libbiscuit_hip is built for gfx950 only, device is ") + prop.gcnArchName;
        return nullptr;
    }
    bq_ctx* c = new (std::nothrow) bq_ctx();
    if (!c) { g_create_error = "out of host memory"; return nullptr; }
    DeviceGuard guard(device_id);            // allocations below go to the context's device; the caller's stays current
    if (!guard.ok) { g_create_error = "hipSetDevice failed"; delete c; return nullptr; }
    c->cfg = *cfg;
    set_dropout(c, (double)cfg->dropout);
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (!reinhard_tables(&c->d_srgb_lut)) {
        g_create_error = "cannot allocate the sRGB tables";
        delete c;
        return nullptr;
    }
    if (hipMalloc(&c->d_stage_stats, (size_t)(cfg->max_batch > 0 ? cfg->max_batch : 1) * 16) != hipSuccess) {
        g_create_error = "cannot allocate the staging statistics";
        (void)hipFree(c->d_srgb_lut);
        delete c;
        return nullptr;
    }
    return c;
}

int bq_set_dropout(bq_ctx* c, double rate) {
    if (!c) return fail(c, BQ_ERR_ARG, "bq_set_dropout: null context");
    if (!(rate >= 0.0) || !(rate < 1.0)) return fail(c, BQ_ERR_ARG, "bq_set_dropout: the rate must lie in [0, 1)");
    set_dropout(c, rate);
    return BQ_OK;
}

void bq_destroy(bq_ctx* c) {
    if (!c) return;
    if (c->d_blob) (void)hipFree(c->d_blob);
    if (c->d_srgb_lut) (void)hipFree(c->d_srgb_lut);
    if (c->d_stage_stats) (void)hipFree(c->d_stage_stats);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
}

const char* bq_last_error(bq_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

size_t bq_workspace_bytes(bq_ctx* c, int batch, int mc_n) {
    if (!c || batch <= 0) return 0;
    return ws_layout(c, batch, mc_n).total;
}

int bq_load_weights(bq_ctx* c, const void* host_blob, size_t nbytes) {
    if (!c || !host_blob || nbytes < 16) return fail(c, BQ_ERR_ARG, "bad weight blob");
    const unsigned char* hb = (const unsigned char*)host_blob;
    uint32_t ver, cnt, dt;
    if (memcmp(hb, "BQW1", 4) != 0) return fail(c, BQ_ERR_WEIGHTS, "bad magic (want BQW1)");
    memcpy(&ver, hb + 4, 4); memcpy(&cnt, hb + 8, 4); memcpy(&dt, hb + 12, 4);
    if (ver != 1 || (size_t)16 + (size_t)cnt * 64 > nbytes) return fail(c, BQ_ERR_WEIGHTS, "bad header");
    if ((int)dt != c->cfg.dtype) return fail(c, BQ_ERR_WEIGHTS, "blob dtype does not match context dtype");
    // validate the directory before anything is allocated (wrap-free bounds: off and len are untrusted 64-bit values)
    for (uint32_t i = 0; i < cnt; ++i) {
        const unsigned char* e = hb + 16 + (size_t)i * 64;
        char name[49]; memcpy(name, e, 48); name[48] = 0;
        uint64_t off, len; memcpy(&off, e + 48, 8); memcpy(&len, e + 56, 8);
        if (off > nbytes || len > nbytes - off || (off & 255)) return fail(c, BQ_ERR_WEIGHTS, std::string("bad entry ") + name);
    }
    DeviceGuard guard(c->device);            // restores the caller's current device on every exit path
    if (!guard.ok) return fail(c, BQ_ERR_HIP, "hipSetDevice failed");
    if (c->d_blob) { (void)hipFree(c->d_blob); c->d_blob = nullptr; }
    c->entries.clear(); c->loaded = false;
    for (GemmLayer& g : c->layers) g = GemmLayer{};
    c->head[0] = c->head[1] = HeadLayer{};
    HIPCHK(c, hipMalloc((void**)&c->d_blob, nbytes));
    HIPCHK(c, hipMemcpy(c->d_blob, hb, nbytes, hipMemcpyHostToDevice));
    c->blob_bytes = nbytes;
    for (uint32_t i = 0; i < cnt; ++i) {
        const unsigned char* e = hb + 16 + (size_t)i * 64;
        char name[49]; memcpy(name, e, 48); name[48] = 0;
        uint64_t off, len; memcpy(&off, e + 48, 8); memcpy(&len, e + 56, 8);
        c->entries[name] = Blob{c->d_blob + off, (size_t)len};
    }
    const int vec = is16(c->cfg.dtype) ? 8 : 4;
    const int elt = is16(c->cfg.dtype) ? 2 : 4;
    c->stem_w = entry_f32(c, "block1_conv1/w");
    c->stem_s = entry_f32(c, "block1_conv1/scale");
    c->stem_b = entry_f32(c, "block1_conv1/bias");
    c->logits_w = entry_f32(c, "logits/w");
    c->logits_b = entry_f32(c, "logits/bias");
    if (!c->stem_w || !c->stem_s || !c->stem_b || !c->logits_w || !c->logits_b)
        return fail(c, BQ_ERR_WEIGHTS, "missing stem/logits tensors");
    c->feat_mul = 1.f;
    {
        auto fm = c->entries.find("act/feat_mul");
        if (fm != c->entries.end()) {
            if (fm->second.n < 4) return fail(c, BQ_ERR_WEIGHTS, "bad size for act/feat_mul");
            memcpy(&c->feat_mul, hb + (fm->second.p - c->d_blob), 4);
            if (!(c->feat_mul > 0.f) || !std::isfinite(c->feat_mul)) return fail(c, BQ_ERR_WEIGHTS, "act/feat_mul must be a positive finite number");
        }
    }
    c->trunk_mul = 1.f;
    {
        auto tm = c->entries.find("act/trunk_mul");
        if (tm != c->entries.end()) {
            if (tm->second.n < 4) return fail(c, BQ_ERR_WEIGHTS, "bad size for act/trunk_mul");
            memcpy(&c->trunk_mul, hb + (tm->second.p - c->d_blob), 4);
            if (!(c->trunk_mul > 0.f) || !std::isfinite(c->trunk_mul)) return fail(c, BQ_ERR_WEIGHTS, "act/trunk_mul must be a positive finite number");
        }
    }
    c->front_ws16 = c->front_wc16 = nullptr;
    {
        auto a = c->entries.find("block1_conv1/w16"), b = c->entries.find("block1_conv2/wp16");
        if (a != c->entries.end() && b != c->entries.end()) {
            if (a->second.n != 2 * 2 * 1024 || b->second.n != 9 * 4 * 1024)
                return fail(c, BQ_ERR_WEIGHTS, "bad size for block1_conv1/w16 or block1_conv2/wp16");
            c->front_ws16 = a->second.p;
            c->front_wc16 = b->second.p;
        }
    }
    for (int li = 0; li < kNumLayers; ++li) RUN(register_gemm_layer(c, li, vec, elt));
    for (int layer = 0; layer < 2; ++layer) {
        const std::string name = layer == 0 ? "hidden_0" : "hidden_1";
        const int K = layer == 0 ? 2048 : 1024;
        auto wh = c->entries.find(name + "/wph"), wl = c->entries.find(name + "/wpl"), bi = c->entries.find(name + "/bias");
        const size_t want = (size_t)32 * (K / 16) * 64 * 16;       // [1024 / 32][K / 16][64] x 16 B
        if (wh == c->entries.end() || wl == c->entries.end() || bi == c->entries.end() || wh->second.n != want ||
            wl->second.n != want || bi->second.n < 1024 * 4)
            return fail(c, BQ_ERR_WEIGHTS, "missing or malformed head tensors of " + name);
        int wexp = 0;
        auto we = c->entries.find(name + "/wexp");
        if (we != c->entries.end()) {
            if (we->second.n < 4) return fail(c, BQ_ERR_WEIGHTS, "bad size for " + name + "/wexp");
            memcpy(&wexp, hb + (we->second.p - c->d_blob), 4);
            if (wexp < -64 || wexp > 64) return fail(c, BQ_ERR_WEIGHTS, name + "/wexp must lie in [-64, 64]");
        }
        c->head[layer] = HeadLayer{wh->second.p, wl->second.p, reinterpret_cast<const float*>(bi->second.p), K, wexp};
    }
    c->loaded = true;
    return BQ_OK;
}

int bq_stream_create_masked(bq_ctx* c, const uint32_t* cu_mask, int mask_words, bq_stream_t* out) {
    if (!c || !cu_mask || mask_words <= 0 || !out) return fail(c, BQ_ERR_ARG, "bq_stream_create_masked: bad argument");
    hipStream_t s = nullptr;
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(c, BQ_ERR_HIP, "hipSetDevice failed");
    HIPCHK(c, hipExtStreamCreateWithCUMask(&s, (uint32_t)mask_words, cu_mask));
    *out = (bq_stream_t)s;
    return BQ_OK;
}

int bq_set_option(bq_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(c, BQ_ERR_ARG, "bq_set_option: bad argument");
    if (strcmp(name, "inflate_variant") == 0 && (value == 0 || value == 5)) { c->inflate_variant = value; return BQ_OK; }
    return fail(c, BQ_ERR_ARG, std::string("bq_set_option: unknown option or value: ") + name);
}

int bq_set_num_cus(bq_ctx* c, int n) {
    if (!c || n < 0 || n > 1024) return fail(c, BQ_ERR_ARG, "bq_set_num_cus: bad argument");
    int dev_cus = 256;
    if (n == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) dev_cus = prop.multiProcessorCount;
    }
    c->num_cus = n > 0 ? n : dev_cus;
    return BQ_OK;
}

int bq_stream_destroy(bq_ctx* c, bq_stream_t stream) {
    if (!c || !stream) return fail(c, BQ_ERR_ARG, "bq_stream_destroy: bad argument");
    HIPCHK(c, hipStreamDestroy((hipStream_t)stream));
    return BQ_OK;
}

int bq_backbone(bq_ctx* c, const void* d_in, int n, float* d_feat, void* d_ws, size_t ws_bytes,
                bq_stream_t stream) {
    if (!c || !d_in || !d_feat || !d_ws || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_backbone: bad argument");
    WsLayout L;
    RUN(ready(c, n, 1, ws_bytes, &L));
    return backbone_impl({c, n, (hipStream_t)stream, nullptr, nullptr}, d_in, d_feat, (unsigned char*)d_ws);
}

int bq_mc_head(bq_ctx* c, const float* d_feat, int n, int64_t tile_idx0, int mc_n, int pass0, uint64_t seed,
               int init, int finalize, float* d_state, float* d_mean2, float* d_std2, void* d_ws,
               size_t ws_bytes, bq_stream_t stream) {
    if (!c || !d_feat || !d_state || !d_ws || n <= 0 || mc_n <= 0 || n > c->cfg.max_batch ||
        mc_n > c->cfg.max_mc || pass0 < 0 || (finalize && (!d_mean2 || !d_std2)))
        return fail(c, BQ_ERR_ARG, "bq_mc_head: bad argument");
    WsLayout L;
    RUN(ready(c, n, mc_n, ws_bytes, &L));
    return head_impl(c, d_feat, n, tile_idx0, mc_n, pass0, seed, init, finalize, d_state, d_mean2, d_std2,
                     (unsigned char*)d_ws, (hipStream_t)stream);
}

int bq_set_tile_index_ptr(bq_ctx* c, const int64_t* d_tile_idx0) {
    if (!c) return BQ_ERR_ARG;
    c->d_tile0 = reinterpret_cast<const long long*>(d_tile_idx0);
    return BQ_OK;
}

int bq_set_tile_index_array(bq_ctx* c, const int64_t* d_tile_idx) {
    if (!c) return BQ_ERR_ARG;
    c->d_tile_idx = reinterpret_cast<const long long*>(d_tile_idx);
    return BQ_OK;
}

// uint8 tiles -> pooled features, the kernels bq_mc_infer runs: in a 16-bit context with the front weights loaded staging +
// block1_conv1 + block1_conv2 are ONE kernel straight from the bytes (kernels_front.hip) -- up to front_supported's batch, beyond
// it the walker stages the tiles itself --, otherwise bq_stage + the backbone on the planar tensor.  bq_mc_infer and bq_backbone_u8 share it, so a tile's features do not depend on which of the two a
// caller used for its batch.
static int features_from_u8(bq_ctx* c, const uint8_t* d_tiles, int n, float* feat, unsigned char* ws, const WsLayout& L,
                            bq_stream_t stream) {
    const Walk w{c, n, (hipStream_t)stream, nullptr, nullptr};
    if (has_front(c)) return backbone_impl(w, nullptr, feat, ws, d_tiles);
    void* staged = ws + L.staged;
    RUN(bq_stage(c, d_tiles, n, staged, stream));
    return backbone_impl(w, staged, feat, ws);
}

int bq_mc_infer(bq_ctx* c, const uint8_t* d_tiles, int n, int64_t tile_idx0, int mc_n, uint64_t seed,
                int mc_mode, float* d_mean2, float* d_std2, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || !d_tiles || !d_mean2 || !d_std2 || !d_ws || n <= 0 || mc_n <= 0 || n > c->cfg.max_batch ||
        mc_n > c->cfg.max_mc || (mc_mode != BQ_MC_HEAD && mc_mode != BQ_MC_FULL))
        return fail(c, BQ_ERR_ARG, "bq_mc_infer: bad argument");
    WsLayout L;
    RUN(ready(c, n, mc_n, ws_bytes, &L));
    unsigned char* ws = (unsigned char*)d_ws;
    hipStream_t s = (hipStream_t)stream;
    float* feat = (float*)(ws + L.feat);
    float* state = (float*)(ws + L.state);
    if (mc_mode == BQ_MC_HEAD) {
        RUN(features_from_u8(c, d_tiles, n, feat, ws, L, stream));
        return head_impl(c, feat, n, tile_idx0, mc_n, 0, seed, 1, 1, state, d_mean2, d_std2, ws, s);
    }
    // BQ_MC_FULL: the reference's loop structure -- the whole network once per pass.
    for (int p = 0; p < mc_n; ++p) {
        RUN(features_from_u8(c, d_tiles, n, feat, ws, L, stream));
        RUN(head_impl(c, feat, n, tile_idx0, 1, p, seed, p == 0, p == mc_n - 1, state, d_mean2, d_std2, ws, s));
    }
    return BQ_OK;
}

int bq_backbone_u8(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_feat, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || !d_tiles || !d_feat || !d_ws || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_backbone_u8: bad argument");
    WsLayout L;
    RUN(ready(c, n, 1, ws_bytes, &L));
    return features_from_u8(c, d_tiles, n, d_feat, (unsigned char*)d_ws, L, stream);
}

// bq_backbone_u8's walk up to block13_out -- the same launches by the same routes: the tap's name is no layer's, so it moves no
// route -- written as fp32 NHWC at true scale (the blob's activation exponent of the tensor removed, a power of two).
// d_out16: the packed form (bq_trunk_u8_packed) -- the tap copies the stored 16-bit tensor and nothing scales it.
static int trunk_impl(bq_ctx* c, const char* entry, const uint8_t* d_tiles, int n, float* d_out, void* d_out16, void* d_ws, size_t ws_bytes,
                      bq_stream_t stream) {
    const std::string e(entry);
    if (!c || !d_tiles || (!d_out && !d_out16) || !d_ws || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, e + ": bad argument");
    WsLayout L;
    RUN(ready(c, n, 1, ws_bytes, &L));
    unsigned char* ws = (unsigned char*)d_ws;
    const long long count = (long long)n * 100 * 1024;
    Tap t; t.want = "block13_out"; t.out = d_out; t.out16 = d_out16; t.out_elems = (size_t)count;
    const Walk w{c, n, (hipStream_t)stream, &t, nullptr};
    if (has_front(c)) {
        RUN(backbone_impl(w, nullptr, (float*)(ws + L.feat), ws, d_tiles));
    } else {
        void* staged = ws + L.staged;
        RUN(bq_stage(c, d_tiles, n, staged, stream));
        RUN(backbone_impl(w, staged, (float*)(ws + L.feat), ws));
    }
    if (t.written != count) return fail(c, BQ_ERR_HIP, e + ": block13_out was not written");
    if (!d_out16 && c->trunk_mul != 1.f && launch_scale_f32(d_out, count, c->trunk_mul, (hipStream_t)stream))
        return fail(c, BQ_ERR_HIP, e + ": scale launch failed");
    return BQ_OK;
}

int bq_trunk_u8(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_out, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    return trunk_impl(c, "bq_trunk_u8", d_tiles, n, d_out, nullptr, d_ws, ws_bytes, stream);
}

// The same walk with the tap's copy in the engine's own 16-bit type: what bq_trunk_u8 widens and multiplies by trunk_mul, unwidened.
int bq_trunk_u8_packed(bq_ctx* c, const uint8_t* d_tiles, int n, void* d_out16, float* mul, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || !d_out16 || !mul || ((uintptr_t)d_out16 & 15)) return fail(c, BQ_ERR_ARG, "bq_trunk_u8_packed: bad argument");
    if (!is16(c->cfg.dtype))
        return fail(c, BQ_ERR_ARG, "bq_trunk_u8_packed: a float32 engine stores block13_out in 32 bits: a 16-bit copy would not be lossless");
    *mul = c->trunk_mul;
    return trunk_impl(c, "bq_trunk_u8_packed", d_tiles, n, nullptr, d_out16, d_ws, ws_bytes, stream);
}

int bq_profile_enable(bq_ctx* c, int on) {
    if (!c) return BQ_ERR_ARG;
    c->prof = on != 0;
    if (on) {
        c->prof_recs.clear(); c->ev_used = 0;
        c->prof_names.clear(); c->prof_flops.clear(); c->prof_bytes.clear();
        c->prof_launches.clear(); c->prof_ms.clear();
    }
    return BQ_OK;
}

int bq_profile_read(bq_ctx* c, bq_prof_entry* out, int max_entries) {
    if (!c || !out || max_entries <= 0) return BQ_ERR_ARG;
    for (const ProfRec& r : c->prof_recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) return fail(c, BQ_ERR_HIP, "event sync failed");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return fail(c, BQ_ERR_HIP, "event elapsed failed");
        c->prof_ms[r.cls] += ms;
        c->prof_launches[r.cls] += 1;
    }
    c->prof_recs.clear();
    c->ev_used = 0;
    int k = 0;
    for (size_t i = 0; i < c->prof_names.size() && k < max_entries; ++i, ++k) {
        memset(&out[k], 0, sizeof out[k]);
        strncpy(out[k].name, c->prof_names[i].c_str(), sizeof out[k].name - 1);
        out[k].launches = c->prof_launches[i];
        out[k].ms = c->prof_ms[i];
        const double nl = c->prof_launches[i] > 0 ? (double)c->prof_launches[i] : 1.0;
        out[k].flops = c->prof_flops[i] / nl;      // per launch, averaged over the class's launches
        out[k].bytes = c->prof_bytes[i] / nl;
    }
    return k;
}

int64_t bq_debug_activation(bq_ctx* c, const char* name, const void* d_in, int n, void* d_ws, size_t ws_bytes,
                            float* d_out, size_t out_elems, bq_stream_t stream) {
    if (!c || !name || !d_in || !d_ws || !d_out || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_debug_activation: bad argument");
    return debug_tap(c, name, d_in, nullptr, n, d_ws, ws_bytes, d_out, out_elems, stream);
}

int64_t bq_debug_activation_u8(bq_ctx* c, const char* name, const uint8_t* d_tiles, int n, void* d_ws, size_t ws_bytes,
                               float* d_out, size_t out_elems, bq_stream_t stream) {
    if (!c || !name || !d_tiles || !d_ws || !d_out || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_debug_activation_u8: bad argument");
    return debug_tap(c, name, nullptr, d_tiles, n, d_ws, ws_bytes, d_out, out_elems, stream);
}

// The routes of one walk as text, one "<layer or block output> <route>" line per step, through the walker and choose_route of
// the calls above; nothing is launched.  from_u8: the walk of bq_mc_infer / bq_backbone_u8 (tap: of bq_debug_activation_u8),
// otherwise of bq_backbone / bq_debug_activation.  Ends behind the tapped tensor.  Returns the text's length.
int bq_describe_schedule(bq_ctx* c, int n, int from_u8, const char* tap, char* out, size_t cap) {
    if (!c || !out || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_describe_schedule: bad argument");
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    std::string plan;
    Tap t; t.want = tap;
    // (the tiles' pointer only says which entry the walk takes: nothing is read)
    const uint8_t* tiles = from_u8 && (tap || has_front(c)) ? reinterpret_cast<const uint8_t*>(out) : nullptr;
    RUN(backbone_impl({c, n, nullptr, &t, &plan}, nullptr, nullptr, nullptr, tiles));
    if (plan.size() + 1 > cap) return fail(c, BQ_ERR_ARG, "bq_describe_schedule: output too small");
    memcpy(out, plan.c_str(), plan.size() + 1);
    return (int)plan.size();
}

}  // extern "C"
