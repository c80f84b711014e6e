// C ABI of libbiscuit_hip.so (see include/biscuit_hip.h): context, BQW1 weight blob,
// the Xception launch schedule, the MC-dropout head and event-based per-kernel timing.
#include "../../include/biscuit_hip.h"
#include "bq_common.h"
#include "roi_device.h"

#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

namespace {

std::string g_create_error;

struct Blob { const unsigned char* p = nullptr; size_t n = 0; };

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
constexpr int kNumLayers = sizeof kLayers / sizeof kLayers[0];
// first rows of the blocks the walker names: three rows per block up to block 13 (a strided block's third is its shortcut)
constexpr int kConv2 = 0, kBlock2 = 1, kBlock5 = 10, kBlock13 = 34, kBlock14 = 37;
static_assert(kNumLayers == 39, "block1_conv2, 34 separable convolutions, 4 shortcuts");

struct GemmLayer {   // what the blob holds for row i of kLayers
    const void* wp = nullptr;
    const void* wp16 = nullptr;   // the same weights in 16x16x32 fragment order (kernels_wide / stream / exit.hip)
    const float* scale = nullptr;
    const float* bias = nullptr;
    const float* dw = nullptr;
    int nfp = 0;             // padded n-frags in wp
};


struct HeadLayer {
    const void* wh = nullptr; const void* wl = nullptr; const float* bias = nullptr; int k = 0;
    int wexp = 0;                  // "hidden_N/wexp" of the blob: wh / wl hold W * 2^-wexp (weights.py: head_weight_exponent)
};

struct ProfRec { int cls; hipEvent_t a, b; };

}  // namespace

struct bq_ctx {
    bq_config cfg{};
    int device = 0;
    std::string err;
    unsigned char* d_blob = nullptr;
    size_t blob_bytes = 0;
    std::map<std::string, Blob> entries;
    GemmLayer layers[kNumLayers];   // by row of kLayers
    const float* stem_w = nullptr; const float* stem_s = nullptr; const float* stem_b = nullptr;
    const void* front_ws16 = nullptr;   // "block1_conv1/w16" + "block1_conv2/wp16": the fused front kernel (kernels_front.hip)
    const void* front_wc16 = nullptr;
    const float* logits_w = nullptr; const float* logits_b = nullptr;
    HeadLayer head[2];             // hidden_0, hidden_1: weights split into two halves (kernels_head.hip)
    unsigned drop_thresh = 0;      // the dropout contract of oracle/philox.py from the rate as a double (bq_set_dropout):
    float drop_scale = 1.f;        // keep = r >= floor(rate * 2^32), y = x * fp32(1 / (1 - rate))
    bool loaded = false;
    int num_cus = 256;
    float* d_srgb_lut = nullptr;   // tables of the Reinhard normaliser
    const long long* d_tile0 = nullptr;   // bq_set_tile_index_ptr
    const long long* d_tile_idx = nullptr;   // bq_set_tile_index_array
    int inflate_variant = 5;       // bq_set_option("inflate_variant"): 5 = rounds of a literal-only fast phase + a general phase (LDS), 0 = the
                                   // kernel without LDS, tables in global memory (kernels_inflate.hip; profiles/r05_inflate.txt)
    float feat_mul = 1.f;          // "act/feat_mul" of the blob: 2^k of the pooled tensor's activation exponent (weights.py: pack_blob)
    double* d_stage_stats = nullptr;   // 2 x 64-bit integer sums per tile for the staging kernel pair
    // profiling
    bool prof = false;
    std::vector<std::string> prof_names;
    std::vector<double> prof_flops, prof_bytes;
    std::vector<int64_t> prof_launches;
    std::vector<double> prof_ms;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
};

namespace {

int fail(bq_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HIPCHK(c, expr)                                                                 \
    do {                                                                                \
        hipError_t _e = (hipError_t)(expr);                                             \
        if (_e != hipSuccess)                                                           \
            return fail((c), BQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct DeviceGuard {
    int prev = -1; bool ok = false;
    explicit DeviceGuard(int dev) { ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool is16(int dtype) { return dtype == BQ_DTYPE_BF16 || dtype == BQ_DTYPE_F16; }
inline size_t esize(const bq_ctx* c) { return is16(c->cfg.dtype) ? 2 : 4; }

constexpr long long kStaged = 3LL * 299 * 299;
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

// ---- profiling -----------------------------------------------------------------
// A class sums the algorithmic FLOPs and bytes of its launches: the instances of one class differ (8 of the 25
// 728 -> 728 layers read a residual, 406 against 270 MB), and bq_profile_read reports the launch-weighted average.
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

struct ProfScope {
    bq_ctx* c; hipStream_t s; int cls = -1; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(bq_ctx* c_, hipStream_t s_, const std::string& name, double flops, double bytes)
        : c(c_), s(s_) {
        if (!c->prof) return;
        if (c->ev_used + 2 > c->ev_pool.size()) {
            for (int i = 0; i < 256; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) return;
                c->ev_pool.push_back(e);
            }
        }
        cls = prof_class(c, name, flops, bytes);
        a = c->ev_pool[c->ev_used++];
        b = c->ev_pool[c->ev_used++];
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (cls < 0) return;
        (void)hipEventRecord(b, s);
        c->prof_recs.push_back({cls, a, b});
    }
};

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
        return conv(R_FRONT);
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
    const int e = launch_to_f32_nhwc(buf, rows, C, ld, t->out, w.c->cfg.dtype, w.s);
    if (e) return fail(w.c, BQ_ERR_HIP, "debug copy failed");
    t->written = rows * C;
    return 1;
}

#define RUN(expr) do { int _r = (expr); if (_r != BQ_OK) return _r; } while (0)
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
    {   // tables of the Reinhard normaliser (oracle/stain.py states the same arithmetic):
        // [0,256)   sRGB -> linear, float64 evaluation rounded to float32
        // [256,511) linear -> 8-bit sRGB as 255 switching points: entry v-1 is the smallest float32 c for which
        //           clip(trunc(255 * clip(gamma(c), 0, 1)), 0, 255) >= v, gamma(c) = c > 0.0031308 ?
        //           1.055f * float(pow(double(c), 1/2.4)) - 0.055f : 12.92f * c, found by bisection on the
        //           float bit pattern over [0, 2] (the function is monotone).  Not over [0, 1]: 1.055f * 1 - 0.055f rounds to the
        //           float below 1, so c = 1 is level 254 and the last point lies a few ulps ABOVE 1 (oracle/stain.py
        //           srgb_switch_points states the same search)
        float lut[512];
        for (int v = 0; v < 256; ++v) {
            const double x = (double)v / 255.0;
            lut[v] = (float)(x > 0.04045 ? std::pow((x + 0.055) / 1.055, 2.4) : x / 12.92);
        }
        auto level = [](float cf) {
            float g;
            if (cf > 0.0031308f) { const float p = (float)std::pow((double)cf, 1.0 / 2.4); g = 1.055f * p - 0.055f; }
            else g = cf * 12.92f;
            g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
            const float t = truncf(g * 255.0f);
            return (int)(t < 0.f ? 0.f : (t > 255.f ? 255.f : t));
        };
        for (int v = 1; v <= 255; ++v) {
            uint32_t lo = 0, hi = 0x40000000u;               // bit patterns of 0.0f and 2.0f; level(2.0f) = 255
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                float f;
                memcpy(&f, &mid, 4);
                if (level(f) >= v) hi = mid; else lo = mid + 1;
            }
            memcpy(&lut[256 + v - 1], &lo, 4);
        }
        lut[511] = 0.f;
        if (hipMalloc(&c->d_srgb_lut, sizeof lut) != hipSuccess ||
            hipMemcpy(c->d_srgb_lut, lut, sizeof lut, hipMemcpyHostToDevice) != hipSuccess) {
            g_create_error = "cannot allocate the sRGB tables";
            delete c;
            return nullptr;
        }
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

int bq_stage(bq_ctx* c, const uint8_t* d_tiles, int n, void* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || n < 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_stage: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stage_u8_standardize", 4.0 * n * kStaged, (double)n * kStaged * (1.0 + esize(c)));
    if (launch_stage_u8(d_tiles, n, 299, d_out, c->cfg.dtype, c->d_stage_stats, s))
        return fail(c, BQ_ERR_HIP, "stage launch failed");
    return BQ_OK;
}

namespace {
// float32 colour constants of the Reinhard normaliser: XYZ<-RGB, RGB<-XYZ (its float64 inverse rounded),
// D65 white (oracle/stain.py: constants())
const float kReinhardConsts[21] = {
    0.412452996f, 0.357580006f, 0.180423006f, 0.212670997f, 0.715160012f, 0.0721689984f, 0.0193339996f,
    0.119193003f, 0.950227022f,
    3.24048138f, -1.53715158f, -0.498536319f, -0.969254971f, 1.87599003f, 0.0415559262f, 0.0556466393f,
    -0.204041332f, 1.05731106f,
    0.950469971f, 1.0f, 1.08882999f};
}  // namespace

int bq_stain_reinhard_fast(bq_ctx* c, const uint8_t* d_tiles, int n, const float* target_means3,
                           const float* target_stds3, uint8_t* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || !target_means3 || !target_stds3 || n < 0)
        return fail(c, BQ_ERR_ARG, "bq_stain_reinhard_fast: bad argument");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(target_stds3[i]) || !std::isfinite(target_means3[i]))      // (a std of 0 or below is defined arithmetic)
            return fail(c, BQ_ERR_ARG, "bq_stain_reinhard_fast: non-finite target statistics");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_reinhard_fast", 300.0 * n * 299 * 299, 3.0 * n * kStaged);
    if (launch_reinhard(d_tiles, n, 299, c->d_srgb_lut, kReinhardConsts, target_means3, target_stds3, d_out, nullptr, s))
        return fail(c, BQ_ERR_HIP, "reinhard launch failed");
    return BQ_OK;
}

int bq_stain_lab_stats(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_stats6, bq_stream_t stream) {
    if (!c || !d_tiles || !d_stats6 || n < 0) return fail(c, BQ_ERR_ARG, "bq_stain_lab_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (launch_reinhard(d_tiles, n, 299, c->d_srgb_lut, kReinhardConsts, nullptr, nullptr, nullptr, d_stats6, s))
        return fail(c, BQ_ERR_HIP, "lab stats launch failed");
    return BQ_OK;
}

int bq_stain_macenko(bq_ctx* c, const uint8_t* d_tiles, int n, const float* he_ref6, const float* maxc_ref2,
                     uint8_t* d_out, int* d_status, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || !he_ref6 || !maxc_ref2 || n < 0)
        return fail(c, BQ_ERR_ARG, "bq_stain_macenko: bad argument");
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(he_ref6[i])) return fail(c, BQ_ERR_ARG, "bq_stain_macenko: non-finite stain matrix");
    for (int i = 0; i < 2; ++i)
        if (!std::isfinite(maxc_ref2[i]) || !(maxc_ref2[i] > 0.f))
            return fail(c, BQ_ERR_ARG, "bq_stain_macenko: target concentrations must be finite and > 0");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_macenko", 400.0 * n * 299 * 299, 3.0 * n * kStaged);
    if (launch_macenko(d_tiles, n, 299, he_ref6, maxc_ref2, d_out, nullptr, d_status, 1, s))
        return fail(c, BQ_ERR_HIP, "macenko launch failed");
    return BQ_OK;
}

int bq_stain_macenko_stats(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_stats8, int* d_status2, bq_stream_t stream) {
    if (!c || !d_tiles || !d_stats8 || n < 0) return fail(c, BQ_ERR_ARG, "bq_stain_macenko_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stain_macenko_stats", 350.0 * n * 299 * 299, 1.0 * n * kStaged);
    if (launch_macenko(d_tiles, n, 299, nullptr, nullptr, nullptr, d_stats8, d_status2, 2, s))
        return fail(c, BQ_ERR_HIP, "macenko stats launch failed");
    return BQ_OK;
}

size_t bq_range_ws_bytes(int n) { return n < 0 ? 0 : range_ws_bytes(n); }

int bq_range_key(bq_ctx* c, const uint8_t* d_tiles, int n, float* d_key, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || n < 0 || (n > 0 && (!d_tiles || !d_key || !d_ws))) return fail(c, BQ_ERR_ARG, "bq_range_key: bad argument");
    if (ws_bytes < range_ws_bytes(n)) return fail(c, BQ_ERR_ARG, "bq_range_key: scratch smaller than bq_range_ws_bytes(n)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "range_key", 2.0 * n * kStaged, (double)n * kStaged);
    if (launch_range_key(d_tiles, n, 299, d_ws, d_key, s)) return fail(c, BQ_ERR_HIP, "range key launch failed");
    return BQ_OK;
}

int bq_range_screen(bq_ctx* c, const uint8_t* d_tiles, int n, int64_t tile_idx0, const int64_t* d_tile_idx, float* d_cand_key,
                    int64_t* d_cand_idx, uint8_t* d_cand_tiles, int k, int filled, void* d_ws, size_t ws_bytes, bq_stream_t stream) {
    if (!c || n < 0 || n > 2048 || (n > 0 && (!d_tiles || !d_cand_key || !d_cand_idx || !d_cand_tiles || !d_ws)))
        return fail(c, BQ_ERR_ARG, "bq_range_screen: bad argument");
    if (k < 1 || k > range_max_slots() || filled < 0 || filled > k)
        return fail(c, BQ_ERR_ARG, "bq_range_screen: need 1 <= k <= " + std::to_string(range_max_slots()) + " and 0 <= filled <= k");
    if (ws_bytes < range_ws_bytes(n)) return fail(c, BQ_ERR_ARG, "bq_range_screen: scratch smaller than bq_range_ws_bytes(n)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "range_screen", 2.0 * n * kStaged, (double)n * kStaged);
    if (launch_range_screen(d_tiles, n, 299, (long long)tile_idx0, reinterpret_cast<const long long*>(d_tile_idx), d_cand_key,
                            reinterpret_cast<long long*>(d_cand_idx), d_cand_tiles, k, filled, d_ws, s))
        return fail(c, BQ_ERR_HIP, "range screen launch failed");
    return BQ_OK;
}

int bq_png_unfilter(bq_ctx* c, const uint8_t* d_rows, int n, int px, uint8_t* d_out, bq_stream_t stream) {
    if (!c || !d_rows || !d_out || n < 0 || px <= 0) return fail(c, BQ_ERR_ARG, "bq_png_unfilter: bad argument");
    if (launch_png_unfilter(d_rows, n, px, d_out, (hipStream_t)stream)) return fail(c, BQ_ERR_HIP, "png unfilter launch failed");
    return BQ_OK;
}

size_t bq_png_inflate_scratch_bytes(int n) { return inflate_scratch_bytes(n); }

int bq_png_inflate(bq_ctx* c, const uint8_t* d_z, const uint32_t* d_off, const uint32_t* d_len, int n, int px, uint8_t* d_rows,
                   size_t rows_stride, void* d_scratch, size_t scratch_bytes, int32_t* d_status, bq_stream_t stream) {
    if (!c || !d_z || !d_off || !d_len || !d_rows || !d_scratch || !d_status || n < 0 || px <= 0 || px > 4096)
        return fail(c, BQ_ERR_ARG, "bq_png_inflate: bad argument");
    const size_t row_bytes = (size_t)px * (3 * (size_t)px + 1);
    if (rows_stride < row_bytes + 4 || (rows_stride & 3) || rows_stride > 0xffffffffull) return fail(c, BQ_ERR_ARG, "bq_png_inflate: rows_stride must be a multiple of 4, >= px (1 + 3 px) + 4");
    if (scratch_bytes < inflate_scratch_bytes(n)) return fail(c, BQ_ERR_WORKSPACE, "bq_png_inflate: scratch too small");
    ProfScope ps(c, (hipStream_t)stream, "png_inflate", 0.0, (double)n * row_bytes * 2.0);
    const int e = launch_inflate(d_z, d_off, d_len, n, d_rows, (unsigned)row_bytes, (unsigned)rows_stride, d_scratch, d_status, (hipStream_t)stream,
                                 c->inflate_variant, (unsigned)(1 + 3 * px));
    if (e) return fail(c, BQ_ERR_HIP, std::string("png inflate launch: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
}

size_t bq_jpeg_scratch_bytes(int n, int px) { return jpeg_scratch_bytes(n, px); }

int bq_jpeg_decode(bq_ctx* c, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int px,
                   uint8_t* d_out, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || px <= 0 || px > 4096 || n_tables < 0) return fail(c, BQ_ERR_ARG, "bq_jpeg_decode: bad argument");
    if (n == 0) return BQ_OK;
    if (!d_scan || !d_desc || !d_tables || n_tables == 0 || !d_out || !d_status || !d_scratch || ((uintptr_t)d_tables & 3) ||
        ((uintptr_t)d_scan & 15) || ((uintptr_t)d_desc & 3))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode: bad argument");
    if (scratch_bytes < jpeg_scratch_bytes(n, px)) return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_decode: scratch too small");
    ProfScope ps(c, (hipStream_t)stream, "jpeg_decode", 0.0, (double)n * px * px * 3.0);
    const int e = launch_jpeg_decode(d_scan, d_desc, d_tables, n_tables, n, px, d_out, d_status, d_scratch, scratch_bytes, (hipStream_t)stream);
    if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg decode launch: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
}

size_t bq_jpeg_canvas_scratch_bytes(int n, int seg_w, int seg_h) { return jpeg_canvas_scratch_bytes(n, seg_w, seg_h); }

int bq_jpeg_decode_canvas(bq_ctx* c, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int seg_w,
                          int seg_h, const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0, int clip_x1,
                          int clip_y1, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || seg_w <= 0 || seg_w > 4096 || seg_h <= 0 || seg_h > 4096 || n_tables < 0 || H <= 0 || W <= 0 || H > (1 << 28) ||
        W > (1 << 28))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode_canvas: bad argument (need 0 < seg_w, seg_h <= 4096 and 0 < H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_scan || !d_desc || !d_tables || n_tables == 0 || !d_place || !d_canvas || !d_status || !d_scratch || ((uintptr_t)d_tables & 3) ||
        ((uintptr_t)d_scan & 15) || ((uintptr_t)d_desc & 3) || ((uintptr_t)d_place & 3))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_decode_canvas: bad argument");
    if (scratch_bytes < jpeg_canvas_scratch_bytes(1, seg_w, seg_h))
        return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_decode_canvas: scratch smaller than one segment's (bq_jpeg_canvas_scratch_bytes(1, seg_w, seg_h))");
    const int32_t clip[4] = {clip_x0, clip_y0, clip_x1, clip_y1};
    ProfScope ps(c, (hipStream_t)stream, "jpeg_decode_canvas", 0.0, (double)n * seg_w * seg_h * 3.0);
    const int e = launch_jpeg_decode_canvas(d_scan, d_desc, d_tables, n_tables, n, seg_w, seg_h, d_place, d_canvas, H, W, clip, d_status,
                                            d_scratch, scratch_bytes, (hipStream_t)stream);
    if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg canvas decode launch: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
}

size_t bq_jpeg_encode_scratch_bytes(int n, int px, int subsampling) { return jpeg_encode_scratch_bytes(n, px, subsampling); }

int bq_jpeg_encode(bq_ctx* c, const uint8_t* d_tiles, int n, int px, int quality, int subsampling, uint8_t* d_out, int64_t cap,
                   int64_t* d_off, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream) {
    if (!c || n < 0 || cap < 0) return fail(c, BQ_ERR_ARG, "bq_jpeg_encode: bad argument");
    if (px < 1 || px > 4096 || quality < 1 || quality > 100 || (subsampling != 0 && subsampling != 2))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_encode: outside the encoder's subset (need 1 <= px <= 4096, 1 <= quality <= 100, subsampling 0 = 4:4:4 or 2 = 4:2:0)");
    if (n == 0) return BQ_OK;
    if (!d_tiles || !d_off || !d_status || !d_scratch || (!d_out && cap) || ((uintptr_t)d_off & 7) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_scratch & 15))
        return fail(c, BQ_ERR_ARG, "bq_jpeg_encode: bad argument (null pointer, d_off not 8-byte or d_scratch not 16-byte aligned)");
    const int m = jpeg_encode_round_tiles(px, subsampling, scratch_bytes);
    if (m < 1) return fail(c, BQ_ERR_WORKSPACE, "bq_jpeg_encode: scratch smaller than one tile's (bq_jpeg_encode_scratch_bytes(1, px, subsampling))");
    hipStream_t s = (hipStream_t)stream;
    static const char* const kStage[JPEG_ENC_STAGES] = {"jpeg_encode_pixel", "jpeg_encode_size", "jpeg_encode_pack", "jpeg_encode_stuff"};
    const double blocks = (double)jpeg_encode_scratch_bytes(1, px, subsampling) / 344.0;       // (for the profile's byte column only: about the blocks of a tile)
    for (long long t0 = 0; t0 < n; t0 += m) {
        const int cnt = (int)(n - t0 < m ? n - t0 : m);
        for (int stage = 0; stage < JPEG_ENC_STAGES; ++stage) {
            ProfScope ps(c, s, kStage[stage], 0.0, stage == JPEG_ENC_PIXEL ? (double)cnt * px * px * 3.0 : (double)cnt * blocks * 128.0);
            const int e = launch_jpeg_encode_stage(stage, d_tiles, t0, cnt, m, px, quality, subsampling, d_scratch, d_out, (long long)cap,
                                                   (long long*)d_off, d_status, s);
            if (e) return fail(c, BQ_ERR_HIP, std::string("jpeg encode launch: ") + hipGetErrorString((hipError_t)e));
        }
    }
    return BQ_OK;
}

int bq_tile_resample(bq_ctx* c, const uint8_t* d_canvas, int H, int W, const int32_t* d_origin, int n, int src_px, int px,
                     const int32_t* d_bounds, const int32_t* d_coef, int ksize, uint8_t* d_out, bq_stream_t stream) {
    if (!c || n < 0 || n > (1 << 20) || px <= 0 || px > 4096 || src_px <= 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28) ||
        (int64_t)src_px > 8ll * px || (int64_t)px > 8ll * src_px)
        return fail(c, BQ_ERR_ARG, "bq_tile_resample: bad argument (need 0 < px <= 4096, px / 8 <= src_px <= 8 px, 0 <= n <= 2^20, H, W <= 2^28)");
    if (n == 0) return BQ_OK;
    if (!d_canvas || !d_origin || !d_out || ((uintptr_t)d_origin & 3)) return fail(c, BQ_ERR_ARG, "bq_tile_resample: bad argument");
    if (src_px != px) {
        if (!d_bounds || !d_coef || ((uintptr_t)d_bounds & 3) || ((uintptr_t)d_coef & 3) || ksize != resample_ksize(src_px, px))
            return fail(c, BQ_ERR_ARG, "bq_tile_resample: the tap tables are not bqio_resample_taps(src_px, px)'s");
        int rows = 0;
        if (!resample_strip_rows(src_px, px, ksize, &rows))
            return fail(c, BQ_ERR_ARG, "bq_tile_resample: the taps of one output row do not fit the kernel's LDS at this px and ratio");
    }
    if (resample_grid(n, src_px, px, ksize) > 0x7fffffffll)
        return fail(c, BQ_ERR_ARG, "bq_tile_resample: n x strips of output rows exceeds 2^31 - 1 workgroups; split the call");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tile_resample", 2.0 * 2 * 3 * (double)n * px * px * (src_px == px ? 0 : ksize),
                 (double)n * 3 * ((double)src_px * src_px + (double)px * px));
    if (launch_tile_resample(d_canvas, H, W, d_origin, n, src_px, px, d_bounds, d_coef, ksize, d_out, s))
        return fail(c, BQ_ERR_HIP, "tile resample launch failed");
    return BQ_OK;
}

int bq_tile_grayspace(bq_ctx* c, const uint8_t* d_tiles, int n, int px, const int32_t* d_limit256, int32_t* d_count, bq_stream_t stream) {
    if (!c || n < 0 || px <= 0 || px > 4096) return fail(c, BQ_ERR_ARG, "bq_tile_grayspace: bad argument");
    if (n == 0) return BQ_OK;
    if (!d_tiles || !d_limit256 || !d_count || ((uintptr_t)d_limit256 & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tile_grayspace: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tile_grayspace", 6.0 * n * px * px, 3.0 * n * px * px);
    if (launch_tile_grayspace(d_tiles, n, px, d_limit256, d_count, s)) return fail(c, BQ_ERR_HIP, "grayspace launch failed");
    return BQ_OK;
}

int bq_heatmap_render(bq_ctx* c, const float* d_values, int gh, int gw, const int32_t* d_col, const int32_t* d_row, int interpolation,
                      const uint8_t* d_lut, const uint8_t* d_thumb, uint8_t* d_out, int H, int W, float vmin, float inv_span, int A,
                      bq_stream_t stream) {
    if (!c || gh <= 0 || gw <= 0 || gh > (1 << 15) || gw > (1 << 15) || H <= 0 || W <= 0 || H > 16384 || W > 16384)
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument (need 0 < gh, gw <= 32768 and 0 < H, W <= 16384)");
    if (interpolation != 0 && interpolation != 1) return fail(c, BQ_ERR_ARG, "bq_heatmap_render: interpolation must be 0 (none) or 1 (bicubic)");
    if (!(A >= 0 && A <= 256) || !std::isfinite(vmin) || !std::isnormal(inv_span) || !(inv_span > 0.0f))
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument (need 0 <= A <= 256, vmin finite, inv_span a normal positive float)");
    if (!d_values || !d_col || !d_row || !d_lut || !d_thumb || !d_out || ((uintptr_t)d_values & 3) || ((uintptr_t)d_col & 3) ||
        ((uintptr_t)d_row & 3))
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: bad argument");
    const size_t bytes = (size_t)3 * H * W;
    if (d_out != d_thumb && d_out < d_thumb + bytes && d_thumb < d_out + bytes)
        return fail(c, BQ_ERR_ARG, "bq_heatmap_render: out must be the thumbnail itself or not overlap it");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "heatmap_render", 0.0, 2.0 * (double)bytes);
    if (launch_heatmap_render(d_values, gh, gw, d_col, d_row, interpolation, d_lut, d_thumb, d_out, H, W, vmin, inv_span, A, s))
        return fail(c, BQ_ERR_HIP, "heatmap render launch failed");
    return BQ_OK;
}

int bq_tissue_blur(bq_ctx* c, const uint8_t* d_thumb, int H, int W, const int32_t* d_sdiv256, uint8_t* d_plane, int32_t* d_hist,
                   bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31))
        return fail(c, BQ_ERR_ARG, "bq_tissue_blur: bad argument (need 0 < H, W and H * W < 2^31)");
    if (!d_thumb || !d_sdiv256 || !d_plane || !d_hist || ((uintptr_t)d_sdiv256 & 3) || ((uintptr_t)d_hist & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_blur: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_blur", 0.0, 4.0 * (double)H * W);
    if (launch_tissue_blur(d_thumb, H, W, d_sdiv256, d_plane, d_hist, s)) return fail(c, BQ_ERR_HIP, "tissue blur launch failed");
    return BQ_OK;
}

// The cells' ranges of a W x H plane, [a, b) pairs: 0 <= a < b <= W for a column, <= H for a row.  -> the refusal's text, or empty.
static std::string bad_cell_range(const char* plane, const int32_t* col_ranges, int gw, int W, const int32_t* row_ranges, int gh, int H) {
    for (int i = 0; i < gw; ++i)
        if (col_ranges[2 * i] < 0 || col_ranges[2 * i] >= col_ranges[2 * i + 1] || col_ranges[2 * i + 1] > W)
            return std::string("a column range is empty or outside the ") + plane;
    for (int i = 0; i < gh; ++i)
        if (row_ranges[2 * i] < 0 || row_ranges[2 * i] >= row_ranges[2 * i + 1] || row_ranges[2 * i + 1] > H)
            return std::string("a row range is empty or outside the ") + plane;
    return std::string();
}

int bq_tissue_cells(bq_ctx* c, const uint8_t* d_plane, int H, int W, int T, const int32_t* col_ranges, int gw, const int32_t* row_ranges,
                    int gh, int32_t* d_ranges, int32_t* d_count, bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) || gw <= 0 || gh <= 0 || gw > (1 << 15) || gh > (1 << 15) || T < 0 || T > 255)
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells: bad argument (need 0 < H, W, H * W < 2^31, 0 < gw, gh <= 32768 and 0 <= T <= 255)");
    if (!d_plane || !col_ranges || !row_ranges || !d_ranges || !d_count || ((uintptr_t)d_ranges & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells: bad argument");
    const std::string bad = bad_cell_range("plane", col_ranges, gw, W, row_ranges, gh, H);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, "bq_tissue_cells: " + bad);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_cells", 0.0, (double)H * W);
    HIPCHK(c, hipMemcpyAsync(d_ranges, col_ranges, (size_t)gw * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ranges + 2 * gw, row_ranges, (size_t)gh * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_tissue_cells(d_plane, H, W, T, d_ranges, d_ranges + 2 * gw, gw, gh, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue cells launch failed");
    return BQ_OK;
}

int bq_tissue_focus(bq_ctx* c, const uint8_t* d_thumb, int H, int W, const int32_t* d_taps, int r, int thr, int32_t* d_work,
                    int32_t* d_value_or_null, uint8_t* d_plane, int32_t* d_count, bq_stream_t stream) {
    if (!c || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) || r < 1 || r > 16 || thr < 0)
        return fail(c, BQ_ERR_ARG, "bq_tissue_focus: bad argument (need 0 < H, W, H * W < 2^31, 1 <= r <= 16 and 0 <= thr)");
    if (!d_thumb || !d_taps || !d_work || !d_plane || !d_count || ((uintptr_t)d_taps & 3) || ((uintptr_t)d_work & 3) ||
        ((uintptr_t)d_value_or_null & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_focus: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_focus", 2.0 * 2 * (2.0 * r + 1) * (double)H * W, (d_value_or_null ? 16.0 : 12.0) * (double)H * W);
    if (launch_tissue_focus(d_thumb, H, W, d_taps, r, thr, d_work, d_value_or_null, d_plane, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue focus launch failed");
    return BQ_OK;
}

int bq_tissue_cells_union(bq_ctx* c, const uint8_t* d_otsu_plane, int Ho, int Wo, int T, const uint8_t* d_focus_plane, int Hf, int Wf,
                          const int32_t* xmap, const int32_t* ymap, const int32_t* col_ranges, int gw, const int32_t* row_ranges, int gh,
                          int32_t* d_tables, int32_t* d_count, bq_stream_t stream) {
    if (!c || Ho <= 0 || Wo <= 0 || (int64_t)Ho * Wo >= (1ll << 31) || Hf <= 0 || Wf <= 0 || (int64_t)Hf * Wf >= (1ll << 31) || gw <= 0 ||
        gh <= 0 || gw > (1 << 15) || gh > (1 << 15) || T < 0 || T > 255)
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: bad argument (need 0 < H, W and H * W < 2^31 for both planes, 0 < gw, gh <= "
                                   "32768 and 0 <= T <= 255)");
    if (!d_otsu_plane || !d_focus_plane || !xmap || !ymap || !col_ranges || !row_ranges || !d_tables || !d_count ||
        ((uintptr_t)d_tables & 3) || ((uintptr_t)d_count & 3))
        return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: bad argument");
    const std::string bad = bad_cell_range("Otsu plane", col_ranges, gw, Wo, row_ranges, gh, Ho);
    if (!bad.empty()) return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: " + bad);
    for (int i = 0; i < Wo; ++i)
        if (xmap[i] < 0 || xmap[i] >= Wf || (i && xmap[i] < xmap[i - 1]))
            return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: the column map leaves the focus plane or decreases");
    for (int i = 0; i < Ho; ++i)
        if (ymap[i] < 0 || ymap[i] >= Hf || (i && ymap[i] < ymap[i - 1]))
            return fail(c, BQ_ERR_ARG, "bq_tissue_cells_union: the row map leaves the focus plane or decreases");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "tissue_cells_union", 0.0, 2.0 * (double)Ho * Wo);
    int32_t* d_xmap = d_tables;
    int32_t* d_ymap = d_xmap + Wo;
    int32_t* d_col = d_ymap + Ho;
    int32_t* d_row = d_col + 2 * gw;
    HIPCHK(c, hipMemcpyAsync(d_xmap, xmap, (size_t)Wo * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ymap, ymap, (size_t)Ho * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_col, col_ranges, (size_t)gw * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_row, row_ranges, (size_t)gh * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_tissue_cells_union(d_otsu_plane, Ho, Wo, T, d_focus_plane, Hf, Wf, d_xmap, d_ymap, d_col, d_row, gw, gh, d_count, s))
        return fail(c, BQ_ERR_HIP, "tissue cells union launch failed");
    return BQ_OK;
}

int bq_roi_plane(bq_ctx* c, const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys, int H,
                 int32_t* d_tables, uint8_t* d_plane, bq_stream_t stream) {
    if (!c || !d_tables || !d_plane || ((uintptr_t)d_tables & 15)) return fail(c, BQ_ERR_ARG, "bq_roi_plane: bad argument");
    if (const char* why = bqroi::check_tables(edges, E, starts, P, xs, W, ys, H)) return fail(c, BQ_ERR_ARG, std::string("bq_roi_plane: ") + why);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "roi_plane", 0.0, (double)H * W);
    int32_t* d_edges = d_tables;                                             // (first: the kernel loads an edge as 16 bytes)
    int32_t* d_starts = d_edges + (size_t)4 * E;
    int32_t* d_xs = d_starts + P + 1;
    int32_t* d_ys = d_xs + W;
    HIPCHK(c, hipMemcpyAsync(d_edges, edges, (size_t)4 * E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_starts, starts, ((size_t)P + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_xs, xs, (size_t)W * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ys, ys, (size_t)H * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (launch_roi_plane(d_edges, E, d_starts, P, d_xs, d_ys, H, W, d_plane, s)) return fail(c, BQ_ERR_HIP, "roi plane launch failed");
    return BQ_OK;
}

int bq_png_unfilter_strided(bq_ctx* c, const uint8_t* d_rows, size_t rows_stride, int n, int px, uint8_t* d_out, bq_stream_t stream) {
    if (!c || !d_rows || !d_out || n < 0 || px <= 0) return fail(c, BQ_ERR_ARG, "bq_png_unfilter_strided: bad argument");
    if (launch_png_unfilter(d_rows, n, px, d_out, (hipStream_t)stream, rows_stride)) return fail(c, BQ_ERR_HIP, "png unfilter launch failed");
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

int bq_stage_f32(bq_ctx* c, const float* d_tiles, int n, void* d_out, bq_stream_t stream) {
    if (!c || !d_tiles || !d_out || n < 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_stage_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "stage_f32_to_planar", 0.0, (double)n * kStaged * (4.0 + esize(c)));
    if (launch_stage_f32(d_tiles, n, 299, d_out, c->cfg.dtype, s)) return fail(c, BQ_ERR_HIP, "stage launch failed");
    return BQ_OK;
}

int bq_backbone(bq_ctx* c, const void* d_in, int n, float* d_feat, void* d_ws, size_t ws_bytes,
                bq_stream_t stream) {
    if (!c || !d_in || !d_feat || !d_ws || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_backbone: bad argument");
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    if (ws_bytes < ws_layout(c, n, 1).total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
    return backbone_impl({c, n, (hipStream_t)stream, nullptr, nullptr}, d_in, d_feat, (unsigned char*)d_ws);
}

int bq_mc_head(bq_ctx* c, const float* d_feat, int n, int64_t tile_idx0, int mc_n, int pass0, uint64_t seed,
               int init, int finalize, float* d_state, float* d_mean2, float* d_std2, void* d_ws,
               size_t ws_bytes, bq_stream_t stream) {
    if (!c || !d_feat || !d_state || !d_ws || n <= 0 || mc_n <= 0 || n > c->cfg.max_batch ||
        mc_n > c->cfg.max_mc || pass0 < 0 || (finalize && (!d_mean2 || !d_std2)))
        return fail(c, BQ_ERR_ARG, "bq_mc_head: bad argument");
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    if (ws_bytes < ws_layout(c, n, mc_n).total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
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
// block1_conv1 + block1_conv2 are ONE kernel straight from the bytes (kernels_front.hip), otherwise bq_stage + the backbone on
// the planar tensor.  bq_mc_infer and bq_backbone_u8 share it, so a tile's features do not depend on which of the two a
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
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    const WsLayout L = ws_layout(c, n, mc_n);
    if (ws_bytes < L.total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
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
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    const WsLayout L = ws_layout(c, n, 1);
    if (ws_bytes < L.total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
    return features_from_u8(c, d_tiles, n, d_feat, (unsigned char*)d_ws, L, stream);
}

int bq_slide_reduce(bq_ctx* c, const float* d_mean2, const float* d_std2, const int32_t* d_slide_idx, int n,
                    int n_slides, float tile_uq, int64_t* d_acc_pred, int64_t* d_acc_unc, int32_t* d_count,
                    bq_stream_t stream) {
    if (!c || !d_mean2 || !d_std2 || !d_slide_idx || !d_acc_pred || !d_acc_unc || !d_count || n < 0 || n_slides <= 0)
        return fail(c, BQ_ERR_ARG, "bq_slide_reduce: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "slide_reduce", 2.0 * n, 20.0 * n);
    if (launch_slide_reduce(d_mean2, d_std2, d_slide_idx, n, n_slides, tile_uq, (long long*)d_acc_pred,
                            (long long*)d_acc_unc, d_count, s))
        return fail(c, BQ_ERR_HIP, "slide_reduce launch failed");
    return BQ_OK;
}

int bq_slide_finish(bq_ctx* c, const int64_t* d_acc_pred, const int64_t* d_acc_unc, const int32_t* d_count,
                    int n_slides, double* d_mean_pred, double* d_mean_unc, bq_stream_t stream) {
    if (!c || !d_acc_pred || !d_acc_unc || !d_count || !d_mean_pred || !d_mean_unc || n_slides <= 0)
        return fail(c, BQ_ERR_ARG, "bq_slide_finish: bad argument");
    if (launch_slide_finish((const long long*)d_acc_pred, (const long long*)d_acc_unc, d_count, n_slides,
                            d_mean_pred, d_mean_unc, (hipStream_t)stream))
        return fail(c, BQ_ERR_HIP, "slide_finish launch failed");
    return BQ_OK;
}

size_t bq_roc_workspace_bytes(int64_t n) { return roc_workspace_bytes((long long)n); }

int bq_roc_youden(bq_ctx* c, const double* d_score, const uint8_t* d_label, int64_t n, void* d_ws, size_t ws_bytes,
                  double* d_out6, bq_stream_t stream) {
    if (!c || !d_score || !d_label || !d_ws || !d_out6 || n <= 0 || n > 0x7fffffffLL)
        return fail(c, BQ_ERR_ARG, "bq_roc_youden: bad argument");
    if (ws_bytes < roc_workspace_bytes(n)) return fail(c, BQ_ERR_ARG, "bq_roc_youden: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(c, s, "roc_youden", 4.0 * n, 60.0 * n);
    const int e = launch_roc_youden(d_score, d_label, (long long)n, (unsigned char*)d_ws, ws_bytes, d_out6, s);
    if (e) return fail(c, BQ_ERR_HIP, std::string("roc_youden: ") + hipGetErrorString((hipError_t)e));
    return BQ_OK;
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
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    const WsLayout L = ws_layout(c, n, 1);
    if (ws_bytes < L.total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
    Tap t; t.want = name; t.out = d_out; t.out_elems = out_elems;
    unsigned char* ws = (unsigned char*)d_ws;
    const int r = backbone_impl({c, n, (hipStream_t)stream, &t, nullptr}, d_in, (float*)(ws + L.feat), ws);
    if (r != BQ_OK) return r;
    return t.written;
}

int64_t bq_debug_activation_u8(bq_ctx* c, const char* name, const uint8_t* d_tiles, int n, void* d_ws, size_t ws_bytes,
                               float* d_out, size_t out_elems, bq_stream_t stream) {
    if (!c || !name || !d_tiles || !d_ws || !d_out || n <= 0 || n > c->cfg.max_batch) return fail(c, BQ_ERR_ARG, "bq_debug_activation_u8: bad argument");
    if (!c->loaded) return fail(c, BQ_ERR_WEIGHTS, "weights not loaded");
    const WsLayout L = ws_layout(c, n, 1);
    if (ws_bytes < L.total) return fail(c, BQ_ERR_WORKSPACE, "workspace too small");
    Tap t; t.want = name; t.out = d_out; t.out_elems = out_elems;
    unsigned char* ws = (unsigned char*)d_ws;
    const int r = backbone_impl({c, n, (hipStream_t)stream, &t, nullptr}, nullptr, (float*)(ws + L.feat), ws, d_tiles);
    if (r != BQ_OK) return r;
    return t.written;
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
