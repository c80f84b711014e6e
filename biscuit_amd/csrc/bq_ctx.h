// The context behind the C ABI (include/biscuit_hip.h), for the files that define bq_* entry points: biscuit_hip.hip (the context,
// the weight blob, whatever walks the network) and each tool's kernels_*.hip, where a tool's entry point stands beside its kernel.
// Internal: not installed.  What has state has one definition, in biscuit_hip.hip: fail (and the create error behind
// fail(nullptr, ...)) and prof_class.
#pragma once
#include "../../include/biscuit_hip.h"
#include "bq_common.h"
#include "bq_rounds.h"

#include <map>
#include <string>
#include <vector>

struct Blob { const unsigned char* p = nullptr; size_t n = 0; };

constexpr int kNumLayers = 39;   // rows of kLayers (biscuit_hip.hip): block1_conv2, 34 separable convolutions, 4 shortcuts

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
    float* d_srgb_lut = nullptr;   // tables of the Reinhard normaliser (kernels_reinhard.hip: reinhard_tables)
    const long long* d_tile0 = nullptr;   // bq_set_tile_index_ptr
    const long long* d_tile_idx = nullptr;   // bq_set_tile_index_array
    int inflate_variant = 5;       // bq_set_option("inflate_variant"): 5 = rounds of a literal-only fast phase + a general phase (LDS), 0 = the
                                   // kernel without LDS, tables in global memory (kernels_inflate.hip; profiles/r05_inflate.txt)
    float trunk_mul = 1.f;         // "act/trunk_mul" of the blob: 2^k of block13_out's activation exponent (bq_trunk_u8)
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

// What these files share stays inside the library: not in its dynamic symbol table, so nothing outside can interpose on it.
#define BQ_INTERNAL __attribute__((visibility("hidden")))

// records the text bq_last_error(c) returns (c null: the create error) and hands the code back
BQ_INTERNAL int fail(bq_ctx* c, int code, const std::string& msg);

#define HIPCHK(c, expr)                                                                 \
    do {                                                                                \
        hipError_t _e = (hipError_t)(expr);                                             \
        if (_e != hipSuccess)                                                           \
            return fail((c), BQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define RUN(expr) do { int _r = (expr); if (_r != BQ_OK) return _r; } while (0)

struct DeviceGuard {
    int prev = -1; bool ok = false;
    explicit DeviceGuard(int dev) { ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline bool is16(int dtype) { return dtype == BQ_DTYPE_BF16 || dtype == BQ_DTYPE_F16; }
inline size_t esize(const bq_ctx* c) { return is16(c->cfg.dtype) ? 2 : 4; }

constexpr long long kStaged = 3LL * 299 * 299;   // bytes of a 299-px tile

// ---- profiling -----------------------------------------------------------------
// A class sums the algorithmic FLOPs and bytes of its launches: the instances of one class differ (8 of the 25
// 728 -> 728 layers read a residual, 406 against 270 MB), and bq_profile_read reports the launch-weighted average.
BQ_INTERNAL int prof_class(bq_ctx* c, const std::string& name, double flops, double bytes);

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

// ---- what the tile codecs share: rounds (bq_rounds.h: round_items, round_cap) and the encoders' arguments --------
// The pointers of bq_jpeg_encode / bq_png_encode (`entry`), which share their output contract: tiles in, files packed into
// d_out[cap] at d_off[n + 1].  -> the refusal's text, or empty.
inline std::string bad_encode_args(const char* entry, const void* d_tiles, const void* d_out, int64_t cap, const void* d_off,
                                   const void* d_status, const void* d_scratch) {
    if (d_tiles && d_off && d_status && d_scratch && (d_out || !cap) && !((uintptr_t)d_off & 7) && !((uintptr_t)d_status & 3) &&
        !((uintptr_t)d_scratch & 15))
        return "";
    return std::string(entry) + ": bad argument (null pointer, d_off not 8-byte or d_scratch not 16-byte aligned)";
}

// ---- what two files share -------------------------------------------------------
// kernels_reinhard.hip: the normaliser's sRGB tables on the current device, once per context (bq_create); false: no memory
BQ_INTERNAL bool reinhard_tables(float** d_lut);
// kernels_tissue.hip (bq_tissue_cells; bq_tissue_cells_union of kernels_focus.hip): the cells' ranges of a W x H plane, [a, b)
// pairs: 0 <= a < b <= W for a column, <= H for a row.  -> the refusal's text, or empty.
BQ_INTERNAL std::string bad_cell_range(const char* plane, const int32_t* col_ranges, int gw, int W, const int32_t* row_ranges, int gh, int H);
