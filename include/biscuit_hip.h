/* biscuit_hip.h -- C ABI of libbiscuit_hip.so: the MI355X (gfx950) implementation of
 * BISCUIT's tile-level MC-dropout inference hot path.
 *
 * The reference (jamesdolezal/biscuit) has no FFI/plugin interface: the path is entered
 * through Python calls into Slideflow/TensorFlow and leaves through a tile-prediction
 * table.  Each entry point below names the reference call site it replaces:
 *
 *   bq_stain_reinhard_fast  interface.wsi_normalizer.rgb_to_rgb(image)   results.py:251-252, hp.py:19
 *   bq_stain_macenko        the same, for a model trained with normalizer='macenko'
 *   bq_stain_reinhard       the same, for normalizer='reinhard', 'reinhard_mask' or 'reinhard_fast_mask'
 *   bq_stage        tf.image.per_image_standardization(norm_image)      results.py:256
 *   bq_range_screen no reference counterpart: picks the tiles for the f16 range taps
 *   bq_backbone     keras Xception(include_top=False, pooling='avg')     biscuit/hp.py:4,20,22
 *   bq_mc_head      the UQ loop behind UncertaintyInterface(model)(batch) -> (mean, std)
 *                                                                        results.py:234,257-258
 *                   (dropout 0.1 hard-wired on, 2x Dense(1024)           biscuit/hp.py:11,13,21;
 *                    hp.uq = True                                        biscuit/experiment.py:849)
 *   bq_mc_infer     Project.evaluate(model, outcome, ..., save_predictions=True) inner loop
 *                                                                        biscuit/experiment.py:917-922
 *   bq_slide_reduce groupby(level).mean() of y_pred / uncertainty after the
 *                   `uncertainty < tile_uq` filter                       biscuit/threshold.py:191-204,297-298
 *
 * Conventions: every device buffer and the stream belong to the caller; the library
 * allocates only the weights (bq_load_weights) and small per-context scratch at
 * bq_create.  All work is enqueued on the caller's stream with no hidden
 * synchronisation (except bq_profile_read).  Return 0 on success, <0 on error; the
 * message is available from bq_last_error.  One context per device per process; a
 * context is not re-entrant.  No C++ exception crosses this boundary.
 *
 * Where the definitions are: the context, the weights, the network calls and the profile in csrc/biscuit_hip.hip; every other
 * entry point in the csrc/kernels_*.hip of the kernel it launches (csrc/bq_ctx.h is the context they share).
 */
#ifndef BISCUIT_HIP_H
#define BISCUIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bq_ctx bq_ctx;
typedef void* bq_stream_t; /* hipStream_t */

/* Storage / matrix-core type of the backbone activations and weights (accumulation, folded BN, the MC head and
 * every statistic are fp32 in all three).  F16 = IEEE half: the matrix-core rate of BF16 with 8x finer rounding;
 * values beyond +-65504 saturate (MODE.FP16_OVFL) instead of overflowing to inf. */
enum { BQ_DTYPE_F32 = 0, BQ_DTYPE_BF16 = 1, BQ_DTYPE_F16 = 2 };
enum { BQ_MC_HEAD = 0, BQ_MC_FULL = 1 };

enum {
    BQ_OK = 0,
    BQ_ERR_ARG = -1,      /* bad argument / shape */
    BQ_ERR_HIP = -2,      /* a HIP runtime call failed */
    BQ_ERR_WEIGHTS = -3,  /* weight blob malformed or not loaded */
    BQ_ERR_WORKSPACE = -4 /* workspace too small */
};

typedef struct bq_config {
    int32_t dtype;        /* BQ_DTYPE_*: storage/matrix-core type of the backbone activations */
    int32_t tile_px;      /* 299 (biscuit/hp.py:5) */
    int32_t n_classes;    /* 2 (LUAD vs LUSC) */
    float dropout;        /* 0.1 (biscuit/hp.py:11); the default rate, taken as the double of this float: a caller
                             with a double rate (0.3 is 0.30000001 as a float) passes it to bq_set_dropout */
    int32_t max_batch;    /* largest n any call will pass (sizes the workspace) */
    int32_t max_mc;       /* largest mc_n any call will pass */
} bq_config;

/* Lifetime. */
bq_ctx* bq_create(int device_id, const bq_config* cfg);
void bq_destroy(bq_ctx* ctx);

/* The dropout rate of the head, as a double (0 <= rate < 1, else BQ_ERR_ARG and the rate stays): the keep threshold
 * floor(rate * 2^32) and the scale fp32(1 / (1 - rate)) of the mask contract (oracle/philox.py) are computed from it.  Applies
 * to the launches enqueued after the call; bq_create sets it from cfg->dropout. */
int bq_set_dropout(bq_ctx* ctx, double rate);
const char* bq_last_error(bq_ctx* ctx); /* ctx may be NULL: last creation error */

/* Bytes of device workspace bq_backbone/bq_mc_head/bq_mc_infer need for `batch` tiles
 * and `mc_n` passes. */
size_t bq_workspace_bytes(bq_ctx* ctx, int batch, int mc_n);

/* Upload a "BQW1" weight blob (biscuit_amd/weights.py:pack_blob; folded-BN scale/bias,
 * matrix-core weights pre-swizzled into MFMA fragment order).  The blob's dtype must
 * match cfg.dtype. */
int bq_load_weights(bq_ctx* ctx, const void* host_blob, size_t nbytes);

/* K0: uint8 NHWC tiles [n,px,px,3] -> per-image standardised planar NCHW [n,3,px,px]
 * of the context dtype.  (x - mean) / max(std, 1/sqrt(N)). */
int bq_stage(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, void* d_out_nchw,
             bq_stream_t stream);

/* A HIP stream restricted to the compute units whose bits are set in cu_mask (mask_words 32-bit
 * words, bit i = CU i): lets two batches in flight own disjoint halves of the chip instead of
 * interleaving workgroups on every CU.  No reference counterpart (scheduling only). */
int bq_stream_create_masked(bq_ctx* ctx, const uint32_t* cu_mask, int mask_words, bq_stream_t* out_stream);
int bq_stream_destroy(bq_ctx* ctx, bq_stream_t stream);
/* Number of compute units the persistent kernels of this context size their grids for (default: all of the device's; 0 restores
 * that).  A context whose launches go to a CU-masked stream sets it to the CUs of the mask: a grid sized for the whole chip runs
 * there as two rounds of workgroups, each with its own prologue.  Results do not depend on it. */
int bq_set_num_cus(bq_ctx* ctx, int n);
/* Tuning knobs that change no result.  "inflate_variant": 5 (default) = bq_png_inflate decodes in rounds of a literal-only fast
 * phase (a 7-bit table and a 32-byte output ring per lane in LDS, 8 waves per CU) and a general phase only stalled lanes enter:
 * 27.6 k incompressible / 38.8 k photograph-like tiles a second on 16 CUs; 0 = the kernel without LDS, decode tables in the scratch
 * buffer (global memory / L2): the fallback, 2-3 x slower (profiles/r05_inflate.txt).  Anything else: BQ_ERR_ARG. */
int bq_set_option(bq_ctx* ctx, const char* name, int value);

/* K0, optional front half (kernels_reinhard.hip): the `reinhard_fast` stain normaliser hp.py:19 selects, applied to the
 * uint8 tile before the standardisation exactly where results.py:251-252 calls
 * interface.wsi_normalizer.rgb_to_rgb(image).  uint8 NHWC [n,px,px,3] -> uint8 NHWC; d_out may equal
 * d_tiles.  target_means3 / target_stds3 are HOST pointers to the model's params.json `norm_fit`
 * (CIE-LAB L, a, b); a NaN or an infinity among them is BQ_ERR_ARG, a std of 0 or below is legal.  The algorithm lives in Slideflow, not in the reference: parity unpinned
 * (oracle/stain.py states the arithmetic both sides implement). */
int bq_stain_reinhard_fast(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, const float* target_means3,
                           const float* target_stds3, uint8_t* d_out_nhwc, bq_stream_t stream);

/* Per-tile CIE-LAB channel statistics [n][6] = mean L, a, b, population std L, a, b: what the
 * normaliser's fit() stores as norm_fit for a target image. */
int bq_stain_lab_stats(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, float* d_stats6, bq_stream_t stream);

/* K0, optional front half (kernels_reinhard.hip): Slideflow's Reinhard family ("Reinhard family").  flags:
 * 1 = brightness standardisation in front (the 90th percentile of the tile's L becomes L = 100), 2 = statistics and transform over
 * the tissue pixels only (L < mask_L, strict); 0 `reinhard_fast`, 1 `reinhard`, 2 `reinhard_fast_mask`, 3 `reinhard_mask`.  uint8
 * NHWC [n,px,px,3] -> uint8 NHWC, 1 <= px <= 1024; d_out may equal d_tiles.  target_means3 / target_stds3: as above (HOST pointers,
 * finite).  mask_L: finite, whatever the flags.  d_status (nullable): int [n], 0 = normalised, 1 = no tissue pixel (the output is
 * the brightness stage's), 2 = the percentile is not finite or <= 0 (the tile passes through unchanged).  Flags 0 gives
 * bq_stain_reinhard_fast's bytes.  Allocates nothing, does not synchronise.  Unpinned, like reinhard_fast. */
int bq_stain_reinhard(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, int px, int flags, float mask_L,
                      const float* target_means3, const float* target_stds3, uint8_t* d_out_nhwc, int* d_status,
                      bq_stream_t stream);

/* What the family's fit() stores, per tile: d_stats8 float [n][8] = mean L, a, b, population std L, a, b over the tissue pixels of
 * the brightness-standardised tile (NaN when the status is not 0), the percentile p (100 without flag 1), tissue pixels / pixels
 * (0 when the status is not 0).  d_status (nullable): as above. */
int bq_stain_reinhard_stats(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, int px, int flags, float mask_L, float* d_stats8,
                            int* d_status, bq_stream_t stream);

/* K0, optional front half: the `macenko` stain normaliser (Slideflow's normalizer='macenko'; DESIGN.md "Macenko" states the
 * spec, the precision contract and the degenerate-tile rule).  uint8 NHWC [n,px,px,3] -> uint8 NHWC; d_out may equal d_tiles.
 * he_ref6 (row-major 3x2, columns H and E) and maxc_ref2 are HOST pointers to the model's fit (norm_fit
 * stain_matrix_target / target_concentrations; finite, concentrations > 0).  d_status (nullable): int [n], 0 = normalised,
 * 1 = fewer than 2 tissue pixels, 2 = |det(HE^T HE)| < 1e-12, 3 = a maxC <= 0 or a non-finite intermediate; a tile whose
 * status is not 0 passes through unchanged.  Unpinned, like reinhard_fast. */
int bq_stain_macenko(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, const float* he_ref6, const float* maxc_ref2,
                     uint8_t* d_out_nhwc, int* d_status, bq_stream_t stream);

/* The Macenko fit of each tile: d_stats8 float [n][8] = HE row-major 3x2, maxC 2 (NaN where a degenerate tile stopped before
 * computing them); d_status2 (nullable) int [n][2] = status (as above), number of tissue pixels. */
int bq_stain_macenko_stats(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, float* d_stats8, int* d_status2,
                           bq_stream_t stream);

/* The f16 range screen: f16 storage clamps at +-65504 without a signal, and an input-driven extreme is what
 * the stem amplifies, so the tiles whose standardised input reaches furthest are the ones to run through the range taps.
 *
 * A tile's key is the largest |value| tf.image.per_image_standardization gives it (what bq_stage feeds the network):
 *     key = max(hi - mu, mu - lo) / max(sd, 1/sqrt(N))     N = 299 * 299 * 3
 * hi, lo: its largest and smallest byte; mu = S1/N, var = max(S2/N - mu^2, 0), sd = sqrt(var) from the exact integer sums S1, S2
 * of its bytes, in float64 without FP contraction, rounded once to float32 (a float64 numpy restatement gives the same bits).
 *
 * Both calls take caller-owned device scratch d_ws of bq_range_ws_bytes(n) bytes, used only by the launches of that call (it may be
 * reused by the next call on the same stream), enqueue everything on `stream` without a host synchronisation, and return 0 for n = 0
 * without a launch (the device pointers may then be NULL).  Errors as everywhere: BQ_ERR_ARG for a bad argument (nothing enqueued), BQ_ERR_HIP for a failed launch. */
size_t bq_range_ws_bytes(int n);

/* Keys only (tests, diagnostics): uint8 NHWC tiles [n,299,299,3] (any byte alignment) -> d_key float [n]. */
int bq_range_key(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, float* d_key, void* d_ws, size_t ws_bytes, bq_stream_t stream);

/* Keys of a batch merged into k candidate slots (1 <= k <= 64), all caller-owned device memory: d_cand_key float [k], d_cand_idx
 * int64 [k] (global tile index), d_cand_tiles uint8 [k][299][299][3].  The first `filled` slots (0 <= filled <= k) hold candidates
 * from earlier calls; the rest are empty and are not read.  The batch's global tile indices follow bq_mc_infer: d_tile_idx[i]
 * (int64 [n], device) when it is not NULL, else tile_idx0 + i.  Afterwards the first min(k, filled + n) slots hold the top of
 * (candidates + batch) by key descending, global index ascending (equal key and index: the older entry first), a total order:
 * candidates that stay keep their slot, newly admitted tiles take the freed slots in rank order, lowest slot first, and their bytes
 * are copied there.  So the caller knows the number of filled slots without reading the device: min(k, tiles since it started
 * from filled = 0).  Stream order is the only synchronisation: work on `stream` enqueued before the call may read the slots, work
 * after it sees the update.  n <= 2048. */
int bq_range_screen(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, int64_t tile_idx0, const int64_t* d_tile_idx,
                    float* d_cand_key, int64_t* d_cand_idx, uint8_t* d_cand_tiles, int k, int filled, void* d_ws,
                    size_t ws_bytes, bq_stream_t stream);

/* Input side, PNG tiles: the reversal of the PNG scanline filters on the device.  d_rows:
 * [n][px][1 + 3*px] bytes -- per row the filter-type byte and the filtered RGB bytes, i.e. the inflated IDAT stream of an
 * 8-bit RGB non-interlaced PNG, as libbiscuit_io's bqio_decode_rows delivers it (include/biscuit_io.h).  d_out: uint8 NHWC
 * [n][px][px][3], the tiles bq_stage / bq_mc_infer take.  Bit-exact with a host PNG decoder (tests/test_png_unfilter.py). */
int bq_png_unfilter(bq_ctx* ctx, const uint8_t* d_rows, int n, int px, uint8_t* d_out_nhwc, bq_stream_t stream);

/* Input side, PNG tiles, the inflate itself on the device (round 5): n zlib streams -- the concatenated IDAT payloads of n 8-bit RGB
 * non-interlaced PNG tiles, as libbiscuit_io's bqio_extract_z packs them: stream i = d_z[d_off[i] .. d_off[i] + d_len[i]), every
 * d_off[i] a multiple of 16, 32 readable bytes behind every stream -- are inflated to their px rows of 1 + 3 px bytes at d_rows +
 * i * rows_stride (rows_stride a multiple of 4, >= px (1 + 3 px) + 4), one stream per lane.  d_status[i] = 0 iff stream i is a
 * well-formed zlib stream that inflates to exactly px (1 + 3 px) bytes with a matching Adler-32 (what zlib's uncompress() accepts)
 * and every row's filter-type byte is 0..4 (what a PNG decoder accepts);
 * any other value: the tile's rows are undefined and the caller decodes that record on the host.  The bytes of a stride behind
 * its px (1 + 3 px) row bytes are unspecified (the literal collector stores whole dwords; bq_png_unfilter_strided does not read
 * them): the one output region of this header that is.  d_scratch: table space,
 * bq_png_inflate_scratch_bytes(n), contents unspecified on entry like every scratch buffer and workspace here.  Follow with bq_png_unfilter_strided.  No reference counterpart (tf.io.decode_png under tf.data). */
size_t bq_png_inflate_scratch_bytes(int n);
int bq_png_inflate(bq_ctx* ctx, const uint8_t* d_z, const uint32_t* d_off, const uint32_t* d_len, int n, int px, uint8_t* d_rows,
                   size_t rows_stride, void* d_scratch, size_t scratch_bytes, int32_t* d_status, bq_stream_t stream);
int bq_png_unfilter_strided(bq_ctx* ctx, const uint8_t* d_rows, size_t rows_stride, int n, int px, uint8_t* d_out_nhwc,
                            bq_stream_t stream);

/* Input side, JPEG tiles, decoded on the device: n baseline-JPEG tiles (8-bit, Huffman, one interleaved scan of three components
 * at 4:4:4 / 4:2:2 / 4:2:0, no restart intervals) as libbiscuit_io's bqio_extract_jpeg packs them -- d_scan: the entropy-coded
 * segments, stuffed zeros removed, each at a multiple of 16 with bqio_jpeg_ecs_pad() zero bytes behind it; d_desc: n x 4 uint32
 * (offset, length, sampling, table set); d_tables: n_tables table sets of bqio_jpeg_table_bytes() each, 4-byte aligned -- become
 * uint8 NHWC tiles d_out_nhwc[n][px][px][3]: THE BYTES libjpeg's defaults give (islow IDCT, fancy upsampling, 16-bit BT.601), i.e.
 * those of the host decoder and of Pillow.  An entropy kernel (one tile per lane, tables in LDS) leaves dequantised int16
 * coefficients in d_scratch, a pixel stage (IDCT per block, then upsampling and colour per pixel) writes the tiles; tiles whose
 * table sets, samplings and lengths differ may stand side by side.  d_status[i] = 0 iff tile i decoded; otherwise bits -- 1 a code
 * that does not exist, 2 a zero run past coefficient 63, 4 data used from beyond the segment's end, 8 outside the range in which
 * libjpeg's builds agree (a product or intermediate beyond 15 bits, a sample beyond -512..511), 16 a descriptor outside the subset
 * -- and the tile's bytes are no image: the caller decodes that record on the host.  Scratch: 128 bytes per 8 x 8 block of a 4:4:4
 * tile rounded up to whole 16 x 16 units -- 554 496 bytes per 299-px tile --; bq_jpeg_scratch_bytes(n, px) asks for min(n, 2048)
 * tiles' worth (1.14 GB at 299 px) and the call works in rounds of as many tiles as d_scratch holds (more scratch: fewer, fuller
 * rounds).  The scratch is zeroed as part of the call.  No reference counterpart (tf.io.decode_jpeg under tf.data). */
size_t bq_jpeg_scratch_bytes(int n, int px);
int bq_jpeg_decode(bq_ctx* ctx, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int px,
                   uint8_t* d_out_nhwc, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* The same decoder for a TIFF page's own JPEG tiles, written straight into a slide canvas (DESIGN.md "Heatmap input", "Decode"):
 * n segments of seg_w x seg_h (each <= 4096) as libbiscuit_io's bqio_extract_jpeg_segments packs them -- d_scan, d_desc, d_tables as
 * above -- are decoded by the same entropy and IDCT kernels, and a colour-and-place kernel writes them into d_canvas uint8
 * [H][W][3] (H, W <= 2^28; row pitch 3 W, any alignment).  d_place int32 [n][2] = the canvas position (x, y) of each segment's
 * top-left pixel; it may be negative or reach past the canvas.  (clip_x0, clip_y0, clip_x1, clip_y1) is a rectangle in canvas
 * coordinates, the level's image extent: exactly the pixels of a segment inside both the canvas and the rectangle are written --
 * aligned dword stores where four pixels of a row fall into one 12-byte group, byte stores at a row's ends -- and NOTHING else:
 * the caller fills the canvas with 255 beforehand, so that what a border tile holds beyond the image stays white.  Segments do
 * not overlap in a canvas (a page's tiles never do); none is checked.  d_status as bq_jpeg_decode; a segment whose descriptor is
 * refused (16) writes nothing.  The result is bqio_jpeg_decode_canvas's byte for byte.  Scratch: 128 bytes per 8 x 8 block of a
 * 4:4:4 segment rounded up to whole 16 x 16 units (393 216 bytes at 256 x 256); bq_jpeg_canvas_scratch_bytes(n, seg_w, seg_h)
 * asks for min(n, 2048) segments' worth, and the call works in rounds of as many segments as d_scratch holds -- one at least,
 * BQ_ERR_WORKSPACE below that.  Everything is enqueued on `stream` without a host synchronisation; n = 0 returns 0 without a
 * launch. */
size_t bq_jpeg_canvas_scratch_bytes(int n, int seg_w, int seg_h);
int bq_jpeg_decode_canvas(bq_ctx* ctx, const uint8_t* d_scan, const void* d_desc, const void* d_tables, int n_tables, int n, int seg_w,
                          int seg_h, const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0, int clip_x1,
                          int clip_y1, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* A TIFF page's JPEG 2000 tiles (compression 33003 / 33005 / 34712) decoded on the device into a slide canvas (kernels_j2k.hip;
 * DESIGN.md "Heatmap input", JPEG 2000 tiles): the counterpart of bq_jpeg_decode_canvas.  n segments of seg_w x seg_h (each <= 512)
 * as libbiscuit_io's bqio_j2k_extract packs them -- d_seg (n descriptors of 128 bytes), d_blocks (n_blocks code-block rows of 48
 * bytes), d_bytes (n_bytes of codewords), all device memory, 4-byte aligned -- go through tier 1 (a lane per code block),
 * dequantisation and the inverse 5/3 or 9/7 transform (a workgroup per segment and component) and a store kernel (inverse RCT /
 * ICT, rounding, level shift, clamp; ycc != 0: the full-range YCbCr -> RGB of csrc/j2k_ycc.h) that writes d_canvas uint8
 * [H][W][3] exactly as bq_jpeg_decode_canvas does: at d_place[i] = (x, y), inside the canvas and the clip rectangle only.
 * d_status int32 [n]: 0, the extractor's status (32: outside the subset, 64: damaged) or 16 for a descriptor or block row
 * that fails the decoder's own bounds checks; a segment whose status is not 0 writes nothing.  The result is
 * bqio_j2k_decode_canvas's byte for byte and status for status.  Scratch: 24 bytes per pixel of a segment (1 572 864 at
 * 256 x 256); bq_j2k_canvas_scratch_bytes(n, seg_w, seg_h) asks for min(n, 256) segments' worth, and the call works in rounds
 * of as many segments as d_scratch holds -- one at least, BQ_ERR_WORKSPACE below that -- without a host synchronisation;
 * n = 0 returns 0 without a launch. */
size_t bq_j2k_canvas_scratch_bytes(int n, int seg_w, int seg_h);
int bq_j2k_decode_canvas(bq_ctx* ctx, const void* d_seg, int n, const void* d_blocks, int64_t n_blocks, const uint8_t* d_bytes,
                         size_t n_bytes, int seg_w, int seg_h, int ycc, const int32_t* d_place, uint8_t* d_canvas, int H, int W,
                         int clip_x0, int clip_y0, int clip_x1, int clip_y1, int32_t* d_status, void* d_scratch, size_t scratch_bytes,
                         bq_stream_t stream);

/* A TIFF page's LZW tiles (compression 5, predictor 1 or 2) decoded on the device into a slide canvas (kernels_lzw.hip; DESIGN.md
 * "Heatmap input", LZW tiles): the counterpart of bq_jpeg_decode_canvas.  Nothing is parsed on the host: d_data holds the n
 * segments of seg_w x seg_h (each <= 1024) as the file has them, segment i at d_desc[i] = (offset, length) -- two uint32, the
 * offset a multiple of 16, readable zero bytes behind every segment up to the next multiple of 16.  lzw_decode (a wave per
 * segment; the stream is the statement of csrc/lzw_device.h) leaves the unpredicted bytes in d_scratch; lzw_place (a wave per
 * segment row) undoes predictor 2 -- the running sum per sample modulo 256 -- and writes d_canvas uint8 [H][W][3] exactly as
 * bq_jpeg_decode_canvas does: at d_place[i] = (x, y), inside the canvas and the clip rectangle only, in its store shape.
 * d_status int32 [n]: 0 = decoded; otherwise bits -- 1 the first code is not ClearCode, 2 a code beyond the next free index,
 * 4 the data ends or EndOfInformation arrives before seg_w * seg_h * 3 bytes, 8 the table ran to its end without a ClearCode,
 * 16 a descriptor that fails the decoder's checks (offset not a multiple of 16, length above 2^28) -- and such a segment
 * writes nothing.  The result is bqio_lzw_decode_canvas's byte for byte and status for status.  Scratch: seg_w * seg_h * 3
 * bytes per segment rounded up to 16 (196 608 at 256 x 256); bq_lzw_canvas_scratch_bytes(n, seg_w, seg_h) asks for
 * min(n, 1024) segments' worth, and the call works in rounds of as many segments as d_scratch holds -- one at least,
 * BQ_ERR_WORKSPACE below that -- without a host synchronisation; no result depends on what the scratch held; n = 0 returns 0
 * without a launch. */
size_t bq_lzw_canvas_scratch_bytes(int n, int seg_w, int seg_h);
int bq_lzw_decode_canvas(bq_ctx* ctx, const uint8_t* d_data, const void* d_desc, int n, int seg_w, int seg_h, int predictor,
                         const int32_t* d_place, uint8_t* d_canvas, int H, int W, int clip_x0, int clip_y0, int clip_x1, int clip_y1,
                         int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* Output side, JPEG tiles, encoded on the device (kernels_jpeg_encode.hip; DESIGN.md "Tile extraction"): n tiles d_tiles uint8
 * [n][px][px][3] -- the batch bq_tile_resample fills -- become the COMPLETE baseline-JPEG files Pillow writes for `save(buf, 'JPEG',
 * quality=quality, subsampling=subsampling)` with everything else at its default (libjpeg's 16-bit BT.601, h2v2 box filter, islow
 * fDCT, rounded-division quantisers, the Annex K Huffman tables), byte for byte, back to back in d_out: file i = d_out[d_off[i] ..
 * d_off[i + 1]), d_off int64 [n + 1] (device memory, 8-byte aligned) with d_off[0] = 0.  subsampling: 0 = 4:4:4, 2 = 4:2:0 (Pillow's
 * numbering); quality 1..100; px 1..4096 -- anything else returns BQ_ERR_ARG with bq_last_error set and launches nothing.  Four
 * stages, each timed as its own class under bq_profile_*: pixel (one thread per 8 x 8 block: colour, edges, downsampling, fDCT,
 * quantisation; int16 zigzag coefficients to scratch), size (a block's code length from its coefficients and one neighbour's DC, then
 * an exclusive scan per tile), pack (every block writes its bits at its bit offset; words shared by two blocks are merged with
 * atomicOr, the last byte is padded with ones), stuff (0xFF bytes counted per chunk and scanned, the file lengths scanned into
 * d_off, then header + stuffed segment + EOI copied out).  d_status[i] = 0, or 1 when file i would end beyond `cap` (the bytes of
 * d_out): that file and the ones behind it are not written, d_off still holds every exact length, so the caller repeats the call
 * with a buffer that fits (cap = 0 with d_out = NULL sizes a call).  Scratch (16-byte aligned): 128 bytes of coefficients, 4 of
 * offsets, the worst-case 248 of code and 31 of chunk counts per block, 888 768 bytes per 299-px tile at 4:2:0; bq_jpeg_encode_scratch_bytes(n, px,
 * subsampling) asks for min(n, 256) tiles' worth and the call works in rounds of as many tiles as d_scratch holds -- one at least,
 * BQ_ERR_WORKSPACE below that.  The result is bqio_jpeg_encode's byte for byte and does not depend on the rounds.  Everything is
 * enqueued on `stream`; the library allocates nothing and does not wait for the device; n = 0 returns 0 without a launch.  The
 * reference's counterpart is Slideflow's extract_tiles writing image_raw. */
size_t bq_jpeg_encode_scratch_bytes(int n, int px, int subsampling);
int bq_jpeg_encode(bq_ctx* ctx, const uint8_t* d_tiles, int n, int px, int quality, int subsampling, uint8_t* d_out, int64_t cap,
                   int64_t* d_off, int32_t* d_status, void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* Output side, PNG tiles, encoded on the device (kernels_png_encode.hip; DESIGN.md "Tile extraction"): n tiles d_tiles uint8
 * [n][px][px][3] become COMPLETE PNG files -- signature, IHDR (8-bit, colour type 2, no interlace), IDAT chunks of 8 192 bytes
 * that together hold one zlib stream (32 KB window, Adler-32), IEND, a CRC-32 on every chunk, no ancillary chunk -- back to back in
 * d_out: file i = d_out[d_off[i] .. d_off[i + 1]), d_off int64 [n + 1] (device memory, 8-byte aligned) with d_off[0] = 0.  The
 * filtered scanlines are the ones Pillow writes, byte for byte (per row None, Up, Sub, Paeth in that order by the sum of |int8|,
 * strictly smaller wins); the deflate stream is this library's own: blocks of 16 384 filtered bytes that share nothing, greedy
 * matching against a 3-byte hash table in groups of 64 positions (a match is taken from 5 bytes on), per block the smallest of
 * dynamic, fixed and stored.  There is no quality: a tile has exactly one encoding, bqio_png_encode's byte for byte, whatever n,
 * the tile's place in the batch or the scratch size.  px 1..4096 -- anything else returns BQ_ERR_ARG with bq_last_error set and
 * launches nothing.  Four stages, each timed as its own class under bq_profile_*: filter (one wave per row: scores, choice,
 * filtered bytes, Adler sums), match (one wave per block: tokens and histogram), code (one wave per block: length-limited Huffman
 * lengths, header, the three sizes; one wave per tile: bit offsets), pack (every token's bits at its own offset through atomicOr,
 * the file lengths scanned into d_off, the zlib bytes copied between the chunk frames, one wave per chunk for its CRC).
 * d_status[i] = 0, or 1 when file i would end beyond `cap` (the bytes of d_out): that file and the ones behind it are not written,
 * d_off still holds every exact length, so the caller repeats the call with a buffer that fits (cap = 0 with d_out = NULL sizes a
 * call).  A file is at most L + L / 256 + 128 bytes, L = px (1 + 3 px).  Scratch (16-byte aligned): the filtered stream, 4 bytes of
 * token per input byte, codes, headers and the deflate buffer, 1 707 536 bytes per 299-px tile; bq_png_encode_scratch_bytes(n, px)
 * asks for min(n, 128) tiles' worth and the call works in rounds of as many tiles as d_scratch holds -- one at least,
 * BQ_ERR_WORKSPACE below that.  Everything is enqueued on `stream`; the library allocates nothing and does not wait for the
 * device; n = 0 returns 0 without a launch.  The reference's counterpart is extract_tiles(img_format='png'). */
size_t bq_png_encode_scratch_bytes(int n, int px);
int bq_png_encode(bq_ctx* ctx, const uint8_t* d_tiles, int n, int px, uint8_t* d_out, int64_t cap, int64_t* d_off, int32_t* d_status,
                  void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* Training augmentation on the device (kernels_augment.hip; DESIGN.md section 7 "Training augmentation"): Slideflow's 'xyrjb' with
 * the random draws made by the caller (biscuit_amd/augment.py: draw).  n tiles d_tiles uint8 [n][px][px][3], 8 <= px <= 4096, and
 * d_params uint8 [n][4] = (k, flips, quality, blur) per tile, both in device memory ->
 *     d_out[i] = blur_s( flip_ud^(flips >> 1 & 1)( flip_lr^(flips & 1)( rot90^k( jpeg_q(d_tiles[i]) ))))
 * as csrc/augment_device.h states each step: jpeg_q the pixels Pillow returns after a JPEG round trip at quality 1..100 and 4:2:0
 * (0: the tile itself), rot90^k numpy's counter-clockwise quarter turns (k 0..3), the flips x[:, ::-1] (bit 0) and x[::-1] (bit
 * 1), blur_s an integer separable Gaussian of sigma = 0.5 blur (blur 1..4; 0: the identity).  The result is bqio_augment's byte
 * for byte and status for status, whatever the rounds and whatever d_scratch and d_out held.  d_status[i] = 0, or 1 where a block
 * of the round trip left the range in which libjpeg's builds agree (samples clamped).  The parameter bytes are in device memory,
 * where this call cannot read them without waiting: a row out of range (k or flips > 3, quality > 100, blur > 4) gets status 2
 * and its tile comes out unchanged (callers with the table on the host check it there: Engine.augment).  Four stages, each
 * timed as its own class under bq_profile_*: augment_jpeg (quality > 0: one thread per 8 x 8 block, coefficients -> samples in
 * scratch), augment_place (four output pixels per thread: the inverse dihedral map over those samples or the input tile),
 * augment_blur_h and augment_blur_v (blur > 0: the row pass into a uint16 plane in scratch, the column pass back into d_out).
 * d_out must not overlap d_tiles.  Scratch (16-byte aligned): the decoder's planes, 128 bytes per block, and 6 bytes per pixel
 * rounded up to 16, 1 090 912 bytes per 299-px tile; bq_augment_scratch_bytes(n, px) asks for min(n, 256) tiles' worth and the
 * call works in rounds of as many tiles as d_scratch holds -- one at least, BQ_ERR_WORKSPACE below that.  px outside 8..4096
 * returns BQ_ERR_ARG with bq_last_error set and launches nothing.  Everything is enqueued on `stream`; the library allocates
 * nothing and does not wait for the device; n = 0 returns 0 without a launch.  No atomics and no inline assembly.  The
 * reference's counterpart is the augment='xyrjb' of biscuit/hp.py:23 inside Slideflow's tf.data pipeline. */
size_t bq_augment_scratch_bytes(int n, int px);
int bq_augment(bq_ctx* ctx, const uint8_t* d_tiles, int n, int px, const uint8_t* d_params, uint8_t* d_out, int32_t* d_status,
               void* d_scratch, size_t scratch_bytes, bq_stream_t stream);

/* The whole-slide heatmap's input stage (kernels_resample.hip; DESIGN.md "Heatmap input"): n tiles cut out of a slide canvas in
 * device memory and resampled to px x px -- what sf.Heatmap's slide reader does per tile on the host (results.py:217).  d_canvas
 * uint8 [H][W][3]; tile t is the src_px x src_px window at (d_origin[2 t], d_origin[2 t + 1]) = (x, y) (int32; windows may
 * overlap, and may leave the canvas: pixels outside read as 255); d_bounds int32 [px][2] and d_coef int32 [px][ksize] are
 * bqio_resample_taps(src_px, px)'s tables (include/biscuit_io.h), uploaded by the caller; d_out uint8 NHWC [n][px][px][3], the
 * batch bq_mc_infer takes.  The bytes are those of Pillow's Image.resize((px, px), Image.LANCZOS) of the window: horizontal pass
 * rounded to bytes (kept in LDS), then the vertical pass, integer arithmetic throughout.  src_px == px copies the window (the
 * tables may then be NULL).  Supported: 0 < px <= 4096, px / 8 <= src_px <= 8 px, and (ksize + 1) * 3 px <= 64 000 bytes of
 * LDS (px = 299: the whole ratio range); H, W <= 2^28; n <= 2^20 and n x (strips of output rows per tile: ceil(px / R), R <= 32 the
 * rows whose taps fit the LDS, 10 strips at px = 299) <= 2^31 - 1.  Origins are device memory and are not checked: a coordinate
 * beyond +-2^28 is used as +-2^28, where the window lies outside the canvas (white), as bqio_tile_resample refuses it on the host.
 * Everything is enqueued on `stream` without a host synchronisation; n = 0 returns 0
 * without a launch; a bad argument -- a ksize that is not the ratio's included -- is BQ_ERR_ARG with nothing enqueued. */
int bq_tile_resample(bq_ctx* ctx, const uint8_t* d_canvas, int H, int W, const int32_t* d_origin, int n, int src_px, int px,
                     const int32_t* d_bounds, const int32_t* d_coef, int ksize, uint8_t* d_out_nhwc, bq_stream_t stream);

/* The background filter's measure (Slideflow's grayspace filter at extraction, restated: DESIGN.md "Heatmap input"): d_count[t] =
 * the number of pixels of tile t whose HSV saturation is below the threshold.  With mx = max(r, g, b), mn = min(r, g, b) a pixel
 * counts iff mx - mn < d_limit256[mx]; the host builds the 256 int32 entries from the float64 definition (s = 0 if mx == 0 else
 * (mx - mn) / mx; grey iff s < threshold), so the device compares integers.  d_tiles uint8 NHWC [n][px][px][3], d_count int32 [n].
 * Enqueued on `stream`, no host synchronisation; n = 0 returns 0 without a launch. */
int bq_tile_grayspace(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, int px, const int32_t* d_limit256, int32_t* d_count,
                      bq_stream_t stream);

/* The whole-slide heatmap's output stage (kernels_render.hip; DESIGN.md "Heatmap output"): one plane of the grid drawn over the
 * slide's thumbnail through a colour table -- the picture sf.Heatmap(...).save(dir, cmap=...) writes on the host, for the full map
 * and again after the uncertain cells are set to -1 (results.py:217-227).  d_values float32 [gh][gw] (hm.logits[:, :, c] or
 * hm.uncertainty[:, :, c]); a cell whose value is -1 or not finite is transparent.  d_col / d_row are render.render_tables'
 * tables, one entry per output column / row, built on the host in float64 -- the kernel does no coordinate arithmetic:
 * interpolation 0 ('none'): int32 [W] / [H], the pixel's cell or -1; interpolation 1 ('bicubic'): int32 [W][9] / [H][9] = the
 * pixel's cell or -1, four tap cells clamped to the grid and four Catmull-Rom weights with 12 fractional bits that sum to 4096.
 * d_lut uint8 [256][3]; d_thumb, d_out uint8 [H][W][3] (row pitch 3 W, any alignment); d_out may be d_thumb (in place), otherwise
 * the two must not overlap.  Per cell q = clamp(floor(((v - vmin) * inv_span) * 65536), 0, 65535) with the float32 subtraction
 * and multiplication un-fused; 'none' takes lut[q >> 8] of the pixel's cell; 'bicubic' the weighted mean of q over the live taps
 * in 64-bit integers, rounded, clamped (the pixel's own q where the live weights do not sum above 0); a pixel whose own cell is
 * transparent, or that has none, keeps the thumbnail's bytes.  Blend per channel: (A colour + (256 - A) thumb + 128) >> 8, A in
 * [0, 256].  Cell indices are device memory and are clamped to the grid, not checked.  0 < gh, gw <= 32768, 0 < H, W <= 16384,
 * vmin finite, inv_span = 1 / (vmax - vmin) a normal positive float32.  Allocates nothing; enqueued on `stream` without a host
 * synchronisation; a bad argument is BQ_ERR_ARG with nothing enqueued. */
int bq_heatmap_render(bq_ctx* ctx, const float* d_values, int gh, int gw, const int32_t* d_col_table, const int32_t* d_row_table,
                      int interpolation, const uint8_t* d_lut, const uint8_t* d_thumb, uint8_t* d_out, int H, int W, float vmin,
                      float inv_span, int A, bq_stream_t stream);

/* The whole-slide heatmap's tissue mask (kernels_tissue.hip; DESIGN.md "Heatmap input", Tissue mask): Otsu QC on the slide's
 * thumbnail, restated in integers (Slideflow's qc='otsu', from memory: unpinned).  bq_tissue_blur: d_thumb uint8 [H][W][3] ->
 * d_plane uint8 [H][W], the 7 x 7 median (the 25th smallest of the 49 neighbours, coordinates clamped to the image; H or W below
 * 7 are legal) of the 8-bit saturation S = ((mx - mn) d_sdiv256[mx] + 2048) >> 12 with mx / mn the largest / smallest of r, g,
 * b, and d_hist int32 [256], the histogram of d_plane (zeroed by the call).  d_sdiv256 int32 [256] is the host's table
 * (tissue.sdiv_table: 0, then rint(255 * 4096 / v)).  One launch.  0 < H, W and H * W < 2^31.
 * bq_tissue_cells: d_count[gy][gx] (int32 [gh][gw]) = the number of pixels of d_plane with value <= T inside columns
 * [col_ranges[2 gx], col_ranges[2 gx + 1]) x rows [row_ranges[2 gy], row_ranges[2 gy + 1]).  The two range tables (int32 [gw][2],
 * [gh][2]: tissue.cell_ranges) are HOST memory: every range is checked here -- non-empty and inside the plane -- and the tables
 * are then copied into d_ranges (device, int32 [2 (gw + gh)], caller-owned) on `stream`; they must stay valid until the stream
 * has passed the call.  Ranges may overlap and may be one pixel wide.  0 <= T <= 255, 0 < gw, gh <= 32768.
 * Both allocate nothing and are enqueued on `stream` without a host synchronisation; a bad argument -- a null pointer, H * W >=
 * 2^31, an empty range or one outside the plane -- is BQ_ERR_ARG with nothing enqueued. */
int bq_tissue_blur(bq_ctx* ctx, const uint8_t* d_thumb, int H, int W, const int32_t* d_sdiv256, uint8_t* d_plane, int32_t* d_hist,
                   bq_stream_t stream);
int bq_tissue_cells(bq_ctx* ctx, const uint8_t* d_plane, int H, int W, int T, const int32_t* col_ranges, int gw,
                    const int32_t* row_ranges, int gh, int32_t* d_ranges, int32_t* d_count, bq_stream_t stream);

/* The heatmap's focus mask (kernels_focus.hip; DESIGN.md "Heatmap input", Focus mask): Slideflow's Gaussian blur QC on a 4 um /
 * pixel thumbnail, restated in integers (from memory: unpinned against Slideflow and scikit-image; pinned to scipy.ndimage in float64
 * within a derived band by a CPU test).  bq_tissue_focus: d_thumb uint8 [H][W][3] ->
 *     G = 2125 r + 7154 g + 721 b                                   (scikit-image's luma weights x 10 000; 2 550 000 per unit)
 *     L = |4 G(y,x) - G(y-1,x) - G(y+1,x) - G(y,x-1) - G(y,x+1)|    (coordinates clamped to the image)
 *     A(y,x) = (sum_k w[k] L(y, clamp(x + k - r)) + 32768) >> 16    (d_work, int32 [H][W], caller-owned)
 *     V(y,x) = (sum_k w[k] A(clamp(y + k - r), x) + 32768) >> 16    (64-bit sums; d_value_or_null int32 [H][W] receives V if given)
 * d_plane uint8 [H][W] = 1 where V > thr (in focus), 0 where V <= thr (out of focus); d_count, one int32, = the number of zeros
 * (zeroed by the call, one add per workgroup).  d_taps int32 [2 r + 1] is the host's table in device memory (tissue.focus_taps:
 * rint(65536 g_k) of the normalised Gaussian, the centre corrected so that the sum is 65536, every tap >= 0) and is not checked.
 * Two launches.  0 < H, W, H * W < 2^31, 1 <= r <= 16, 0 <= thr.
 * bq_tissue_cells_union: d_count[gy][gx] (int32 [gh][gw]) = the pixels (x, y) of the cell's range of the Otsu plane d_otsu_plane
 * uint8 [Ho][Wo] with d_otsu_plane[y][x] <= T or d_focus_plane[ymap[y]][xmap[x]] == 0, d_focus_plane uint8 [Hf][Wf].  xmap int32
 * [Wo], ymap int32 [Ho] (tissue.plane_map: ((2 i + 1) n_focus) / (2 n_otsu), a nearest-neighbour resize) and the two range tables
 * (as bq_tissue_cells') are HOST memory: checked here -- ranges non-empty and inside the Otsu plane, maps inside the focus plane and
 * non-decreasing -- then copied into d_tables (device, int32 [Wo + Ho + 2 (gw + gh)], caller-owned) on `stream`; they must stay
 * valid until the stream has passed the call.  0 <= T <= 255, 0 < gw, gh <= 32768, both planes below 2^31 pixels.
 * Both allocate nothing and are enqueued on `stream` without a host synchronisation; a bad argument is BQ_ERR_ARG with nothing
 * enqueued. */
int bq_tissue_focus(bq_ctx* ctx, const uint8_t* d_thumb, int H, int W, const int32_t* d_taps, int r, int thr, int32_t* d_work,
                    int32_t* d_value_or_null, uint8_t* d_plane, int32_t* d_count, bq_stream_t stream);
int bq_tissue_cells_union(bq_ctx* ctx, const uint8_t* d_otsu_plane, int Ho, int Wo, int T, const uint8_t* d_focus_plane, int Hf, int Wf,
                          const int32_t* xmap, const int32_t* ymap, const int32_t* col_ranges, int gw, const int32_t* row_ranges,
                          int gh, int32_t* d_tables, int32_t* d_count, bq_stream_t stream);

/* The heatmap's region-of-interest mask (kernels_roi.hip; DESIGN.md "Heatmap input", Region-of-interest mask): a pathologist's
 * polygons -> the grid cells inside them, Slideflow's ROI filter restated in integers (from memory: unpinned against Slideflow and
 * shapely; pinned to a numpy restatement integer for integer).  bq_roi_plane: d_plane[y][x] (uint8 [H][W]) = 1 iff the sample point
 * p = (xs[x], ys[y]) is inside any polygon, else 0.  All coordinates are DOUBLED level-0 pixels, so that a pixel centre is an
 * integer; the kernel does no coordinate arithmetic.  edges int32 [E][4] = (a.x, a.y, b.x, b.y), one row per polygon edge a -> b
 * (the closing edge included; roi.edge_table); starts int32 [P + 1]: polygon i owns edges [starts[i], starts[i + 1]).  An edge
 * counts for p iff (a.y > p.y) != (b.y > p.y) and, with d = (b.x - a.x)(p.y - a.y) - (p.x - a.x)(b.y - a.y) in int64, d > 0 when
 * b.y > a.y and d < 0 when b.y < a.y (csrc/roi_device.h, compiled for host and device): a point on an edge does not count for it,
 * a horizontal edge never counts.  p is inside a polygon iff an odd number of its edges count (even-odd: self-intersection and zero
 * area are legal) and inside the region iff inside any polygon (union).  The four tables are HOST memory and are checked here --
 * 0 < W, H, H * W < 2^31, 3 <= E <= 2^20, starts[0] = 0, starts[P] = E, every polygon at least 3 edges, every edge coordinate in
 * [-2^28, 2^28], every sample coordinate in [0, 2^29] (which keeps |d| < 2^62) -- then copied into d_tables (device, int32 [4 E +
 * P + 1 + W + H], 16-byte aligned, caller-owned) on `stream`; they must stay valid until the stream has passed the call.  One
 * launch.  Allocates nothing; enqueued on `stream` without a host synchronisation; a bad argument is BQ_ERR_ARG with nothing
 * enqueued. */
int bq_roi_plane(bq_ctx* ctx, const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys,
                 int H, int32_t* d_tables, uint8_t* d_plane, bq_stream_t stream);

/* Variant for callers that already hold standardised float32 NHWC tiles (the
 * UncertaintyInterface contract, results.py:256-257): converts to planar NCHW. */
int bq_stage_f32(bq_ctx* ctx, const float* d_tiles_nhwc_f32, int n, void* d_out_nchw,
                 bq_stream_t stream);

/* K1-K5: staged tiles -> [n,2048] fp32 global-average-pooled features. */
int bq_backbone(bq_ctx* ctx, const void* d_in_nchw, int n, float* d_feat2048, void* d_ws,
                size_t ws_bytes, bq_stream_t stream);

/* K0-K5 straight from the bytes: uint8 NHWC tiles -> [n,2048] features through the kernels bq_mc_infer runs (16-bit contexts:
 * standardisation + block1_conv1 + block1_conv2 fused into one launch; fp32 contexts: bq_stage + bq_backbone).  For callers
 * that need the features of a batch before they decide how to drive the head -- biscuit_amd.inference.evaluate on a batch whose
 * Philox tile indices are not one consecutive run: a tile's result is then the same whichever entry its batch took. */
int bq_backbone_u8(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, float* d_feat2048, void* d_ws,
                   size_t ws_bytes, bq_stream_t stream);

/* K6: mc_n stochastic passes of the dropout head over n feature rows, Welford-folded
 * on the device.  Dropout masks are Philox4x32-10 keyed by `seed` with counter
 * (unit/4, layer, pass, tile_idx0 + row): independent of batching.
 * pass0/init/finalize let a caller fold passes over several calls (BQ_MC_FULL):
 * init=1 zeroes the running state, finalize=1 writes mean/std.  d_state is
 * [n][5] fp32 (count, mean0, mean1, M2_0, M2_1), caller-owned. */
int bq_mc_head(bq_ctx* ctx, const float* d_feat, int n, int64_t tile_idx0, int mc_n,
               int pass0, uint64_t seed, int init, int finalize, float* d_state,
               float* d_mean2, float* d_std2, void* d_ws, size_t ws_bytes,
               bq_stream_t stream);

/* Optional device-side addend to tile_idx0 of bq_mc_head / bq_mc_infer (NULL: none; the pointer must stay valid while
 * launches that were enqueued with it are in flight).  The Philox tile counter of row i becomes
 * tile_idx0 + *d_tile_idx0 + i, read by the kernels when they RUN: a captured HIP graph of the path (the one-tile
 * loop of results.py:250-258) can then be replayed for tile after tile by updating 8 bytes of device memory. */
int bq_set_tile_index_ptr(bq_ctx* ctx, const int64_t* d_tile_idx0);

/* Optional per-tile Philox indices for the bq_mc_head / bq_mc_infer calls that follow (NULL: back to consecutive indices; the array
 * -- int64 [n of the call], device memory -- must stay valid while launches enqueued with it are in flight): the tile counter of
 * row i becomes tile_idx0 (+ *d_tile_idx0) + d_tile_idx[i] instead of ... + i.  A batch that holds the ends and beginnings of
 * several slides -- tiles whose global indices are not one consecutive run -- then takes ONE call instead of one head call per run
 * (biscuit_amd.inference.evaluate; results identical to the per-run calls, tests/test_gpu_parity.py). */
int bq_set_tile_index_array(bq_ctx* ctx, const int64_t* d_tile_idx);

/* Fused convenience: uint8 tiles -> (mean[n,2], std[n,2]).  mc_mode BQ_MC_HEAD runs
 * the backbone once and the head mc_n times; BQ_MC_FULL re-runs the whole network per
 * pass like the reference loop.  Results are bit-identical between the two. */
int bq_mc_infer(bq_ctx* ctx, const uint8_t* d_tiles_nhwc, int n, int64_t tile_idx0,
                int mc_n, uint64_t seed, int mc_mode, float* d_mean2, float* d_std2,
                void* d_ws, size_t ws_bytes, bq_stream_t stream);

/* K7: per-slide sums of y_pred (= mean of P(class 1)) and uncertainty (= std of
 * P(class 1)) plus tile counts, restricted to tiles with uncertainty < tile_uq when
 * tile_uq is a positive finite number (threshold.py:297-298: `if tile_uq:` and strict
 * `<`).  Accumulates into caller-zeroed 64-bit fixed-point buffers (order-independent,
 * bit-reproducible); call bq_slide_finish to convert to doubles. */
int bq_slide_reduce(bq_ctx* ctx, const float* d_mean2, const float* d_std2,
                    const int32_t* d_slide_idx, int n, int n_slides, float tile_uq,
                    int64_t* d_acc_pred, int64_t* d_acc_unc, int32_t* d_count,
                    bq_stream_t stream);
int bq_slide_finish(bq_ctx* ctx, const int64_t* d_acc_pred, const int64_t* d_acc_unc,
                    const int32_t* d_count, int n_slides, double* d_mean_pred,
                    double* d_mean_unc, bq_stream_t stream);

/* Threshold search of the consumer on the device: Youden's J over the ROC curve of (label, score), i.e.
 * `thresh[argmax(tpr - fpr)]` of sklearn.metrics.roc_curve as the reference uses it for the tile-level
 * prediction threshold (threshold.py:145-155), the tile-level uncertainty threshold over every tile of the
 * cohort (threshold.py:417-426) and the slide-level ones (threshold.py:212-218, 449-455): first maximum, curve
 * starting at (0, 0) with threshold +inf, one point per distinct score, rates in float64 from exact counts.
 * d_score [n] float64, d_label [n] uint8 (non-zero = positive); d_out6 = [threshold, J, tpr, fpr, n_pos,
 * n_neg] (float64, device).  With only one class present the rates are undefined (the reference raises):
 * callers check n_pos / n_neg.  Workspace: bq_roc_workspace_bytes(n). */
size_t bq_roc_workspace_bytes(int64_t n);
int bq_roc_youden(bq_ctx* ctx, const double* d_score, const uint8_t* d_label, int64_t n,
                  void* d_ws, size_t ws_bytes, double* d_out6, bq_stream_t stream);

/* Per-kernel timing with HIP events on the launch stream (bench.py roofline leg).
 * bq_profile_enable(1) brackets every subsequent launch with events;
 * bq_profile_read synchronises and returns, per kernel class, the number of launches,
 * total milliseconds, algorithmic FLOPs and algorithmic bytes since the last enable. */
enum { BQ_PROF_MAX = 64 };
typedef struct bq_prof_entry {
    char name[48];
    int64_t launches;
    double ms;
    double flops;
    double bytes;
} bq_prof_entry;
int bq_profile_enable(bq_ctx* ctx, int on);
int bq_profile_read(bq_ctx* ctx, bq_prof_entry* out, int max_entries);

/* Test hook: run the backbone on staged tiles up to and including the named layer
 * ("staged", "block1_conv1", "block1_conv2", "block{2,3,4}_{res,sepconv1,sepconv2,out}",
 * "block{5..12}_sepconv{1,2}", "block{5..13}_out", "block13_{res,sepconv1,sepconv2}", "block14_sepconv{1,2}") and copy that
 * activation -- as STORED: with activation exponents in the blob (weights.py: pack_blob(act_exp=...)) 2^-k times the network's
 * value -- as fp32 NHWC
 * [n,H,W,C] (true channel count, padding stripped) into d_out.  Returns the number of
 * elements written, or <0. */
int64_t bq_debug_activation(bq_ctx* ctx, const char* name, const void* d_in_nchw, int n,
                            void* d_ws, size_t ws_bytes, float* d_out, size_t out_elems,
                            bq_stream_t stream);

/* The same test hook on the path bq_mc_infer takes in a 16-bit context: from the uint8 tiles [n,299,299,3] through the fused
 * front kernel (standardise + block1_conv1 + block1_conv2 in one launch, csrc/kernels_front.hip), then as above.  "staged"
 * and "block1_conv1" are not materialised on this path and are refused; every name from "block1_conv2" on is available.
 * A batch beyond the front kernel's 32-bit offsets (n > 1552) is staged into the workspace and runs the kernels of the float
 * entry, here as in bq_mc_infer and bq_backbone_u8 ("Size limits of the routes"). */
int64_t bq_debug_activation_u8(bq_ctx* ctx, const char* name, const uint8_t* d_tiles, int n,
                               void* d_ws, size_t ws_bytes, float* d_out, size_t out_elems,
                               bq_stream_t stream);

/* Which kernel family would run each matrix layer: the launch schedule of a batch of n tiles as text, one line
 * "<layer or block output> <route>" per step in launch order (the routes are the RouteKind names of csrc/biscuit_hip.hip, e.g.
 * "block5_sepconv1 WIDE", "block3_out BLOCK_TAIL", "block14_sepconv2 DW_THEN_EXIT GAP_EPILOGUE=yes"), NUL-terminated, into
 * out[cap].  from_u8 != 0: the walk of bq_mc_infer / bq_backbone_u8 (with `name`: of bq_debug_activation_u8), otherwise of
 * bq_backbone (bq_debug_activation).  name: a debug tap as above, or NULL; the text ends behind the tapped tensor, and a call
 * those hooks refuse is refused here with the same error.  Decided by the code that launches; launches nothing.  Returns the
 * text's length, or <0. */
int bq_describe_schedule(bq_ctx* ctx, int n, int from_u8, const char* name, char* out, size_t cap);

/* The feature map (kernels_knn.hip, kernels_umap.hip; DESIGN.md "Feature map (Figure 6)"): exact nearest neighbours, the fuzzy
 * graph's rows and the layout's epochs of UMAP, restated from memory (unpinned against umap-learn; pinned to a float64 numpy
 * restatement, tests/_umap_ref.py).  The per-row arithmetic is csrc/umap_device.h, compiled for host and device.
 *
 * bq_knn: d_x fp32 [n][D] (16-byte aligned, D a multiple of 16, 16 .. 2^20) -> d_idx int32 [n][k] and d_dist fp32 [n][k], the k
 * nearest rows of every row by Euclidean distance, each row sorted by (distance, index) ascending; the row itself is a candidate
 * like any other, so it is normally rank 0.  1 <= k <= 64, k <= n, n <= 2^31 / 160: anything else is BQ_ERR_ARG.  The distance
 * is the direct form sum (x - y)^2 in fp32 in one fixed order, its square root correctly rounded, and the table is the one over
 * ALL n rows in that arithmetic (bqio_knn's, bit for bit) on every row: a pruning pass in the GEMM form on the fp32 matrix
 * instruction keeps 2 (k + 16) candidates per row and, with a worst-case bound on its own error, a lower bound on the distance
 * of everything it dropped; a row whose k-th candidate does not lie strictly below that bound is ranked again over all n rows.
 * The n x n matrix is never stored.  Precondition: every value of d_x is finite (not checked here: no host synchronisation;
 * Engine.knn checks).  Where it is broken, a pair whose distance is not finite is no candidate, and a row with fewer than k
 * candidates ends in d_idx = -1, d_dist = NaN; every element of d_idx and d_dist is written in any case.  d_ws:
 * bq_knn_workspace_bytes(n, D, k) = 2 pad256(4 n) + 8 n (k + 16) + 8 n bytes, pad256 rounding up to a multiple of 256 (0 for
 * arguments the call refuses), 16-byte aligned, caller-owned, contents unspecified on entry; BQ_ERR_WORKSPACE below that.  On
 * return (in stream order) its first n int32 hold 1 for the rows that were ranked again over all rows, 0 for the others.  No
 * atomics: the same bits every run.
 *
 * bq_umap_smooth: the table of bq_knn -> d_rho [n], d_sigma [n] and the membership weights d_w [n][k] (local connectivity 1,
 * bandwidth 1): rho the smallest non-zero distance of the row, sigma by 64 bisection steps for sum_{j >= 1} exp(-max(0, d_j -
 * rho) / sigma) = log2(k), floored at 1e-3 x the row's mean distance (x the mean of all distances where rho = 0); w = 0 for the
 * row itself, 1 where d - rho <= 0, else exp(-(d - rho) / sigma).  d_scratch: bq_umap_smooth_scratch_bytes(n) bytes, 8-byte
 * aligned.
 *
 * bq_umap_epoch: one epoch (1-based) of the layout in gather form.  The graph is a symmetric CSR on the device -- d_indptr int64
 * [n + 1] from 0, non-decreasing; d_nbr int32 [nnz] in 0 .. n - 1, ascending within a row (the caller's to guarantee: nothing
 * here reads them back); d_eps fp32 [nnz] epochs per sample; d_next fp32 [nnz] the epoch of the next sample, advanced here.
 * Vertex i reads d_prev fp32 [n][2] and writes d_out[i] (d_out != d_prev): for every edge of its row with next <= epoch the
 * attractive step, then 5 repulsive steps against vertices drawn by Philox4x32-10 (key seed; counter epoch, vertex, slot in
 * the row, draw), every component clipped to +-4 and scaled by alpha.  block: threads per workgroup, a multiple of 64 up to
 * 1024 (0: 64); the result does not depend on it.
 *
 * All three allocate nothing and are enqueued on `stream` without a host synchronisation; a bad argument is BQ_ERR_ARG with
 * nothing enqueued. */
size_t bq_knn_workspace_bytes(int64_t n, int D, int k);
int bq_knn(bq_ctx* ctx, const float* d_x, int64_t n, int D, int k, int32_t* d_idx, float* d_dist, void* d_ws, size_t ws_bytes,
           bq_stream_t stream);
size_t bq_umap_smooth_scratch_bytes(int64_t n);
int bq_umap_smooth(bq_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t n, int k, float* d_rho, float* d_sigma, float* d_w,
                   void* d_scratch, size_t scratch_bytes, bq_stream_t stream);
int bq_umap_epoch(bq_ctx* ctx, const float* d_prev, float* d_out, int64_t n, const int64_t* d_indptr, const int32_t* d_nbr,
                  const float* d_eps, float* d_next, int epoch, float alpha, float a, float b, uint64_t seed, int block,
                  bq_stream_t stream);

/* The data behind the UQ calibration figure over every row of a tile table (kernels_calib.hip; DESIGN.md section 7 "UQ
 * calibration"; biscuit/threshold.py:15-122): d_x float64 [n] the uncertainty (finite: the caller checks), d_correct uint8 [n]
 * (non-zero = correct), in any order; 1 <= n <= 2^31 - 1, 2 <= grid <= 1024.  All arithmetic is float64; the rows are summed in
 * chunks of bq_uq_chunk_rows(n) and the chunks in order, without atomics: the same bits every call.
 *
 * bq_uq_kde: the Gaussian kernel density of x per group g (0 = incorrect, 1 = correct) with Scott's bandwidth bw = std(ddof 1)
 * n_g^(-1/5) at grid points linspace(min_g - cut bw, max_g + cut bw, grid).  d_out float64 [4 grid + 16] = support [2][grid],
 * density [2][grid] (integrating to 1 per group: scipy.stats.gaussian_kde), stat [2][8] = n_g, min, max, mean, std, bw, valid,
 * 1 / (n_g bw sqrt(2 pi)).  A group with n_g < 2 or std = 0 has valid = 0 and NaN support and density.
 *
 * bq_uq_loess: local quadratic regression of y = (correct != 0) on x at the vertices linspace(min x, max x, grid): window of
 * q = floor(span n + 1e-5) rows (1 <= q <= n), tricube weights.  d_out float64 [5 grid + 4] = vertex, fit, l2 (squared norm of
 * the smoother's row), lam (self-influence at the vertex), h (the window's half-width), each [grid], then nu = sum_i lam~(x_i),
 * rss = sum_i (y_i - fit~(x_i))^2 (~: linear interpolation over the vertices), the number of degenerate vertices, q.  A
 * degenerate vertex (h = 0, or fewer than three distinct x inside the window) has NaN fit, l2 and lam.
 *
 * d_ws: bq_uq_*_workspace_bytes(n, grid) bytes (0 for arguments the call refuses), 256-byte aligned, caller-owned, contents
 * unspecified on entry; BQ_ERR_WORKSPACE below that.  Both allocate nothing and are enqueued on `stream` without a host
 * synchronisation; a bad argument is BQ_ERR_ARG with nothing enqueued. */
int64_t bq_uq_chunk_rows(int64_t n);
size_t bq_uq_kde_workspace_bytes(int64_t n, int grid);
int bq_uq_kde(bq_ctx* ctx, const double* d_x, const uint8_t* d_correct, int64_t n, int grid, double cut, double* d_out, void* d_ws,
              size_t ws_bytes, bq_stream_t stream);
size_t bq_uq_loess_workspace_bytes(int64_t n, int grid);
int bq_uq_loess(bq_ctx* ctx, const double* d_x, const uint8_t* d_correct, int64_t n, int grid, double span, double* d_out, void* d_ws,
                size_t ws_bytes, bq_stream_t stream);

/* DeLong's covariance of the AUROCs of k classifiers scored on the same n rows (kernels_delong.hip; DESIGN.md section 7
 * "Prediction metrics"; biscuit/delong.py): d_scores float64 [k][n] (no NaN: the caller checks; +-inf and both zeros are
 * ordinary values, the zeros equal), d_label uint8 [n] (non-zero = positive; both classes present: the caller checks), in any
 * order; 1 <= k <= 8, 1 <= n <= 2^25 (the midrank sums stay exact integers below 2^53).
 *
 * d_out float64 [k + k k + 2] = auc [k], S [k][k], m, n0 (the positives and the negatives).  For a positive row V = (negatives
 * below + tied negatives / 2) / n0, for a negative row V = 1 - (positives below + tied positives / 2) / m; auc = (sum of the
 * positives' midranks) / m / n0 - ((m + 1) / 2) / n0; both equal the reference's values bit for bit.  S = cov(V | positive) / m +
 * cov(V | negative) / n0 with the unbiased covariance (NaN entries where a class has one row), summed in chunks of
 * bq_delong_chunk_rows(n) rows and the chunks in order, without floating-point atomics: the same bits every call.  d_V: NULL, or
 * float64 [k][n] that receives V in row order.
 *
 * d_ws: bq_delong_workspace_bytes(k, n) bytes (0 for arguments the call refuses), 256-byte aligned, caller-owned, contents
 * unspecified on entry; BQ_ERR_WORKSPACE below that.  Allocates nothing and is enqueued on `stream` without a host
 * synchronisation; a bad argument is BQ_ERR_ARG with nothing enqueued. */
size_t bq_delong_workspace_bytes(int k, int64_t n);
int64_t bq_delong_chunk_rows(int64_t n);
int bq_delong(bq_ctx* ctx, const double* d_scores, const uint8_t* d_label, int k, int64_t n, void* d_ws, size_t ws_bytes, double* d_out,
              double* d_V, bq_stream_t stream);

/* Training the MC-dropout head on cached features (kernels_train.hip; DESIGN.md section 7 "Head training"): features [.][2048] ->
 * Dense 1024 + ReLU -> Dense 1024 + ReLU -> Dense 2 -> softmax with inverted dropout on the input of each layer, the head of
 * bq_mc_head in plain fp32.  d_params, d_m, d_v, d_grad: float32 [P], P = 3 149 826, caller-owned, 16-byte aligned, in the order
 * hidden_0/kernel [2048][1024], hidden_0/bias [1024], hidden_1/kernel [1024][1024], hidden_1/bias [1024], logits/kernel [1024][2],
 * logits/bias [2] (row-major [K][N]).  The weights a context loaded are neither read nor changed.
 *
 * bq_head_grad: the gradient of the mean sparse categorical cross-entropy over the n rows d_feats[d_rows[i]] (d_feats float32
 * [n_feat][2048], d_rows int64 [n], d_labels uint8 [n] in {0, 1}; 1 <= n <= 1024; the rows are gathered by the kernels) -> d_grad
 * [P] and d_loss [1].  The keep mask of unit u of layer l is Philox4x32-10 with counter (u / 4, l, step, d_rows[i]) and key seed,
 * keep = r >= floor(rate 2^32), scale fp32(1 / (1 - rate)): the contract of bq_mc_head with pass = step and tile = the row's index;
 * the backward pass draws the masks again.  ReLU's derivative is 0 at 0.  A feature that is not finite, a row index outside
 * 0 .. n_feat - 1 (never read) or a label above 1 gives a NaN loss.  Every sum runs in a fixed order and there are no floating-point
 * atomics: the same bits every call.
 *
 * bq_head_adam: one pass of Keras Adam over P, t = step + 1: m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g^2,
 * w' = w - lr sqrt(1 - b2^t) / (1 - b1^t) m' / (sqrt(v') + eps), evaluated in float64 per element and rounded once per stored value.
 *
 * bq_head_train_steps: `steps` pairs of the two above, step = step0 + i, over d_rows / d_labels [steps][batch] (the last step takes its
 * first last_n entries, 1 <= last_n <= batch), learning rate h_lr[i] (host memory, read before the call returns), loss of step i to
 * d_losses[i]: one linear chain of launches on `stream`, the same bits as the single calls.
 *
 * d_ws: bq_head_train_workspace_bytes(n) bytes (n = batch; 0 for an n the calls refuse), 256-byte aligned, caller-owned, contents
 * unspecified on entry; BQ_ERR_WORKSPACE below that.  All allocate nothing and are enqueued without a host synchronisation; a bad
 * argument is BQ_ERR_ARG with nothing enqueued.
 *
 * bq_head_validate: the forward half of bq_head_grad on the same d_params, for scoring a head in the middle of its training
 * (DESIGN.md section 7 "Training schedule"): 1 <= n <= 4096 rows gathered through d_rows, the same arithmetic (the exact-f32 MFMA
 * GEMMs with their four accumulators, the logits on the vector ALU, softmax and the row's loss in float64 from the fp32 logits).
 * rate == 0 is inference mode: no mask is drawn; rate > 0 draws the masks of the contract above with pass in the place of step.
 * -> d_stats [2] float64: the sum of the rows' losses, and the number of rows whose larger logit is their label's (a tie goes to
 * class 0); d_rowloss float64 [n] and d_hit uint8 [n], each or NULL: the rows' own loss and 0 / 1 hit.  A feature that is not finite,
 * a row index outside 0 .. n_feat - 1 (never read) or a label above 1 gives that row a NaN loss and a hit of 0, and d_stats[0] is NaN.
 * Every sum runs in a fixed order without floating-point atomics: the same bits every call; a row's loss and hit do not depend on n
 * or on the row's place in d_rows.  d_params is only read.  d_ws: bq_head_validate_workspace_bytes(n) bytes (0 for an n the call
 * refuses), under the rules of the training workspace above, which keeps its own limit of 1024. */
size_t bq_head_train_workspace_bytes(int n);
int bq_head_grad(bq_ctx* ctx, const float* d_params, const float* d_feats, int64_t n_feat, const int64_t* d_rows, const uint8_t* d_labels,
                 int n, int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws, size_t ws_bytes,
                 bq_stream_t stream);
size_t bq_head_validate_workspace_bytes(int n);
int bq_head_validate(bq_ctx* ctx, const float* d_params, const float* d_feats, int64_t n_feat, const int64_t* d_rows, const uint8_t* d_labels,
                     int n, int64_t pass, uint64_t seed, double rate, double* d_stats, double* d_rowloss, uint8_t* d_hit, void* d_ws,
                     size_t ws_bytes, bq_stream_t stream);
int bq_head_adam(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, const float* d_grad, int64_t step, double lr, double b1, double b2,
                 double eps, bq_stream_t stream);
int bq_head_train_steps(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_feats, int64_t n_feat,
                        const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0, uint64_t seed,
                        double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws, size_t ws_bytes,
                        bq_stream_t stream);

/* Exit-flow fine-tuning (kernels_train.hip; DESIGN.md section 7 "Exit-flow fine-tuning"): Xception's block 14 trained together with
 * the head, on a cache of block13_out.
 *
 * bq_trunk_u8: bq_backbone_u8's launches, by the same routes and under the same size limits, up to block13_out -> d_out_f32
 * [n][10][10][1024], the network's value (the blob's activation exponent of the tensor removed: a power of two, exact).  d_ws:
 * bq_workspace_bytes(ctx, n, 1).
 *
 * The trainable exit vector, float32 [P_EXIT], P_EXIT = 4 748 800, in the order D1 [3][3][1024], P1 [1024][1536], gamma1 [1536],
 * beta1 [1536], D2 [3][3][1536], P2 [1536][2048], gamma2 [2048], beta2 [2048] (block14_sepconv{1,2}'s depthwise and pointwise
 * kernels and their BN's gamma and beta); the head's P follow in their order above: P_ALL = 7 898 626.  d_bn_stats, float32 [7168],
 * only read: moving_mean1 [1536], moving_variance1 [1536], moving_mean2 [2048], moving_variance2 [2048] -- the statistics stay
 * frozen.  With a = gamma / sqrt(var + 1e-3), b = beta - a mean, dw the 3 x 3 depthwise convolution (zero padding 1, stride 1):
 *     u1 = dw(x, D1), z1 = u1 P1, h1 = relu(a1 z1 + b1), u2 = dw(h1, D2), z2 = u2 P2, h2 = relu(a2 z2 + b2), f = mean_100 h2
 * for each row x = d_acts[d_rows[i]] (d_acts float32 [n_act][10][10][1024], offsets in 64 bits), 1 <= n <= 256.
 *
 * bq_exit_features: d_exit_params [P_EXIT] -> d_feat2048 [n][2048].  A row of f depends on its tile and the parameters only, not
 * on n or on its place in d_rows.
 * bq_exit_grad: d_params [P_ALL] -> d_grad [P_ALL], d_loss [1]: the gradient of bq_head_grad's loss on f (the same kernels, the
 * Philox counters d_rows[i], layers 0 .. 2: the last P entries and the loss are bit for bit bq_head_grad's on bq_exit_features'
 * output), carried back through block 14; ReLU's derivative is 0 at 0.  A row index outside 0 .. n_act - 1 (never read), an
 * activation that is not finite or a label above 1 gives a NaN loss.  The pointwise products run on the exact f32-input MFMA; every
 * sum has a fixed order and there are no floating-point atomics: the same bits every call.
 * bq_adam_n: bq_head_adam's pass over `count` elements.
 * bq_exit_train_steps: bq_head_train_steps' loop of bq_exit_grad + one Adam over P_ALL; the same bits as the single calls.
 *
 * d_ws: bq_exit_features_workspace_bytes(n) / bq_exit_train_workspace_bytes(n) bytes (0 for an n the calls refuse), under the rules
 * of the head's training workspace.  All are one linear chain of launches on `stream`: nothing is captured, allocated or waited for.
 *
 * The cache in other forms (DESIGN.md section 7 "Exit-flow fine-tuning", Sizes): the three calls with a trailing _c take a descriptor
 * where the ones above take d_acts, n_act, and are otherwise the same calls -- the ones above are the _c calls with {BQ_ACT_F32, mul 1,
 * BQ_ACT_DEVICE}.  A 16-bit cache (BQ_ACT_F16 / BQ_ACT_BF16) holds the engine's stored block13_out h, [n_rows][10][10][1024] of 2 bytes,
 * and its row's x is float(h) * mul, mul a positive finite power of two: the float32 cache's numbers exactly, so every result has the
 * float32 cache's bits.  A float32 cache has mul 1.  A 16-bit infinity or NaN reads as NaN, like a float32 one.
 * where == BQ_ACT_HOST: the cache lies in mapped pinned host memory and p is its device pointer (bq_host_device_pointer).  Every
 * step first copies its rows into a staging region at the end of the workspace with one kernel on `stream` (class exit_gather: whole
 * rows, a row outside the cache filled with NaN) and reads only that copy; host memory is read once per step and row, by that kernel
 * alone.  d_ws is then bq_exit_features_staged_workspace_bytes(n, type) / bq_exit_staged_workspace_bytes(n, type) bytes: the sizes
 * above plus n rows of the cache's type (0 for an n or a type the calls refuse).  Still one linear chain on `stream`.
 * bq_host_device_pointer: the device pointer of mapped pinned host memory `host` (hipHostMalloc / hipHostRegister, which need not
 * be its first byte) -> *dev; BQ_ERR_ARG, *dev NULL, for any other memory, asked of the runtime without touching the memory.
 * bq_trunk_u8_packed: bq_trunk_u8's walk -- the same launches by the same routes -- with block13_out written as the engine stores
 * it, compact 16-bit [n][10][10][1024] in the engine's own type, neither widened nor scaled, and the power of two bq_trunk_u8
 * multiplies by -> *mul: float(d_out16) * *mul is bq_trunk_u8's output bit for bit.  BQ_ERR_ARG on a float32 engine. */
enum { BQ_ACT_F32 = 0, BQ_ACT_BF16 = 1, BQ_ACT_F16 = 2 };   /* the values of BQ_DTYPE_* */
enum { BQ_ACT_DEVICE = 0, BQ_ACT_HOST = 1 };
typedef struct bq_act_cache {
    const void* p;     /* [n_rows][10][10][1024] of `type`, 16-byte aligned; BQ_ACT_HOST: the device pointer of the host memory */
    int64_t n_rows;
    int type;          /* BQ_ACT_F32 / BQ_ACT_F16 / BQ_ACT_BF16 */
    float mul;         /* x = float(stored) * mul; 1 for BQ_ACT_F32 */
    int where;         /* BQ_ACT_DEVICE / BQ_ACT_HOST */
} bq_act_cache;
int bq_trunk_u8_packed(bq_ctx* ctx, const uint8_t* d_tiles_u8, int n, void* d_out16, float* mul, void* d_ws, size_t ws_bytes,
                       bq_stream_t stream);
int bq_host_device_pointer(void* host, void** dev);
size_t bq_exit_features_staged_workspace_bytes(int n, int type);
size_t bq_exit_staged_workspace_bytes(int n, int type);
int bq_exit_features_c(bq_ctx* ctx, const float* d_exit_params, const float* d_bn_stats, const bq_act_cache* cache, const int64_t* d_rows,
                       int n, float* d_feat2048, void* d_ws, size_t ws_bytes, bq_stream_t stream);
int bq_exit_grad_c(bq_ctx* ctx, const float* d_params, const float* d_bn_stats, const bq_act_cache* cache, const int64_t* d_rows,
                   const uint8_t* d_labels, int n, int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws,
                   size_t ws_bytes, bq_stream_t stream);
int bq_exit_train_steps_c(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_bn_stats,
                          const bq_act_cache* cache, const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n,
                          int64_t step0, uint64_t seed, double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses,
                          void* d_ws, size_t ws_bytes, bq_stream_t stream);
int bq_trunk_u8(bq_ctx* ctx, const uint8_t* d_tiles_u8, int n, float* d_out_f32, void* d_ws, size_t ws_bytes, bq_stream_t stream);
size_t bq_exit_features_workspace_bytes(int n);
size_t bq_exit_train_workspace_bytes(int n);
int bq_exit_features(bq_ctx* ctx, const float* d_exit_params, const float* d_bn_stats, const float* d_acts, int64_t n_act,
                     const int64_t* d_rows, int n, float* d_feat2048, void* d_ws, size_t ws_bytes, bq_stream_t stream);
int bq_exit_grad(bq_ctx* ctx, const float* d_params, const float* d_bn_stats, const float* d_acts, int64_t n_act, const int64_t* d_rows,
                 const uint8_t* d_labels, int n, int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, void* d_ws,
                 size_t ws_bytes, bq_stream_t stream);
int bq_adam_n(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, const float* d_grad, int64_t count, int64_t step, double lr, double b1,
              double b2, double eps, bq_stream_t stream);
int bq_exit_train_steps(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, float* d_grad, const float* d_bn_stats, const float* d_acts,
                        int64_t n_act, const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n, int64_t step0,
                        uint64_t seed, double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses, void* d_ws,
                        size_t ws_bytes, bq_stream_t stream);

/* Training-mode batch norm (DESIGN.md section 7 "Exit-flow fine-tuning", Two modes; unpinned: Keras' fused BatchNormalization,
 * momentum 0.99, epsilon 1e-3, restated).  The calls above keep the moving statistics frozen; these normalise a batch by its own.
 * For one layer, z [M][C] with M = 100 n -- every position of every tile of the batch --, in fp32:
 *     mu = (1/M) sum z        var = (1/M) sum (z - mu)^2        (biased; two passes, never E[z^2] - mu^2)
 *     a = gamma / sqrt(var + eps)    b = beta - a mu    h = relu(a z + b)
 *     g = dh [h > 0]    xhat = (z - mu) / sqrt(var + eps)    dbeta = sum g    dgamma = sum g xhat
 *     dz = a (g - dbeta / M - xhat dgamma / M)
 *     moving_mean <- 0.99 moving_mean + 0.01 mu       moving_var <- 0.99 moving_var + 0.01 var M / (M - 1)
 * Layer 1's statistics are taken over z1, layer 2's over z2, which already depends on layer 1's.  Only the training step depends on
 * the batch: bq_exit_features, validation and the packed engine use the moving statistics.
 *
 * bq_exit_grad_bn: bq_exit_grad_c without d_bn_stats -- training mode does not read the moving statistics -- and with d_batch_stats
 * float32 [7168], 16-byte aligned, written: mu1 [1536] | var1 [1536] | mu2 [2048] | var2 [2048], the biased statistics the step
 * used.  The forward chain is bq_exit_grad_c's with each layer's statistics (per-tile partial sums, then the tiles in a fixed order;
 * classes exit_train_stat1 / stat2) and coefficients behind its pointwise product: bq_exit_grad_c given d_batch_stats as d_bn_stats
 * reproduces the loss, the head's gradient and dgamma2 | dbeta2 bit for bit.  Backwards, one in-place pass per layer (classes
 * exit_train_bnfix2 / bnfix1) subtracts a (dbeta / M + xhat dgamma / M) from dz before the transposed products.  The same refusals; a
 * NaN activation, a row outside the cache or a label above 1 gives a NaN loss, and a channel's NaN statistic spreads to every tile of
 * the batch -- training-mode BN's nature.  Every sum has a fixed order and there are no floating-point atomics: the same bits every
 * call.  One linear chain on `stream`: nothing is captured, allocated or waited for.
 * bq_exit_bn_move: the moving statistics d_bn_stats [7168] in place after a step over n tiles whose statistics were d_batch_stats,
 * M = 100 n: two products and a sum per element, evaluated in float64 and rounded once (class exit_train_bnmove).
 * bq_exit_train_steps_bn: bq_exit_train_steps_c's loop of bq_exit_grad_bn + one Adam over P_ALL + bq_exit_bn_move on d_bn_stats, which
 * changes in place; the last, shorter batch uses its own M.  The same bits as the single calls.
 * d_ws: bq_exit_bn_workspace_bytes(n, type, where) bytes for either call, type and where the cache's: the training workspace of that
 * cache plus a step's statistics; 0 for an n, a type or a place the calls refuse. */
size_t bq_exit_bn_workspace_bytes(int n, int type, int where);
int bq_exit_grad_bn(bq_ctx* ctx, const float* d_params, const bq_act_cache* cache, const int64_t* d_rows, const uint8_t* d_labels, int n,
                    int64_t step, uint64_t seed, double rate, float* d_grad, float* d_loss, float* d_batch_stats, void* d_ws,
                    size_t ws_bytes, bq_stream_t stream);
int bq_exit_bn_move(bq_ctx* ctx, float* d_bn_stats, const float* d_batch_stats, int n, bq_stream_t stream);
int bq_exit_train_steps_bn(bq_ctx* ctx, float* d_params, float* d_m, float* d_v, float* d_grad, float* d_bn_stats,
                           const bq_act_cache* cache, const int64_t* d_rows, const uint8_t* d_labels, int steps, int batch, int last_n,
                           int64_t step0, uint64_t seed, double rate, const double* h_lr, double b1, double b2, double eps, float* d_losses,
                           void* d_ws, size_t ws_bytes, bq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BISCUIT_HIP_H */
