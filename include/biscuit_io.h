/* biscuit_io.h -- C ABI of libbiscuit_io.so: host-side reader of Slideflow tile TFRecords
 * (SURVEY.md section 8f row 1), the data format in front of the staging kernel.
 *
 * Replaces, for the hot path's input side, what the reference gets from Slideflow's tf.data
 * pipeline (`Project.evaluate(...)`, experiment.py:917-922; tiles are PNG, 299 px / 302 um,
 * configure.py:118-124): TFRecord framing
 *     uint64 length | uint32 masked_crc32c(length) | bytes[length] | uint32 masked_crc32c(data)
 * a `tf.train.Example` holding `slide` (bytes), `image_raw` (bytes, PNG or JPEG), `loc_x`,
 * `loc_y` (int64), the PNG decode (zlib inflate + scanline unfilter written here; the image
 * has no libpng) and the baseline-JPEG decode (csrc/jpeg_baseline.h: the arithmetic of libjpeg's
 * defaults -- islow IDCT, fancy upsampling -- which is what TensorFlow's decode_jpeg runs, so the
 * bytes are the ones the reference's pipeline saw).  JPEG streams outside that subset are reported,
 * not decoded: the caller hands those bytes to its own decoder.  No TensorFlow, no Slideflow.
 * Plain pointers and sizes only.
 */
#ifndef BISCUIT_IO_H
#define BISCUIT_IO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bqio_reader bqio_reader;

enum { BQIO_OK = 0, BQIO_ERR_ARG = -1, BQIO_ERR_IO = -2, BQIO_ERR_FORMAT = -3, BQIO_ERR_CORRUPT = -4,
       BQIO_ERR_UNSUPPORTED = -5, BQIO_ERR_NAN = -6 };
enum { BQIO_VERIFY_NONE = 0, BQIO_VERIFY_LENGTH = 1, BQIO_VERIFY_FULL = 2 };
enum { BQIO_IMG_UNKNOWN = 0, BQIO_IMG_PNG = 1, BQIO_IMG_JPEG = 2 };

/* Map the file and index its records (checking the CRCs `verify` asks for).  NULL on failure;
 * bqio_last_error(NULL) then says why. */
bqio_reader* bqio_open(const char* path, int verify);
void bqio_close(bqio_reader* r);
const char* bqio_last_error(bqio_reader* r);

/* Number of records (= tiles of the slide). */
int64_t bqio_count(bqio_reader* r);

/* `slide` feature of the first record, NUL-terminated into buf; returns its length or <0. */
int bqio_slide_name(bqio_reader* r, char* buf, int buflen);

/* Format of record `index`'s image_raw payload (BQIO_IMG_*), and a pointer to / length of the
 * payload inside the mapping (valid until bqio_close). */
int bqio_image_format(bqio_reader* r, int64_t index);
int bqio_image_bytes(bqio_reader* r, int64_t index, const uint8_t** data, size_t* len);

/* Decode records [first, first+count): RGB uint8 tiles into out[count][tile_px][tile_px][3],
 * loc_x/loc_y into loc[count][2] (may be NULL), with n_threads worker threads.  PNG (8-bit grey,
 * RGB, palette, RGBA -- alpha dropped; non-interlaced) and baseline JPEG (8-bit, Huffman, one
 * interleaved scan, grey or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, restart markers allowed).  Any other
 * payload -- progressive JPEG, a damaged JPEG stream, ... -- returns BQIO_ERR_UNSUPPORTED and
 * leaves the index of the first such record in *bad_index (may be NULL); a tile of the wrong size
 * returns BQIO_ERR_FORMAT. */
int bqio_decode(bqio_reader* r, int64_t first, int64_t count, int tile_px, uint8_t* out, int64_t* loc,
                int n_threads, int64_t* bad_index);

/* The same records with the PNG scanline filters LEFT IN, for a caller that reverses them on the GPU (bq_png_unfilter,
 * include/biscuit_hip.h): out_rows[count][tile_px][1 + 3*tile_px] -- per row the filter-type byte (0..4) and the filtered RGB
 * bytes, which for an 8-bit RGB non-interlaced PNG is the inflated IDAT stream as it is (a third of a photo-like tile's decode
 * time stays off the host).  Tiles of any other kind -- grey / palette / RGBA PNGs, JPEGs -- are decoded completely here and
 * delivered as rows of filter type 0.  Errors as bqio_decode. */
int bqio_decode_rows(bqio_reader* r, int64_t first, int64_t count, int tile_px, uint8_t* out_rows, int64_t* loc,
                     int n_threads, int64_t* bad_index);

/* Would bqio_decode take records [first, first + count)?  Checks what can be checked without decoding: every record parses,
 * every image is a PNG or a JPEG whose markers and scan structure the baseline decoder accepts (one pass over the bytes of the
 * JPEG records; PNG records are not looked into -- PNG is lossless, any decoder gives the same pixels).  A caller that falls
 * back to another JPEG decoder for what this library refuses can so decide ONCE per slide, before the first chunk, and never
 * mixes two decoders' IDCTs inside a slide.  BQIO_OK, or the error bqio_decode would report, *bad_index = the record. */
int bqio_probe(bqio_reader* r, int64_t first, int64_t count, int tile_px, int64_t* bad_index);

/* The compressed side of the PNG tiles for the DEVICE inflate (libbiscuit_hip: bq_png_inflate): the zlib streams (concatenated
 * IDAT payloads) of records [first, first + count), packed into out_z -- stream i at off[i] (a multiple of 16), len[i] bytes, at
 * least 32 zero bytes behind each -- plus the records' loc_x / loc_y (loc may be NULL).  The host does no decompression: it walks the
 * record framing and the PNG chunk headers and copies.  Only 8-bit RGB non-interlaced tiles of tile_px x tile_px pass
 * (BQIO_ERR_UNSUPPORTED / BQIO_ERR_FORMAT / BQIO_ERR_CORRUPT with *bad_index otherwise: decode that slide with bqio_decode).
 * *used = bytes written; a capacity `cap` that is too small returns BQIO_ERR_ARG with *used = the bytes needed. */
int bqio_extract_z(bqio_reader* r, int64_t first, int64_t count, int tile_px, uint8_t* out_z, size_t cap, uint32_t* off,
                   uint32_t* len, int64_t* loc, size_t* used, int n_threads, int64_t* bad_index);

/* The compressed side of baseline-JPEG tiles for the DEVICE decoder (libbiscuit_hip: bq_jpeg_decode), the JPEG counterpart of
 * bqio_extract_z.  For records [first, first + count) the host parses the markers -- the header walk of the host decoder
 * (csrc/jpeg_baseline.h: the same subset, the same refusals as bqio_probe) -- and copies every entropy-coded segment into
 * out_scan with the stuffed zero bytes removed: segment i at its offset (a multiple of 16), bqio_jpeg_ecs_pad() zero bytes behind
 * it.  desc[i] = four uint32: offset, length, hmax | vmax << 8 | components << 16 (4:4:4 / 4:2:2 / 4:2:0), index of the tile's
 * TABLE SET.  tables receives the call's distinct table sets (Huffman lookups and quantisers per component,
 * bqio_jpeg_table_bytes() each); the tiles of a slide normally share one, tiles with different sets may stand side by side.
 * Narrower than the host decoder in two places: grey (one-component) tiles and files with restart intervals are
 * BQIO_ERR_UNSUPPORTED here -- such a slide stays on bqio_decode.  Errors as bqio_extract_z (*bad_index = the record).
 * *used = bytes of out_scan, *n_tables = table sets needed; too small a `cap` or `table_cap`: BQIO_ERR_ARG with both set.
 * out_scan == NULL: nothing is copied, BQIO_OK with the two sizes (the once-per-slide check). */
int bqio_extract_jpeg(bqio_reader* r, int64_t first, int64_t count, int tile_px, uint8_t* out_scan, size_t cap, uint32_t* desc,
                      void* tables, int table_cap, int* n_tables, int64_t* loc, size_t* used, int n_threads, int64_t* bad_index);
size_t bqio_jpeg_table_bytes(void);
size_t bqio_jpeg_ecs_pad(void);
/* int16 coefficient space the decoder uses per tile of this size (the device decoder's scratch per tile). */
size_t bqio_jpeg_coef_bytes(int tile_px);

/* The device decoder's own routines (csrc/jpeg_device.h) run on the CPU over what bqio_extract_jpeg wrote: n tiles ->
 * out[n][tile_px][tile_px][3] and status[n] (0 = decoded; otherwise bits: 1 a code that does not exist, 2 a zero run past
 * coefficient 63, 4 data used from beyond the segment's end, 8 outside the range in which libjpeg's builds agree, 16 a
 * descriptor outside the subset; the tile's bytes are then not an image).  What bq_jpeg_decode computes, byte for byte and
 * status for status: for tests and the fuzzer. */
int bqio_jpeg_decode_extracted(const uint8_t* scan, const uint32_t* desc, const void* tables, int n_tables, int n, int tile_px,
                               uint8_t* out, int32_t* status, int n_threads);

/* A TIFF page's own JPEG tiles for the DEVICE decoder (libbiscuit_hip: bq_jpeg_decode_canvas; DESIGN.md "Heatmap input"):
 * bqio_extract_jpeg for n raw segments of one page instead of tile records -- segment i = data[off[i] .. off[i] + len[i]) (all
 * inside data_len bytes, or BQIO_ERR_ARG), every one a seg_w x seg_h frame (the page's TileWidth x TileLength, each <= 4096),
 * jpeg_tables = the page's JPEGTables tag (NULL / 0: none).  A segment is read as the stream a TIFF reader hands libjpeg: the
 * tables stream without its trailing EOI, then the segment without its leading SOI, so an abbreviated segment finds the
 * page's tables and a table the segment defines itself replaces the page's; without JPEGTables the segment must be a complete
 * stream.  The output -- out_scan, desc, tables, *used, *n_tables, the sizes-only probe with out_scan == NULL, BQIO_ERR_ARG for
 * too small a cap or table_cap -- is bqio_extract_jpeg's, and so are the refusals, the same header walk: BQIO_ERR_UNSUPPORTED
 * for anything but three components at 4:4:4 / 4:2:2 / 4:2:0 in one baseline scan, for restart intervals, for a stream
 * libjpeg would read as RGB or CMYK (by its markers; the TIFF photometric tag is not consulted) and for a scan that is not
 * clean; BQIO_ERR_FORMAT for a frame that is not seg_w x seg_h (a reader that crops larger frames keeps such a page on the
 * host).  *bad_index (may be NULL) = the first refused segment. */
int bqio_extract_jpeg_segments(const uint8_t* data, size_t data_len, const uint64_t* off, const uint64_t* len, int64_t n,
                               const uint8_t* jpeg_tables, size_t jpeg_tables_len, int seg_w, int seg_h, uint8_t* out_scan, size_t cap,
                               uint32_t* desc, void* tables, int table_cap, int* n_tables, size_t* used, int n_threads,
                               int64_t* bad_index);

/* The CPU restatement of bq_jpeg_decode_canvas over the same routines (csrc/jpeg_device.h: entropy_tile, idct_in_place,
 * place_window, pixel_rgb), the counterpart of bqio_jpeg_decode_extracted: n extracted seg_w x seg_h segments decoded INTO
 * canvas uint8 [H][W][3].  place int32 [n][2] = the canvas position (x, y) of each segment's top-left pixel, which may be
 * negative or beyond the canvas; clip int32 [4] = {x0, y0, x1, y1}, a rectangle in canvas coordinates.  Exactly the pixels of a
 * segment that lie inside both the canvas and the rectangle are written, every other byte of the canvas is left as it is
 * (the caller fills it beforehand: white, for a slide).  status[n] as bqio_jpeg_decode_extracted; a segment whose descriptor
 * is refused (16) writes nothing, any other non-zero status leaves bytes that are no image.  Segments must not overlap in the
 * canvas when n_threads > 1.  BQIO_ERR_ARG: seg_w / seg_h outside 1..4096, H / W outside 1..2^28, a NULL pointer.  For
 * tests, the sanitizer build and the fuzzer. */
int bqio_jpeg_decode_canvas(const uint8_t* scan, const uint32_t* desc, const void* tables, int n_tables, int n, int seg_w, int seg_h,
                            const int32_t* place, uint8_t* canvas, int H, int W, const int32_t* clip, int32_t* status, int n_threads);

/* ---- a TIFF page's JPEG 2000 tiles for the DEVICE decoder (libbiscuit_hip: bq_j2k_decode_canvas; csrc/j2k_host.cpp,
 * csrc/j2k_device.h; DESIGN.md "Heatmap input", JPEG 2000 tiles) ----
 * bqio_j2k_extract is tier 2 of the codec: segment i = data[off[i], off[i] + len[i]) (all inside data_len bytes, or
 * BQIO_ERR_ARG) is a raw codestream of seg_w x seg_h pixels.  Its main header, tile-part headers and packet headers are
 * walked; out come a descriptor per segment (seg_desc: n * bqio_j2k_seg_bytes() bytes: status, size, levels, transform, MCT
 * flag, half step sizes per sub-band, guard bits), a row per code block with at least one coding pass (blocks: rows of
 * bqio_j2k_block_bytes() bytes: segment, component, sub-band, rectangle in the component's plane, Mb, missing bit-planes,
 * passes, offset and length of its codeword) and the codewords (bytes: each 4-aligned, FF FF FF FF behind it).  The subset:
 * one tile, three 8-bit unsigned components without sub-sampling, code-block style 0, blocks up to 64 x 64, 0..6 levels, 5/3
 * without or 9/7 with scalar-expounded quantisation, no SOP / EPH / ROI / POC / PPM / PPT / COC / QCC, at most 512 x 512.  A
 * segment outside it, or damaged, has a non-zero status in its descriptor (32: outside the subset, 64: damaged) and no
 * blocks; the call still returns BQIO_OK.  *n_blocks and *n_bytes are always set; blocks == bytes == NULL: a probe that
 * writes the descriptors and the two sizes only; a cap that is too small: BQIO_ERR_ARG. */
size_t bqio_j2k_seg_bytes(void);
size_t bqio_j2k_block_bytes(void);
int bqio_j2k_extract(const uint8_t* data, size_t data_len, const uint64_t* off, const uint64_t* len, int64_t n, int seg_w, int seg_h,
                     int32_t* seg_desc, int32_t* blocks, int64_t blocks_cap, uint8_t* bytes, size_t bytes_cap, int64_t* n_blocks,
                     size_t* n_bytes, int n_threads);

/* The CPU statement of bq_j2k_decode_canvas over the same routines (csrc/j2k_device.h: t1_block, dequant_sample, synth_row /
 * synth_col, finish_pixel, place_window): what bqio_j2k_extract packed, decoded INTO canvas (uint8 [H][W][3]) at place[i] =
 * (x, y), inside clip = (x0, y0, x1, y1) only; ycc != 0: the samples are full-range YCbCr and are converted with Pillow's bytes
 * (csrc/j2k_ycc.h).  status[i] = 0, the descriptor's status, or 16 for a descriptor or block row that fails the decoder's own
 * checks; a segment whose status is not 0 writes nothing.  t1_out (NULL: none): int32 [n][3][seg_h][seg_w], tier 1's output in
 * the planes' sub-band layout -- signed quantiser indices times two, plus the half of the last decoded bit-plane.  For tests,
 * the sanitizer build and the fuzzer. */
int bqio_j2k_decode_canvas(const int32_t* seg_desc, int n, const int32_t* blocks, int64_t n_blocks, const uint8_t* bytes, size_t n_bytes,
                           int seg_w, int seg_h, int ycc, const int32_t* place, uint8_t* canvas, int H, int W, const int32_t* clip,
                           int32_t* status, int32_t* t1_out, int n_threads);

/* pixels full-range YCbCr triples -> RGB with the bytes of Pillow's convert('RGB') (csrc/j2k_ycc.h); in place allowed. */
void bqio_ycc_to_rgb(const uint8_t* ycc, uint8_t* rgb, size_t pixels);

/* ---- TIFF pages with LZW compression (csrc/lzw_host.cpp, csrc/lzw_device.h; DESIGN.md "Heatmap input", LZW tiles) ----
 * bqio_lzw_decode is the slide reader's segment decoder: raw[len], one strip or tile as libtiff writes it (TIFF 6.0 LZW: codes
 * MSB first, ClearCode 256 first, early change), -> out uint8 [rows][seg_w][3] with the predictor undone (predictor 1: none,
 * 2: horizontal differencing per sample modulo 256).  Returns 0 and the pixels libtiff gives, or a status > 0 -- bits: 1 the
 * first code is not ClearCode (old-style or damaged), 2 a code beyond the next free index, 4 the data ends or EndOfInformation
 * arrives before rows * seg_w * 3 bytes, 8 the table ran to its end (libtiff's: index 5119) without a ClearCode, 16 a stream
 * of more than 2^28 bytes -- after which out is no image; BQIO_ERR_ARG (< 0) for an argument outside rows <= 2^15, seg_w <=
 * 2^20, rows * seg_w * 3 <= 2^30, predictor 1 or 2. */
int bqio_lzw_decode(const uint8_t* raw, size_t len, int rows, int seg_w, int predictor, uint8_t* out);
/* The longest segment side bq_lzw_decode_canvas and bqio_lzw_decode_canvas take (1024). */
int bqio_lzw_max_side(void);
/* The CPU statement of bq_lzw_decode_canvas over the same routines: n segments of seg_w x seg_h (each <= 1024), segment i =
 * data[desc[2 i] .. + desc[2 i + 1]) with desc[2 i] a multiple of 16 (status 16 otherwise), decoded INTO canvas (uint8 [H][W][3])
 * at place[i] = (x, y), inside clip = (x0, y0, x1, y1) only.  status[i] as bqio_lzw_decode; a segment whose status is not 0
 * writes nothing.  What bq_lzw_decode_canvas computes, byte for byte and status for status.  For tests. */
int bqio_lzw_decode_canvas(const uint8_t* data, const uint32_t* desc, int n, int seg_w, int seg_h, int predictor, const int32_t* place,
                           uint8_t* canvas, int H, int W, const int32_t* clip, int32_t* status, int n_threads);

/* ---- tile resampling for the whole-slide heatmap (csrc/resample_host.cpp, csrc/resample_device.h) ----
 * The tap tables of Pillow's 8-bit resampler for Image.resize((px, px), Image.LANCZOS) of a src_px x src_px image: per output
 * coordinate i, bounds[2 i] = first source coordinate, bounds[2 i + 1] = number of taps, coef[i * ksize + j] = tap j with 22
 * fractional bits (zero behind the count).  Built as Pillow builds them: support 3, filterscale = max(src_px / px, 1), ksize =
 * 2 ceil(3 filterscale) + 1, the window clamped to the source, taps normalised by their sum in float64 and rounded away from
 * zero.  Supported: 0 < px <= 4096 and px / 8 <= src_px <= 8 px (ksize <= 49); anything else is BQIO_ERR_ARG and nothing is
 * written.  The tables serve both passes (a tile is square).  bqio_resample_ksize returns ksize; bqio_resample_taps fills
 * bounds [px][2] and coef [px][ksize] and returns ksize too (BQIO_ERR_ARG when ksize_cap < ksize; BQIO_ERR_UNSUPPORTED if
 * 2^21 + 255 * sum |tap| of a row did not fit 31 bits -- the 32-bit accumulators of both passes rest on it). */
int bqio_resample_ksize(int src_px, int px);
int bqio_resample_taps(int src_px, int px, int32_t* bounds, int32_t* coef, int ksize_cap);

/* The CPU restatement of bq_tile_resample, over the same per-pixel routines: n tiles cut from canvas uint8 [H][W][3] -- tile t
 * is the src_px x src_px window at (origin[2 t], origin[2 t + 1]) = (x, y), parts of it outside the canvas read as 255 -- each
 * resampled to out[t][px][px][3]: the horizontal pass rounded to bytes, then the vertical pass, the bytes Pillow gives.
 * src_px == px copies the window.  BQIO_ERR_ARG for a ratio outside the range above, px <= 0, n < 0, an empty canvas or an
 * origin beyond +-2^28; n = 0 returns BQIO_OK and touches nothing.  For tests and the sanitizer build. */
int bqio_tile_resample(const uint8_t* canvas, int H, int W, const int32_t* origin, int n, int src_px, int px, uint8_t* out);

/* The CPU build of bq_roi_plane (include/biscuit_hip.h; csrc/roi_host.cpp over csrc/roi_device.h, the crossing rule and the table
 * checks the GPU entry is compiled from): plane[y][x] (uint8 [H][W]) = 1 iff the doubled sample point (xs[x], ys[y]) is inside any
 * polygon of the edge table -- edges int32 [E][4] = (a.x, a.y, b.x, b.y) doubled, starts int32 [P + 1] -- even-odd per polygon,
 * union across polygons.  BQIO_ERR_ARG, with the plane untouched, for what bq_roi_plane refuses: W or H <= 0, H * W >= 2^31, E
 * outside 3 .. 2^20, starts that do not run from 0 to E in steps of at least 3, an edge coordinate outside [-2^28, 2^28], a
 * sample coordinate outside [0, 2^29], a null pointer.  For tests. */
int bqio_roi_plane(const int32_t* edges, int E, const int32_t* starts, int P, const int32_t* xs, int W, const int32_t* ys, int H,
                   uint8_t* plane);

/* The CPU build of bq_jpeg_encode (include/biscuit_hip.h; csrc/jpeg_encode_host.cpp over csrc/jpeg_encode_device.h, the routines
 * the GPU kernels are compiled from): n tiles uint8 [n][px][px][3] -> the complete baseline-JPEG files Pillow writes for
 * `save(buf, 'JPEG', quality=quality, subsampling=subsampling)` with everything else at its default, byte for byte, back to back
 * in `out`: file i = out[off[i] .. off[i + 1]), off int64 [n + 1] with off[0] = 0.  subsampling: 0 = 4:4:4, 2 = 4:2:0 (Pillow's
 * numbering).  A file that would end beyond `cap` is not written and status[i] = 1 (0 otherwise); off still holds the exact
 * lengths, so cap = 0 with out = NULL sizes a call.  BQIO_ERR_ARG, with nothing written, outside the subset -- px in 1..4096,
 * quality in 1..100, the two samplings -- or for a null pointer; bqio_jpeg_encode_last_error() then says which.
 * bqio_jpeg_encode_header writes the bqio_jpeg_encode_header_bytes() (623) bytes from SOI through the SOS header, which depend
 * on (px, quality, subsampling) only.  For tests. */
int bqio_jpeg_encode(const uint8_t* tiles, int64_t n, int px, int quality, int subsampling, uint8_t* out, size_t cap, int64_t* off,
                     int32_t* status);
int bqio_jpeg_encode_header(int px, int quality, int subsampling, uint8_t* out);
size_t bqio_jpeg_encode_header_bytes(void);
const char* bqio_jpeg_encode_last_error(void);

/* The CPU build of bq_png_encode (include/biscuit_hip.h; csrc/png_encode_host.cpp over csrc/png_encode_device.h, the routines the
 * GPU kernels are compiled from): n tiles uint8 [n][px][px][3] -> complete PNG files (signature, IHDR 8-bit colour type 2, IDAT
 * chunks of 8 192 zlib bytes, IEND), back to back in `out`: file i = out[off[i] .. off[i + 1]), off int64 [n + 1] with off[0] =
 * 0.  The filtered rows are Pillow's byte for byte; the deflate stream is this project's (blocks of 16 384 input bytes, greedy
 * hash matching in groups of 64, per-block dynamic / fixed / stored) and is what bq_png_encode writes, byte for byte.  There is no
 * quality: a tile has one encoding.  A file that would end beyond `cap` is not written and status[i] = 1 (0 otherwise); off still
 * holds the exact lengths, so cap = 0 with out = NULL sizes a call.  BQIO_ERR_ARG, with nothing written, for px outside 1..4096 or
 * a null pointer; bqio_png_encode_last_error() then says which.  For tests. */
int bqio_png_encode(const uint8_t* tiles, int64_t n, int px, uint8_t* out, size_t cap, int64_t* off, int32_t* status);
const char* bqio_png_encode_last_error(void);

/* The CPU build of bq_augment (include/biscuit_hip.h; csrc/augment_host.cpp over csrc/augment_device.h, the routines the GPU
 * kernels are compiled from): Slideflow's training augmentation 'xyrjb' with the random draws made by the caller.  n tiles uint8
 * [n][px][px][3], 8 <= px <= 4096, and params uint8 [n][4] = (k, flips, quality, blur) per tile ->
 *     out[i] = blur_s( flip_ud^(flips >> 1 & 1)( flip_lr^(flips & 1)( rot90^k( jpeg_q(tiles[i]) ))))
 * jpeg_q: quality 0 the tile itself, 1..100 the pixels Pillow returns for Image.open(save(tile, 'JPEG', quality=q, subsampling=
 * '4:2:0')), byte for byte (the encoder's coefficients, dequantised, through the decoder's IDCT, upsampling and colour stage: no
 * bitstream).  rot90^k: numpy.rot90(x, k), k 0..3; flips bit 0: x[:, ::-1], bit 1: x[::-1].  blur_s: blur 0 the identity, 1..4 a
 * separable Gaussian of sigma = 0.5 blur in integers (radius int(3 sigma + 0.5), weights that sum to 65536, mirror padding, a
 * uint16 row pass with 8 fractional bits, one rounding per pass): within one level of the rounded float64 filter.  status[i] =
 * 0, or 1 where a block of the round trip left the range in which libjpeg's builds agree (its samples are clamped).  `out`
 * must not overlap `tiles`.  Tiles are shared among `threads` host threads (1..64).  BQIO_ERR_ARG, with nothing written, for px or
 * a parameter byte out of range, n < 0, a null pointer or overlapping buffers; bqio_augment_last_error() then says which.
 * bqio_augment_blur_weights writes the 2 r + 1 weights of blur index 1..4 (uint16, 13 entries, zero behind the last) and returns
 * the radius r.  For tests and as the device entry's timing baseline. */
int bqio_augment(const uint8_t* tiles, int64_t n, int px, const uint8_t* params, uint8_t* out, int32_t* status, int threads);
int bqio_augment_blur_weights(int blur, uint16_t* out);
const char* bqio_augment_last_error(void);

/* One JPEG file (as bqio_image_bytes returns it) -> out[tile_px][tile_px][3], the decoder
 * bqio_decode uses, exported for tests.  BQIO_OK / BQIO_ERR_UNSUPPORTED / BQIO_ERR_FORMAT. */
int bqio_decode_jpeg(const uint8_t* data, size_t len, int tile_px, uint8_t* out);

/* masked CRC-32C of a buffer (the TFRecord checksum), exported for tests and writers. */
uint32_t bqio_masked_crc32c(const uint8_t* data, size_t len);

/* The reader's own zlib-stream decompressor (csrc/inflate_fast.h), exported for tests: inflates `n` bytes at zdata into
 * exactly out_len bytes at out.  BQIO_OK, or BQIO_ERR_CORRUPT for anything zlib's uncompress() would refuse (bad header,
 * invalid or over-subscribed codes, a distance before the start, wrong length, Adler-32 mismatch, trailing bytes). */
int bqio_inflate(const uint8_t* zdata, size_t n, uint8_t* out, size_t out_len);

/* The same for two streams decoded in one loop (what bqio_decode does with pairs of tiles): *ok_a / *ok_b = 1 where
 * bqio_inflate would have returned BQIO_OK.  Returns BQIO_OK unless an argument is bad. */
int bqio_inflate2(const uint8_t* za, size_t na, uint8_t* out_a, size_t len_a, const uint8_t* zb, size_t nb, uint8_t* out_b,
                  size_t len_b, int* ok_a, int* ok_b);

/* How many PNG streams bqio_decode handed to zlib after the decompressor above refused them and zlib accepted them
 * (process-wide).  Always 0 unless that decompressor has a bug; the tests assert it. */
int64_t bqio_inflate_fallbacks(void);

/* ---- The output side: the tile-prediction table -------------------------------------------------------------------------
 * Replaces the `DataFrame.to_csv(index=False)` with which Slideflow's `Project.evaluate(..., save_predictions=True)`
 * (experiment.py:917-922) leaves `tile_predictions_eval.csv`, the file biscuit reads back with
 * `pd.read_csv(path, dtype={'slide': str})` (experiment.py:688-699; validation: `tile_predictions_val_epoch1.csv`,
 * experiment.py:982-988, utils.py:216) and renames by the column contract of utils.py:19-53.  Rows are appended while the GPU
 * works (one call per run of tiles of one slide), in the bytes pandas would write: float64 cells as the shortest string that
 * reads back to the same double, laid out as Python's repr(float); NaN = empty cell; slide names quoted only when they must be. */
typedef struct bqio_table bqio_table;

/* Create (append = 0: truncate and write the header line
 *     slide[,loc_x,loc_y],{outcome}-y_true0,{outcome}-y_pred0,{outcome}-y_pred1,{outcome}-uncertainty0,{outcome}-uncertainty1)
 * or extend (append = 1: no header) the table at `path`.  NULL on failure; bqio_table_last_error(NULL) says why. */
bqio_table* bqio_table_open(const char* path, const char* outcome, int with_loc, int append);
const char* bqio_table_last_error(bqio_table* t);

/* Append `count` rows of ONE slide: mean2 / std2 = float32 [count][2] (the MC mean and population std of the two class
 * probabilities, widened to float64 exactly as the in-memory table holds them), loc = int64 [count][2] (loc_x, loc_y) exactly
 * when the table was opened with_loc.  A NaN in mean2 returns BQIO_ERR_NAN and writes nothing of this call (threshold.py:141-142
 * refuses such a table: the Python wrapper raises PredsContainNaNError). */
int bqio_table_rows(bqio_table* t, const char* slide, int64_t y_true, const int64_t* loc, const float* mean2, const float* std2,
                    int64_t count);

/* Bytes of the table so far (written or buffered): a rank notes it per slide, so that the per-rank shards of a multi-rank run
 * can be spliced into ONE table in dataset order without parsing them. */
int64_t bqio_table_tell(bqio_table* t);

/* Append bytes [offset, offset + length) of the file at src_path (a slide's rows in another rank's shard). */
int bqio_table_append_file(bqio_table* t, const char* src_path, int64_t offset, int64_t length);

/* Flush and close; *rows / *bytes (may be NULL) = what bqio_table_rows wrote / the file's size increase.  Frees t. */
int bqio_table_close(bqio_table* t, int64_t* rows, int64_t* bytes);

/* repr(float) of one double into out (NUL-terminated), exported for tests.  Returns its length or BQIO_ERR_ARG. */
int bqio_format_f64(double v, char* out, int cap);

/* The CPU builds of the feature map's three entries (include/biscuit_hip.h: bq_knn, bq_umap_smooth, bq_umap_epoch;
 * csrc/umap_host.cpp over csrc/umap_device.h, the per-row arithmetic the GPU kernels are compiled from), on host memory with the
 * same shapes and types.  bqio_knn ranks all n rows by the direct form sum (x - y)^2 -- no pruning pass --, and is what the
 * device returns on every row, bit for bit.  X must be finite: BQIO_ERR_ARG otherwise.  A pair whose fp32 sum overflows is no
 * candidate; a row with fewer than k candidates ends in idx -1, dist NaN.  bqio_knn_gemm_bound: out[e] = the worst-case bound
 * E(nq[e], nc[e], D) on |GEMM-form value - exact squared distance| that bq_knn's certificate uses (csrc/umap_device.h:
 * gemm_form_err), nq and nc the two rows' fp32 sums of squares, `count` pairs.  bqio_umap_epoch checks the CSR (indptr from 0 and non-decreasing, neighbours in
 * 0 .. n - 1).  BQIO_ERR_ARG for what the GPU entries refuse.  For tests. */
int bqio_knn_gemm_bound(const float* nq, const float* nc, int64_t count, int D, float* out);
int bqio_knn(const float* X, int n, int D, int k, int32_t* idx, float* dist);
int bqio_umap_smooth(const int32_t* idx, const float* dist, int n, int k, float* rho, float* sigma, float* w);
int bqio_umap_epoch(const float* prev, float* out, int n, const int64_t* indptr, const int32_t* nbr, const float* eps, float* next,
                    int epoch, float alpha, float a, float b, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
