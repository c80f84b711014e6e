"""ctypes binding of libbiscuit_io.so (include/biscuit_io.h): the native TFRecord / PNG reader.

`NativeReader(path)` indexes one slide's TFRecord; `decode(first, count)` returns uint8 tiles
``[count, px, px, 3]`` decoded by a pool of host threads, optionally straight into a caller-supplied
(e.g. pinned) buffer so the H2D copy of one batch overlaps the decode of the next.  PNG and baseline JPEG
payloads are decoded natively; for anything else (progressive JPEG, a damaged stream) `decode` raises
`UnsupportedImage` and the caller (tfrecord.read_slide) decodes the slide with Pillow.
"""
import ctypes as C
import os

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libbiscuit_io.so')

VERIFY = {None: 0, False: 0, 'none': 0, 'length': 1, 'full': 2}
IMG_PNG, IMG_JPEG = 1, 2
ERR_UNSUPPORTED = -5
ERR_FORMAT = -3

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
ABI = {
    'bqio_open': (_vp, [C.c_char_p, _i]),
    'bqio_close': (None, [_vp]),
    'bqio_last_error': (C.c_char_p, [_vp]),
    'bqio_count': (_i64, [_vp]),
    'bqio_slide_name': (_i, [_vp, C.c_char_p, _i]),
    'bqio_image_format': (_i, [_vp, _i64]),
    'bqio_image_bytes': (_i, [_vp, _i64, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]),
    'bqio_decode': (_i, [_vp, _i64, _i64, _i, _vp, _vp, _i, C.POINTER(_i64)]),
    'bqio_decode_rows': (_i, [_vp, _i64, _i64, _i, _vp, _vp, _i, C.POINTER(_i64)]),
    'bqio_probe': (_i, [_vp, _i64, _i64, _i, C.POINTER(_i64)]),
    'bqio_extract_z': (_i, [_vp, _i64, _i64, _i, _vp, C.c_size_t, _vp, _vp, _vp, C.POINTER(C.c_size_t), _i, C.POINTER(_i64)]),
    'bqio_extract_jpeg': (_i, [_vp, _i64, _i64, _i, _vp, C.c_size_t, _vp, _vp, _i, C.POINTER(_i), _vp, C.POINTER(C.c_size_t), _i,
                               C.POINTER(_i64)]),
    'bqio_jpeg_table_bytes': (C.c_size_t, []),
    'bqio_jpeg_ecs_pad': (C.c_size_t, []),
    'bqio_jpeg_coef_bytes': (C.c_size_t, [_i]),
    'bqio_jpeg_decode_extracted': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i]),
    'bqio_extract_jpeg_segments': (_i, [_vp, C.c_size_t, _vp, _vp, _i64, _vp, C.c_size_t, _i, _i, _vp, C.c_size_t, _vp, _vp, _i,
                                        C.POINTER(_i), C.POINTER(C.c_size_t), _i, C.POINTER(_i64)]),
    'bqio_jpeg_decode_canvas': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i]),
    'bqio_j2k_seg_bytes': (C.c_size_t, []),
    'bqio_j2k_block_bytes': (C.c_size_t, []),
    'bqio_j2k_extract': (_i, [_vp, C.c_size_t, _vp, _vp, _i64, _i, _i, _vp, _vp, _i64, _vp, C.c_size_t, C.POINTER(_i64),
                              C.POINTER(C.c_size_t), _i]),
    'bqio_j2k_decode_canvas': (_i, [_vp, _i, _vp, _i64, _vp, C.c_size_t, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i]),
    'bqio_ycc_to_rgb': (None, [_vp, _vp, C.c_size_t]),
    'bqio_lzw_decode': (_i, [_vp, C.c_size_t, _i, _i, _i, _vp]),
    'bqio_lzw_max_side': (_i, []),
    'bqio_lzw_decode_canvas': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i]),
    'bqio_resample_ksize': (_i, [_i, _i]),
    'bqio_resample_taps': (_i, [_i, _i, _vp, _vp, _i]),
    'bqio_tile_resample': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp]),
    'bqio_roi_plane': (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp]),
    'bqio_jpeg_encode': (_i, [_vp, _i64, _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
    'bqio_jpeg_encode_header': (_i, [_i, _i, _i, _vp]),
    'bqio_jpeg_encode_header_bytes': (C.c_size_t, []),
    'bqio_jpeg_encode_last_error': (C.c_char_p, []),
    'bqio_png_encode': (_i, [_vp, _i64, _i, _vp, C.c_size_t, _vp, _vp]),
    'bqio_png_encode_last_error': (C.c_char_p, []),
    'bqio_augment': (_i, [_vp, _i64, _i, _vp, _vp, _vp, _i]),
    'bqio_augment_blur_weights': (_i, [_i, _vp]),
    'bqio_augment_last_error': (C.c_char_p, []),
    'bqio_masked_crc32c': (C.c_uint32, [C.c_char_p, C.c_size_t]),
    'bqio_inflate': (_i, [C.c_char_p, C.c_size_t, _vp, C.c_size_t]),
    'bqio_inflate2': (_i, [C.c_char_p, C.c_size_t, _vp, C.c_size_t, C.c_char_p, C.c_size_t, _vp, C.c_size_t,
                          C.POINTER(_i), C.POINTER(_i)]),
    'bqio_inflate_fallbacks': (_i64, []),
    'bqio_decode_jpeg': (_i, [C.c_char_p, C.c_size_t, _i, _vp]),
    # the output side: the tile-prediction table (biscuit_amd/predictions.py)
    'bqio_table_open': (_vp, [C.c_char_p, C.c_char_p, _i, _i]),
    'bqio_table_last_error': (C.c_char_p, [_vp]),
    'bqio_table_rows': (_i, [_vp, C.c_char_p, _i64, _vp, _vp, _vp, _i64]),
    'bqio_table_tell': (_i64, [_vp]),
    'bqio_table_append_file': (_i, [_vp, C.c_char_p, _i64, _i64]),
    'bqio_table_close': (_i, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    'bqio_format_f64': (_i, [C.c_double, C.c_char_p, _i]),
    # the CPU builds of the feature map's entries (biscuit_amd/umap.py)
    'bqio_knn': (_i, [_vp, _i, _i, _i, _vp, _vp]),
    'bqio_knn_gemm_bound': (_i, [_vp, _vp, _i64, _i, _vp]),
    'bqio_umap_smooth': (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    'bqio_umap_epoch': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, C.c_float, C.c_float, C.c_float, C.c_uint64]),
}


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(f'{path} not found; build it with `make -C biscuit_amd/csrc`')
    lib = C.CDLL(path)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load()
    return _lib


def available():
    return os.path.exists(LIB_PATH)


def inflate(zdata, out_len):
    """The reader's own zlib-stream decompressor (csrc/inflate_fast.h): ``zlib.decompress(zdata)`` when that has exactly
    ``out_len`` bytes, ValueError for anything zlib would refuse.  For tests."""
    import numpy as np
    out = np.empty(out_len, np.uint8)
    e = lib().bqio_inflate(bytes(zdata), len(zdata), out.ctypes.data, out_len)
    if e != 0:
        raise ValueError(f'bqio_inflate: error {e}')
    return out.tobytes()


def inflate2(za, len_a, zb, len_b):
    """Two zlib streams through the reader's two-stream loop: (bytes | None, bytes | None), None where ``inflate`` would
    raise.  For tests."""
    import numpy as np
    oa, ob = np.empty(len_a, np.uint8), np.empty(len_b, np.uint8)
    ka, kb = C.c_int(0), C.c_int(0)
    e = lib().bqio_inflate2(bytes(za), len(za), oa.ctypes.data, len_a, bytes(zb), len(zb), ob.ctypes.data, len_b,
                            C.byref(ka), C.byref(kb))
    if e != 0:
        raise ValueError(f'bqio_inflate2: error {e}')
    return (oa.tobytes() if ka.value else None), (ob.tobytes() if kb.value else None)


def decode_jpeg(raw, tile_px=299):
    """One JPEG file's bytes -> uint8 [px,px,3] through the reader's own baseline decoder (csrc/jpeg_baseline.h);
    UnsupportedImage for streams outside its subset, ValueError for a tile of another size.  For tests."""
    out = np.empty((tile_px, tile_px, 3), np.uint8)
    e = lib().bqio_decode_jpeg(bytes(raw), len(raw), tile_px, out.ctypes.data)
    if e == ERR_UNSUPPORTED:
        raise UnsupportedImage(0)
    if e != 0:
        raise ValueError(f'bqio_decode_jpeg: error {e}')
    return out


def jpeg_table_bytes():
    """Bytes of one table set of ``NativeReader.extract_jpeg`` (the Huffman lookups and quantisers of a tile's three components)."""
    return int(lib().bqio_jpeg_table_bytes())


def jpeg_decode_extracted(scan, desc, tables, px=299, threads=None):
    """The device JPEG decoder's routines (csrc/jpeg_device.h) on the CPU, over what ``NativeReader.extract_jpeg`` wrote:
    -> (tiles uint8 [n,px,px,3], status int32 [n]); a tile whose status is not 0 was refused and its bytes are no image.
    What ``Engine.jpeg_decode`` computes, byte for byte and status for status.  For tests."""
    scan, desc, tables = np.ascontiguousarray(scan, np.uint8), np.ascontiguousarray(desc, np.uint32), np.ascontiguousarray(tables, np.uint8)
    n = desc.shape[0]
    assert desc.shape == (n, 4) and tables.size % jpeg_table_bytes() == 0
    out = np.zeros((n, px, px, 3), np.uint8)
    status = np.zeros(n, np.int32)
    e = lib().bqio_jpeg_decode_extracted(scan.ctypes.data, desc.ctypes.data, tables.ctypes.data, tables.size // jpeg_table_bytes(), n, px,
                                         out.ctypes.data, status.ctypes.data, threads or default_threads())
    if e != 0:
        raise ValueError(f'bqio_jpeg_decode_extracted: error {e}')
    return out, status


def extract_jpeg_segments(data, offsets, lengths, seg_w, seg_h, jpeg_tables=None, threads=None, probe=False):
    """A TIFF page's raw JPEG segments packed for the device decoder (``bqio_extract_jpeg_segments``): ``data`` uint8 [bytes],
    segment i = ``data[offsets[i]:offsets[i] + lengths[i]]``, every one a ``seg_w`` x ``seg_h`` frame, ``jpeg_tables`` the page's
    ``JPEGTables`` bytes or None -> ``(scan uint8 [bytes], desc uint32 [n, 4], tables uint8 [k, jpeg_table_bytes()])`` as
    ``NativeReader.extract_jpeg`` fills them (``probe=True``: only ``(bytes of scan, k)``, nothing packed).  Raises
    ``UnsupportedImage`` (``.index`` = the first refused segment) for a stream outside the device decoder's subset -- not three
    components at 4:4:4 / 4:2:2 / 4:2:0, restart intervals, RGB / CMYK coded, progressive, damaged -- and ``ValueError`` for a
    frame of another size."""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1)
    off, ln = np.ascontiguousarray(offsets, np.uint64).reshape(-1), np.ascontiguousarray(lengths, np.uint64).reshape(-1)
    n = len(off)
    assert len(ln) == n
    jt = np.frombuffer(bytes(jpeg_tables or b''), np.uint8)
    tb = jpeg_table_bytes()
    # a segment's entropy-coded bytes only shrink when the stuffed zeros go: the packed size is bounded beforehand
    pad, cap_t = int(lib().bqio_jpeg_ecs_pad()), 8
    cap = 0 if probe else int(((ln.astype(np.int64) + pad + 31) // 16 * 16).sum()) + 16
    while True:
        scan = None if probe else np.empty(cap, np.uint8)
        desc = np.empty((n, 4), np.uint32)
        tables = np.empty((cap_t, tb), np.uint8)
        nt, used, bad = C.c_int(0), C.c_size_t(0), C.c_int64(-1)
        e = lib().bqio_extract_jpeg_segments(data.ctypes.data, data.size, off.ctypes.data, ln.ctypes.data, n,
                                             jt.ctypes.data if jt.size else None, jt.size, int(seg_w), int(seg_h),
                                             None if probe else scan.ctypes.data, cap, desc.ctypes.data, tables.ctypes.data, cap_t,
                                             C.byref(nt), C.byref(used), threads or default_threads(), C.byref(bad))
        if e == ERR_UNSUPPORTED:
            raise UnsupportedImage(int(bad.value))
        if e == ERR_FORMAT:
            err = ValueError(f'segment {bad.value}: frame size differs from {seg_w} x {seg_h}')
            err.index = int(bad.value)
            raise err
        if e == -1 and not probe and nt.value > cap_t and used.value <= cap:      # more table sets than guessed: once more
            cap_t = nt.value
            continue
        if e != 0:
            raise ValueError(f'bqio_extract_jpeg_segments: error {e}')
        if probe:
            return int(used.value), int(nt.value)
        return scan[:used.value], desc, tables[:nt.value].copy()


def _canvas_arrays(n, place, canvas, clip):
    """What the CPU canvas decoders take alike -> ``(place int32 [n, 2], clip int32 [4], status int32 [n] of zeros)``."""
    place = np.ascontiguousarray(place, np.int32).reshape(-1, 2)
    clip = np.ascontiguousarray(clip, np.int32).reshape(4)
    assert place.shape == (n, 2)
    assert canvas.dtype == np.uint8 and canvas.ndim == 3 and canvas.shape[2] == 3 and canvas.flags.c_contiguous and canvas.flags.writeable
    return place, clip, np.zeros(n, np.int32)


def jpeg_decode_canvas(scan, desc, tables, seg_w, seg_h, place, canvas, clip, threads=None):
    """The device canvas decoder's routines (csrc/jpeg_device.h) on the CPU (``bqio_jpeg_decode_canvas``): the segments
    ``extract_jpeg_segments`` packed, written INTO ``canvas`` (uint8 [H, W, 3], C-contiguous, modified in place) at ``place`` int32
    [n, 2] (x, y), clipped to ``clip`` = (x0, y0, x1, y1) in canvas coordinates.  -> status int32 [n].  What
    ``Engine.jpeg_decode_canvas`` computes, byte for byte and status for status.  For tests."""
    scan, desc, tables = np.ascontiguousarray(scan, np.uint8), np.ascontiguousarray(desc, np.uint32), np.ascontiguousarray(tables, np.uint8)
    n = desc.shape[0]
    assert desc.shape == (n, 4) and tables.size % jpeg_table_bytes() == 0
    place, clip, status = _canvas_arrays(n, place, canvas, clip)
    e = lib().bqio_jpeg_decode_canvas(scan.ctypes.data, desc.ctypes.data, tables.ctypes.data, tables.size // jpeg_table_bytes(), n,
                                      int(seg_w), int(seg_h), place.ctypes.data, canvas.ctypes.data, canvas.shape[0], canvas.shape[1],
                                      clip.ctypes.data, status.ctypes.data, threads or default_threads())
    if e != 0:
        raise ValueError(f'bqio_jpeg_decode_canvas: error {e}')
    return status


J2K_SUBSET, J2K_DAMAGED = 32, 64        # a segment's status from ``j2k_extract`` (csrc/j2k_device.h); 16: refused by the decoder
J2K_MAX_SIDE = 512                      # the longest segment side the JPEG 2000 decoder takes (MAX_SIDE of csrc/j2k_device.h)


def j2k_extract(data, offsets, lengths, seg_w, seg_h, threads=None, strict=True):
    """A TIFF page's raw JPEG 2000 segments packed for the device decoder (``bqio_j2k_extract``, tier 2 of the codec): ``data``
    uint8 [bytes], segment i = ``data[offsets[i]:offsets[i] + lengths[i]]``, every one a codestream of ``seg_w`` x ``seg_h``
    pixels -> ``(desc int32 [n, 32], blocks int32 [k, 12], cw uint8 [bytes])``: a descriptor per segment (``desc[:, 0]`` its
    status), a row per code block and the blocks' codewords.  ``strict``: raise ``UnsupportedImage`` (``.index`` = the first
    such segment) when a segment is outside the device decoder's subset or damaged; otherwise such a segment keeps its status
    (``J2K_SUBSET`` / ``J2K_DAMAGED``), has no blocks, and the decoder writes nothing for it."""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1)
    off, ln = np.ascontiguousarray(offsets, np.uint64).reshape(-1), np.ascontiguousarray(lengths, np.uint64).reshape(-1)
    n = len(off)
    assert len(ln) == n and lib().bqio_j2k_seg_bytes() == 128 and lib().bqio_j2k_block_bytes() == 48
    desc = np.zeros((n, 32), np.int32)
    nb, used = C.c_int64(0), C.c_size_t(0)
    # one call parses and fills: room for the rows of 32 x 32 blocks and some, and for the codewords, which are the segments' own
    # bytes plus at most 7 of padding a block; smaller blocks than guessed: once more, with the sizes the first call stated
    cap_b = n * 3 * (-(-int(seg_w) // 32) * -(-int(seg_h) // 32) + 40)
    cap_c = int(ln.sum()) + 8 * cap_b
    while True:
        blocks, cw = np.empty((cap_b, 12), np.int32), np.empty(cap_c, np.uint8)
        e = lib().bqio_j2k_extract(data.ctypes.data, data.size, off.ctypes.data, ln.ctypes.data, n, int(seg_w), int(seg_h),
                                   desc.ctypes.data, blocks.ctypes.data, cap_b, cw.ctypes.data, cap_c, C.byref(nb), C.byref(used),
                                   threads or default_threads())
        if e == -1 and (nb.value > cap_b or used.value > cap_c):
            cap_b, cap_c = max(cap_b, nb.value), max(cap_c, used.value)
            continue
        if e != 0:
            raise ValueError(f'bqio_j2k_extract: error {e}')
        break
    bad = np.flatnonzero(desc[:, 0])
    if strict and len(bad):
        raise UnsupportedImage(int(bad[0]))
    blocks, cw = blocks[:nb.value], cw[:used.value]
    return desc, blocks, cw


def j2k_decode_canvas(desc, blocks, cw, seg_w, seg_h, place, canvas, clip, ycc=False, threads=None, t1=False):
    """The device JPEG 2000 decoder's routines (csrc/j2k_device.h) on the CPU (``bqio_j2k_decode_canvas``): the segments
    ``j2k_extract`` packed, written INTO ``canvas`` (uint8 [H, W, 3], C-contiguous, modified in place) at ``place`` int32 [n, 2]
    (x, y), clipped to ``clip`` = (x0, y0, x1, y1); ``ycc``: the samples are YCbCr (TIFF compression 33003) and are converted.
    -> status int32 [n] (``t1=True``: ``(status, int32 [n, 3, seg_h, seg_w])`` with tier 1's output, doubled quantiser indices
    in sub-band layout).  What ``Engine.j2k_decode_canvas`` computes, byte for byte and status for status.  For tests."""
    desc, blocks = np.ascontiguousarray(desc, np.int32), np.ascontiguousarray(blocks, np.int32).reshape(-1, 12)
    cw = np.ascontiguousarray(cw, np.uint8)
    n = desc.shape[0]
    assert desc.shape == (n, 32)
    place, clip, status = _canvas_arrays(n, place, canvas, clip)
    planes = np.zeros((n, 3, int(seg_h), int(seg_w)), np.int32) if t1 else None
    e = lib().bqio_j2k_decode_canvas(desc.ctypes.data, n, blocks.ctypes.data, len(blocks), cw.ctypes.data, cw.size, int(seg_w), int(seg_h),
                                     int(bool(ycc)), place.ctypes.data, canvas.ctypes.data, canvas.shape[0], canvas.shape[1],
                                     clip.ctypes.data, status.ctypes.data, planes.ctypes.data if t1 else None,
                                     threads or default_threads())
    if e != 0:
        raise ValueError(f'bqio_j2k_decode_canvas: error {e}')
    return (status, planes) if t1 else status


def ycc_to_rgb(a):
    """uint8 [..., 3] full-range YCbCr -> RGB with the bytes of Pillow's ``convert('RGB')`` (csrc/j2k_ycc.h)."""
    a = np.ascontiguousarray(a, np.uint8)
    assert a.shape[-1] == 3
    out = np.empty_like(a)
    lib().bqio_ycc_to_rgb(a.ctypes.data, out.ctypes.data, a.size // 3)
    return out


# a segment's status from the LZW decoders, bits (csrc/lzw_device.h): the first code is not ClearCode; a code beyond the next free
# index; the data or EndOfInformation before the segment is full; the table at its end without a ClearCode; a refused descriptor
LZW_HEAD, LZW_CODE, LZW_SHORT, LZW_FULL, LZW_DESC = 1, 2, 4, 8, 16
LZW_MAX_SIDE = 1024                     # the longest segment side the device LZW decoder takes (MAX_SIDE of csrc/lzw_device.h)


def lzw_decode(raw, rows, seg_w, predictor=1):
    """One TIFF LZW strip or tile -> ``(pixels uint8 [rows, seg_w, 3], status)`` through ``bqio_lzw_decode``: the bytes libtiff
    gives with ``predictor`` (1 or 2) undone and status 0, or a status of ``LZW_*`` bits and no image."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    out = np.empty((int(rows), int(seg_w), 3), np.uint8)
    st = lib().bqio_lzw_decode(raw.ctypes.data if raw.size else None, raw.size, int(rows), int(seg_w), int(predictor), out.ctypes.data)
    if st < 0:
        raise ValueError(f'bqio_lzw_decode: error {st}')
    return out, int(st)


def lzw_pack(data, offsets, lengths):
    """A TIFF page's raw LZW segments packed for the device decoder, in numpy -- nothing is parsed: segment i =
    ``data[offsets[i]:offsets[i] + lengths[i]]`` -> ``(packed uint8 [bytes], desc uint32 [n, 2] of (offset, length))``, every
    segment at a multiple of 16 with zeros behind it.  ``ValueError`` for a band whose packed bytes do not fit 32-bit offsets."""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1)
    off, ln = np.ascontiguousarray(offsets, np.uint64).reshape(-1).astype(np.int64), np.ascontiguousarray(lengths, np.uint64).reshape(-1).astype(np.int64)
    assert len(off) == len(ln) and (len(ln) == 0 or (off.min() >= 0 and ln.min() >= 0 and int((off + ln).max()) <= data.size))
    room = (ln + 15 + 16) // 16 * 16                                          # at least 16 zero bytes behind every segment
    at = np.zeros(len(ln), np.int64)
    at[1:] = np.cumsum(room)[:-1]
    total = int(room.sum())
    if total >= 1 << 32 or (len(ln) and int(ln.max()) > 1 << 28):
        raise ValueError(f'an LZW band of {total} packed bytes does not fit the device decoder\'s 32-bit offsets')
    packed = np.zeros(total, np.uint8)
    for a, o, k in zip(at, off, ln):
        packed[a:a + k] = data[o:o + k]
    return packed, np.stack([at, ln], 1).astype(np.uint32).reshape(-1, 2)


def lzw_decode_canvas(packed, desc, seg_w, seg_h, place, canvas, clip, predictor=1, threads=None):
    """The device LZW decoder's routines (csrc/lzw_device.h) on the CPU (``bqio_lzw_decode_canvas``): the segments ``lzw_pack``
    packed, written INTO ``canvas`` (uint8 [H, W, 3], C-contiguous, modified in place) at ``place`` int32 [n, 2] (x, y), clipped
    to ``clip`` = (x0, y0, x1, y1).  -> status int32 [n].  What ``Engine.lzw_decode_canvas`` computes, byte for byte and status
    for status.  For tests."""
    packed, desc = np.ascontiguousarray(packed, np.uint8), np.ascontiguousarray(desc, np.uint32).reshape(-1, 2)
    n = desc.shape[0]
    assert n == 0 or int((desc[:, 0].astype(np.int64) + desc[:, 1]).max()) <= packed.size
    place, clip, status = _canvas_arrays(n, place, canvas, clip)
    e = lib().bqio_lzw_decode_canvas(packed.ctypes.data, desc.ctypes.data, n, int(seg_w), int(seg_h), int(predictor), place.ctypes.data,
                                     canvas.ctypes.data, canvas.shape[0], canvas.shape[1], clip.ctypes.data, status.ctypes.data,
                                     threads or default_threads())
    if e != 0:
        raise ValueError(f'bqio_lzw_decode_canvas: error {e}')
    return status


SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2, 0: 0, 2: 2}


def jpeg_subsampling(subsampling):
    """Pillow's number for a ``subsampling`` the encoder takes ('4:4:4' / 0, '4:2:0' / 2); ValueError for any other."""
    try:
        return SUBSAMPLING[subsampling]
    except (KeyError, TypeError):
        raise ValueError(f"subsampling {subsampling!r}: the encoder takes '4:2:0' and '4:4:4'") from None


def jpeg_encode_header(px, quality=95, subsampling='4:2:0'):
    """The bytes from SOI through the SOS header that every ``px`` tile encoded at (quality, subsampling) starts with
    (``bqio_jpeg_encode_header``).  ValueError outside the encoder's subset."""
    out = np.empty(int(lib().bqio_jpeg_encode_header_bytes()), np.uint8)
    if lib().bqio_jpeg_encode_header(int(px), int(quality), jpeg_subsampling(subsampling), out.ctypes.data) != 0:
        raise ValueError('bqio_jpeg_encode_header: ' + lib().bqio_jpeg_encode_last_error().decode())
    return out.tobytes()


def _encode_sized(name, tiles, cap, *mid_args):
    """The CPU encoders' calls ``bqio_<name>(tiles, n, px, *mid_args, out, cap, off, status)``: with ``cap`` None a first one without
    a buffer, which states the exact size, then the one that writes.  -> ``(buffer[:cap], offsets, status)``."""
    tiles = np.ascontiguousarray(tiles, np.uint8)
    assert tiles.ndim == 4 and tiles.shape[1] == tiles.shape[2] and tiles.shape[3] == 3, tiles.shape
    n, px = tiles.shape[0], tiles.shape[1]
    off, status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)

    def call(out, cap):
        if getattr(lib(), 'bqio_' + name)(tiles.ctypes.data, n, px, *mid_args, out.ctypes.data if out is not None else None, cap,
                                          off.ctypes.data, status.ctypes.data) != 0:
            raise ValueError(f'bqio_{name}: ' + getattr(lib(), f'bqio_{name}_last_error')().decode())
    if cap is None:
        call(None, 0)
        cap = int(off[-1])
    out = np.zeros(max(int(cap), 1), np.uint8)
    call(out, int(cap))
    return out[:int(cap)], off, status


def jpeg_encode(tiles, quality=95, subsampling='4:2:0', cap=None):
    """uint8 [n, px, px, 3] -> ``(buffer uint8 [bytes], offsets int64 [n + 1], status int32 [n])``: the files Pillow's
    ``save(buf, 'JPEG', quality=quality, subsampling=subsampling)`` writes, back to back (``bqio_jpeg_encode``: the device
    encoder's routines, csrc/jpeg_encode_device.h, on the CPU).  ``cap``: the buffer's size; None sizes it exactly with a first
    call.  A file that would end beyond ``cap`` is left out and its status is 1.  ValueError outside the encoder's subset.
    What ``Engine.jpeg_encode`` computes, byte for byte.  For tests."""
    return _encode_sized('jpeg_encode', tiles, cap, int(quality), jpeg_subsampling(subsampling))


def png_encode(tiles, cap=None):
    """uint8 [n, px, px, 3] -> ``(buffer uint8 [bytes], offsets int64 [n + 1], status int32 [n])``: complete PNG files back to
    back (``bqio_png_encode``: the device encoder's routines, csrc/png_encode_device.h, on the CPU).  The filtered rows are
    Pillow's; the deflate stream is the project's own.  ``cap``: the buffer's size; None sizes it exactly with a first call.  A
    file that would end beyond ``cap`` is left out and its status is 1.  ValueError outside 1 <= px <= 4096.  What
    ``Engine.png_encode`` computes, byte for byte.  For tests."""
    return _encode_sized('png_encode', tiles, cap)


def inflate_fallbacks():
    """Streams handed to zlib after the reader's own decompressor refused them although zlib accepts them (0 = none)."""
    return int(lib().bqio_inflate_fallbacks())


class UnsupportedImage(ValueError):
    def __init__(self, index):
        super().__init__(f'record {index}: image_raw is not a PNG or baseline JPEG the native decoder handles')
        self.index = index


def default_threads():
    """Decoder threads of one process: the cores it may use (its affinity mask, which ``distributed.pin_rank`` narrows to the
    rank's share of the node, capped by the cgroup's CPU quota), at most 64: a 64-core share decodes on 64 threads -- twice what
    one GPU consumes --, and eight ranks on one node do not start 8 x 16 threads on the same cores."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:    # cgroup v2 quota
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


class NativeReader:
    def __init__(self, path, verify='length'):
        self._lib = lib()
        self._h = self._lib.bqio_open(os.fsencode(path), VERIFY[verify])
        if not self._h:
            raise IOError(self._lib.bqio_last_error(None).decode())
        self.path = path

    def close(self):
        if self._h:
            self._lib.bqio_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()

    def __len__(self):
        return int(self._lib.bqio_count(self._h))

    @property
    def slide(self):
        buf = C.create_string_buffer(512)
        n = self._lib.bqio_slide_name(self._h, buf, 512)
        if n < 0:
            raise IOError(self._lib.bqio_last_error(self._h).decode())
        return buf.value.decode() if n else None

    def image_format(self, index):
        return int(self._lib.bqio_image_format(self._h, index))

    def image_bytes(self, index):
        p = C.POINTER(C.c_uint8)()
        n = C.c_size_t()
        if self._lib.bqio_image_bytes(self._h, index, C.byref(p), C.byref(n)) != 0:
            raise IOError(self._lib.bqio_last_error(self._h).decode())
        return C.string_at(p, n.value)

    def probe(self, tile_px=299, first=0, count=None):
        """None when ``decode`` would take records [first, first + count) as far as that shows without decoding (``bqio_probe``:
        record framing, image signatures, the markers and scan structure of JPEG records); otherwise the index of the first
        record it would refuse.  One pass over the bytes of the JPEG records, nothing for PNG records."""
        total = len(self)
        count = total - first if count is None else count
        bad = _i64(-1)
        e = self._lib.bqio_probe(self._h, first, count, tile_px, C.byref(bad))
        return None if e == 0 else int(bad.value)

    def _raise(self, e, bad, tile_px, full=None):
        """The end of a reading call that answered ``e``: nothing for 0, otherwise the exception of the code -- ``full`` (a
        MemoryError: the caller's buffer was too small) in place of the plain ``IOError`` where the caller found that."""
        if e == ERR_UNSUPPORTED:
            raise UnsupportedImage(bad.value)
        if e == ERR_FORMAT:       # same exception the Python reader raises for a tile of the wrong size
            raise ValueError(f'{self.path}: record {bad.value}: tile size differs from {(tile_px, tile_px, 3)}')
        if e != 0:
            raise full or IOError(f'{self.path}: {self._lib.bqio_last_error(self._h).decode()} (record {bad.value})')

    def extract_z(self, first, count, tile_px, out_z, off, length, threads=None):
        """The zlib streams of records [first, first + count) packed into ``out_z`` (uint8 array, usually pinned) for the device
        inflate (``Engine.png_inflate``): ``off`` / ``length`` (uint32 [count]) receive every stream's offset (a multiple of 16)
        and size.  Returns (bytes used, loc int64 [count, 2]).  ``UnsupportedImage`` for a record that is not an 8-bit RGB PNG
        tile of ``tile_px``; ``MemoryError`` (with the bytes needed in ``.args[1]``) when ``out_z`` is too small."""
        assert out_z.dtype == np.uint8 and out_z.flags['C_CONTIGUOUS'] and off.dtype == np.uint32 and length.dtype == np.uint32
        assert off.size >= count and length.size >= count
        loc = np.zeros((count, 2), np.int64)
        used = C.c_size_t(0)
        bad = _i64(-1)
        e = self._lib.bqio_extract_z(self._h, first, count, tile_px, out_z.ctypes.data, out_z.size, off.ctypes.data,
                                     length.ctypes.data, loc.ctypes.data, C.byref(used), threads or default_threads(), C.byref(bad))
        full = used.value > out_z.size and MemoryError(f'extract_z: {used.value} bytes needed, {out_z.size} given', used.value)
        self._raise(e, bad, tile_px, full)
        return int(used.value), loc

    def extract_jpeg(self, first, count, tile_px, out_scan, desc, tables, threads=None):
        """The JPEG counterpart of ``extract_z``, for the device decoder (``Engine.jpeg_decode``): the entropy-coded segments of
        records [first, first + count), stuffed zeros removed and padded, packed into ``out_scan`` (uint8, usually pinned);
        ``desc`` (uint32 [count, 4]: offset, length, sampling, table set) and ``tables`` (uint8 [k, jpeg_table_bytes()]: the call's
        distinct table sets) are filled.  Returns (bytes used, table sets used, loc int64 [count, 2]).  ``out_scan=None``: only the
        two sizes, nothing copied (the once-per-slide check).  The subset is the host decoder's (``probe``) without grey tiles and
        without restart intervals: ``UnsupportedImage`` for a record outside it -- progressive, arithmetic-coded, CMYK, truncated,
        grey, with restart markers, not a JPEG --, ``ValueError`` for a tile of another size; ``MemoryError`` (bytes needed in
        ``.args[1]``, table sets needed in ``.args[2]``) when ``out_scan`` or ``tables`` is too small."""
        loc = np.zeros((count, 2), np.int64)
        used, nt, bad = C.c_size_t(0), C.c_int(0), _i64(-1)
        if out_scan is None:
            args = (None, 0, None, None, 0)
        else:
            assert out_scan.dtype == np.uint8 and out_scan.flags['C_CONTIGUOUS'] and desc.dtype == np.uint32 and desc.flags['C_CONTIGUOUS']
            assert desc.size >= 4 * count and tables.dtype == np.uint8 and tables.flags['C_CONTIGUOUS']
            args = (out_scan.ctypes.data, out_scan.size, desc.ctypes.data, tables.ctypes.data, tables.size // jpeg_table_bytes())
        e = self._lib.bqio_extract_jpeg(self._h, first, count, tile_px, *args, C.byref(nt), loc.ctypes.data, C.byref(used),
                                        threads or default_threads(), C.byref(bad))
        full = bad.value < 0 and out_scan is not None and (used.value > args[1] or nt.value > args[4]) and MemoryError(
            f'extract_jpeg: {used.value} bytes and {nt.value} table sets needed, {args[1]} and {args[4]} given', used.value, nt.value)
        self._raise(e, bad, tile_px, full)
        return int(used.value), int(nt.value), loc

    def decode(self, first=0, count=None, tile_px=299, out=None, threads=None, rows=False):
        """-> (tiles uint8 [count,px,px,3], loc int64 [count,2]).  `out`: optional C-contiguous uint8
        array / tensor-backed numpy view to decode into (e.g. pinned memory).
        rows=True: the PNG scanline filters stay in -- [count,px,1+3*px], filter-type byte + filtered bytes per row, for
        `Engine.png_unfilter` on the GPU (tiles that are not 8-bit RGB PNGs arrive decoded, as rows of filter type 0)."""
        total = len(self)
        count = total - first if count is None else count
        shape = (count, tile_px, 1 + 3 * tile_px) if rows else (count, tile_px, tile_px, 3)
        if out is None:
            out = np.empty(shape, np.uint8)
        assert out.dtype == np.uint8 and out.flags['C_CONTIGUOUS'] and out.size == int(np.prod(shape))
        loc = np.zeros((count, 2), np.int64)
        bad = _i64(-1)
        fn = self._lib.bqio_decode_rows if rows else self._lib.bqio_decode
        e = fn(self._h, first, count, tile_px, out.ctypes.data, loc.ctypes.data, threads or default_threads(), C.byref(bad))
        self._raise(e, bad, tile_px)
        return out, loc
