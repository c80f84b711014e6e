"""A slide reader under the heatmap front-end: what ``sf.WSI(slide, 299, 302, roi_method='ignore')`` and
``wsi.build_generator(shuffle=False, include_loc='grid')`` give the reference's Figure-5 code (``results.py:216-265``) -- the tile grid
of a whole-slide image at a tile width in MICRONS, each tile resampled to ``tile_px`` -- for pyramidal TIFF slides, without Slideflow,
libvips or OpenSlide (none of which exists here).

What is read: classic TIFF and BigTIFF, little or big endian; 8-bit RGB / YCbCr pages in chunky layout, stored as strips or tiles;
compression none (1), zlib / Adobe deflate (8, 32946; horizontal predictor 2 supported), LZW (5: TIFF 6.0 streams as libtiff
writes them, predictor 1 or 2, decoded by libbiscuit_io's ``bqio_lzw_decode``, which tests/test_lzw.py holds against libtiff byte for
byte), JPEG (7: abbreviated streams + the page's ``JPEGTables``, decoded by Pillow's libjpeg) and JPEG 2000 (Aperio's 33003 and 33005, and 34712: one codestream or JP2 file per
segment, decoded by Pillow's OpenJPEG).  That covers Aperio SVS written with JPEG or JPEG 2000 tiles and generic pyramidal TIFFs
(``vips tiffsave --pyramid``, Pillow, the libtiff tools' and Bio-Formats' LZW pyramids); old-style (pre-6.0) LZW and planar layouts
are refused with a message, not mis-read.  Every LZW level is probed at open time: its first segment must begin with ClearCode.
Microns per pixel come from the Aperio description (``MPP = 0.2520``) or from XResolution / ResolutionUnit.

JPEG 2000: a 33005 / 34712 segment's samples are RGB (a multiple-component transform inside the codestream is the decoder's to
undo); a 33003 segment's three components are taken as full-range YCbCr and converted with the bytes of Pillow's own
``Image.merge('YCbCr', ...).convert('RGB')`` (stated for the device and the CPU build in csrc/j2k_ycc.h, pinned against Pillow
over all 2^24 triples in tests/test_j2k.py).  UNPINNED: whether that is the conversion Aperio's ImageScope and OpenSlide apply to
33003 tiles -- no real slide and no OpenSlide exist here.  Every JPEG 2000 level is probed at open time: the first segment's main
header (SOC, SIZ, COD, QCD) must state three 8-bit unsigned components and an image no smaller than the page's tile.

PARITY UNPINNED (like everything on the producer side): Slideflow's reader is not available, no real slide exists here, and the kernel
libvips uses to shrink a region to ``tile_px`` is not reproduced -- tiles are resampled with Pillow's LANCZOS.  What IS pinned
(tests/test_wsi.py): the container layer against libtiff (through Pillow) on files Pillow writes, and against hand-assembled tiled /
BigTIFF / JPEGTables files; the grid arithmetic against its definition.
"""
import io
import re
import struct
import zlib

import numpy as np

TILE_PX, TILE_UM = 299, 302             # biscuit/hp.py:5, results.py:235


class SlideError(ValueError):
    pass


def _guard(fn):
    """A damaged file must end in SlideError, whatever the parser tripped over."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        try:
            return fn(*a, **k)
        except SlideError:
            raise
        except (struct.error, IndexError, KeyError, TypeError, ValueError, ZeroDivisionError, OverflowError, MemoryError, OSError) as e:
            raise SlideError(f'damaged or unsupported slide file: {type(e).__name__}: {e}') from None
    return wrapped


_TYPES = {1: ('B', 1), 2: ('c', 1), 3: ('H', 2), 4: ('I', 4), 5: ('II', 8), 6: ('b', 1), 7: ('B', 1), 8: ('h', 2), 9: ('i', 4),
          10: ('ii', 8), 11: ('f', 4), 12: ('d', 8), 13: ('I', 4), 16: ('Q', 8), 17: ('q', 8), 18: ('Q', 8)}


J2K_COMPRESSIONS = (33003, 33005, 34712)   # Aperio: YCbCr components, RGB components; 34712: the registered JP2000 tag


def j2k_probe(raw, tw, th):
    """The main header of a JPEG 2000 segment (raw codestream or JP2 file), as far as the reader depends on it: SOC, SIZ, then
    marker segments up to the first tile part with a COD and a QCD among them; three 8-bit unsigned components, an image of at
    least ``tw`` x ``th``.  ``SlideError`` otherwise."""
    def bad(why):
        return SlideError(f'JPEG 2000 tile does not open: {why}')
    at = 0
    if raw[:12] == b'\0\0\0\x0cjP  \r\n\x87\n':                        # a JP2 file: the codestream starts its jp2c box
        at = raw.find(b'jp2c\xff\x4f\xff\x51')
        if at < 0:
            raise bad('a JP2 file without a codestream box')
        at += 4
    if raw[at:at + 4] != b'\xff\x4f\xff\x51':
        raise bad('no SOC and SIZ markers')
    pos, seen = at + 2, set()
    while True:
        if pos + 4 > len(raw):
            raise bad('the main header is cut off')
        marker, length = struct.unpack('>HH', raw[pos:pos + 4])
        if marker in (0xFF90, 0xFF93):
            break
        if marker < 0xFF30 or length < 2 or pos + 2 + length > len(raw):
            raise bad(f'marker {marker:04X} with length {length} in the main header')
        body = raw[pos + 4:pos + 2 + length]
        if marker == 0xFF51:
            if len(body) < 36 + 3:
                raise bad('a short SIZ')
            _, xs, ys, xo, yo = struct.unpack('>HIIII', body[:18])
            comps = struct.unpack('>H', body[34:36])[0]
            if len(body) != 36 + 3 * comps:
                raise bad('a SIZ of the wrong length')
            if comps != 3 or any(body[36 + 3 * c] != 7 for c in range(3)):
                raise SlideError(f'JPEG 2000 tile with {comps} components of depths {[(body[36 + 3 * c] & 127) + 1 for c in range(min(comps, 4))]}: '
                                 'only three 8-bit unsigned components are supported')
            if xs - xo < tw or ys - yo < th:
                raise SlideError(f'JPEG 2000 tile of {xs - xo} x {ys - yo} pixels is smaller than the page\'s {tw} x {th} tile')
        seen.add(marker)
        pos += 2 + length
    if not {0xFF51, 0xFF52, 0xFF5C} <= seen:
        raise bad('SIZ, COD or QCD missing from the main header')


def lzw_probe(raw, path, li):
    """The first segment of an LZW level, as far as the reader depends on it at open time: the decoder is built, and the stream
    begins with ClearCode (TIFF 6.0, codes MSB first).  ``SlideError`` otherwise."""
    from . import tfrecord_native as tn
    if not tn.available():
        raise SlideError(f'{path}: level {li} is LZW-compressed, and libbiscuit_io, which decodes it, is not built (make -C biscuit_amd/csrc)')
    if len(raw) < 2 or raw[0] != 0x80 or raw[1] & 0x80:
        old = len(raw) >= 2 and raw[0] == 0 and raw[1] & 1
        raise SlideError(f'{path}: LZW level {li} does not begin with ClearCode: '
                         + ('an old-style (pre-6.0, bit-reversed) stream, which is not supported' if old else 'damaged'))


class _Page:
    """One IFD that holds an 8-bit RGB / YCbCr image."""
    def __init__(self, tags):
        g = tags.get
        self.width, self.height = int(g(256)[0]), int(g(257)[0])
        self.bits = tuple(g(258, (1,)))
        self.compression = int(g(259, (1,))[0])
        # the image codec of the segments, where they are images; ycc: a JPEG 2000 segment's components are YCbCr (33003)
        # ('lzw': not images but byte streams; named here because such tiles, too, decode on the device -- ``region_segments``)
        self.codec = {7: 'jpeg', 5: 'lzw'}.get(self.compression, 'j2k' if self.compression in J2K_COMPRESSIONS else None)
        self.ycc = self.compression == 33003
        self.photometric = int(g(262, (2,))[0])
        self.samples = int(g(277, (1,))[0])
        self.planar = int(g(284, (1,))[0])
        self.predictor = int(g(317, (1,))[0])
        self.subfile = int(g(254, (0,))[0])
        d = g(270, b'')
        self.description = (d if isinstance(d, bytes) else b'').split(b'\0')[0].decode('latin-1')
        self.jpeg_tables = bytes(g(347)) if g(347) is not None else None
        self.subsampling = tuple(g(530, (2, 2)))
        self.xres, self.yres, self.res_unit = g(282), g(283), int(g(296, (2,))[0])
        if g(322) is not None:           # tiles
            self.tiled = True
            self.tw, self.th = int(g(322)[0]), int(g(323)[0])
            self.offsets, self.counts = g(324), g(325)
        else:
            self.tiled = False
            self.tw = self.width
            self.th = int(g(278, (self.height,))[0])
            self.th = min(self.th, self.height)
            self.offsets, self.counts = g(273), g(279)
        if not (0 < self.width <= 1 << 20 and 0 < self.height <= 1 << 20 and 0 < self.tw <= 1 << 15 and 0 < self.th <= 1 << 15):
            raise SlideError(f'implausible page geometry {self.width} x {self.height}, segments {self.tw} x {self.th}')
        self.across = -(-self.width // self.tw)
        self.down = -(-self.height // self.th)

    def usable(self):
        return self.samples == 3 and self.bits[:3] == (8, 8, 8) and self.offsets is not None and self.counts is not None

    def check(self):
        if self.planar != 1:
            raise SlideError('planar (separate-plane) TIFF pages are not supported')
        if self.compression == 5 and self.predictor not in (1, 2):
            raise SlideError(f'LZW-compressed TIFF with predictor {self.predictor}: only 1 (none) and 2 (horizontal) are supported')
        if self.compression == 5 and self.photometric == 6:
            raise SlideError('LZW-compressed YCbCr TIFF pages are not supported')
        if self.compression not in (1, 5, 7, 8, 32946) + J2K_COMPRESSIONS:
            raise SlideError(f'TIFF compression {self.compression} is not supported')
        if len(self.offsets) != len(self.counts) or len(self.offsets) < self.across * self.down:
            raise SlideError('TIFF page: strip / tile tables do not cover the image')


class BandSegments:
    """A band's canvas as the page's own JPEG tiles, not yet decoded (``WSI.band_segments``): ``shape`` = (H, W) of the canvas
    ``WSI.band`` would read; ``data`` uint8 [bytes], the raw segments one after the other, segment i =
    ``data[offsets[i]:offsets[i] + lengths[i]]`` (uint64 each); ``place`` int32 [n, 2], the canvas position (x, y) of each
    segment's top-left pixel (negative where the segment starts left of / above the canvas); ``clip`` = (x0, y0, x1, y1), the
    level's image extent in canvas coordinates, cut to the canvas -- what a segment holds beyond it is padding; ``seg_w``,
    ``seg_h`` the page's tile size; ``jpeg_tables`` the page's ``JPEGTables`` bytes or None.  Decoding every segment as
    ``TiffSlide._jpeg`` reads it into a white canvas, inside ``clip`` only, gives ``WSI.band``'s canvas.  ``codec``: 'jpeg', or
    'j2k' where the segments are JPEG 2000 codestreams (``TiffSlide._j2k`` reads them), 'lzw' where they are TIFF LZW streams of
    ``seg_w`` x ``seg_h`` RGB pixels (``tfrecord_native.lzw_decode`` reads them); ``ycc``: a JPEG 2000 segment's three components
    are YCbCr, to be converted as the reader does (compression 33003); ``predictor``: an LZW page's (1: none, 2: horizontal
    differencing per sample)."""
    __slots__ = ('shape', 'data', 'offsets', 'lengths', 'place', 'clip', 'seg_w', 'seg_h', 'jpeg_tables', 'codec', 'ycc', 'predictor')

    def __init__(self, codec='jpeg', ycc=False, predictor=1, **kw):
        for k in self.__slots__[:-3]:
            setattr(self, k, kw[k])
        self.codec, self.ycc, self.predictor = codec, bool(ycc), int(predictor)

    def __len__(self):
        return len(self.offsets)


class TiffSlide:
    """``TiffSlide(path)``: ``levels`` (pyramid pages, largest first), ``level_downsamples``, ``dimensions`` (width, height of level 0),
    ``mpp`` (microns per pixel of level 0, or None), ``read_region(level, x, y, w, h)`` in that level's pixels -> uint8 [h, w, 3]
    (white outside the image, as slide viewers pad)."""

    def __init__(self, path):
        self.path = path
        self._f = open(path, 'rb')
        try:
            self._open()
        except BaseException:
            self._f.close()
            raise

    @_guard
    def _open(self):
        import os
        self._size = os.fstat(self._f.fileno()).st_size
        path = self.path
        head = self._f.read(16)
        if head[:2] == b'II':
            self._e = '<'
        elif head[:2] == b'MM':
            self._e = '>'
        else:
            raise SlideError(f'{path}: not a TIFF file')
        magic = struct.unpack(self._e + 'H', head[2:4])[0]
        if magic == 42:
            self._big, first = False, struct.unpack(self._e + 'I', head[4:8])[0]
        elif magic == 43:
            if struct.unpack(self._e + 'HH', head[4:8]) != (8, 0):
                raise SlideError(f'{path}: malformed BigTIFF header')
            self._big, first = True, struct.unpack(self._e + 'Q', head[8:16])[0]
        else:
            raise SlideError(f'{path}: not a TIFF file (magic {magic})')
        pages, off, seen = [], first, set()
        while off and off not in seen and len(pages) < 64:
            seen.add(off)
            tags, off = self._ifd(off)
            if 256 in tags and 257 in tags:
                p = _Page(tags)
                if p.usable():
                    pages.append(p)
        if not pages:
            raise SlideError(f'{path}: no 8-bit RGB page')
        # the pyramid: the largest page and every smaller page of the same aspect ratio that is not a label / macro / thumbnail strip
        # image of an Aperio file (those are stripped and named in their descriptions; a pyramid level of an SVS is tiled)
        base = max(pages, key=lambda p: p.width * p.height)
        levels = [base]
        for p in sorted(pages, key=lambda p: -p.width):
            if p is base or p.width >= levels[-1].width:
                continue
            same = abs(p.width / base.width - p.height / base.height) < 0.02
            named = re.search(r'\b(label|macro)\b', p.description, re.I) is not None
            if same and not named and (p.tiled or not base.tiled):
                levels.append(p)
        for li, p in enumerate(levels):
            p.check()
            if p.codec == 'j2k':
                j2k_probe(self._raw_segment(p, 0, li), p.tw, p.th)
            if p.codec == 'lzw':
                lzw_probe(self._raw_segment(p, 0, li), path, li)
        self.levels = levels
        self.dimensions = (base.width, base.height)
        self.level_dimensions = [(p.width, p.height) for p in levels]
        self.level_downsamples = [base.width / p.width for p in levels]
        self.mpp = self._mpp(base)
        self._cache = {}

    # ---- container ---------------------------------------------------------------------------------------------------
    def _ifd(self, off):
        f, e = self._f, self._e
        f.seek(off)
        if self._big:
            n = struct.unpack(e + 'Q', f.read(8))[0]
            raw = f.read(20 * n + 8)
            esz, fmt, inl = 20, 'HHQ', 8
        else:
            n = struct.unpack(e + 'H', f.read(2))[0]
            raw = f.read(12 * n + 4)
            esz, fmt, inl = 12, 'HHI', 4
        if n > 4096 or len(raw) < esz * n:
            raise SlideError(f'{self.path}: corrupt IFD')
        tags = {}
        for i in range(n):
            ent = raw[i * esz:(i + 1) * esz]
            tag, typ, cnt = struct.unpack(e + fmt, ent[:esz - inl])
            if typ not in _TYPES:
                continue
            code, size = _TYPES[typ]
            nbytes = size * cnt
            if nbytes > self._size:
                raise SlideError(f'{self.path}: tag {tag} claims {nbytes} bytes in a file of {self._size}')
            if nbytes <= inl:
                data = ent[esz - inl:esz - inl + nbytes]
            else:
                pos = struct.unpack(e + ('Q' if self._big else 'I'), ent[esz - inl:])[0]
                f.seek(pos)
                data = f.read(nbytes)
                if len(data) != nbytes:
                    raise SlideError(f'{self.path}: tag {tag} runs past the end of the file')
            if typ in (2, 7) or (typ == 1 and tag in (270, 347)):
                tags[tag] = bytes(data)
            elif typ in (5, 10):
                v = struct.unpack(e + code[0] * (2 * cnt), data)
                tags[tag] = tuple((v[2 * k], v[2 * k + 1]) for k in range(cnt))
            else:
                tags[tag] = struct.unpack(e + code * cnt, data)
        nxt = struct.unpack(e + ('Q' if self._big else 'I'), raw[esz * n:esz * n + (8 if self._big else 4)])[0]
        return tags, nxt

    @staticmethod
    def _mpp(p):
        m = re.search(r'MPP\s*=\s*([0-9.]+)', p.description)
        if m:
            return float(m.group(1))
        if p.xres and p.xres[0][1] and p.xres[0][0] and p.res_unit in (2, 3):
            per_unit = p.xres[0][0] / p.xres[0][1]
            return (25400.0 if p.res_unit == 2 else 10000.0) / per_unit
        return None

    # ---- pixels ------------------------------------------------------------------------------------------------------
    def _raw_segment(self, p, index, li):
        """The bytes of strip / tile ``index`` of page ``p`` (level ``li``, for the message), which must lie inside the file."""
        off, cnt = int(p.offsets[index]), int(p.counts[index])
        if cnt > self._size or off + cnt > self._size:
            raise SlideError(f'{self.path}: segment {index} of level {li} claims more bytes than the file holds')
        self._f.seek(off)
        raw = self._f.read(cnt)
        if len(raw) != cnt:
            raise SlideError(f'{self.path}: segment {index} of level {li} runs past the end of the file')
        return raw

    @_guard
    def _segment(self, li, index):
        """Strip / tile ``index`` of level ``li`` decoded to uint8 [th, tw, 3] (a last strip may be shorter)."""
        key = (li, index)
        if key in self._cache:
            return self._cache[key]
        p = self.levels[li]
        raw = self._raw_segment(p, index, li)
        rows = p.th if p.tiled else min(p.th, p.height - (index * p.th))
        if p.codec == 'lzw':
            img = self._lzw(p, raw, rows, li, index)
        elif p.codec:
            img = (self._jpeg if p.codec == 'jpeg' else self._j2k)(p, raw)
            if img.shape[0] < rows or img.shape[1] < p.tw:
                name = 'JPEG' if p.codec == 'jpeg' else 'JPEG 2000'
                raise SlideError(f'{self.path}: {name} segment {index} of level {li} is smaller than its tile')
            img = img[:rows, :p.tw]
        else:
            if p.compression in (8, 32946):
                try:
                    raw = zlib.decompress(raw)
                except zlib.error as e:
                    raise SlideError(f'{self.path}: damaged deflate segment {index} of level {li}: {e}') from None
            need = rows * p.tw * 3
            if len(raw) < need:
                raise SlideError(f'{self.path}: segment {index} of level {li} is short ({len(raw)} of {need} bytes)')
            img = np.frombuffer(raw, np.uint8, need).reshape(rows, p.tw, 3)
            if p.predictor == 2:
                img = np.cumsum(img, axis=1, dtype=np.uint8)          # horizontal differencing, per sample, modulo 256
            elif p.predictor != 1:
                raise SlideError(f'TIFF predictor {p.predictor} is not supported')
            if p.photometric == 6:
                raise SlideError('uncompressed YCbCr TIFF pages are not supported')
        if len(self._cache) > 64:
            self._cache.pop(next(iter(self._cache)))
        self._cache[key] = img
        return img

    _LZW_WHY = ((1, 'it does not begin with ClearCode'), (2, 'a code beyond the table'), (4, 'the data ends before the segment is full'),
                (8, 'the table overflows without a ClearCode'), (16, 'a stream too long'))

    def _lzw(self, p, raw, rows, li, index):
        """One LZW segment -> uint8 [rows, tw, 3], the page's predictor undone (``bqio_lzw_decode``)."""
        from . import tfrecord_native as tn
        if not tn.available():
            raise SlideError(f'{self.path}: level {li} is LZW-compressed, and libbiscuit_io, which decodes it, is not built')
        if rows * p.tw * 3 > 1 << 30:
            raise SlideError(f'{self.path}: LZW segment {index} of level {li} of {p.tw} x {rows} pixels is larger than the reader takes')
        img, status = tn.lzw_decode(raw, rows, p.tw, p.predictor)
        if status:
            why = ', '.join(t for bit, t in self._LZW_WHY if status & bit)
            raise SlideError(f'{self.path}: damaged LZW segment {index} of level {li}: {why} (status {status})')
        return img

    def _jpeg(self, p, raw):
        from PIL import Image
        if p.jpeg_tables:
            t = p.jpeg_tables
            t = t[:-2] if t.endswith(b'\xff\xd9') else t
            raw = t + (raw[2:] if raw[:2] == b'\xff\xd8' else raw)
        try:
            im = Image.open(io.BytesIO(raw))
            if p.photometric == 2 and im.mode == 'YCbCr':
                raise SlideError('RGB-photometric JPEG tiles whose streams carry no colour-space marker are not supported')
            return np.asarray(im.convert('RGB'))
        except (OSError, SyntaxError) as e:
            raise SlideError(f'{self.path}: a JPEG tile does not decode: {e}') from None

    def _j2k(self, p, raw):
        """One JPEG 2000 segment -> uint8 [h, w, 3] RGB.  Pillow opens a three-component codestream without a colour box as
        'RGB' and leaves the samples as they are: a 33003 segment's are YCbCr and are converted here (the module's header)."""
        from PIL import Image
        try:
            im = Image.open(io.BytesIO(raw))
            if im.format != 'JPEG2000':
                raise SlideError(f'{self.path}: a JPEG 2000 tile holds a {im.format} image')
            if im.mode == 'YCbCr':                                       # (a JP2 file that says so: Pillow converts)
                return np.asarray(im.convert('RGB'))
            if im.mode != 'RGB':
                raise SlideError(f'{self.path}: a JPEG 2000 tile decodes to mode {im.mode}, not to three 8-bit components')
            a = np.asarray(im)
        except (OSError, SyntaxError) as e:
            raise SlideError(f'{self.path}: a JPEG 2000 tile does not decode: {e}') from None
        if p.ycc:
            a = np.asarray(Image.merge('YCbCr', [Image.fromarray(np.ascontiguousarray(a[:, :, c])) for c in range(3)]).convert('RGB'))
        return a

    @_guard
    def read_region(self, level, x, y, w, h):
        p = self.levels[level]
        if not (0 < w <= 1 << 16 and 0 < h <= 1 << 16):
            raise SlideError(f'region of {w} x {h} pixels')
        out = np.full((h, w, 3), 255, np.uint8)
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, p.width), min(y + h, p.height)
        if x1 <= x0 or y1 <= y0:
            return out
        for ty in range(y0 // p.th, (y1 - 1) // p.th + 1):
            for tx in range(x0 // p.tw, (x1 - 1) // p.tw + 1):
                seg = self._segment(level, ty * p.across + tx)
                sx0, sy0 = tx * p.tw, ty * p.th
                ax0, ay0 = max(x0, sx0), max(y0, sy0)
                ax1, ay1 = min(x1, sx0 + seg.shape[1]), min(y1, sy0 + seg.shape[0])
                if ax1 > ax0 and ay1 > ay0:
                    out[ay0 - y:ay1 - y, ax0 - x:ax1 - x] = seg[ay0 - sy0:ay1 - sy0, ax0 - sx0:ax1 - sx0]
        return out

    @_guard
    def region_segments(self, level, x, y, w, h):
        """The raw JPEG, JPEG 2000 or LZW tiles ``read_region(level, x, y, w, h)`` would decode, as a ``BandSegments`` over the same
        [h, w] canvas (its ``codec`` says which), or None when the level is not a tiled JPEG / JPEG 2000 / LZW page (compression 7,
        33003, 33005, 34712 or 5 with TileWidth / TileLength: strips, deflate and uncompressed pages stay on ``read_region``).  Read through ``_segment``'s bounds checks -- a byte count beyond the
        file's size, a segment that does not lie inside the file, more segment bytes than the file holds: ``SlideError``."""
        p = self.levels[level]
        if not (p.tiled and p.codec):
            return None
        if not (0 < w <= 1 << 16 and 0 < h <= 1 << 16):
            raise SlideError(f'region of {w} x {h} pixels')
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, p.width), min(y + h, p.height)
        chunks, place, total = [], [], 0
        if x1 > x0 and y1 > y0:
            for ty in range(y0 // p.th, (y1 - 1) // p.th + 1):
                for tx in range(x0 // p.tw, (x1 - 1) // p.tw + 1):
                    index = ty * p.across + tx
                    total += int(p.counts[index])
                    if total > self._size:
                        raise SlideError(f'{self.path}: segment {index} of level {level} claims more bytes than the file holds')
                    chunks.append(self._raw_segment(p, index, level))
                    place.append((tx * p.tw - x, ty * p.th - y))
        lengths = np.array([len(c) for c in chunks], np.uint64)
        offsets = np.zeros(len(chunks), np.uint64)
        offsets[1:] = np.cumsum(lengths)[:-1]
        return BandSegments(shape=(h, w), data=np.frombuffer(b''.join(chunks), np.uint8), offsets=offsets, lengths=lengths,
                            place=np.array(place, np.int32).reshape(-1, 2),
                            clip=(max(0, -x), max(0, -y), min(w, p.width - x), min(h, p.height - y)),
                            seg_w=p.tw, seg_h=p.th, jpeg_tables=p.jpeg_tables, codec=p.codec, ycc=p.ycc, predictor=p.predictor)

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class WSI:
    """The tile grid of one slide at ``tile_um`` microns per tile, each tile ``tile_px`` pixels wide: the object the reference builds
    with ``sf.WSI(slide, 299, 302, roi_method='ignore')`` (results.py:235).  ``extract_px`` = the tile's width in level-0 pixels
    (``tile_um / mpp``), the grid walks the slide at stride ``extract_px / stride_div`` (border remainders dropped), every tile is read
    from the pyramid level with the largest downsample that still has at least ``tile_px`` pixels per tile and resampled to
    ``tile_px`` (Pillow LANCZOS).  ``roi_method``: only 'ignore' (what the reference passes) is implemented here; regions of interest are
    ``Heatmap.from_slide(rois=...)``'s."""

    READ_LIMIT = 1 << 16                 # pixels ``read_region`` reads at once, per side: ``bands`` splits wider grid rows

    @_guard
    def __init__(self, path, tile_px=TILE_PX, tile_um=TILE_UM, stride_div=1, roi_method='ignore', mpp=None):
        if roi_method != 'ignore':
            raise NotImplementedError("only roi_method='ignore' (results.py:235): the reader walks the whole grid; the region-of-interest "
                                      "filter is Heatmap.from_slide(rois=..., roi_method=...)")
        self.slide = TiffSlide(path)
        try:
            self._layout(path, tile_px, tile_um, stride_div, mpp)
        except BaseException:
            self.slide.close()                                           # a refusal below must not leave the file open
            raise

    def _layout(self, path, tile_px, tile_um, stride_div, mpp):
        self.path, self.tile_px, self.tile_um, self.stride_div = path, int(tile_px), float(tile_um), int(stride_div)
        self.mpp = float(mpp) if mpp else self.slide.mpp
        if not self.mpp:
            raise SlideError(f'{path}: no microns-per-pixel in the file (Aperio "MPP =" or XResolution); pass mpp=')
        self.extract_px = int(self.tile_um / self.mpp)                   # level-0 pixels per tile side
        if not np.isfinite(self.mpp) or self.mpp <= 0:
            raise SlideError(f'{path}: implausible microns per pixel {self.mpp}')
        if self.extract_px < 1 or self.stride_div < 1:
            raise SlideError('tile of less than one pixel / bad stride_div')
        self.stride = max(1, self.extract_px // self.stride_div)
        w, h = self.slide.dimensions
        self.grid_w = (w - self.extract_px) // self.stride + 1 if w >= self.extract_px else 0
        self.grid_h = (h - self.extract_px) // self.stride + 1 if h >= self.extract_px else 0
        want = self.extract_px / self.tile_px                            # the downsample the tile asks for
        ok = [i for i, d in enumerate(self.slide.level_downsamples) if d <= want * 1.0001]
        self.level = max(ok, key=lambda i: self.slide.level_downsamples[i]) if ok else 0
        self.level_ds = self.slide.level_downsamples[self.level]
        self.estimated_num_tiles = self.grid_w * self.grid_h

    def _tile(self, gx, gy):
        from PIL import Image
        x0, y0 = gx * self.stride, gy * self.stride
        lx, ly = int(round(x0 / self.level_ds)), int(round(y0 / self.level_ds))
        lw = max(1, int(round(self.extract_px / self.level_ds)))
        reg = self.slide.read_region(self.level, lx, ly, lw, lw)
        if lw != self.tile_px:
            reg = np.asarray(Image.fromarray(reg).resize((self.tile_px, self.tile_px), Image.LANCZOS))
        return reg

    def build_generator(self, shuffle=False, include_loc='grid', show_progress=False, **_):
        """-> a zero-argument callable whose generator yields ``{'image': uint8 [tile_px, tile_px, 3], 'loc' (and 'grid'): (gx, gy)}``
        in row-major grid order -- the dictionaries results.py:236-262 consumes under either Slideflow version's key."""
        if shuffle:
            raise NotImplementedError('shuffle=False is what the reference asks for (results.py:237)')

        def gen():
            for gy in range(self.grid_h):
                for gx in range(self.grid_w):
                    yield {'image': self._tile(gx, gy), 'loc': (gx, gy), 'grid': (gx, gy)}
        return gen

    def tiles(self):
        """(tiles uint8 [T, tile_px, tile_px, 3], grid int64 [T, 2] of (gx, gy)) -- everything at once, for ``heatmap.Heatmap``."""
        n = self.grid_w * self.grid_h
        out = np.empty((n, self.tile_px, self.tile_px, 3), np.uint8)
        grid = np.empty((n, 2), np.int64)
        for i, t in enumerate(self.build_generator()()):
            out[i] = t['image']
            grid[i] = t['loc']
        return out, grid

    # ---- the grid as bands of one canvas each (heatmap.Heatmap.from_slide, resample='gpu') ------------------------------------
    @property
    def src_px(self):
        """A tile's width in pixels of ``self.level`` (``_tile``'s ``lw``)."""
        return max(1, int(round(self.extract_px / self.level_ds)))

    def _level_xy(self, g):
        return int(round(g * self.stride / self.level_ds))               # ``_tile``'s lx / ly of grid column / row g

    def _band_rect(self, gy0, gy1, gx0, gx1):
        """``band``'s geometry without its pixels: (x0, y0, W, H) of the canvas in ``self.level``, origin int32 [T, 2], ``src_px``."""
        gx1 = self.grid_w if gx1 is None else gx1
        if not (0 <= gy0 < gy1 <= self.grid_h and 0 <= gx0 < gx1 <= self.grid_w):
            raise SlideError(f'band rows [{gy0}, {gy1}) x columns [{gx0}, {gx1}) outside the {self.grid_h} x {self.grid_w} grid')
        lw = self.src_px
        xs = np.array([self._level_xy(g) for g in range(gx0, gx1)], np.int64)
        ys = np.array([self._level_xy(g) for g in range(gy0, gy1)], np.int64)
        x0, y0 = int(xs[0]), int(ys[0])
        origin = np.empty((len(ys), len(xs), 2), np.int32)
        origin[:, :, 0] = (xs - x0)[None, :]
        origin[:, :, 1] = (ys - y0)[:, None]
        return (x0, y0, int(xs[-1]) + lw - x0, int(ys[-1]) + lw - y0), origin.reshape(-1, 2), lw

    @_guard
    def band(self, gy0, gy1, gx0=0, gx1=None):
        """Grid rows [gy0, gy1) (and columns [gx0, gx1), default all) as ONE read: ``(canvas, origin, src_px)`` -- canvas uint8
        [H, W, 3], the rectangle of ``self.level`` that covers every tile's ``src_px`` x ``src_px`` window (white where a window
        pokes past the level's edge, as ``read_region`` pads); origin int32 [T, 2], ``(lx - X0, ly - Y0)`` of every tile in
        row-major grid order with ``lx, ly`` as ``_tile`` computes them; ``src_px`` = ``_tile``'s ``lw``.  Cutting the windows
        out of the canvas and resampling them (``resample.tile_resample`` / ``Engine.tile_resample``) gives ``_tile``'s bytes."""
        (x0, y0, cw, ch), origin, lw = self._band_rect(gy0, gy1, gx0, gx1)
        return self.slide.read_region(self.level, x0, y0, cw, ch), origin, lw

    @_guard
    def band_segments(self, gy0, gy1, gx0=0, gx1=None):
        """``band`` with the canvas left compressed, for a caller that decodes it on the device (``Engine.jpeg_decode_canvas``):
        ``(segments, origin, src_px)`` with ``band``'s origin and ``src_px`` and segments = a ``BandSegments`` over ``band``'s
        canvas -- the level's raw JPEG tiles that cover it, their places in it and the clip rectangle -- or None when the level
        is not a tiled JPEG page.  ``SlideError`` where the file's segment tables point outside the file."""
        (x0, y0, cw, ch), origin, lw = self._band_rect(gy0, gy1, gx0, gx1)
        return self.slide.region_segments(self.level, x0, y0, cw, ch), origin, lw

    def bands(self, canvas_bytes=256 << 20, segments=False, keep=None):
        """Iterate the grid as bands whose canvas stays under ``canvas_bytes`` (at least one grid row each): yields ``(gy0, gy1,
        gx0, gx1, canvas, origin, src_px)`` with ``band``'s values.  A band is split into column ranges only where one grid row
        is wider than ``read_region`` reads at once (``READ_LIMIT``, 65 536 pixels); the tiles of such a slide then arrive band by
        band, not in row-major order of the whole grid.

        ``segments=True`` yields ``band_segments``' values instead: a ``BandSegments`` in place of the canvas, or None in its
        place where the band has to be read with ``band`` -- the level is not a tiled JPEG page, or the segment tables point
        outside the file (``band`` then says so).

        ``keep`` (bool [grid_h, grid_w]; None: every cell, the bands above): only what a kept cell needs is read (DESIGN.md
        "Heatmap input", Tissue mask).  Grid rows without a kept cell are never read and end a band; within a band every column
        range is cut down to the rectangle its kept cells span, so no band is without a kept cell and every band's first and
        last row and first and last column hold one.  The rectangles are disjoint and together hold every kept cell once;
        ``origin`` still lists every cell of the rectangle in row-major order, kept or not.

        While a band's rectangles are being yielded ``self.band_rows`` holds that band's ``(gy0, gy1)``: every rectangle still to
        come lies in grid rows >= ``band_rows[0]`` (a rectangle's own first row may be larger than a later one's of the same
        band)."""
        if keep is not None:
            keep = np.asarray(keep)
            if keep.dtype != np.bool_ or keep.shape != (self.grid_h, self.grid_w):
                raise ValueError(f'keep must be bool [{self.grid_h}, {self.grid_w}], not {keep.dtype} {list(keep.shape)}')
            live = keep.any(1)
        lw, limit = self.src_px, self.READ_LIMIT
        cols, gx0 = [], 0
        while gx0 < self.grid_w:                                          # column ranges of at most `limit` pixels
            gx1 = gx0 + 1
            while gx1 < self.grid_w and self._level_xy(gx1) + lw - self._level_xy(gx0) <= limit:
                gx1 += 1
            cols.append((gx0, gx1))
            gx0 = gx1
        widest = max((self._level_xy(b - 1) + lw - self._level_xy(a) for a, b in cols), default=0)
        gy0 = 0
        while gy0 < self.grid_h:
            if keep is not None and not live[gy0]:
                gy0 += 1
                continue
            gy1 = gy0 + 1
            while gy1 < self.grid_h and (keep is None or live[gy1]):
                h = self._level_xy(gy1) + lw - self._level_xy(gy0)
                if h > limit or h * widest * 3 > canvas_bytes:
                    break
                gy1 += 1
            self.band_rows = (gy0, gy1)
            for a, b in cols:
                r0, r1 = gy0, gy1
                if keep is not None:                                      # the rectangle this column range's kept cells span
                    sub = keep[gy0:gy1, a:b]
                    if not sub.any():
                        continue
                    cs, rs = np.flatnonzero(sub.any(0)), np.flatnonzero(sub.any(1))
                    a, b, r0, r1 = a + int(cs[0]), a + int(cs[-1]) + 1, gy0 + int(rs[0]), gy0 + int(rs[-1]) + 1
                if not segments:
                    yield (r0, r1, a, b) + self.band(r0, r1, a, b)
                    continue
                try:
                    yield (r0, r1, a, b) + self.band_segments(r0, r1, a, b)
                except SlideError:
                    yield (r0, r1, a, b, None) + self._band_rect(r0, r1, a, b)[1:]
            gy0 = gy1

    # ---- the picture under a rendered heatmap (heatmap.Heatmap.render) --------------------------------------------------------
    @_guard
    def thumbnail(self, width=2048):
        """The slide as one uint8 [H, W, 3] picture ``width`` pixels wide (DESIGN.md "Heatmap output"): the coarsest pyramid level
        that is still at least ``width`` wide (level 0 if none is), read whole in pieces of at most ``READ_LIMIT`` pixels a side
        and reduced to ``(width, round(h * width / w))`` with Pillow's LANCZOS.  A slide narrower than ``width`` is not
        upsampled: the thumbnail is then level 0 itself.  (Unpinned like ``_tile``: not the libvips resampler Slideflow uses.)"""
        from PIL import Image
        width = int(width)
        if width < 1:
            raise SlideError(f'thumbnail of width {width}')
        dims = self.slide.level_dimensions
        ok = [i for i, (w, _) in enumerate(dims) if w >= width]
        li = min(ok, key=lambda i: dims[i][0]) if ok else 0
        w, h = dims[li]
        img = np.empty((h, w, 3), np.uint8)
        step = self.READ_LIMIT
        for y in range(0, h, step):
            for x in range(0, w, step):
                ph, pw = min(step, h - y), min(step, w - x)
                img[y:y + ph, x:x + pw] = self.slide.read_region(li, x, y, pw, ph)
        if w <= width:
            return img
        return np.asarray(Image.fromarray(img).resize((width, max(1, int(round(h * width / w)))), Image.LANCZOS))

    def close(self):
        self.slide.close()
