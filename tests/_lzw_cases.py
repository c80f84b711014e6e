"""The forge shared by tests/test_lzw.py, tests/test_wsi_lzw.py (CPU), tests/test_gpu_lzw.py and tools/bench_lzw.py: TIFF LZW streams
libtiff writes (through Pillow: one strip, cut out of the file), a small LZW ENCODER for the streams libtiff never writes, the oracle
(a segment wrapped in a one-page TIFF and opened with Pillow: libtiff's decoder), and hand-assembled tiled pages and slide files
whose tiles such streams are (in the manner of tests/_j2k_cases.py)."""
import io

import numpy as np
from PIL import Image

from tests.test_wsi import _img, _tiff, _tiles_of

CLEAR, EOI, FIRST = 256, 257, 258


def content(kind, w, h, seed=0):
    """uint8 [h, w, 3]: 'noise', 'flat', 'smooth' (structure plus grain) or 'white'."""
    if kind == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'flat':
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    if kind == 'white':
        return np.full((h, w, 3), 255, np.uint8)
    assert kind == 'smooth'
    return _img(w, h, seed)


def difference(a):
    """Horizontal differencing per sample modulo 256 (TIFF predictor 2) of uint8 [h, w, 3]."""
    d = a.astype(np.int16)
    d[:, 1:] -= a[:, :-1].astype(np.int16)
    return (d & 255).astype(np.uint8)


def libtiff_stream(a, predictor=1):
    """The one LZW strip libtiff writes for uint8 [h, w, 3] ``a``."""
    bb = io.BytesIO()
    Image.fromarray(a).save(bb, format='TIFF', compression='tiff_lzw', tiffinfo={317: predictor, 278: a.shape[0]})
    raw = bb.getvalue()
    t = Image.open(io.BytesIO(raw)).tag_v2
    assert t[259] == 5 and len(t[273]) == 1 and t.get(317, 1) == predictor
    return raw[t[273][0]:t[273][0] + t[279][0]]


def width_for(n):
    """The width of the next code when the table's next free index is ``n`` (early change)."""
    return 9 if n < 511 else 10 if n < 1023 else 11 if n < 2047 else 12


class Bits:
    """Codes packed MSB first."""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def bytes(self):
        return bytes(self.out) + (bytes([(self.acc << (8 - self.n)) & 255]) if self.n else b'')


def pack(codes, lead_clear=True):
    """A list of codes packed at the widths the decoder will read them with: it follows the decoder's next free index.  With
    ``lead_clear`` False the decoder's first code already adds an entry (as libtiff's does)."""
    b, n, fresh = Bits(), FIRST, False
    for c in codes:
        b.put(c, width_for(n))
        if c == CLEAR:
            n, fresh = FIRST, True
        elif c != EOI:
            if fresh:
                fresh = False
            else:
                n += 1
    return b.bytes()


def codes_of(data, clear_at=4094, lead_clear=True, eoi=True):
    """``data`` as LZW codes: ClearCode first (``lead_clear``), again whenever the table's next free index reaches ``clear_at``
    (None: never -- the table runs full and beyond), EndOfInformation last (``eoi``)."""
    codes = [CLEAR] if lead_clear else []
    table, n, w = {}, FIRST, None
    for c in bytes(data):
        if w is None:
            w = c
            continue
        k = table.get((w, c))
        if k is not None:
            w = k
            continue
        codes.append(w)
        if n < 4096:
            table[(w, c)] = n
        n += 1
        w = c
        if clear_at is not None and n >= clear_at:
            codes.append(CLEAR)
            table, n = {}, FIRST
    if w is not None:
        codes.append(w)
    if eoi:
        codes.append(EOI)
    return codes


def encode(data, **kw):
    lead = kw.get('lead_clear', True)
    return pack(codes_of(data, **kw), lead_clear=lead)


def strip_page(raw, w, rows, predictor=1):
    """A one-page, one-strip TIFF file around the LZW segment ``raw``."""
    return _tiff([dict(w=w, h=rows, tw=w, th=rows, comp=5, predictor=predictor, tiled=False, segs=[raw])])


def oracle(raw, w, rows, predictor=1):
    """libtiff's verdict on segment ``raw`` of ``rows`` x ``w`` pixels: uint8 [rows, w, 3], or None where Pillow raises."""
    try:
        im = Image.open(io.BytesIO(strip_page(raw, w, rows, predictor)))
        return np.asarray(im.convert('RGB')).copy()
    except (OSError, SyntaxError, ValueError):
        return None


# ---- the valid cases: (name, w, h, content) -- each with predictor 1 and 2 --------------------------------------------------------------
IMAGES = [('noise', 96, 80, 'noise'), ('flat', 96, 80, 'flat'), ('white', 96, 80, 'white'), ('smooth', 96, 80, 'smooth'), ('one', 1, 1, 'noise'), ('row', 700, 1, 'smooth')]


def valid_cases():
    """[(name, raw, w, rows, predictor, pixels)]: libtiff's own streams for ``IMAGES`` with both predictors, then the encoder's: a
    final string cut at ``need`` (the stream codes a longer run than the segment holds), EndOfInformation absent, clears at
    another place than libtiff's, and consecutive ClearCodes."""
    out = []
    for name, w, h, kind in IMAGES:
        a = content(kind, w, h, 3)
        for pred in (1, 2):
            out.append((f'{name}-p{pred}', libtiff_stream(a, pred), w, h, pred, a))
    flat = content('flat', 40, 9, 0)
    out.append(('cut-at-need', encode(flat.tobytes() + flat.tobytes()[:77]), 40, 9, 1, flat))
    out.append(('cut-at-need-no-eoi', encode(flat.tobytes() + flat.tobytes()[:77], eoi=False), 40, 9, 1, flat))
    sm = content('smooth', 50, 31, 1)
    out.append(('no-eoi', encode(sm.tobytes(), eoi=False), 50, 31, 1, sm))
    out.append(('no-eoi-p2', encode(difference(sm).tobytes(), eoi=False), 50, 31, 2, sm))
    nz = content('noise', 50, 31, 2)
    out.append(('clear-early', encode(nz.tobytes(), clear_at=700), 50, 31, 1, nz))
    codes = codes_of(sm.tobytes())
    out.append(('double-clear', pack([CLEAR] + codes), 50, 31, 1, sm))
    return out


def malformed_cases():
    """[(name, raw, w, rows)]: streams no encoder should write; the oracle says which of them libtiff still decodes."""
    nz = content('noise', 96, 80, 7)
    good = encode(nz.tobytes())
    out = [('no-lead-clear', encode(nz.tobytes(), lead_clear=False), 96, 80),
           ('garbage', b'x' * 10, 64, 64),
           ('old-style', b'\x00\x01' + good[2:], 96, 80),
           ('old-style-3', b'\x00\x03' + good[2:], 96, 80),
           ('empty', b'', 4, 4),
           ('one-byte', b'\x80', 4, 4),
           ('clear-only', pack([CLEAR, EOI]), 4, 4),
           ('eoi-early', encode(nz.tobytes()[:5000]), 96, 80)]
    # a code beyond the next free index: right after the clear, one past, and far past in mid-stream
    small = content('smooth', 16, 4, 2).tobytes()
    codes = codes_of(small)
    out.append(('beyond-after-clear', pack([CLEAR, FIRST] + codes[2:]), 16, 4))
    # (codes[:10] is the ClearCode and nine strings: the next free index is then 258 + 8)
    out.append(('beyond-by-one', pack(codes[:10] + [FIRST + 9] + codes[11:]), 16, 4))
    out.append(('beyond-far', pack(codes[:10] + [500] + codes[11:]), 16, 4))
    out.append(('kwkwk-at-free', pack(codes[:10] + [FIRST + 8] + codes[11:]), 16, 4))
    for k in (1, 2, 3, 17, 100, len(good) // 2, len(good) - 2, len(good) - 1):
        out.append((f'truncated-{k}', good[:k], 96, 80))
    # the table run full without a ClearCode: up to 4095, beyond it, and to where libtiff's table ends
    for rows in (40, 80):
        out.append((f'no-clear-{rows}', encode(nz[:rows].tobytes(), clear_at=None), 96, rows))
    # ... and pixel by pixel across the two places where something could change: the next free index passing 4096 (1313 ..
    # 1316 pixels of this noise) and reaching 5119 (1670 .. 1675)
    line = content('noise', 2000, 1, 7)
    for k in (1313, 1314, 1315, 1316, 1670, 1671, 1672, 1673, 1674, 1675):
        out.append((f'no-clear-line-{k}', encode(line[:, :k].tobytes(), clear_at=None), k, 1))
    return out


# ---- pages and slide files ---------------------------------------------------------------------------------------------------------------
def page(a, tw, th, predictor=1, tiled=True, libtiff=False, **extra):
    """One LZW page dict for ``tests.test_wsi._tiff`` over RGB image ``a``: tiles of ``tw`` x ``th`` (or strips of ``th`` rows),
    from the encoder above or (``libtiff``) from libtiff's."""
    h, w = a.shape[:2]
    enc = (lambda t: encode(difference(t).tobytes())) if predictor == 2 else (lambda t: encode(t.tobytes()))
    if libtiff:
        enc = lambda t: libtiff_stream(np.ascontiguousarray(t), predictor)                   # noqa: E731
    if tiled:
        segs = _tiles_of(a, tw, th, enc)
    else:
        tw, segs = w, [enc(a[y:y + th]) for y in range(0, h, th)]
    return dict(w=w, h=h, tw=tw, th=th, comp=5, predictor=predictor, tiled=tiled, segs=segs, **extra)


def write_slide(path, pages, **kw):
    with open(path, 'wb') as f:
        f.write(_tiff(pages, **kw))
    return str(path)


def slide_file(tmp_path, mpp, w=600, h=450, tile=64, predictor=2, mutate=None, name='lzw.tif', seed=5, libtiff=False):
    """A two-level tiled LZW slide: level 0 ``w`` x ``h`` (no multiple of the tile), level 1 a quarter of it.  -> (path, level-0
    pixels, level-1 pixels).  ``mutate(pages)`` may change the page dicts before the file is assembled."""
    a = _img(w, h, seed)
    b = np.asarray(Image.fromarray(a).resize((w // 4, h // 4), Image.BILINEAR))
    pages = [page(a, tile, tile, predictor, libtiff=libtiff, desc=f'Aperio |MPP = {mpp}'), page(b, tile, tile, predictor, libtiff=libtiff)]
    if mutate:
        mutate(pages)
    return write_slide(tmp_path / name, pages), a, b
