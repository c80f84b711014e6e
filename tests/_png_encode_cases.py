"""Shared by tests/test_png_encode.py (CPU) and tests/test_gpu_png_encode.py: the PNG encoder's inputs and Pillow's files for
them, each computed once, and the few lines that take a PNG file apart.

Sizes, chosen by L = px (1 + 3 px), the filtered stream the deflate stage sees (blocks of 16 384 bytes, groups of 64 positions):
1 (L = 4: shorter than a hash and a group), 2 (14), 4 (52: one partial group), 5 (80: a group and a partial one), 21 (1 344:
exactly 21 groups), 73 (16 060: just under one block), 74 (16 502: a second block of 118 bytes), 299 (268 502: 17 blocks; three
tiles per call at most)."""
import functools
import io
import struct
import zlib

import numpy as np

from tests import _jpeg_encode_cases as ec

SIZES = (1, 2, 4, 5, 21, 73, 74, 299)
CONTENTS = ec.CONTENTS + ('rows',)
BATCH_299 = 3
BLOCK = 16384
FILTERS = {0, 1, 2, 4}

# Sub, Up and Paeth tie below None in row 1: Pillow writes 2 for it (row 0 is None).
TIE_UP = np.repeat(np.array([[100, 0], [100, 100]], np.uint8)[..., None], 3, -1)
# Above a row of zeros the Paeth predictor of (a, 0, 0) is a, so Paeth = Sub byte for byte; here both score half of None = Up:
# exactly those two tie, in row 0 (the implicit zeros) and in row 2 (a real row of zeros above).  Row 1 is zeros: None.
TIE_PAETH = np.repeat(np.array([[100, 100, 100], [0, 0, 0], [100, 100, 100]], np.uint8)[..., None], 3, -1)


def stream_bytes(px):
    return px * (1 + 3 * px)


@functools.lru_cache(maxsize=None)
def tile(px, what):
    """uint8 [px, px, 3], read-only: tests/_jpeg_encode_cases.py's contents, and 'rows': one noise row repeated (Up is all zeros)."""
    if what != 'rows':
        return ec.tile(px, what)
    row = np.random.default_rng(77 + px).integers(0, 256, (1, px, 3), dtype=np.uint8)
    t = np.ascontiguousarray(np.repeat(row, px, 0))
    t.flags.writeable = False
    return t


def batches(px):
    """The contents of one size as lists of names, one list per encoder call."""
    if px != 299:
        return [list(CONTENTS)]
    return [list(CONTENTS[i:i + BATCH_299]) for i in range(0, len(CONTENTS), BATCH_299)]


def pillow_file(t, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.asarray(t)).save(b, 'PNG', **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pillow_rows(px, what):
    """The filtered scanlines Pillow writes for the tile (``tfrecord.encode_image(tile, 'PNG')``): the oracle of the rows."""
    from biscuit_amd import tfrecord as tfr
    return rows(tfr.encode_image(tile(px, what), 'PNG'))


def chunks(raw):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC-32 and that nothing follows IEND."""
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    p, out = 8, []
    while p < len(raw):
        n, = struct.unpack('>I', raw[p:p + 4])
        kind, data = raw[p + 4:p + 8], raw[p + 8:p + 8 + n]
        assert len(data) == n and struct.unpack('>I', raw[p + 8 + n:p + 12 + n])[0] == zlib.crc32(kind + data), (kind, p)
        out.append((kind, data))
        p += 12 + n
    assert p == len(raw)
    return out


def zstream(raw):
    return b''.join(d for k, d in chunks(raw) if k == b'IDAT')


def rows(raw):
    """The filtered scanlines of a file: its IDAT payloads, concatenated, through zlib."""
    return zlib.decompress(zstream(raw))


def check_container(raw, px):
    """IHDR (8-bit RGB, no interlace), IDAT+, IEND and nothing else; a 32 KB-window zlib header."""
    ch = chunks(raw)
    kinds = [k for k, _ in ch]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and len(kinds) >= 3 and set(kinds[1:-1]) == {b'IDAT'}, kinds
    assert ch[0][1] == struct.pack('>IIBBBBB', px, px, 8, 2, 0, 0, 0) and ch[-1][1] == b''
    z = zstream(raw)
    assert z[0] == 0x78 and ((z[0] << 8) | z[1]) % 31 == 0 and not z[1] & 0x20


def pillow_pixels(raw):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)).convert('RGB'))


def natural(seed):
    """A 299-px photo-like tile (the benchmark's synthetic tissue)."""
    from biscuit_amd.synthetic import make_tiles
    return np.ascontiguousarray(make_tiles(1, seed=seed, grain=4.0)[0])


def pack_streams(streams):
    """zlib streams -> (z uint8, off int32, len int32) in the layout of bqio_extract_z: 16-byte aligned starts, >= 32 zero bytes behind."""
    off, parts, at = [], [], 0
    for s in streams:
        off.append(at)
        pad = (-len(s)) % 16 + 32
        parts.append(s + b'\0' * pad)
        at += len(s) + pad
    return (np.frombuffer(b''.join(parts), np.uint8).copy(), np.asarray(off, np.int32), np.asarray([len(s) for s in streams], np.int32))


split = ec.split
mixed = ec.mixed
