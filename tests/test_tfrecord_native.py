"""libbiscuit_io.so (include/biscuit_io.h): native TFRecord framing / Example parse / PNG decode against
the pure-Python reader and Pillow on self-written records (there are no real TFRecords here)."""
import io
import os
import re
import struct

import numpy as np
import pytest

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


def _tiles(n, seed=0, px=299):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (n, px, px, 3), dtype=np.uint8)
    t[:, :, : px // 2] = (t[:, :, : px // 2] // 32) * 32          # smooth areas: every PNG filter type gets used
    t[:, : px // 3] = np.linspace(0, 255, px, dtype=np.uint8)[None, None, :, None]
    return t


def test_header_symbols_exported():
    text = open(os.path.join(os.path.dirname(tn.LIB_PATH), '..', 'include', 'biscuit_io.h')).read()
    declared = set(re.findall(r'\b(bqio_[a-z0-9_]+)\s*\(', text))
    assert declared == set(tn.ABI), declared ^ set(tn.ABI)
    tn.load()        # every declared symbol resolves


def test_abi_types_are_the_headers():
    """Every restype and argtype of ``tfrecord_native.ABI`` has the width class of the prototype's type at that position."""
    from tests._abi_types import assert_abi_matches_header
    assert_abi_matches_header(tn.ABI, os.path.join(os.path.dirname(tn.LIB_PATH), '..', 'include', 'biscuit_io.h'))


def test_crc_matches_python():
    for data in (b'', b'a', b'123456789', bytes(range(256)) * 7 + b'xyz'):
        assert tn.lib().bqio_masked_crc32c(data, len(data)) == tfr.masked_crc(data)
    assert tfr.crc32c(b'123456789') == 0xE3069283     # CRC-32C check value (RFC 3720)


def test_native_equals_python(tmp_path):
    tiles = _tiles(7, 1)
    locs = np.arange(14, dtype=np.int64).reshape(7, 2) * 302 - 5
    path = str(tmp_path / 's1.tfrecords')
    tfr.write_slide(path, 'slide-1', tiles, locs)
    with tn.NativeReader(path, verify='full') as r:
        assert len(r) == 7 and r.slide == 'slide-1'
        assert r.image_format(0) == tn.IMG_PNG
        assert r.image_bytes(3)[:8] == b'\x89PNG\r\n\x1a\n'
        got, gl = r.decode(threads=3)
        np.testing.assert_array_equal(got, tiles)
        np.testing.assert_array_equal(gl, locs)
        part, pl = r.decode(2, 3, threads=1)
        np.testing.assert_array_equal(part, tiles[2:5])
        np.testing.assert_array_equal(pl, locs[2:5])
        buf = np.zeros((7, 299, 299, 3), np.uint8)              # caller-owned (pinned) buffer
        out, _ = r.decode(out=buf)
        assert out is buf and np.array_equal(buf, tiles)
    name, t2, l2 = tfr.read_slide(path, native=True)
    name3, t3, l3 = tfr.read_slide(path, native=False)
    assert name == name3 == 'slide-1'
    np.testing.assert_array_equal(t2, t3)
    np.testing.assert_array_equal(l2, l3)


def _png(arr, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format='PNG', **kw)
    return b.getvalue()


def _write(path, payloads, slide='s'):
    with open(path, 'wb') as f:
        for raw in payloads:
            rec = tfr.encode_example(slide, raw, 1, 2)
            head = struct.pack('<Q', len(rec))
            f.write(head + struct.pack('<I', tfr.masked_crc(head)) + rec + struct.pack('<I', tfr.masked_crc(rec)))


def test_png_colour_types_and_filters(tmp_path):
    from PIL import Image
    rgb = _tiles(1, 2)[0]
    grey = rgb[..., 0]
    rgba = np.dstack([rgb, np.full(rgb.shape[:2], 200, np.uint8)])
    pal = Image.fromarray(rgb).quantize(64)
    b = io.BytesIO()
    pal.save(b, format='PNG')
    payloads = [_png(rgb, compress_level=1), _png(rgb, optimize=True), _png(grey), _png(rgba), b.getvalue()]
    path = str(tmp_path / 'types.tfrecords')
    _write(path, payloads)
    want = np.stack([rgb, rgb, np.repeat(grey[..., None], 3, 2), rgb, np.asarray(pal.convert('RGB'))])
    with tn.NativeReader(path) as r:
        got, _ = r.decode()
    np.testing.assert_array_equal(got, want)


def test_errors(tmp_path):
    tiles = _tiles(2, 3)
    path = str(tmp_path / 'ok.tfrecords')
    tfr.write_slide(path, 'x', tiles)
    raw = bytearray(open(path, 'rb').read())
    bad = str(tmp_path / 'bad.tfrecords')
    raw[40] ^= 0xFF                                   # payload byte of record 0
    open(bad, 'wb').write(raw)
    tn.NativeReader(bad, verify='length').close()     # header CRCs still fine
    with pytest.raises(IOError, match='corrupt record data'):
        tn.NativeReader(bad, verify='full')
    raw = bytearray(open(path, 'rb').read())
    raw[3] ^= 0x01                                    # length field
    open(bad, 'wb').write(raw)
    with pytest.raises(IOError):
        tn.NativeReader(bad, verify='length')
    open(bad, 'wb').write(open(path, 'rb').read()[:-9])
    with pytest.raises(IOError, match='truncated'):
        tn.NativeReader(bad)
    with pytest.raises(IOError):
        tn.NativeReader(str(tmp_path / 'missing.tfrecords'))
    # wrong tile size, JPEG payloads, empty file
    small = str(tmp_path / 'small.tfrecords')
    _write(small, [_png(tiles[0][:100, :100])])
    with tn.NativeReader(small) as r, pytest.raises(ValueError, match='tile size'):
        r.decode()
    from PIL import Image
    jb, pb = io.BytesIO(), io.BytesIO()
    Image.fromarray(tiles[0]).save(jb, format='JPEG', quality=95)
    Image.fromarray(tiles[0]).save(pb, format='JPEG', quality=95, progressive=True)
    mixed = str(tmp_path / 'mixed.tfrecords')
    _write(mixed, [_png(tiles[0]), jb.getvalue(), _png(tiles[1])])
    with tn.NativeReader(mixed) as r:                # PNG and baseline JPEG records side by side
        assert r.image_format(1) == tn.IMG_JPEG
        t, _ = r.decode()
    assert np.array_equal(t[0], tiles[0]) and np.array_equal(t[2], tiles[1])
    assert np.array_equal(t[1], np.asarray(Image.open(io.BytesIO(jb.getvalue())).convert('RGB')))
    prog = str(tmp_path / 'prog.tfrecords')
    _write(prog, [_png(tiles[0]), pb.getvalue()])
    with tn.NativeReader(prog) as r:                 # progressive: outside the native decoder's subset
        with pytest.raises(tn.UnsupportedImage) as ei:
            r.decode()
        assert ei.value.index == 1
    name, t, _ = tfr.read_slide(prog)                # ... so the slide is decoded with Pillow
    assert t.shape == (2, 299, 299, 3) and np.array_equal(t[0], tiles[0])
    assert np.array_equal(t[1], np.asarray(Image.open(io.BytesIO(pb.getvalue())).convert('RGB')))
    empty = str(tmp_path / 'empty.tfrecords')
    open(empty, 'wb').close()
    with tn.NativeReader(empty) as r:
        assert len(r) == 0 and r.slide is None
    assert tfr.read_slide(empty)[1].shape == (0, 299, 299, 3)


def test_mutated_files_never_crash(tmp_path):
    """Byte-mutated / truncated records must come back as errors, not as a crash of the process
    (the reader parses untrusted files in C++): decode them in a child process and check it survives."""
    import random
    import subprocess
    import sys
    tiles = _tiles(2, 5)
    path = str(tmp_path / 'a.tfrecords')
    tfr.write_slide(path, 's', tiles)
    raw = open(path, 'rb').read()
    rnd = random.Random(7)
    paths = []
    for k in range(120):
        b = bytearray(raw)
        for _ in range(rnd.choice([1, 2, 5, 20])):
            i = rnd.randrange(400) if rnd.random() < 0.4 else rnd.randrange(len(b))
            b[i] = rnd.randrange(256)
        if rnd.random() < 0.2:
            b = b[:rnd.randrange(len(b))]
        q = str(tmp_path / f'm{k}.tfrecords')
        open(q, 'wb').write(b)
        paths.append(q)
    code = (
        "import sys\n"
        "from biscuit_amd import tfrecord_native as tn\n"
        "for p in sys.argv[1:]:\n"
        "    try:\n"
        "        with tn.NativeReader(p, verify=None) as r:\n"
        "            for i in range(len(r)):\n"
        "                try: r.image_format(i); r.image_bytes(i)\n"
        "                except Exception: pass\n"
        "            try: r.slide; r.decode(threads=2)\n"
        "            except Exception: pass\n"
        "    except Exception: pass\n"
        "print('survived')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(tn.LIB_PATH)))
    out = subprocess.run([sys.executable, '-c', code] + paths, capture_output=True, text=True, cwd=root, timeout=300)
    assert out.returncode == 0 and 'survived' in out.stdout, out.stderr[-500:]


# ---- the reader's own zlib-stream decompressor (csrc/inflate_fast.h) against zlib ------------------------------------
def _streams():
    import zlib
    rng = np.random.default_rng(11)
    walk = np.clip(np.cumsum(rng.integers(-3, 4, 70000)), 0, 255).astype(np.uint8).tobytes()
    datas = [b'', b'a', b'ab' * 5, bytes(rng.integers(0, 256, 1000, dtype=np.uint8)), (b'hello world, ' * 6000)[:70000],
             bytes(rng.integers(0, 2, 66000, dtype=np.uint8)), walk, bytes(rng.integers(0, 256, 70000, dtype=np.uint8))]
    for d in datas:
        for level in (0, 1, 6, 9):
            for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
                co = zlib.compressobj(level=level, strategy=strat)
                yield d, co.compress(d) + co.flush()
        co = zlib.compressobj(level=6, wbits=9)               # 512-byte window: short distances only
        yield d, co.compress(d) + co.flush()


def test_inflate_equals_zlib():
    """Stored, fixed and dynamic blocks, every strategy zlib has, empty to multi-block inputs: identical bytes."""
    n = 0
    for data, z in _streams():
        assert tn.inflate(z, len(data)) == data
        n += 1
    assert n == 8 * 21


def test_inflate_rejects_what_zlib_rejects():
    """Flipped bits, truncations, wrong expected length, trailing bytes: the verdict is zlib's (and when both accept,
    the bytes are the same)."""
    import random
    import zlib
    data, z = next(s for s in _streams() if len(s[0]) == 70000 and len(s[1]) < 40000)
    rnd = random.Random(3)
    verdicts = [0, 0]
    for t in range(1500):
        b = bytearray(z)
        for _ in range(rnd.choice([1, 1, 3])):
            b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        if t % 5 == 0:
            b = b[:rnd.randrange(len(b))]
        try:
            ref = zlib.decompress(bytes(b))
            ref_ok = len(ref) == len(data)
        except zlib.error:
            ref_ok = False
        try:
            got = tn.inflate(bytes(b), len(data))
            ok = True
        except ValueError:
            ok = False
        assert ok == ref_ok, t
        if ok:
            assert got == ref
        verdicts[ok] += 1
    assert verdicts[0] > 1000
    for bad in (z + b'\0', z[:-1], z[:2] + z[3:]):
        with pytest.raises(ValueError):
            tn.inflate(bad, len(data))
    with pytest.raises(ValueError):
        tn.inflate(z, len(data) + 1)
    with pytest.raises(ValueError):
        tn.inflate(z, len(data) - 1)
    with pytest.raises(ValueError):
        tn.inflate(b'\x78\x9c' + b'\x07' * 20, 10)          # reserved block type


def test_every_png_filter_and_no_zlib_fallback(tmp_path):
    """Scanline filters None/Sub/Up/Average/Paeth forced one at a time (hand-made PNGs: Pillow picks filters itself),
    for grey, RGB and RGBA, against the arrays they encode; and the decoder never needed zlib as a second opinion."""
    import zlib
    rng = np.random.default_rng(4)
    px = 64

    def png(arr, ftype, ctype):
        h, w = arr.shape[:2]
        rows = arr.reshape(h, -1).astype(np.int32)
        bpp = rows.shape[1] // w
        out = bytearray()
        prev = np.zeros_like(rows[0])
        for y in range(h):
            cur = rows[y]
            left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
            ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
            if ftype == 0: f = cur
            elif ftype == 1: f = cur - left
            elif ftype == 2: f = cur - prev
            elif ftype == 3: f = cur - ((left + prev) >> 1)
            else:
                p = left + prev - ul
                pa, pb, pc = abs(p - left), abs(p - prev), abs(p - ul)
                f = cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
            out += bytes([ftype]) + (f & 255).astype(np.uint8).tobytes()
            prev = cur

        def chunk(t, d):
            return struct.pack('>I', len(d)) + t + d + struct.pack('>I', zlib.crc32(t + d))
        return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, ctype, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(bytes(out), 6)) + chunk(b'IEND', b''))

    base = (rng.integers(0, 256, (px, px, 4)) // 8 * 8).astype(np.uint8)
    base[:, : px // 2] = np.linspace(0, 255, px // 2, dtype=np.uint8)[None, :, None]
    payloads, want = [], []
    for ctype, arr in ((0, base[..., 0]), (2, base[..., :3]), (6, base)):
        for ftype in range(5):
            payloads.append(png(arr, ftype, ctype))
            want.append(np.repeat(arr[..., None], 3, 2) if ctype == 0 else arr[..., :3])
    path = str(tmp_path / 'filters.tfrecords')
    _write(path, payloads)
    before = tn.inflate_fallbacks()
    with tn.NativeReader(path) as r:
        got, _ = r.decode(tile_px=px)
    np.testing.assert_array_equal(got, np.stack(want))
    assert tn.inflate_fallbacks() == before == 0


def test_two_streams_in_one_loop():
    """bqio_decode inflates tiles in pairs (inflate_fast.h: run_symbols2).  Every pairing of streams of different
    block structure and length gives each stream what it gives alone -- also next to a corrupt or truncated partner."""
    import itertools
    import zlib
    streams = list(_streams())[::9]                     # 19 streams: every data kind, mixed levels / strategies
    assert len({len(d) for d, _ in streams}) >= 6
    for (da, za), (db, zb) in itertools.islice(itertools.product(streams, streams), 0, None, 7):
        a, b = tn.inflate2(za, len(da), zb, len(db))
        assert a == da and b == db
    data, z = next(s for s in _streams() if len(s[0]) == 70000 and len(s[1]) < 40000)
    bad = bytearray(z); bad[len(z) // 2] ^= 0x10
    for partner, plen in ((bytes(bad), len(data)), (z[:len(z) // 3], len(data)), (z, len(data) + 1), (b'', 0), (b'\x78\x9c\x07', 5)):
        a, b = tn.inflate2(z, len(data), partner, plen)
        assert a == data and b is None
        a, b = tn.inflate2(partner, plen, z, len(data))
        assert a is None and b == data
    try:
        ref = zlib.decompress(bytes(bad))
    except zlib.error:
        ref = None
    assert ref is None or ref != data


def test_chunk_source_probes_once_per_slide_whoever_opened_the_reader(tmp_path):
    """Round-5 advisory: ``TFRecordSource.z_ok()`` (the gpu_decode pre-check) opens the native reader; ``read()`` used to run the
    once-per-slide probe only when IT opened the reader, so a slide with a progressive JPEG beyond the first chunk -- which sends
    the WHOLE slide to Pillow -- raised UnsupportedImage mid-run under gpu_decode=True.  The probe has its own flag now."""
    from PIL import Image
    from biscuit_amd.inference import TFRecordSource
    from biscuit_amd.synthetic import make_tiles
    t = make_tiles(5, seed=12)
    b = io.BytesIO()
    Image.fromarray(t[3]).save(b, format='JPEG', quality=90, progressive=True)
    path = str(tmp_path / 'mixed.tfrecords')
    tfr.write_slide(path, 'mixed', [tfr.encode_image(t[0]), tfr.encode_image(t[1]), tfr.encode_image(t[2]), b.getvalue(),
                                    tfr.encode_image(t[4])])
    want = tfr.read_slide(path, 299)[1]
    for z in (True, False):
        src = TFRecordSource(path, 5, 299, rows=False, z=z)
        assert src.z_ok() is False                      # a JPEG record: never the compressed way
        out = np.zeros((5, 299, 299, 3), np.uint8)
        src.read(0, 2, out[:2])                         # first chunk: PNG records only
        src.read(2, 3, out[2:])                         # the progressive JPEG sits in the second chunk
        assert src._fallback is not None and np.array_equal(out, want)
        src.close()
    big = TFRecordSource(path, 5, 512, z=True)          # tiles the device un-filter cannot take (rows > 1 024 bytes): host decoder
    assert big.z_ok() is False


def test_extract_z_refuses_what_a_png_reader_may_refuse(tmp_path):
    """``bqio_extract_z`` hands a tile's zlib stream to the DEVICE as it is, so it checks more than the host decoder (round-5
    advisory): IHDR first and 13 bytes, compression / filter method 0, IDAT chunks consecutive, and -- for a reader opened with
    verify='full' -- the PNG chunk CRCs.  What it refuses goes to the host decoder (``TFRecordSource.z_ok`` is False)."""
    import zlib

    def chunk(tag, data, crc=None):
        c = zlib.crc32(tag + data) & 0xFFFFFFFF if crc is None else crc
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', c)
    px = 8
    img = np.random.default_rng(1).integers(0, 256, (px, px, 3), dtype=np.uint8)
    raw = b''.join(b'\x00' + img[y].tobytes() for y in range(px))
    z = zlib.compress(raw)
    sig = b'\x89PNG\r\n\x1a\n'
    ihdr = struct.pack('>IIBBBBB', px, px, 8, 2, 0, 0, 0)
    good = sig + chunk(b'IHDR', ihdr) + chunk(b'IDAT', z[:10]) + chunk(b'IDAT', z[10:]) + chunk(b'tEXt', b'k\0v') + chunk(b'IEND', b'')
    cases = {
        'good': (good, None),
        'split': (sig + chunk(b'IHDR', ihdr) + chunk(b'IDAT', z[:10]) + chunk(b'tEXt', b'k\0v') + chunk(b'IDAT', z[10:]) + chunk(b'IEND', b''), IOError),
        'late_ihdr': (sig + chunk(b'tEXt', b'k\0v') + chunk(b'IHDR', ihdr) + chunk(b'IDAT', z) + chunk(b'IEND', b''), IOError),
        'compression1': (sig + chunk(b'IHDR', struct.pack('>IIBBBBB', px, px, 8, 2, 1, 0, 0)) + chunk(b'IDAT', z) + chunk(b'IEND', b''), IOError),
        'filter1': (sig + chunk(b'IHDR', struct.pack('>IIBBBBB', px, px, 8, 2, 0, 1, 0)) + chunk(b'IDAT', z) + chunk(b'IEND', b''), IOError),
        'two_ihdr': (sig + chunk(b'IHDR', ihdr) + chunk(b'IHDR', ihdr) + chunk(b'IDAT', z) + chunk(b'IEND', b''), IOError),
    }
    for name, (png, err) in cases.items():
        path = str(tmp_path / f'{name}.tfrecords')
        tfr.write_slide(path, name, [png])
        with tn.NativeReader(path) as r:
            buf, off, ln = np.zeros(4096, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
            if err is None:
                used, _ = r.extract_z(0, 1, px, buf, off, ln)
                assert bytes(buf[off[0]:off[0] + ln[0]]) == z and used >= len(z) + 32
            else:
                with pytest.raises(err):
                    r.extract_z(0, 1, px, buf, off, ln)
    # a chunk CRC that does not match: caught when the reader verifies fully, Adler-32's business otherwise
    bad = sig + chunk(b'IHDR', ihdr) + chunk(b'IDAT', z, crc=0x12345678) + chunk(b'IEND', b'')
    path = str(tmp_path / 'badcrc.tfrecords')
    tfr.write_slide(path, 'badcrc', [bad])
    buf, off, ln = np.zeros(4096, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    with tn.NativeReader(path, verify='full') as r:
        with pytest.raises(IOError):
            r.extract_z(0, 1, px, buf, off, ln)
    with tn.NativeReader(path, verify='length') as r:
        assert r.extract_z(0, 1, px, buf, off, ln)[0] > 0
