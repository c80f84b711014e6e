"""Shared by tests/test_jpeg_extract.py (CPU) and tests/test_gpu_jpeg.py: the encodings of tests/test_jpeg.py's matrix, the
byte-flipped files of its damaged-stream test (same seed, same recipe), and the extract step over a list of JPEG files."""
import io
import random

import numpy as np

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn

SIZES = (299, 300, 64, 33, 17)


def photo(px, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:px, 0:px]
    base = np.stack([128 + 100 * np.sin(x / 17.0 + c) + 20 * np.cos(y / 9.0 * c + 1) for c in range(3)], -1)
    base[: px // 4] = 200
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def noise(px, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (px, px, 3), dtype=np.uint8)


def enc(a, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, format='JPEG', **kw)
    return b.getvalue()


def pillow(raw):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)).convert('RGB'))


def matrix(px):
    """[(raw, (q, ss, opt))]: photo-like / noise x quality 30 / 75 / 95 / 100 x 4:4:4 / 4:2:2 / 4:2:0 x default / optimised tables;
    only Pillow's own OSError on tiny incompressible inputs drops a case, as in tests/test_jpeg.py."""
    out = []
    for img in (photo(px), noise(px, 1)):
        for q in (30, 75, 95, 100):
            for ss in (0, 1, 2):
                for opt in (False, True):
                    try:
                        out.append((enc(img, quality=q, subsampling=ss, optimize=opt), (q, ss, opt)))
                    except OSError:
                        continue
    return out


def saturated():
    sat = np.zeros((299, 299, 3), np.uint8)
    cols = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)]
    for i in range(299 // 13 + 1):
        for j in range(299 // 13 + 1):
            sat[13 * i: 13 * i + 13, 13 * j: 13 * j + 13] = cols[(3 * i + j) % 8]
    return [enc(sat, quality=60, subsampling=ss) for ss in (0, 1, 2)]


def byte_flipped(n=600):
    """The files of test_jpeg.py::test_damaged_streams_agree_or_are_refused: seed 7, 1-4 random bytes of a quality-85 tile replaced."""
    raw = enc(photo(299, 4), quality=85)
    rnd = random.Random(7)
    out = []
    for _ in range(n):
        b = bytearray(raw)
        for _ in range(rnd.randint(1, 4)):
            b[rnd.randrange(2, len(b))] = rnd.randrange(256)
        out.append(bytes(b))
    return out


def extract(path, first, count, px):
    """(scan, desc, tables) of records [first, first + count), in buffers of exactly the sizes the extractor asks for."""
    with tn.NativeReader(path) as r:
        used, nt, _ = r.extract_jpeg(first, count, px, None, None, None)
        scan, desc = np.zeros(used, np.uint8), np.zeros((count, 4), np.uint32)
        tables = np.zeros((nt, tn.jpeg_table_bytes()), np.uint8)
        assert r.extract_jpeg(first, count, px, scan, desc, tables)[:2] == (used, nt)
    return scan, desc, tables


def extract_each(tmp_path, raws, px, name='each'):
    """Every file on its own (a refused record fails a whole call): [(scan, desc, tables) | the exception]."""
    path = str(tmp_path / f'{name}.tfrecords')
    tfr.write_slide(path, name, list(raws), np.zeros((len(raws), 2), np.int64))
    out = []
    for i in range(len(raws)):
        try:
            out.append(extract(path, i, 1, px))
        except (tn.UnsupportedImage, ValueError) as e:
            out.append(e)
    return out


def pack(parts):
    """Several single-call extractions side by side in one buffer: (scan, desc, tables) with offsets and table indices moved."""
    scans, descs, tabs, at, nt = [], [], [], 0, 0
    for scan, desc, tables in parts:
        d = desc.copy()
        d[:, 0] += np.uint32(at)
        d[:, 3] += np.uint32(nt)
        scans.append(scan); descs.append(d); tabs.append(tables)
        at += scan.size; nt += tables.shape[0]
    return np.concatenate(scans), np.concatenate(descs), np.concatenate(tabs)
