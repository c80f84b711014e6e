"""Fixtures shared by tests/test_wsi_jpeg_segments.py, tests/test_gpu_wsi_jpeg.py and tools/fuzz/make_wsi_jpeg_corpus.py: hand-assembled
TIFF pages whose tiles are JPEG segments Pillow wrote -- abbreviated streams plus ``JPEGTables`` or complete streams, at the three
samplings -- with border tiles padded by a non-white value, so that a decoder that shows the padding is caught."""
import io

import numpy as np
from PIL import Image

from tests.test_wsi import _img, _tiff, _tiles_of

SAMPLINGS = {'444': 0, '422': 1, '420': 2}
# (page w, page h, segment w, segment h): a single 4:2:0 MCU, 64 x 64, Aperio's 240 x 240, rectangular; every page's size is
# no multiple of its segment's
SHAPES = [(40, 23, 16, 16), (100, 70, 64, 64), (500, 300, 240, 240), (600, 420, 256, 128)]


def jpeg(t, quality=85, subsampling=0, streamtype=0, **kw):
    bb = io.BytesIO()
    Image.fromarray(t).save(bb, format='JPEG', quality=quality, subsampling=subsampling, streamtype=streamtype, **kw)
    return bb.getvalue()


def tables_of(tw, th, quality=85, subsampling=0):
    """The tables-only stream (``JPEGTables``) of the encoder settings the page's tiles are written with."""
    return jpeg(np.zeros((th, tw, 3), np.uint8), quality, subsampling, streamtype=1)


def page(a, tw, th, subsampling, form='abbreviated', quality=85, **extra):
    """One tiled JPEG page dict for ``_tiff`` over image ``a``: ``form`` 'abbreviated' (tiles without tables + JPEGTables) or
    'complete' (whole streams, no JPEGTables)."""
    h, w = a.shape[:2]
    if form == 'abbreviated':
        segs = _tiles_of(a, tw, th, lambda t: jpeg(t, quality, subsampling, streamtype=2))
        assert all(b'\xff\xdb' not in s[:64] for s in segs)
        return dict(w=w, h=h, tw=tw, th=th, comp=7, photometric=6, segs=segs, tables=tables_of(tw, th, quality, subsampling), **extra)
    segs = _tiles_of(a, tw, th, lambda t: jpeg(t, quality, subsampling))
    return dict(w=w, h=h, tw=tw, th=th, comp=7, photometric=6, segs=segs, **extra)


def write_slide(path, pages):
    with open(path, 'wb') as f:
        f.write(_tiff(pages))
    return str(path)


def slide_file(tmp_path, mpp, w=2400, h=1800, mutate=None, name='slide.svs'):
    """The two-level slide of ``tests.test_wsi._slide_file`` with JPEG tiles: 256 x 256, 4:2:0 at level 0 and 4:4:4 at level 1.
    ``mutate(pages)`` may change the page dicts before the file is assembled."""
    a = _img(w, h, 5)
    b = np.asarray(Image.fromarray(a).resize((w // 4, h // 4), Image.BILINEAR))
    pages = [page(a, 256, 256, 2, desc=f'Aperio |MPP = {mpp}'), page(b, 256, 256, 0)]
    if mutate:
        mutate(pages)
    return write_slide(tmp_path / name, pages)


def windows(w, h, tw, th):
    """(x, y, w, h) regions: the whole level, strictly inside one segment, across four segments (or as many as the page has),
    10 pixels outside the image on every side."""
    return [(0, 0, w, h), (2, 3, min(tw, w) - 5, min(th, h) - 6), (tw - 7, th - 5, min(15, w - tw + 7), min(11, h - th + 5)),
            (-10, -10, w + 20, h + 20)]
