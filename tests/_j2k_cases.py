"""The forge shared by tests/test_j2k.py (CPU), tests/test_gpu_j2k.py, tools/bench_j2k.py and tools/fuzz/make_j2k_corpus.py: JPEG 2000
codestreams Pillow (OpenJPEG) writes, hand-assembled TIFF pages and slide files whose tiles they are (in the manner of tests/_wsi_jpeg_cases.py), the
thinned case lists, and the hand-patched streams outside the device decoder's subset."""
import io
import struct

import numpy as np
from PIL import Image

from tests.test_wsi import _img, _tiff, _tiles_of

PROGRESSIONS = ('LRCP', 'RLCP', 'RPCL', 'PCRL', 'CPRL')


def content(kind, w, h, seed=0):
    """uint8 [h, w, 3]: 'flat', 'noise', 'gradient', 'photo' (smooth structure plus grain) or 'white'."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'flat':
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    if kind == 'white':
        return np.full((h, w, 3), 255, np.uint8)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'gradient':
        return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    assert kind == 'photo'
    return _img(w, h, seed)


def j2k(a, **kw):
    """The raw codestream Pillow writes for uint8 [h, w, 3] (or [h, w], or [h, w, 4]) ``a``."""
    bb = io.BytesIO()
    Image.fromarray(a).save(bb, 'JPEG2000', no_jp2=True, **kw)
    return bb.getvalue()


def pillow(raw):
    """Pillow's decode of a codestream, samples as they are."""
    return np.asarray(Image.open(io.BytesIO(raw)))


def pillow_ycc(raw):
    """Pillow's decode of a codestream whose components are YCbCr, converted as Pillow converts."""
    a = pillow(raw)
    return np.asarray(Image.merge('YCbCr', [Image.fromarray(np.ascontiguousarray(a[:, :, c])) for c in range(3)]).convert('RGB'))


def ycc_of(a):
    """RGB -> the YCbCr samples a 33003 tile stores (Pillow's conversion)."""
    return np.asarray(Image.fromarray(a).convert('YCbCr'))


# ---- the thinned cross-product: (w, h, content, encoder keywords) ----------------------------------------------------------------
# every value of every axis appears at least once with a non-square size; num_resolutions 6 needs 32 samples a side (OpenJPEG
# refuses to write more levels than the image has)
REVERSIBLE = [
    (1, 1, 'noise', dict(num_resolutions=1)),
    (1, 1, 'white', dict(num_resolutions=1, mct=1)),
    (7, 5, 'noise', dict(num_resolutions=2, mct=1)),
    (7, 5, 'photo', dict(num_resolutions=1, codeblock_size=(4, 4))),
    (33, 17, 'photo', dict(num_resolutions=2, codeblock_size=(4, 4), progression='RLCP')),
    (33, 17, 'noise', dict(num_resolutions=1, mct=1, codeblock_size=(16, 64), progression='CPRL')),
    (65, 64, 'noise', dict(num_resolutions=1, codeblock_size=(64, 64))),
    (65, 64, 'photo', dict(num_resolutions=6, mct=1, progression='RPCL')),
    (64, 65, 'gradient', dict(num_resolutions=2, codeblock_size=(32, 32), progression='PCRL')),
    (64, 65, 'flat', dict(num_resolutions=6, mct=0, quality_layers=[40, 10, 0])),
    (240, 240, 'photo', dict(num_resolutions=6, mct=1, codeblock_size=(64, 64))),
    (256, 256, 'photo', dict(num_resolutions=6, mct=1, codeblock_size=(32, 32), quality_layers=[40, 10, 0], progression='RLCP')),
    (256, 256, 'white', dict(num_resolutions=6, mct=1)),
    (300, 200, 'photo', dict(num_resolutions=6, mct=1, codeblock_size=(64, 64), progression='LRCP')),
    (300, 200, 'noise', dict(num_resolutions=2, mct=0, codeblock_size=(16, 64), progression='RPCL', precinct_size=(64, 64))),
    (300, 200, 'gradient', dict(num_resolutions=6, mct=1, codeblock_size=(32, 32), progression='PCRL', precinct_size=(128, 128), quality_layers=[40, 10, 0])),
    (300, 200, 'flat', dict(num_resolutions=1, mct=1, codeblock_size=(4, 4), progression='CPRL')),
    (300, 200, 'white', dict(num_resolutions=6, mct=0, progression='RLCP')),
    (200, 300, 'photo', dict(num_resolutions=2, mct=1, codeblock_size=(16, 64), progression='CPRL', quality_layers=[40, 10, 0])),
]

IRREVERSIBLE = [
    (1, 1, 'noise', dict(num_resolutions=1)),
    (7, 5, 'photo', dict(num_resolutions=2, mct=1)),
    (33, 17, 'noise', dict(num_resolutions=2, codeblock_size=(4, 4), progression='RLCP')),
    (33, 17, 'photo', dict(num_resolutions=1, mct=1, codeblock_size=(16, 64))),
    (65, 64, 'photo', dict(num_resolutions=6, mct=1, progression='RPCL')),
    (64, 65, 'gradient', dict(num_resolutions=2, codeblock_size=(32, 32), progression='PCRL')),
    (64, 65, 'flat', dict(num_resolutions=6, mct=0)),
    (240, 240, 'photo', dict(num_resolutions=6, mct=1, quality_mode='rates', quality_layers=[8])),
    (256, 256, 'photo', dict(num_resolutions=6, mct=1, codeblock_size=(32, 32), quality_mode='rates', quality_layers=[20, 8], progression='RLCP')),
    (256, 256, 'white', dict(num_resolutions=6, mct=1)),
    (300, 200, 'photo', dict(num_resolutions=6, mct=1, quality_mode='dB', quality_layers=[30])),
    (300, 200, 'photo', dict(num_resolutions=6, mct=0, quality_mode='dB', quality_layers=[30, 45], progression='CPRL')),
    (300, 200, 'noise', dict(num_resolutions=2, mct=0, codeblock_size=(16, 64), progression='RPCL', precinct_size=(64, 64), quality_mode='rates', quality_layers=[20])),
    (300, 200, 'gradient', dict(num_resolutions=6, mct=1, codeblock_size=(32, 32), progression='PCRL', precinct_size=(128, 128), quality_mode='dB', quality_layers=[45])),
    (300, 200, 'flat', dict(num_resolutions=1, mct=1, codeblock_size=(4, 4), progression='LRCP')),
    (300, 200, 'white', dict(num_resolutions=6, mct=1)),
    (200, 300, 'noise', dict(num_resolutions=6, mct=1, codeblock_size=(64, 64), quality_mode='rates', quality_layers=[20, 8])),
]

# the GPU's thinned list: (w, h, content, irreversible, ycc, keywords)
GPU_CASES = [
    (1, 1, 'noise', False, False, dict(num_resolutions=1)),
    (65, 64, 'photo', False, False, dict(num_resolutions=6, mct=1, progression='RPCL')),
    (65, 64, 'noise', True, False, dict(num_resolutions=1, mct=0)),
    (300, 200, 'photo', False, True, dict(num_resolutions=6, mct=0, codeblock_size=(32, 32), quality_layers=[40, 10, 0])),
    (300, 200, 'photo', True, False, dict(num_resolutions=6, mct=1, quality_mode='rates', quality_layers=[40, 20, 8])),
    (300, 200, 'white', False, False, dict(num_resolutions=6, mct=1)),
    (300, 200, 'noise', True, True, dict(num_resolutions=2, mct=0, codeblock_size=(16, 64), progression='PCRL', precinct_size=(64, 64))),
]


def encode(a, irreversible, **kw):
    return j2k(a, irreversible=irreversible, **kw)


# ---- pages and slide files -------------------------------------------------------------------------------------------------------
def page(a, tw, th, comp=33005, **kw):
    """One tiled JPEG 2000 page dict for ``tests.test_wsi._tiff`` over RGB image ``a``; ``comp`` 33003 stores YCbCr components
    (``mct=0``), 33005 / 34712 RGB.  Extra ``desc`` goes to the page, the rest to the encoder."""
    h, w = a.shape[:2]
    extra = {k: kw.pop(k) for k in ('desc',) if k in kw}
    kw.setdefault('irreversible', False)
    if comp == 33003:
        kw['mct'] = 0
        segs = _tiles_of(a, tw, th, lambda t: j2k(ycc_of(t), **kw))
    else:
        segs = _tiles_of(a, tw, th, lambda t: j2k(t, **kw))
    return dict(w=w, h=h, tw=tw, th=th, comp=comp, photometric=6 if comp == 33003 else 2, segs=segs, **extra)


def write_slide(path, pages):
    with open(path, 'wb') as f:
        f.write(_tiff(pages))
    return str(path)


def slide_file(tmp_path, mpp, w=600, h=450, tile=64, comp=33005, mutate=None, name='j2k.svs', seed=5, **kw):
    """A two-level JPEG 2000 slide: level 0 ``w`` x ``h`` (no multiple of the tile), level 1 a quarter of it.  -> (path, level-0
    pixels, level-1 pixels).  ``mutate(pages)`` may change the page dicts before the file is assembled."""
    a = _img(w, h, seed)
    b = np.asarray(Image.fromarray(a).resize((w // 4, h // 4), Image.BILINEAR))
    pages = [page(a, tile, tile, comp, desc=f'Aperio |MPP = {mpp}', **kw), page(b, tile, tile, comp, **kw)]
    if mutate:
        mutate(pages)
    return write_slide(tmp_path / name, pages), a, b


# ---- streams outside the subset ---------------------------------------------------------------------------------------------------
def marker_at(raw, marker):
    """Offset of the first marker segment ``marker`` (two bytes) in the main header of a codestream."""
    pos = 2
    while raw[pos:pos + 2] != marker:
        assert raw[pos] == 0xFF and raw[pos:pos + 2] != b'\xff\x90', 'marker not in the main header'
        pos += 2 + struct.unpack('>H', raw[pos + 2:pos + 4])[0]
    return pos


def patched(raw, marker, offset, value):
    """``raw`` with the byte ``offset`` bytes behind the marker's length field set to ``value``."""
    at = marker_at(raw, marker) + 4 + offset
    return raw[:at] + bytes([value]) + raw[at + 1:]


def refusals(w=64, h=64):
    """name -> (codestream of w x h, expected status of the extractor: 32 outside the subset, 64 damaged)."""
    a = content('photo', w, h, 3)
    good = j2k(a, irreversible=False, num_resolutions=3)
    cod, sot = b'\xff\x52', good.index(b'\xff\x90')
    out = {
        'tiles': (j2k(a, irreversible=False, tile_size=(32, 32)), 32),
        'gray': (j2k(a[:, :, 0], irreversible=False), 32),
        'rgba': (j2k(np.dstack([a, a[:, :, :1]]), irreversible=False), 32),
        'sixteen': (j2k(a[:, :, 0].astype(np.uint16) * 257, irreversible=False), 32),
        'cblk_style': (patched(good, cod, 8, 1), 32),                 # SPcod: selective arithmetic coding bypass
        'sop': (patched(good, cod, 0, 2), 32),                        # Scod bit 1
        'eph': (patched(good, cod, 0, 4), 32),                        # Scod bit 2
        'truncated': (good[:sot + 14 + (len(good) - sot - 14) // 2], 64),
        'psot_past_end': (good[:sot + 6] + struct.pack('>I', len(good)) + good[sot + 10:], 64),
        'garbage': (b'x' * 10, 64),
    }
    return good, out
