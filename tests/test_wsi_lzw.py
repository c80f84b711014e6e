"""LZW pages in the slide reader (``biscuit_amd/wsi.py``, TIFF compression 5): striped pyramids Pillow (libtiff) writes and
hand-assembled TILED pages -- plain and BigTIFF, both byte orders, border tiles, predictor 1 and 2 -- against libtiff's read of the
very same file (through Pillow); what is refused at open time and what a damaged segment ends in; ``region_segments`` for the
device decoder.  The codec itself is tests/test_lzw.py's."""
import numpy as np
import pytest
from PIL import Image

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI, BandSegments, SlideError, TiffSlide
from tests import _lzw_cases as lc
from tests.test_wsi import _img

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


def _pillow_pages(path):
    ref = Image.open(path)
    out = []
    for k in range(getattr(ref, 'n_frames', 1)):
        ref.seek(k)
        out.append(np.asarray(ref.convert('RGB')).copy())
    return out


@pytest.mark.parametrize('predictor', [1, 2])
def test_pillow_written_lzw_pyramid_reads_like_libtiff(tmp_path, predictor):
    a = _img(1000, 700, 1)
    levels = [Image.fromarray(a), Image.fromarray(a).resize((500, 350), Image.BILINEAR), Image.fromarray(a).resize((250, 175), Image.BILINEAR)]
    path = str(tmp_path / 's.tif')
    levels[0].save(path, format='TIFF', compression='tiff_lzw', save_all=True, append_images=levels[1:], dpi=(25400 / 0.5, 25400 / 0.5),
                   tiffinfo={317: predictor})
    want = _pillow_pages(path)
    with TiffSlide(path) as s:
        assert s.level_dimensions == [(1000, 700), (500, 350), (250, 175)] and abs(s.mpp - 0.5) < 1e-6
        assert all(p.compression == 5 and p.predictor == predictor and not p.tiled for p in s.levels)
        assert len(s.levels[0].offsets) > 1                               # several strips, the last one shorter or not
        for li, (w, h) in enumerate(s.level_dimensions):
            got = s.read_region(li, 0, 0, w, h)
            assert np.array_equal(got, want[li]), li
            win = s.read_region(li, w - 40, h - 30, 100, 80)              # across strip borders, partly outside: white outside
            assert np.array_equal(win[:30, :40], got[h - 30:, w - 40:]) and (win[30:] == 255).all() and (win[:, 40:] == 255).all()
        assert s.region_segments(0, 0, 0, 100, 100) is None                # strips stay on read_region
    assert np.array_equal(want[0], a)


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('big,endian', [(False, '<'), (True, '<'), (False, '>'), (True, '>')])
def test_tiled_lzw_pages_read_like_libtiff(tmp_path, big, endian, predictor):
    a = _img(300, 210, 2)
    b = np.asarray(Image.fromarray(a).resize((150, 105), Image.BILINEAR))
    pages = [lc.page(a, 128, 64, predictor, desc='Aperio Image Library v1\n300x210 |AppMag = 20|MPP = 0.4990'), lc.page(b, 64, 64, predictor),
             lc.page(np.zeros((52, 150, 3), np.uint8), 150, 52, 1, tiled=False, desc='label 150x52')]
    path = lc.write_slide(tmp_path / 't.svs', pages, big=big, endian=endian)
    if big and endian == '>':
        # Pillow (12.2) does not open a big-endian BigTIFF, whatever its compression (it looks for the magic 43 in the header's third
        # byte, where only a little-endian file has it): for this one combination libtiff reads the same pages, the very same
        # segment bytes, from the classic big-endian file
        with pytest.raises(Exception):
            with pytest.warns(UserWarning):
                Image.open(path)
        want = _pillow_pages(lc.write_slide(tmp_path / 'classic.tif', pages, big=False, endian=endian))
    else:
        want = _pillow_pages(path)                                         # libtiff reads the hand-assembled file, tiles and all
    assert np.array_equal(want[0], a) and np.array_equal(want[1], b)
    with TiffSlide(path) as s:
        assert s.level_dimensions == [(300, 210), (150, 105)] and abs(s.mpp - 0.499) < 1e-9
        assert np.array_equal(s.read_region(0, 0, 0, 300, 210), want[0]) and np.array_equal(s.read_region(1, 0, 0, 150, 105), want[1])
        assert np.array_equal(s.read_region(0, 120, 60, 20, 20), a[60:80, 120:140])       # across four tiles
        edge = s.read_region(0, 250, 180, 80, 60)                          # border tiles: their padding never shows
        assert np.array_equal(edge[:30, :50], a[180:, 250:]) and (edge[30:] == 255).all() and (edge[:, 50:] == 255).all()
        sg = s.region_segments(0, 100, 50, 150, 100)
        assert isinstance(sg, BandSegments) and sg.codec == 'lzw' and sg.predictor == predictor and (sg.seg_w, sg.seg_h) == (128, 64)
        assert len(sg) == 6 and sg.place.tolist()[0] == [-100, -50] and not sg.ycc
        # the segments decoded one by one and placed give the region
        canvas = np.full((100, 150, 3), 255, np.uint8)
        packed, desc = tn.lzw_pack(sg.data, sg.offsets, sg.lengths)
        status = tn.lzw_decode_canvas(packed, desc, sg.seg_w, sg.seg_h, sg.place, canvas, sg.clip, predictor=sg.predictor)
        assert not status.any() and np.array_equal(canvas, s.read_region(0, 100, 50, 150, 100))


def test_band_segments_keeps_its_constructor():
    """``predictor`` is a new field with a default: a call without it stays valid."""
    sg = BandSegments(shape=(1, 1), data=np.zeros(0, np.uint8), offsets=np.zeros(0, np.uint64), lengths=np.zeros(0, np.uint64),
                      place=np.zeros((0, 2), np.int32), clip=(0, 0, 1, 1), seg_w=1, seg_h=1, jpeg_tables=None)
    assert (sg.codec, sg.ycc, sg.predictor) == ('jpeg', False, 1)


def test_refusals_at_open(tmp_path, monkeypatch):
    a = _img(64, 64, 4)
    good = lc.encode(a.tobytes())
    cases = [('pred3', dict(w=64, h=64, tw=64, th=64, comp=5, predictor=3, segs=[good]), 'predictor 3'),
             ('ycbcr', dict(w=64, h=64, tw=64, th=64, comp=5, photometric=6, segs=[good]), 'LZW-compressed YCbCr'),
             ('old', dict(w=64, h=64, tw=64, th=64, comp=5, segs=[b'\x00\x01' + good[2:]]), 'old-style'),
             ('damaged', dict(w=64, h=64, tw=64, th=64, comp=5, segs=[b'\x81' + good[1:]]), 'LZW.*ClearCode'),
             ('empty', dict(w=64, h=64, tw=64, th=64, comp=5, segs=[b'']), 'LZW'),
             ('second', dict(w=64, h=64, tw=32, th=32, comp=5, segs=[b'\x80\x00'] * 3), 'cover')]
    for name, pg, msg in cases:
        path = lc.write_slide(tmp_path / f'{name}.tif', [pg])
        with pytest.raises(SlideError, match=msg):
            TiffSlide(path)
    # a level whose FIRST segment passes the probe opens; the damage shows where it is read
    path = lc.write_slide(tmp_path / 'later.tif', [dict(w=64, h=64, tw=32, th=32, comp=5, segs=[lc.encode(a[:32, :32].tobytes()), b'x' * 10,
                                                                                                 good[:50], lc.encode(a[32:, 32:].tobytes())])])
    with TiffSlide(path) as s:
        assert np.array_equal(s.read_region(0, 0, 0, 32, 32), a[:32, :32]) and np.array_equal(s.read_region(0, 32, 32, 32, 32), a[32:, 32:])
        with pytest.raises(SlideError, match=r'later\.tif: damaged LZW segment 1 of level 0.*ClearCode'):
            s.read_region(0, 32, 0, 32, 32)
        with pytest.raises(SlideError, match=r'damaged LZW segment 2 of level 0.*ends before'):
            s.read_region(0, 0, 32, 32, 32)
    # without libbiscuit_io the page is refused with a message that says so
    good_path = lc.write_slide(tmp_path / 'good.tif', [dict(w=64, h=64, tw=64, th=64, comp=5, segs=[good])])
    TiffSlide(good_path).close()
    monkeypatch.setattr(tn, 'available', lambda: False)
    with pytest.raises(SlideError, match='libbiscuit_io.*not built'):
        TiffSlide(good_path)


def test_mutated_lzw_slide_files_fail_with_slide_errors_only(tmp_path):
    """The mutation test of tests/test_wsi.py on an LZW slide: bytes flipped anywhere, or the file cut: pixels or ``SlideError``."""
    path, _, _ = lc.slide_file(tmp_path, 0.5045, w=600, h=420, tile=256)
    good = bytearray(open(path, 'rb').read())
    rng = np.random.default_rng(0)
    spots = np.concatenate([rng.integers(0, 16, 40), rng.integers(len(good) - 1200, len(good), 300), rng.integers(0, len(good), 160)])
    outcomes = {'ok': 0, 'refused': 0}
    for k, at in enumerate(spots):
        bad = bytearray(good)
        bad[int(at)] ^= int(rng.integers(1, 256))
        if k % 5 == 0:
            bad = bad[:int(at)]
        p = tmp_path / 'm.svs'
        p.write_bytes(bytes(bad))
        try:
            w = WSI(str(p), 299, 302)
            if w.estimated_num_tiles:
                next(iter(w.build_generator()()))
            w.close()
            outcomes['ok'] += 1
        except SlideError:
            outcomes['refused'] += 1
    assert outcomes['ok'] > 20 and outcomes['refused'] > 20, outcomes
