"""A slide page's own JPEG tiles for the device decoder, on the CPU: ``bqio_extract_jpeg_segments`` (abbreviated streams plus the
page's ``JPEGTables``, rectangular tiles) and ``bqio_jpeg_decode_canvas`` (the device canvas decoder's routines, csrc/jpeg_device.h,
run by libbiscuit_io) against the path the heatmap has today, ``TiffSlide.read_region`` -- which is Pillow.  Every comparison is
byte equality; there is no tolerance."""
import numpy as np
import pytest

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI, TiffSlide
from tests._wsi_jpeg_cases import SAMPLINGS, SHAPES, jpeg, page, tables_of, windows, write_slide
from tests.test_wsi import _img, _tiles_of

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


def canvas_of(slide, level, x, y, w, h, threads=2):
    """``read_region``'s array through the new entries: segments -> extractor -> CPU canvas decode.  -> (canvas, status, segs)"""
    sg = slide.region_segments(level, x, y, w, h)
    assert sg is not None and sg.shape == (h, w)
    scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables, threads=threads)
    canvas = np.full((h, w, 3), 255, np.uint8)
    status = tn.jpeg_decode_canvas(scan, desc, tables, sg.seg_w, sg.seg_h, sg.place, canvas, sg.clip, threads=threads)
    return canvas, status, (sg, scan, desc, tables)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_%dx%d' % s)
@pytest.mark.parametrize('sampling', sorted(SAMPLINGS))
def test_canvas_equals_read_region(tmp_path, shape, sampling):
    w, h, tw, th = shape
    a = _img(w, h, 11)
    path = write_slide(tmp_path / 's.tif', [page(a, tw, th, SAMPLINGS[sampling])])
    with TiffSlide(path) as s:
        for (x, y, ww, hh) in windows(w, h, tw, th):
            want = s.read_region(0, x, y, ww, hh)
            got, status, (sg, _, desc, tables) = canvas_of(s, 0, x, y, ww, hh)
            assert (status == 0).all(), (x, y, status)
            assert np.array_equal(got, want), (x, y, ww, hh)
            assert len(tables) == 1 and (desc[:, 2] == ([1, 2, 2][SAMPLINGS[sampling]] | [1, 1, 2][SAMPLINGS[sampling]] << 8 | 3 << 16)).all()
        full = s.read_region(0, -10, -10, w + 20, h + 20)
        assert (full[:10] == 255).all() and (full[:, :10] == 255).all() and (full[h + 10:] == 255).all() and (full[:, w + 10:] == 255).all()
        # the windows count their segments as read_region walks them
        assert len(s.region_segments(0, 2, 3, min(tw, w) - 5, min(th, h) - 6)) == 1
        assert len(s.region_segments(0, tw - 7, th - 5, min(15, w - tw + 7), min(11, h - th + 5))) == 4
        assert len(s.region_segments(0, 0, 0, w, h)) == -(-w // tw) * -(-h // th)
    assert np.abs(want[10:-10, 10:-10].astype(int) - a.astype(int)).mean() < 12          # (and it is the picture)


@pytest.mark.parametrize('form', ['abbreviated', 'complete'])
def test_stream_forms(tmp_path, form):
    a = _img(200, 150, 12)
    path = write_slide(tmp_path / 's.tif', [page(a, 64, 64, 2, form=form)])
    with TiffSlide(path) as s:
        assert (s.levels[0].jpeg_tables is not None) == (form == 'abbreviated')
        got, status, _ = canvas_of(s, 0, -3, -4, 210, 160)
        assert (status == 0).all() and np.array_equal(got, s.read_region(0, -3, -4, 210, 160))


def test_a_segment_with_its_own_quantiser_stands_beside_the_others(tmp_path):
    a = _img(128, 128, 13)
    pg = page(a, 64, 64, 1)
    pg['segs'][2] = jpeg(a[64:128, 0:64], quality=40, subsampling=1)         # complete stream: its tables override the page's
    path = write_slide(tmp_path / 's.tif', [pg])
    with TiffSlide(path) as s:
        want = s.read_region(0, 0, 0, 128, 128)
        got, status, (_, _, desc, tables) = canvas_of(s, 0, 0, 0, 128, 128)
        assert (status == 0).all() and np.array_equal(got, want)
        assert len(tables) == 2 and desc[2, 3] != desc[0, 3] and desc[0, 3] == desc[1, 3] == desc[3, 3]
    other = write_slide(tmp_path / 'o.tif', [page(a, 64, 64, 1)])
    with TiffSlide(other) as s:
        assert not np.array_equal(s.read_region(0, 0, 64, 64, 64), want[64:, :64])      # (the other quality really shows)


def _refuse(tw, th, segs, tables, bad, errors):
    data = np.frombuffer(b''.join(segs), np.uint8)
    lengths = np.array([len(x) for x in segs], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    for probe in (False, True):
        with pytest.raises(errors) as e:
            tn.extract_jpeg_segments(data, offsets, lengths, tw, th, tables, probe=probe)
        assert e.value.index == bad


def test_refusals_name_the_first_refused_segment():
    t = _img(64, 64, 14)
    good = [jpeg(t, subsampling=2, streamtype=2)] * 3
    tables = tables_of(64, 64, subsampling=2)
    for k, bad in enumerate([jpeg(t, subsampling=2, streamtype=2, restart_marker_blocks=2),       # restart intervals
                             jpeg(t, subsampling=0, keep_rgb=True),                              # RGB coded
                             jpeg(np.ascontiguousarray(t[:, :, 0])),                              # grey
                             jpeg(t, subsampling=2, progressive=True)]):
        segs = list(good)
        segs.insert(1 + k % 3, bad)
        _refuse(64, 64, segs, tables, 1 + k % 3, tn.UnsupportedImage)
    # a 256 x 256 frame in a 240 x 240 page: the host path crops it, the device path does not take it
    big, small = _img(256, 256, 15), _img(240, 240, 15)
    segs = [jpeg(small, subsampling=2, streamtype=2), jpeg(small, subsampling=2, streamtype=2), jpeg(big, subsampling=2, streamtype=2)]
    with pytest.raises(ValueError) as e:
        tn.extract_jpeg_segments(np.frombuffer(b''.join(segs), np.uint8), np.cumsum([0] + [len(x) for x in segs[:-1]]),
                                 [len(x) for x in segs], 240, 240, tables_of(240, 240, subsampling=2))
    assert not isinstance(e.value, tn.UnsupportedImage) and e.value.index == 2
    # an abbreviated stream without the page's tables, and bytes that are no JPEG
    _refuse(64, 64, good, None, 0, tn.UnsupportedImage)
    _refuse(64, 64, good + [b'\x00' * 40], tables, 3, tn.UnsupportedImage)


def test_sizes_only_probe_matches_the_packed_sizes():
    t = _img(64, 64, 16)
    segs = [jpeg(t, subsampling=1, streamtype=2), jpeg(t[::-1].copy(), subsampling=1, streamtype=2)]
    data = np.frombuffer(b''.join(segs), np.uint8)
    ln = [len(x) for x in segs]
    scan, desc, tables = tn.extract_jpeg_segments(data, [0, ln[0]], ln, 64, 64, tables_of(64, 64, subsampling=1))
    assert tn.extract_jpeg_segments(data, [0, ln[0]], ln, 64, 64, tables_of(64, 64, subsampling=1), probe=True) == (len(scan), len(tables))
    pad = int(tn.lib().bqio_jpeg_ecs_pad())
    assert desc[0, 0] == 0 and desc[1, 0] % 16 == 0 and desc[1, 0] >= desc[0, 1] + pad and len(scan) >= desc[1, 0] + desc[1, 1] + pad
    assert not scan[desc[0, 0] + desc[0, 1]:desc[1, 0]].any() and not scan[desc[1, 0] + desc[1, 1]:].any()
    with pytest.raises(ValueError):                                                   # a segment outside the buffer
        tn.extract_jpeg_segments(data, [0, ln[0] + 1], ln, 64, 64, tables_of(64, 64, subsampling=1))


def test_square_tile_entries_are_unchanged(tmp_path):
    """``bqio_extract_jpeg`` / ``bqio_jpeg_decode_extracted`` share the generalised code: a 299-px record still gives Pillow's bytes."""
    import io

    from PIL import Image

    from biscuit_amd.tfrecord import write_slide as write_records
    tiles = np.stack([_img(299, 299, 17), _img(299, 299, 18)])
    path = str(tmp_path / 'j.tfrecords')
    write_records(path, 'j', tiles, fmt='JPEG')
    with tn.NativeReader(path) as r:
        used, nt, _ = r.extract_jpeg(0, 2, 299, None, None, None)
        scan, desc, tables = np.empty(used, np.uint8), np.empty((2, 4), np.uint32), np.empty((nt, tn.jpeg_table_bytes()), np.uint8)
        r.extract_jpeg(0, 2, 299, scan, desc, tables)
        got, status = tn.jpeg_decode_extracted(scan, desc, tables, 299)
        assert (status == 0).all()
        for i in range(2):
            assert np.array_equal(got[i], np.asarray(Image.open(io.BytesIO(r.image_bytes(i))).convert('RGB')))


def test_band_segments_is_band_left_compressed(tmp_path):
    """``WSI.band_segments`` / ``bands(segments=True)``: band's geometry, origins and src_px, the canvas as segments -- and None
    for a level that is not a tiled JPEG page."""
    from tests._wsi_jpeg_cases import slide_file
    from tests.test_wsi import _slide_file
    path = slide_file(tmp_path, 0.5045, w=1300, h=900)
    w = WSI(path, 299, 302)
    plain, segd = list(w.bands(1 << 20)), list(w.bands(1 << 20, segments=True))
    assert len(plain) == len(segd) >= 1
    for (a, b) in zip(plain, segd):
        assert a[:4] == b[:4] and np.array_equal(a[5], b[5]) and a[6] == b[6] and b[4].shape == a[4].shape[:2]
        sg = b[4]
        scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)
        canvas = np.full(sg.shape + (3,), 255, np.uint8)
        assert (tn.jpeg_decode_canvas(scan, desc, tables, sg.seg_w, sg.seg_h, sg.place, canvas, sg.clip) == 0).all()
        assert np.array_equal(canvas, a[4])
    w.close()
    deflate, _ = _slide_file(tmp_path, w=1300, h=900)
    w = WSI(deflate, 299, 302)
    assert w.band_segments(0, 1)[0] is None and all(b[4] is None for b in w.bands(1 << 20, segments=True))
    w.close()
