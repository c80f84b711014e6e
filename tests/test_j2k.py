"""JPEG 2000 slides on the CPU: the reader's host path (``TiffSlide`` / ``WSI`` over pages whose tiles Pillow's OpenJPEG wrote) and the
device decoder's CPU statement -- ``bqio_j2k_extract`` (tier 2) and ``bqio_j2k_decode_canvas`` (csrc/j2k_device.h, the routines the
kernels of kernels_j2k.hip are compiled from) -- against Pillow's decode: byte for byte on reversible streams, within one level
and on at most 1 % of the samples on irreversible ones.  The forge is tests/_j2k_cases.py."""
import io

import numpy as np
import pytest
from PIL import Image

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI, SlideError, TiffSlide
from tests import _j2k_cases as jc
from tests.test_wsi import _img, _tiff, _tiles_of


def _decode(raw, w, h, ycc=False, t1=False, strict=True):
    d = np.frombuffer(raw, np.uint8)
    packed = tn.j2k_extract(d, [0], [len(raw)], w, h, strict=strict)
    canvas = np.full((h, w, 3), 255, np.uint8)
    out = tn.j2k_decode_canvas(*packed, w, h, [[0, 0]], canvas, (0, 0, w, h), ycc=ycc, t1=t1)
    return (canvas,) + (out if t1 else (out,)) + (packed,)


# ---- host reader -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('comp', [33005, 33003])
@pytest.mark.parametrize('tile', [240, 256])
def test_reader_reads_jpeg2000_pages_as_pillow_decodes_their_tiles(tmp_path, comp, tile):
    path, a, b = jc.slide_file(tmp_path, 0.5, w=600, h=450, tile=tile, comp=comp, irreversible=True, quality_mode='dB', quality_layers=[40])
    with TiffSlide(path) as s:
        assert s.level_dimensions == [(600, 450), (150, 112)]
        for li, img in enumerate((a, b)):
            h, w = img.shape[:2]
            want = np.full((h, w, 3), 255, np.uint8)
            p = s.levels[li]
            for ty in range(p.down):
                for tx in range(p.across):
                    s._f.seek(int(p.offsets[ty * p.across + tx]))
                    raw = s._f.read(int(p.counts[ty * p.across + tx]))
                    t = (jc.pillow_ycc if comp == 33003 else jc.pillow)(raw)
                    y0, x0 = ty * tile, tx * tile
                    want[y0:y0 + tile, x0:x0 + tile] = t[:h - y0, :w - x0]
            assert np.array_equal(s.read_region(li, 0, 0, w, h), want), li
            assert np.abs(want.astype(int) - img.astype(int)).mean() < 8                     # (and it is the picture)
            win = s.read_region(li, w - 40, h - 30, 100, 80)
            assert np.array_equal(win[:30, :40], want[h - 30:, w - 40:]) and (win[30:] == 255).all() and (win[:, 40:] == 255).all()
            sg = s.region_segments(li, -5, -5, w + 10, h + 10)
            assert sg.codec == 'j2k' and sg.ycc == (comp == 33003) and len(sg) == p.across * p.down and sg.jpeg_tables is None


def test_wsi_grid_over_reversible_jpeg2000_equals_the_uncompressed_slide(tmp_path):
    """The grid ``tests/test_wsi.py`` expects of the same pixels stored uncompressed, from reversible RGB (33005) tiles."""
    a = _img(2400, 1800, 5)
    b = np.asarray(Image.fromarray(a).resize((600, 450), Image.BILINEAR))
    kw = dict(num_resolutions=4)
    path = jc.write_slide(tmp_path / 'r.svs', [jc.page(a, 256, 256, 33005, desc='Aperio |MPP = 0.5045', **kw), jc.page(b, 256, 256, 33005, **kw)])
    raw = tmp_path / 'raw.svs'
    raw.write_bytes(_tiff([dict(w=2400, h=1800, tw=256, th=256, comp=1, segs=_tiles_of(a, 256, 256, lambda t: t.tobytes()), desc='Aperio |MPP = 0.5045'),
                           dict(w=600, h=450, tw=256, th=256, comp=1, segs=_tiles_of(b, 256, 256, lambda t: t.tobytes()))]))
    w, ref = WSI(path, 299, 302), WSI(str(raw), 299, 302)
    assert (w.grid_w, w.grid_h, w.level, w.extract_px) == (ref.grid_w, ref.grid_h, ref.level, ref.extract_px) == (4, 3, 0, 598)
    got, grid = w.tiles()
    want, grid_ref = ref.tiles()
    assert np.array_equal(grid, grid_ref) and np.array_equal(got, want)
    assert np.array_equal(got[6], np.asarray(Image.fromarray(a[598:1196, 1196:1794]).resize((299, 299), Image.LANCZOS)))
    big = WSI(path, 299, 800)                                                                # the second level, JPEG 2000 too
    assert big.level == 1 and np.array_equal(big.tiles()[0], WSI(str(raw), 299, 800).tiles()[0])
    for x in (w, ref, big):
        x.close()


def test_reader_refuses_what_it_cannot_read(tmp_path):
    good, bad = jc.refusals()
    for name in ('gray', 'rgba', 'sixteen', 'garbage', 'truncated'):
        raw = bad[name][0] if name != 'truncated' else good[:60]
        p = tmp_path / f'{name}.tif'
        p.write_bytes(_tiff([dict(w=64, h=64, tw=64, th=64, comp=33005, segs=[raw])]))
        with pytest.raises(SlideError, match='JPEG 2000'):
            TiffSlide(str(p))
    small = jc.j2k(jc.content('photo', 32, 32), irreversible=False)                          # an image smaller than the page's tile
    (tmp_path / 'small.tif').write_bytes(_tiff([dict(w=64, h=64, tw=64, th=64, comp=33005, segs=[small])]))
    with pytest.raises(SlideError, match='JPEG 2000'):
        TiffSlide(str(tmp_path / 'small.tif'))
    # a second tile that is damaged: found when it is read, as a SlideError
    (tmp_path / 'late.tif').write_bytes(_tiff([dict(w=128, h=64, tw=64, th=64, comp=33005, segs=[good, good[:len(good) // 3]])]))
    with TiffSlide(str(tmp_path / 'late.tif')) as s:
        assert s.read_region(0, 0, 0, 64, 64).shape == (64, 64, 3)
        try:                                                            # (OpenJPEG may decode a truncated stream as far as it goes)
            s.read_region(0, 64, 0, 64, 64)
        except SlideError:
            pass
    # a JP2 file as a tile is read too
    bb = io.BytesIO()
    Image.fromarray(jc.content('photo', 64, 64, 2)).save(bb, 'JPEG2000', irreversible=False)
    (tmp_path / 'jp2.tif').write_bytes(_tiff([dict(w=64, h=64, tw=64, th=64, comp=34712, segs=[bb.getvalue()])]))
    with TiffSlide(str(tmp_path / 'jp2.tif')) as s:
        assert np.array_equal(s.read_region(0, 0, 0, 64, 64), jc.content('photo', 64, 64, 2))


# ---- the colour conversion ---------------------------------------------------------------------------------------------------------
def test_ycc_to_rgb_is_pillows_over_all_triples():
    cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for y in range(256):
        a = np.stack([np.full_like(cb, y), cb, cr], -1)
        want = np.asarray(Image.fromarray(a, 'YCbCr').convert('RGB'))
        assert np.array_equal(tn.ycc_to_rgb(a), want), y


# ---- the decoder's CPU statement against Pillow --------------------------------------------------------------------------------------
def _id(c):
    return '%dx%d_%s_%s' % (c[0], c[1], c[2], '_'.join(f'{k[:4]}{v}' for k, v in c[3].items()).replace(' ', ''))


@pytest.mark.parametrize('case', jc.REVERSIBLE, ids=_id)
def test_reversible_streams_equal_pillow_byte_for_byte(case):
    w, h, kind, kw = case
    a = jc.content(kind, w, h, 7)
    raw = jc.encode(a, False, **kw)
    got, status, packed = _decode(raw, w, h)
    assert status[0] == 0 and np.array_equal(got, jc.pillow(raw)) and np.array_equal(got, a)
    if kind == 'white':                                                  # blocks without a pass are not in the table
        assert len(packed[1]) <= 3
    if kw.get('mct', 0) == 0:                                            # the same stream read as a 33003 tile
        got, status, _ = _decode(raw, w, h, ycc=True)
        assert status[0] == 0 and np.array_equal(got, jc.pillow_ycc(raw))


def test_every_axis_value_appears_with_a_non_square_size():
    for cases in (jc.REVERSIBLE, jc.IRREVERSIBLE):
        ns = [c for c in cases if c[0] != c[1]]
        assert {c[3].get('num_resolutions') for c in ns} >= {1, 2, 6}
        assert {c[3].get('codeblock_size', (64, 64)) for c in ns} >= {(64, 64), (32, 32), (4, 4), (16, 64)}
        assert {c[3].get('mct', 0) for c in ns} >= {0, 1}
        assert {c[3].get('progression', 'LRCP') for c in ns} >= set(jc.PROGRESSIONS)
        assert any('precinct_size' in c[3] for c in ns) and {c[2] for c in ns} >= {'flat', 'noise', 'gradient', 'photo', 'white'}
        assert {(c[0], c[1]) for c in cases} >= {(1, 1), (7, 5), (33, 17), (65, 64), (64, 65), (240, 240), (256, 256), (300, 200)}
    assert {len(c[3].get('quality_layers', [0])) for c in jc.REVERSIBLE if c[0] != c[1]} >= {1, 3}
    modes = {(c[3].get('quality_mode'), tuple(c[3].get('quality_layers', ()))) for c in jc.IRREVERSIBLE}
    assert modes >= {('rates', (8,)), ('rates', (20,)), ('rates', (20, 8)), ('dB', (30,)), ('dB', (45,)), ('dB', (30, 45))}


@pytest.mark.parametrize('case', jc.IRREVERSIBLE, ids=_id)
def test_irreversible_streams_are_within_one_of_pillow_on_at_most_one_percent(case, capsys):
    """Two correct decoders round the same real value: they differ where it lies next to a half, by one, and a different order of
    operations moves only the samples within about 1e-3 of a half -- far fewer than 1 %."""
    w, h, kind, kw = case
    raw = jc.encode(jc.content(kind, w, h, 7), True, **kw)
    got, status, _ = _decode(raw, w, h)
    d = np.abs(got.astype(int) - jc.pillow(raw).astype(int))
    with capsys.disabled():
        print(f'\n  j2k irreversible {_id(case)}: max {d.max()}, share {(d > 0).mean():.6f}', end='')
    assert status[0] == 0
    assert d.max() <= 1
    assert (d > 0).mean() <= 0.01


def test_truncated_blocks_occur_in_the_rate_limited_cases():
    w, h, kind, kw = next(c for c in jc.IRREVERSIBLE if c[3].get('quality_layers') == [20, 8] and c[0] == 200)
    raw = jc.encode(jc.content(kind, w, h, 7), True, **kw)
    _, _, (desc, blocks, _) = _decode(raw, w, h)
    full = 3 * (blocks[:, 7] - blocks[:, 8]) - 2
    assert (blocks[:, 9] < full).any() and (blocks[:, 9] <= full).all() and desc[0, 28] == 2      # passes cut by the layers; two layers


def test_tier1_indices_equal_the_forward_transform_of_the_decoded_pixels():
    """A second route to the quantiser indices of a reversible stream: the 5/3 analysis of the decoded (= the original) pixels,
    written here from its definition, gives the integers tier 1 must have decoded."""
    def analyse(x):                                                     # one level along axis 0: -> (low, high)
        x = x.astype(np.int64)
        n = x.shape[0]
        if n == 1:
            return x, x[:0]
        ev, od = x[0::2], x[1::2]
        right = np.concatenate([ev[1:], ev[-1:]])[:len(od)] if n % 2 == 0 else ev[1:]
        hi = od - ((ev[:len(od)] + right) >> 1)
        left = np.concatenate([hi[:1], hi])[:len(ev)]
        rgt = np.concatenate([hi, hi[-1:]])[:len(ev)]
        return ev + ((left + rgt + 2) >> 2), hi
    w, h, levels = 77, 53, 3
    a = jc.content('photo', w, h, 9)
    raw = jc.encode(a, False, num_resolutions=levels + 1, mct=1, codeblock_size=(32, 32))
    got, status, planes, _ = _decode(raw, w, h, t1=True)
    assert status[0] == 0 and np.array_equal(got, a)
    r, g, b = (a[:, :, c].astype(np.int64) for c in range(3))
    comps = [((r + 2 * g + b) >> 2) - 128, b - g, r - g]
    for c in range(3):
        plane = np.zeros((h, w), np.int64)
        ll = comps[c]
        for _ in range(levels):
            lo, hi = analyse(ll)                                        # columns (the encoder's first pass), then rows
            ll_, hl = analyse(lo.T)
            lh, hh = analyse(hi.T)
            hh_, hw_ = ll.shape
            sh, sw = lo.shape[0], ll_.shape[0]
            plane[:sh, sw:hw_] = hl.T
            plane[sh:hh_, :sw] = lh.T
            plane[sh:hh_, sw:hw_] = hh.T
            ll = ll_.T
        plane[:ll.shape[0], :ll.shape[1]] = ll
        t1 = planes[0, c].astype(np.int64)
        assert np.array_equal(np.sign(t1) * (np.abs(t1) >> 1), plane), c      # (tier 1 holds indices times two, plus a half bit)


# ---- canvas placement ------------------------------------------------------------------------------------------------------------
def _page_file(tmp_path, comp=33005, **kw):
    a = _img(128, 128, 21)
    return jc.write_slide(tmp_path / 'p.tif', [jc.page(a, 64, 64, comp, **kw)]), a


@pytest.mark.parametrize('comp,irreversible', [(33005, False), (33003, True)])
def test_canvas_of_a_band_equals_read_region(tmp_path, comp, irreversible):
    a = _img(300, 170, 12)
    path = jc.write_slide(tmp_path / 's.tif', [jc.page(a, 64, 64, comp, irreversible=irreversible, num_resolutions=4)])
    with TiffSlide(path) as s:
        for x, y, ww, hh in ((0, 0, 300, 170), (2, 3, 59, 58), (57, 59, 15, 11), (-10, -10, 320, 190)):
            sg = s.region_segments(0, x, y, ww, hh)
            packed = tn.j2k_extract(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h)
            buf = np.full((hh + 4, ww, 3), 0xA5, np.uint8)
            buf[2:-2] = 255
            status = tn.j2k_decode_canvas(*packed, 64, 64, sg.place, buf[2:-2], sg.clip, ycc=sg.ycc, threads=3)
            assert (status == 0).all() and (buf[:2] == 0xA5).all() and (buf[-2:] == 0xA5).all()
            want = s.read_region(0, x, y, ww, hh)
            d = np.abs(buf[2:-2].astype(int) - want.astype(int))
            assert (d.max() == 0) if not irreversible else (d.max() <= 1 and (d > 0).mean() <= 0.01), (x, y)


def test_clip_and_places_outside_the_canvas_write_nothing_else(tmp_path):
    path, a = _page_file(tmp_path)
    with TiffSlide(path) as s:
        sg = s.region_segments(0, 0, 0, 128, 128)
    packed = tn.j2k_extract(sg.data, sg.offsets, sg.lengths, 64, 64)
    place = np.array([[-30, -20], [60, -63], [-64, 40], [90, 74]], np.int32)               # the last two: wholly outside
    tiles = [a[:64, :64], a[:64, 64:], a[64:, :64], a[64:, 64:]]
    for clip in ((0, 0, 91, 75), (7, 5, 80, 60), (-1000, -1000, 1 << 30, 1 << 30), (50, 50, 50, 60)):
        buf = np.full((75 + 4, 91, 3), 0xA5, np.uint8)
        buf[2:-2] = 255
        status = tn.j2k_decode_canvas(*packed, 64, 64, place, buf[2:-2], clip)
        assert (status == 0).all() and (buf[:2] == 0xA5).all() and (buf[-2:] == 0xA5).all()
        want = np.full((75, 91, 3), 255, np.uint8)
        x0, y0, x1, y1 = max(clip[0], 0), max(clip[1], 0), min(clip[2], 91), min(clip[3], 75)
        for (px, py), t in zip(place, tiles):
            for y in range(max(y0, py), min(y1, py + 64)):
                want[y, max(x0, px):max(min(x1, px + 64), max(x0, px))] = t[y - py, max(x0, px) - px:max(min(x1, px + 64), max(x0, px)) - px]
        assert np.array_equal(buf[2:-2], want), clip
    assert (buf[2:-2] == 255).all()                                                          # (the empty rectangle came last)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_streams_outside_the_subset_have_a_status_and_write_nothing(tmp_path):
    good, bad = jc.refusals()
    for name, (raw, want) in bad.items():
        canvas, status, packed = _decode(raw, 64, 64, strict=False)
        assert status[0] == want == packed[0][0, 0], name
        assert len(packed[1]) == 0 and (canvas == 255).all(), name
        with pytest.raises(tn.UnsupportedImage):
            tn.j2k_extract(np.frombuffer(raw, np.uint8), [0], [len(raw)], 64, 64)
    # a refused segment between two good ones: its neighbours are decoded, and the table rows of the good ones stay usable
    data = np.frombuffer(good + bad['sop'][0] + good, np.uint8)
    ln = [len(good), len(bad['sop'][0]), len(good)]
    with pytest.raises(tn.UnsupportedImage) as e:
        tn.j2k_extract(data, [0, ln[0], ln[0] + ln[1]], ln, 64, 64)
    assert e.value.index == 1
    packed = tn.j2k_extract(data, [0, ln[0], ln[0] + ln[1]], ln, 64, 64, strict=False)
    canvas = np.full((64, 192, 3), 255, np.uint8)
    status = tn.j2k_decode_canvas(*packed, 64, 64, [[0, 0], [64, 0], [128, 0]], canvas, (0, 0, 192, 64))
    assert status.tolist() == [0, 32, 0] and (canvas[:, 64:128] == 255).all()
    assert np.array_equal(canvas[:, :64], jc.pillow(good)) and np.array_equal(canvas[:, 128:], jc.pillow(good))
    # a block row that points outside its plane, and one outside the codewords: status 16, nothing written, nothing read
    desc, blocks, cw = tn.j2k_extract(np.frombuffer(good, np.uint8), [0], [len(good)], 64, 64)
    for col, value in ((3, 60), (4, -1), (5, 65), (9, 200), (10, len(cw)), (7, 40)):
        b = blocks.copy()
        b[0, col] = value
        canvas = np.full((64, 64, 3), 255, np.uint8)
        assert tn.j2k_decode_canvas(desc, b, cw, 64, 64, [[0, 0]], canvas, (0, 0, 64, 64)).tolist() == [16] and (canvas == 255).all(), col
    b = blocks.copy()
    b[0, 0], b[0, 3] = 1, 60                                             # a bad row that names a segment it does not belong to: nobody's
    canvas = np.full((64, 64, 3), 255, np.uint8)
    assert tn.j2k_decode_canvas(desc, b, cw, 64, 64, [[0, 0]], canvas, (0, 0, 64, 64)).tolist() == [0] and (canvas != 255).any()
    # a segment of another size than the page's tile is the host's
    assert _decode(jc.j2k(jc.content('photo', 96, 64), irreversible=False), 64, 64, strict=False)[1][0] == 32
    # the host path: a page with such a tile is read by Pillow, or refused with a SlideError
    a = _img(128, 64, 3)
    pg = jc.page(a, 64, 64, 33005)
    pg['segs'][1] = jc.j2k(a[:, 64:], irreversible=False, tile_size=(32, 32))
    path = jc.write_slide(tmp_path / 't.tif', [pg])
    with TiffSlide(path) as s:
        assert np.array_equal(s.read_region(0, 0, 0, 128, 64), a)
        sg = s.region_segments(0, 0, 0, 128, 64)
        with pytest.raises(tn.UnsupportedImage):
            tn.j2k_extract(sg.data, sg.offsets, sg.lengths, 64, 64)
