"""The host side of the heatmap's input stage: Pillow's LANCZOS tap tables (``bqio_resample_taps``), the CPU restatement of the
tile resampler (``bqio_tile_resample``: the routines the GPU kernel is compiled from), the band reader of ``wsi.WSI`` and the
table of the background filter.  No GPU."""
import numpy as np
import pytest
from PIL import Image

from biscuit_amd import resample, tfrecord_native
from biscuit_amd.wsi import WSI
from tests import _resample_ref as R
from tests.test_wsi import _img, _slide_file, _tiff, _tiles_of


@pytest.mark.parametrize('src', R.WIDTHS)
def test_taps_equal_the_numpy_restatement(src):
    bounds, coef = resample.taps(src, R.PX)
    rb, rc = R.taps_ref(src, R.PX)
    assert coef.shape == rc.shape and resample.ksize(src, R.PX) == rc.shape[1]
    assert np.array_equal(bounds, rb) and np.array_equal(coef, rc)
    # the 32-bit accumulators of both passes rest on this
    assert 255 * int(np.abs(coef.astype(np.int64)).sum(1).max()) + (1 << 21) < 1 << 31


def test_numpy_restatement_equals_pillow():
    """The restatement the taps are checked against is itself Pillow's resampler: same bytes on a random image."""
    rng = np.random.default_rng(3)
    for src in (150, 302, 604):
        a = rng.integers(0, 256, (src, src, 3), dtype=np.uint8)
        a[: src // 4] = 255
        assert np.array_equal(R.resize_ref(a), np.asarray(Image.fromarray(a).resize((R.PX, R.PX), Image.LANCZOS)))


@pytest.mark.parametrize('src', R.WIDTHS)
def test_tile_resample_equals_pillow(src):
    canvas, origin = R.case(src)
    got = resample.tile_resample(canvas, origin, src, R.PX)
    want = R.pillow_tiles(canvas, origin, src)
    for i in range(len(origin)):
        assert np.array_equal(got[i], want[i]), (src, origin[i].tolist(), int(np.abs(got[i].astype(int) - want[i]).max()))
    assert (want[-1] == 255).all() and not (want[3] == 255).all()          # a window wholly outside is white; a partial one is not


def _bands_against_tiles(path, budget, **kw):
    w = WSI(path, **kw)
    try:
        tiles, grid = w.tiles()
        got, cells, n_bands = [], [], 0
        for gy0, gy1, gx0, gx1, canvas, origin, src_px in w.bands(budget):
            assert canvas.dtype == np.uint8 and canvas.ndim == 3 and origin.dtype == np.int32
            assert origin.shape == ((gy1 - gy0) * (gx1 - gx0), 2) and src_px == w.src_px
            assert (origin >= 0).all() and (origin[:, 0] + src_px <= canvas.shape[1]).all() and (origin[:, 1] + src_px <= canvas.shape[0]).all()
            got.append(resample.tile_resample(canvas, origin, src_px, w.tile_px))
            cells += [(gx, gy) for gy in range(gy0, gy1) for gx in range(gx0, gx1)]
            n_bands += 1
        assert cells == [tuple(g) for g in grid.tolist()]
        assert np.array_equal(np.concatenate(got), tiles)
        return w, n_bands
    finally:
        w.close()


@pytest.mark.parametrize('stride_div', [1, 2])
def test_bands_reproduce_tiles_two_level_slide(tmp_path, stride_div):
    path, _ = _slide_file(tmp_path)
    w, n_bands = _bands_against_tiles(path, 1, stride_div=stride_div)      # a budget of one byte: one grid row per band
    assert n_bands == w.grid_h >= 3 and w.src_px == 598
    # a budget that holds two grid rows but not three
    row = w.src_px * ((w.grid_w - 1) * w.stride + w.src_px) * 3
    _, n2 = _bands_against_tiles(path, int(row * (2.2 if stride_div == 1 else 1.7)), stride_div=stride_div)
    assert 2 <= n2 < n_bands
    _, n1 = _bands_against_tiles(path, 256 << 20, stride_div=stride_div)
    assert n1 == 1


def test_bands_reproduce_tiles_uneven_4x_level(tmp_path):
    """A slide read from its 4 x level, with an MPP that puts the grid between level pixels (x0 / level_ds = 313.5) and a last
    window that leaves the level by one pixel (white there, as read_region pads)."""
    found = R.uneven_slide_geometry()
    assert found is not None, 'no MPP / width pair in the searched range has a window that leaves the level'
    mpp, wd, e = found
    ht = 3 * e + 5
    a = _img(wd, ht, 9)
    b = np.asarray(Image.fromarray(a).resize((wd // 4, ht // 4), Image.BILINEAR))
    import zlib
    raw = lambda t: zlib.compress(t.tobytes(), 1)                                            # noqa: E731
    path = tmp_path / 'uneven.svs'
    path.write_bytes(_tiff([dict(w=wd, h=ht, tw=256, th=256, comp=8, segs=_tiles_of(a, 256, 256, raw), desc=f'Aperio |MPP = {mpp}'),
                            dict(w=wd // 4, h=ht // 4, tw=256, th=256, comp=8, segs=_tiles_of(b, 256, 256, raw))]))
    w, n_bands = _bands_against_tiles(str(path), 1)
    assert w.level == 1 and n_bands == w.grid_h == 3 and w.grid_w == 2 and w.src_px != w.tile_px
    lx = int(round(w.stride / w.level_ds))
    assert abs(w.stride / w.level_ds - lx) > 0.2                              # the grid falls between level pixels
    assert lx + w.src_px == w.slide.level_dimensions[1][0] + 1                # the last window leaves the level by a pixel


@pytest.mark.parametrize('thr', [0.05, 0.1, 0.5])
def test_grayspace_limit_is_the_float64_definition(thr):
    limit = resample.grayspace_limit(thr)
    n = 0
    for mx in range(256):
        for mn in range(mx + 1):
            s = 0.0 if mx == 0 else (mx - mn) / mx
            assert ((mx - mn) < limit[mx]) == (s < thr), (mx, mn)
            n += 1
    assert n == 32896
    # and the count over tiles, against the numpy definition
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, (3, 31, 31, 3), dtype=np.uint8)
    t[1, :10] = 200
    t[2, :, :7] = 0
    d = t.max(-1).astype(int) - t.min(-1)
    assert np.array_equal((d < limit[t.max(-1)]).reshape(3, -1).sum(1), resample.grayspace_count(t, thr))


def test_refusals():
    lib = tfrecord_native.lib()
    canvas = np.zeros((64, 64, 3), np.uint8)
    origin = np.zeros((1, 2), np.int32)
    out = np.full((1, 8, 8, 3), 77, np.uint8)
    b, c = np.full((8, 2), -5, np.int32), np.full((8, 64), -5, np.int32)
    for src, px in ((65, 8), (8, 65), (100, 0), (100, -3), (0, 8)):
        assert lib.bqio_resample_ksize(src, px) < 0
        assert lib.bqio_resample_taps(src, px, b.ctypes.data, c.ctypes.data, 64) < 0
        assert lib.bqio_tile_resample(canvas.ctypes.data, 64, 64, origin.ctypes.data, 1, src, px, out.ctypes.data) < 0
        with pytest.raises(resample.ResampleError):
            resample.taps(src, px)
    assert lib.bqio_tile_resample(canvas.ctypes.data, 64, 64, origin.ctypes.data, -1, 16, 8, out.ctypes.data) < 0
    assert lib.bqio_resample_taps(16, 8, b.ctypes.data, c.ctypes.data, 3) < 0         # table too small for ksize 13
    assert (out == 77).all() and (b == -5).all() and (c == -5).all()                   # the error code, not output
    assert lib.bqio_tile_resample(canvas.ctypes.data, 64, 64, origin.ctypes.data, 0, 16, 8, out.ctypes.data) == 0 and (out == 77).all()
    # the edges of the range are served: 8 x down and 8 x up
    assert resample.tile_resample(canvas, origin, 64, 8).shape == (1, 8, 8, 3) and resample.ksize(64, 8) == 49
    assert resample.tile_resample(canvas, origin, 8, 64).shape == (1, 64, 64, 3) and resample.ksize(8, 64) == 7


def test_wsi_closes_its_file_when_it_refuses(tmp_path):
    path, _ = _slide_file(tmp_path, w=700, h=700)
    opened = []
    import biscuit_amd.wsi as wsi_mod

    class Spy(wsi_mod.TiffSlide):
        def __init__(self, p):
            super().__init__(p)
            opened.append(self)
    orig, wsi_mod.TiffSlide = wsi_mod.TiffSlide, Spy
    try:
        with pytest.raises(wsi_mod.SlideError):
            WSI(path, tile_um=0.0001)                                       # a tile of less than one pixel
    finally:
        wsi_mod.TiffSlide = orig
    assert len(opened) == 1 and opened[0]._f.closed


@pytest.mark.parametrize('stride_div', [1, 2])
def test_bands_split_columns_of_a_row_wider_than_one_read(tmp_path, monkeypatch, stride_div):
    """A grid row wider than ``read_region`` reads at once (``WSI.READ_LIMIT``, lowered here so that the test slide is too wide)
    is split into column ranges: every cell still comes exactly once, with ``_tile``'s bytes; the order is band by band."""
    path, _ = _slide_file(tmp_path)
    monkeypatch.setattr(WSI, 'READ_LIMIT', 1300)                             # two 598-px columns (1 196 px) fit, three do not
    w = WSI(path, stride_div=stride_div)
    try:
        tiles, grid = w.tiles()
        at = {tuple(g): i for i, g in enumerate(grid.tolist())}
        seen, ranges = [], set()
        for gy0, gy1, gx0, gx1, canvas, origin, src_px in w.bands(256 << 20):
            assert canvas.shape[0] <= 1300 and canvas.shape[1] <= 1300
            ranges.add((gx0, gx1))
            got = resample.tile_resample(canvas, origin, src_px, w.tile_px)
            cells = [(gx, gy) for gy in range(gy0, gy1) for gx in range(gx0, gx1)]
            assert len(cells) == len(got)
            for c, t in zip(cells, got):
                assert np.array_equal(t, tiles[at[c]]), c
            seen += cells
        assert len(ranges) >= 2 and sorted(seen) == sorted(at) and len(seen) == len(at)
        assert seen != [tuple(g) for g in grid.tolist()]                    # not the row-major order of the whole grid
    finally:
        w.close()
