"""CPU tests of the heatmap's output stage (DESIGN.md "Heatmap output"): the geometry tables against the numpy restatement and
against their definition, the colour table and the bin rule against matplotlib, the argument checks, the slide thumbnail."""
import numpy as np
import pytest
from PIL import Image

from biscuit_amd import render as R
from tests import _render_ref as ref

# (gw, gh, W, H, slide_w0, slide_h0, stride, extract_px): a margin on every side; stride_div = 2; a grid that fills the slide; one
# cell and one pixel; more pixels than level-0 pixels
GEOMETRIES = [(5, 7, 83, 61, 4000, 5200, 600, 600), (9, 6, 97, 64, 3100, 2150, 302, 604), (4, 3, 64, 48, 2400, 1800, 600, 600),
              (1, 1, 1, 1, 700, 650, 598, 598), (3, 2, 2049, 5, 1200, 900, 377, 377)]


@pytest.mark.parametrize('geom', GEOMETRIES)
@pytest.mark.parametrize('mode', R.INTERPOLATIONS)
def test_tables_equal_the_restatement(geom, mode):
    gw, gh, W, H = geom[:4]
    col, row = R.render_tables(*geom, interpolation=mode)
    want_col, want_row = ref.tables(*geom, interpolation=mode)
    assert col.dtype == row.dtype == np.int32 and col.shape == want_col.shape and row.shape == want_row.shape
    assert np.array_equal(col, want_col) and np.array_equal(row, want_row)
    if mode == 'bicubic':
        assert col.shape == (W, R.RENDER_ENTRY) and row.shape == (H, R.RENDER_ENTRY)
        for t, n in ((col, gw), (row, gh)):
            assert (t[:, 5:9].sum(1) == R.RENDER_WEIGHT_ONE).all()                    # every weight group sums to 4 096
            assert t[:, 1:5].min() >= 0 and t[:, 1:5].max() <= n - 1 and (np.diff(t[:, 1:5], axis=1) >= 0).all()
            assert t[:, 5:9].min() >= -R.RENDER_WEIGHT_ONE // 8 and t[:, 5:9].max() <= R.RENDER_WEIGHT_ONE
        none_col, none_row = R.render_tables(*geom, interpolation='none')
        assert np.array_equal(col[:, 0], none_col) and np.array_equal(row[:, 0], none_row)


def test_weights_at_a_cell_centre_and_between_two():
    # extract = stride = 8 level-0 pixels a cell, one output pixel per level-0 pixel: pixel centre x + 0.5, cell centres at 4 + 8 g
    col, _ = R.render_tables(4, 1, 32, 8, 32, 8, 8, 8, 'bicubic')
    f = (np.arange(32) + 0.5 - 4) / 8.0                                               # u - 0.5
    assert np.array_equal(col[:, 2], np.clip(np.floor(f), 0, 3))
    x = 16                                                                            # u - 0.5 = 1.5625: between cells 1 and 2, nearer 2
    assert col[x, 1:5].tolist() == [0, 1, 2, 3] and col[x, 5:9].tolist() == [-220, 1950, 2649, -283]    # CR(0.5625) * 4096, rounded
    half, _ = R.render_tables(4, 1, 4, 1, 32, 8, 8, 8, 'bicubic')                     # pixel centres ON the cell centres
    assert half[:, 5:9].tolist() == [[0, 4096, 0, 0]] * 4 and half[:, 2].tolist() == [0, 1, 2, 3]


def test_adjacent_grid_covers_every_pixel():
    """stride_div = 1 on a grid that fills the slide: every pixel has a cell, and cell gx starts at gx * stride * W / slide_w0."""
    gw, gh, W, H, w0, h0, stride = 4, 3, 67, 50, 2400, 1800, 600
    col, row = R.render_tables(gw, gh, W, H, w0, h0, stride, stride, 'none')
    assert col.min() == 0 and col.max() == gw - 1 and row.min() == 0 and row.max() == gh - 1
    for table, n, extent in ((col, W, w0), (row, H, h0)):
        for x in range(n):
            centre = (x + 0.5) * extent / n                                           # the pixel centre in level-0 pixels
            assert table[x] * stride <= centre < (table[x] + 1) * stride
        for g in range(1, int(table.max()) + 1):
            first = int(np.argmax(table == g))
            edge = g * stride * n / extent                                            # the boundary in output pixels
            assert first == int(np.ceil(edge - 0.5)), (g, first, edge)


def test_overlapping_grid_starts_half_a_stride_inside():
    """stride_div = 2: cells are stride wide around the tile centres, so the first starts at extract_px / 2 - stride / 2."""
    extract, stride, w0, W = 600, 300, 3000, 3000                                     # one output pixel per level-0 pixel
    gw = (w0 - extract) // stride + 1
    col, _ = R.render_tables(gw, 1, W, 1, w0, extract, stride, extract, 'none')
    start = extract // 2 - stride // 2
    assert (col[:start] == -1).all() and col[start] == 0 and col[start + stride - 1] == 0 and col[start + stride] == 1
    end = start + gw * stride
    assert col[end - 1] == gw - 1 and (col[end:] == -1).all() and end == w0 - start
    assert np.array_equal(np.bincount(col[col >= 0]), np.full(gw, stride))            # no overlap, no gap


def test_colour_table_equals_matplotlib():
    pytest.importorskip('matplotlib')
    import matplotlib
    from matplotlib.colors import LinearSegmentedColormap
    cmap = LinearSegmentedColormap.from_list('t', matplotlib.colormaps['PRGn'](np.linspace(0.1, 0.9, 100)))
    live = cmap(np.arange(256), bytes=True)[:, :3]
    assert R.PRGN_TRUNC.dtype == np.uint8 and R.PRGN_TRUNC.shape == (256, 3) and np.array_equal(R.PRGN_TRUNC, live)
    assert np.array_equal(R.lut_from(cmap), R.PRGN_TRUNC) and R.lut_from(None) is R.PRGN_TRUNC
    assert np.array_equal(R.lut_from(R.PRGN_TRUNC[::-1].copy()), R.PRGN_TRUNC[::-1])


@pytest.mark.parametrize('vmin,vmax', [(0.0, 1.0), (-0.25, 0.75)])
def test_bin_rule_equals_matplotlib(vmin, vmax):
    """lut[q >> 8] is the colour matplotlib gives Normalize(vmin, vmax)(v): 4 097 values k / 4096 of the way through the range,
    shifted by 2^-14 -- off every bin edge by more than float32's error -- plus values below vmin and above vmax."""
    pytest.importorskip('matplotlib')
    import matplotlib
    from matplotlib.colors import LinearSegmentedColormap, Normalize
    cmap = LinearSegmentedColormap.from_list('t', matplotlib.colormaps['PRGn'](np.linspace(0.1, 0.9, 100)))
    sweep = vmin + (np.arange(4097) / 4096.0 + 2.0 ** -14) * (vmax - vmin)
    v = np.concatenate([sweep, [vmin - 0.5, vmin - 1e-3, vmax + 1e-3, vmax + 7.0]]).astype(np.float32)
    q = ref.cell_q(v[None, :], vmin, vmax)[0]
    assert q.min() == 0 and q.max() == 65535 and len(np.unique(q >> 8)) == 256
    want = cmap(Normalize(vmin, vmax)(v.astype(np.float64)), bytes=True)[:, :3]
    assert np.array_equal(R.PRGN_TRUNC[q >> 8], want)
    # and through the whole restatement: one cell per value, alpha 1, one pixel per cell
    n = len(v)
    img = ref.render(v[None, :], np.zeros((1, n, 3), np.uint8), R.PRGN_TRUNC, n * 10, 10, 10, 10, vmin, vmax, alpha=1.0)
    assert np.array_equal(img[0], want)


def test_check_params():
    lo, inv, a, mode = R.check_params()
    assert (lo, inv, a, mode) == (0.0, 1.0, 154, 0) and lo.dtype == inv.dtype == np.float32
    assert R.check_params(alpha=0.0)[2] == 0 and R.check_params(alpha=1.0)[2] == 256 and R.check_params(interpolation='bicubic')[3] == 1
    assert R.check_params(-0.25, 0.75)[1] == np.float32(1.0) / np.float32(1.0)
    assert R.check_params(0.0, 0.3)[1] == np.float32(1.0) / np.float32(0.3)           # the reciprocal is float32's
    bad = [dict(vmin=1.0, vmax=1.0), dict(vmin=2.0, vmax=1.0), dict(vmin=float('nan')), dict(vmax=float('inf')),
           dict(vmin=float('-inf')), dict(vmax=1e39), dict(vmin=-3e38, vmax=3e38), dict(alpha=-0.01), dict(alpha=1.01),
           dict(alpha=float('nan')), dict(interpolation='bilinear'), dict(interpolation=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            R.check_params(**kw)


def test_refusals():
    for lut in (np.zeros((256, 4), np.uint8), np.zeros((255, 3), np.uint8), np.zeros((256, 3), np.float32), 'PRGn'):
        with pytest.raises(ValueError):
            R.lut_from(lut)
    for kw in (dict(W=0), dict(H=0), dict(W=R.RENDER_MAX_PX + 1), dict(gw=0), dict(stride=0), dict(interpolation='nearest')):
        args = dict(gw=3, gh=2, W=10, H=8, slide_w0=1200, slide_h0=900, stride=377, extract_px=377, interpolation='none')
        with pytest.raises(ValueError):
            R.render_tables(**dict(args, **kw))


def test_render_without_a_slide_asks_for_the_geometry():
    """A heatmap built by ``Heatmap(...)`` or ``from_region`` has no slide: ``render`` says what it needs before it touches the
    engine (None here), and bad scalars are refused first."""
    from biscuit_amd.heatmap import Heatmap
    hm = Heatmap.__new__(Heatmap)
    hm.logits = np.full((2, 3, 2), 0.5, np.float32)
    hm.uncertainty = np.full((2, 3, 2), 0.1, np.float32)
    thumb = np.zeros((8, 10, 3), np.uint8)
    with pytest.raises(ValueError, match='slide_w0, slide_h0, stride, extract_px'):
        hm.render(None, thumb=thumb)
    with pytest.raises(ValueError, match='missing: stride'):
        hm.render(None, thumb=thumb, slide_w0=1200, slide_h0=900, extract_px=377)
    with pytest.raises(ValueError, match='from_slide'):
        hm.thumbnail()
    geom = dict(slide_w0=1200, slide_h0=900, stride=377, extract_px=377)
    for kw in (dict(vmin=1.0, vmax=0.0), dict(vmax=float('nan')), dict(alpha=2.0), dict(interpolation='cubic'),
               dict(cmap=np.zeros((3, 256), np.uint8)), dict(plane='probabilities'), dict(index=2),
               dict(plane=np.zeros((3, 2), np.float32))):
        with pytest.raises(ValueError):
            hm.render(None, thumb=thumb, **dict(geom, **kw))
    with pytest.raises(ValueError):
        hm.render(None, thumb=np.zeros((8, 10), np.uint8), **geom)


def _pyramid(tmp_path):
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:700, 0:1000]
    a = np.stack([128 + 100 * np.sin(xx / 31.0), 128 + 90 * np.cos(yy / 23.0), (xx + yy) % 256], -1)
    a = np.clip(a + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    levels = [Image.fromarray(a)]
    for d in (2, 4):
        levels.append(levels[0].resize((1000 // d, 700 // d), Image.BILINEAR))
    path = str(tmp_path / 'pyramid.tif')
    levels[0].save(path, format='TIFF', compression='tiff_adobe_deflate', save_all=True, append_images=levels[1:],
                   dpi=(25400 / 0.5, 25400 / 0.5))
    return path


def _pillow_level(path, i):
    im = Image.open(path)
    im.seek(i)
    return im.convert('RGB')


def test_thumbnail(tmp_path, monkeypatch):
    from biscuit_amd.wsi import WSI, SlideError
    path = _pyramid(tmp_path)
    w = WSI(path)
    try:
        assert w.slide.level_dimensions == [(1000, 700), (500, 350), (250, 175)]
        t = w.thumbnail(400)                                                          # the coarsest level >= 400 wide is level 1
        assert t.dtype == np.uint8 and t.shape == (280, 400, 3)
        assert np.array_equal(t, np.asarray(_pillow_level(path, 1).resize((400, 280), Image.LANCZOS)))
        assert np.array_equal(w.thumbnail(500), np.asarray(_pillow_level(path, 1)))   # a level of exactly that width: itself
        t = w.thumbnail(333)
        assert t.shape == (int(round(350 * 333 / 500)), 333, 3)
        assert np.array_equal(t, np.asarray(_pillow_level(path, 1).resize((333, t.shape[0]), Image.LANCZOS)))
        assert np.array_equal(w.thumbnail(200), np.asarray(_pillow_level(path, 2).resize((200, 140), Image.LANCZOS)))
        full = np.asarray(_pillow_level(path, 0))
        assert np.array_equal(w.thumbnail(), full)                                    # narrower than 2 048: level 0, not upsampled
        assert np.array_equal(w.thumbnail(1001), full)
        monkeypatch.setattr(WSI, 'READ_LIMIT', 300)                                   # read in pieces: the same bytes
        assert np.array_equal(w.thumbnail(2048), full)
        assert np.array_equal(w.thumbnail(400), np.asarray(_pillow_level(path, 1).resize((400, 280), Image.LANCZOS)))
        with pytest.raises(SlideError):
            w.thumbnail(0)
    finally:
        w.close()
