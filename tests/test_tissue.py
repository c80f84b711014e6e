"""The heatmap's tissue mask on the host (DESIGN.md "Heatmap input", Tissue mask; ``biscuit_amd/tissue.py``): the numpy restatement's
median against scipy, the exact Otsu threshold against brute force over fractions, the cells' thumbnail ranges, ``WSI.bands(keep=
...)`` and what ``Heatmap.from_slide`` refuses.  The device side is tests/test_gpu_tissue.py."""
import numpy as np
import pytest

from biscuit_amd import tissue
from tests import _tissue_ref as T
from tests.test_wsi import _slide_file


@pytest.mark.parametrize('shape', [(1, 1), (3, 9), (7, 7), (9, 3), (40, 33)])
def test_reference_median_equals_scipy(shape):
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for hi in (256, 4):                                                      # (4: many ties inside a window)
        s = rng.integers(0, hi, shape, dtype=np.uint8)
        assert np.array_equal(T.median7(s), median_filter(s, size=7, mode='nearest'))


def test_sdiv_table_and_saturation():
    t = tissue.sdiv_table()
    assert t.dtype == np.int32 and t.shape == (256,) and t[0] == 0 and t[255] == 4096 and t[1] == 255 * 4096
    img = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [200, 100, 100], [7, 7, 6]]], np.uint8)
    assert T.saturation(img).tolist() == [[0, 0, 255, 127, 36]]              # 100 * 5222 / 4096 = 127.49 (sdiv[200] = rint(5222.4)) and 255 / 7 = 36.4


def _hists():
    rng = np.random.default_rng(5)
    out = {f'random{i}': rng.integers(0, 1000, 256) for i in range(4)}
    sparse = np.zeros(256, np.int64)
    sparse[rng.choice(256, 9, replace=False)] = rng.integers(1, 50, 9)
    out['sparse'] = sparse
    out['bimodal'] = np.bincount(np.concatenate([rng.integers(0, 4, 5000), rng.integers(90, 256, 3000)]), minlength=256)
    return out


@pytest.mark.parametrize('name', sorted(_hists()))
def test_otsu_equals_brute_force(name):
    h = _hists()[name]
    assert tissue.otsu_threshold(h) == T.otsu(h)


def test_otsu_corner_cases():
    def hist(**bins):
        h = np.zeros(256, np.int64)
        for k, v in bins.items():
            h[int(k[1:])] = v
        return h
    assert tissue.otsu_threshold(np.zeros(256, np.int32)) == 0
    for b in (0, 17, 255):
        assert tissue.otsu_threshold(hist(**{f'b{b}': 9})) == T.otsu(hist(**{f'b{b}': 9})) == 0          # one occupied bin
    two = hist(b20=3, b200=11)
    assert tissue.otsu_threshold(two) == T.otsu(two) == 20                   # every t in 20 .. 199 ties: the smallest
    assert tissue.otsu_threshold(hist(b254=1, b255=1)) == 254
    sym = hist(b0=7, b100=4, b200=7)                                         # mirror-symmetric: t = 0 .. 99 ties with t = 100 .. 199
    assert tissue.otsu_threshold(sym) == T.otsu(sym) == 0
    big = (1 << 31) - 2
    for h in (hist(b0=big, b100=3, b200=big), hist(b0=big, b100=3, b200=big - 1), hist(b0=big - 1, b100=3, b200=big),
              hist(b3=big, b4=big, b250=big, b251=big + 1)):
        assert tissue.otsu_threshold(h) == T.otsu(h)                         # float64 scores would round these ties away
    assert tissue.otsu_threshold(hist(b0=big, b100=3, b200=big)) == 0
    for bad in (np.zeros(255, np.int32), np.zeros(256, np.float32), -np.ones(256, np.int32)):
        with pytest.raises(ValueError):
            tissue.otsu_threshold(bad)


GEOMETRIES = [                            # gw, gh, W, H, slide_w0, slide_h0, stride, extract_px
    (4, 3, 600, 450, 2400, 1800, 598, 598),
    (7, 5, 600, 450, 2400, 1800, 299, 598),
    (4, 3, 2048, 1536, 2400, 1800, 598, 598),
    (167, 120, 2048, 1475, 100000, 72000, 598, 598),
    (40, 30, 13, 9, 24000, 18000, 598, 598),                                 # cells narrower than a thumbnail pixel
    (1, 1, 1, 1, 700, 650, 598, 598),
]


@pytest.mark.parametrize('geom', GEOMETRIES)
def test_cell_ranges(geom):
    gw, gh, W, H, w0, h0, stride, px = geom
    col, row = tissue.cell_ranges(*geom)
    rc, rr = T.cell_ranges(*geom)
    assert col.dtype == row.dtype == np.int32 and np.array_equal(col, rc) and np.array_equal(row, rr)
    for r, n, cells in ((col, W, gw), (row, H, gh)):
        assert r.shape == (cells, 2) and (r[:, 0] >= 0).all() and (r[:, 0] < r[:, 1]).all() and (r[:, 1] <= n).all()
        assert (np.diff(r[:, 0]) >= 0).all() and (np.diff(r[:, 1]) >= 0).all()          # monotone in the cell index
        if stride == px:                                                     # stride_div = 1: neighbours leave no column out
            assert r[0, 0] == 0 and (r[1:, 0] <= r[:-1, 1]).all()
    with pytest.raises(ValueError):
        tissue.cell_ranges(gw, gh, W, H, w0, h0, 0, px)
    with pytest.raises(ValueError):
        tissue.cell_ranges(gw, gh, 0, H, w0, h0, stride, px)
    with pytest.raises(ValueError):
        tissue.cell_ranges(gw, gh, 1 << 16, 1 << 15, w0, h0, stride, px)


def test_keep_from_counts():
    col, row = np.array([[0, 5], [5, 6]], np.int32), np.array([[0, 2], [2, 5], [5, 6]], np.int32)
    counts = np.array([[6, 2], [9, 1], [4, 0]], np.int32)                   # areas 10, 2 / 15, 3 / 5, 1
    keep = tissue.keep_from_counts(counts, col, row, 0.6)
    assert keep.dtype == np.bool_ and keep.tolist() == [[True, False], [True, True], [False, True]]     # 0.6 itself is kept
    assert tissue.keep_from_counts(counts, col, row, 1.0).all() and not tissue.keep_from_counts(counts + (counts == 0), col, row, 0.0).any()
    for bad in (dict(counts=counts[:2]), dict(qc_fraction=1.5), dict(counts=counts + 20)):
        with pytest.raises(ValueError):
            tissue.keep_from_counts(**dict(dict(counts=counts, col=col, row=row, qc_fraction=0.6), **bad))


def _same_bands(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[:4] == y[:4] and np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]) and x[6] == y[6]


def _check_bands(w, keep, canvas_bytes):
    """The band rule: -> the bands."""
    bands = list(w.bands(canvas_bytes, keep=keep))
    seen = np.zeros(keep.shape, np.int64)
    for gy0, gy1, gx0, gx1, canvas, origin, src_px in bands:
        sub = keep[gy0:gy1, gx0:gx1]
        assert sub.size and sub[0].any() and sub[-1].any() and sub[:, 0].any() and sub[:, -1].any()
        assert keep[gy0:gy1].any(1).all()                                    # no grid row without a kept cell is read
        want = w.band(gy0, gy1, gx0, gx1)
        assert len(origin) == sub.size and np.array_equal(origin, want[1]) and np.array_equal(canvas, want[0]) and src_px == want[2]
        seen[gy0:gy1, gx0:gx1] += 1
    assert seen.max(initial=0) <= 1 and (seen[keep] == 1).all()             # disjoint, and every kept cell once
    return bands


def _masks(gh, gw):
    one = np.zeros((gh, gw), bool)
    one[3, 5] = True
    blob = np.zeros((gh, gw), bool)                                          # empty rows above, between and below
    blob[1, 2:5] = True
    blob[3, 1] = blob[3, 4] = blob[3, 6] = True
    rng = np.random.default_rng(2)
    return {'all': np.ones((gh, gw), bool), 'one': one, 'blob': blob, 'random': rng.random((gh, gw)) < 0.4}


@pytest.mark.parametrize('limit', [None, 1300], ids=['one_range', 'split_columns'])
@pytest.mark.parametrize('canvas_bytes', [1, 256 << 20])
def test_bands_with_a_mask(tmp_path, monkeypatch, limit, canvas_bytes):
    from biscuit_amd.wsi import WSI
    path, _ = _slide_file(tmp_path)
    if limit:
        monkeypatch.setattr(WSI, 'READ_LIMIT', limit)
    w = WSI(path, stride_div=2)
    try:
        assert (w.grid_h, w.grid_w) == (5, 7)
        plain = list(w.bands(canvas_bytes))
        assert len(plain) == (5 if canvas_bytes == 1 else 2 if limit else 1) * (3 if limit else 1)     # (READ_LIMIT bounds a band's rows too)
        _same_bands(plain, list(w.bands(canvas_bytes, keep=None)))
        _same_bands(plain, list(w.bands(canvas_bytes, segments=False, keep=None)))
        masks = _masks(w.grid_h, w.grid_w)
        got = {k: _check_bands(w, m, canvas_bytes) for k, m in masks.items()}
        _same_bands(plain, got['all'])
        assert [b[:4] for b in got['one']] == [(3, 4, 5, 6)]
        rows = sorted({(b[0], b[1]) for b in got['blob']})
        assert rows == [(1, 2), (3, 4)]                                      # the empty row between ends a band whatever the budget
        assert [b[:4] for b in got['blob']] == ([(1, 2, 2, 3), (1, 2, 3, 5), (3, 4, 1, 2), (3, 4, 4, 5), (3, 4, 6, 7)] if limit else
                                                [(1, 2, 2, 5), (3, 4, 1, 7)])
        assert list(w.bands(canvas_bytes, keep=np.zeros((5, 7), bool))) == []
        for bad in (np.ones((5, 6), bool), np.ones((5, 7), np.uint8)):
            with pytest.raises(ValueError):
                list(w.bands(canvas_bytes, keep=bad))
        seg = list(w.bands(canvas_bytes, segments=True, keep=masks['blob']))  # (not a JPEG page: geometry only)
        assert [b[:4] for b in seg] == [b[:4] for b in got['blob']] and all(b[4] is None for b in seg)
    finally:
        w.close()


def test_from_slide_refusals(tmp_path):
    """None of these reaches the engine."""
    from biscuit_amd.heatmap import Heatmap
    path, _ = _slide_file(tmp_path)
    ok = np.ones((3, 4), bool)
    for kw in (dict(resample='host', qc='otsu'), dict(resample='host', cell_mask=ok), dict(qc='blur'), dict(qc='both'),
               dict(cell_mask=np.ones((4, 3), bool)), dict(cell_mask=np.ones((3, 4), np.uint8)), dict(cell_mask=ok[:2]),
               dict(qc='otsu', qc_fraction=1.5), dict(qc='otsu', qc_width=0)):
        with pytest.raises(ValueError):
            Heatmap.from_slide(None, path, **kw)
