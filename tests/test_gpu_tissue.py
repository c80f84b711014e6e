"""The heatmap's tissue mask on the device (DESIGN.md "Heatmap input", Tissue mask): ``Engine.tissue_blur`` and ``Engine.tissue_cells``
against the numpy restatement (tests/_tissue_ref.py) integer for integer, their refusals, the lifetime of their host tables, ``Heatmap.from_slide(qc='otsu')`` against
the unmasked run bit for bit, and the command line: ``-m gpu``."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import _tissue_ref as T
from tests import _wsi_jpeg_cases as J
from tests.test_wsi import _tiff, _tiles_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(mc_n=8, seed=3, batch=16, canvas_bytes=1)
QC = dict(qc='otsu', qc_width=600)                                           # the coarse level's own width: no resize


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (5, 3), (7, 7), (64, 64), (67, 131), (300, 517)]           # (H, W): below the window, one tile, several ragged tiles


def _contents(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    black = noise.copy()
    black[rng.random((h, w)) < 0.5] = 0                                      # mx = 0
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
    grad = np.zeros((h, w, 3), np.uint8)
    grad[:, :, 0] = np.linspace(0, 255, w).astype(np.uint8)[None, :]
    grad[:, :, 1] = 255 - grad[:, :, 0]
    grad[:, :, 2] = 128
    half = (255 - rng.integers(0, 3, (h, w, 3))).astype(np.uint8)            # near-white ...
    half[:, w // 2:] = rng.integers(0, 256, (h, w - w // 2, 3), dtype=np.uint8) // np.array([1, 4, 2], np.uint8)   # ... and saturated
    return {'noise': noise, 'constant': np.full((h, w, 3), (201, 77, 140), np.uint8), 'black': black,
            'primaries': prim[rng.integers(0, len(prim), (h, w))], 'gradient': grad, 'half': half}


def _blur(eng, img):
    import torch
    plane, hist = eng.tissue_blur(torch.from_numpy(img).to(eng.device))
    return plane.cpu().numpy(), hist.cpu().numpy()


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_blur_equals_reference(eng, size):
    for name, img in _contents(*size).items():
        want_plane, want_hist = T.blur(img)
        plane, hist = _blur(eng, img)
        assert plane.dtype == np.uint8 and hist.dtype == np.int32 and plane.shape == size and hist.shape == (256,)
        assert np.array_equal(plane, want_plane), (name, size, int((plane != want_plane).sum()))
        assert np.array_equal(hist, want_hist) and int(hist.sum()) == size[0] * size[1], (name, size)


def test_cells_equal_reference(eng):
    import torch
    from biscuit_amd import tissue
    img = _contents(67, 131)['half']
    plane = T.blur(img)[0]
    d_plane = torch.from_numpy(plane).to(eng.device)
    otsu = T.otsu(T.blur(img)[1])
    assert otsu < 200 and tissue.otsu_threshold(_blur(eng, img)[1]) == otsu
    geoms = [(7, 5, 131, 67, 2400, 1800, 299, 598),                          # stride_div = 2: cells overlap
             (4, 3, 131, 67, 2400, 1800, 598, 598),
             (131, 30, 131, 67, 131 * 598, 67 * 598, 598, 598),              # a cell is one thumbnail pixel
             (40, 30, 131, 67, 24000, 18000, 598, 598),
             (1, 1, 131, 67, 131, 67, 131, 67)]                              # one cell = the whole plane
    for g in geoms:
        col, row = T.cell_ranges(*g)
        if g[0] == 131:
            assert ((col[:, 1] - col[:, 0]) == 1).all() and ((row[:, 1] - row[:, 0]) == 1).all()
        if g[0] == 7:
            assert (col[1:, 0] < col[:-1, 1]).all()
        for thr in (0, 255, otsu):
            want = T.cell_counts(plane, thr, col, row)
            got = eng.tissue_cells(d_plane, thr, col, row).cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, want), (g, thr)
            if thr == 255:
                assert np.array_equal(got, (row[:, 1] - row[:, 0])[:, None] * (col[:, 1] - col[:, 0])[None, :])
        assert len(np.unique(T.cell_counts(plane, otsu, col, row))) > 1 or g[0] == 1


def test_bad_arguments(eng):
    """Argument checks only: every refusal is BQ_ERR_ARG (-1) from the C entry before anything is enqueued."""
    import torch
    dev = eng.device
    thumb = torch.zeros((8, 9, 3), dtype=torch.uint8, device=dev)
    plane, hist = eng.tissue_blur(thumb)
    sdiv = eng._tables['tissue_blur', None]
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()                                               # noqa: E731
    blur = lambda th, h, w, sd, pl, hi: eng._lib.bq_tissue_blur(eng._ctx, th, h, w, sd, pl, hi, st)      # noqa: E731
    assert blur(p(thumb), 8, 9, p(sdiv), p(plane), p(hist)) == 0
    for args in ((None, 8, 9, p(sdiv), p(plane), p(hist)), (p(thumb), 8, 9, None, p(plane), p(hist)),
                 (p(thumb), 8, 9, p(sdiv), None, p(hist)), (p(thumb), 8, 9, p(sdiv), p(plane), None),
                 (p(thumb), 0, 9, p(sdiv), p(plane), p(hist)), (p(thumb), 8, -1, p(sdiv), p(plane), p(hist)),
                 (p(thumb), 1 << 16, 1 << 15, p(sdiv), p(plane), p(hist))):  # H * W = 2^31
        assert blur(*args) == -1
    assert b'bq_tissue_blur' in eng._lib.bq_last_error(eng._ctx)
    col, row = np.array([[0, 4], [4, 9]], np.int32), np.array([[0, 8]], np.int32)
    ranges = torch.zeros(6, dtype=torch.int32, device=dev)
    count = torch.full((1, 2), -7, dtype=torch.int32, device=dev)

    def cells(pl=p(plane), h=8, w=9, t=3, c=col, r=row, rg=p(ranges), cn=p(count)):
        return eng._lib.bq_tissue_cells(eng._ctx, pl, h, w, t, None if c is None else c.ctypes.data, 0 if c is None else len(c),
                                        None if r is None else r.ctypes.data, 0 if r is None else len(r), rg, cn, st)
    a = lambda *v: np.array(v, np.int32).reshape(-1, 2)                      # noqa: E731
    for kw in (dict(pl=None), dict(rg=None), dict(cn=None), dict(t=-1), dict(t=256), dict(h=1 << 16, w=1 << 15),
               dict(c=a(0, 4, 4, 4)), dict(c=a(0, 4, 5, 4)), dict(c=a(0, 4, 4, 10)), dict(c=a(-1, 4, 4, 9)),
               dict(r=a(0, 9)), dict(r=a(8, 8)), dict(r=a(3, 2))):
        assert cells(**kw) == -1, kw
    assert b'bq_tissue_cells' in eng._lib.bq_last_error(eng._ctx)
    assert (count.cpu().numpy() == -7).all()                                 # nothing was enqueued
    assert cells() == 0 and count.cpu().numpy().tolist() == [[32, 40]]       # (a black thumbnail: S = 0 <= 3 everywhere)
    for bad in (dict(col=a(0, 4, 4, 10)), dict(row=a(2, 2)), dict(T=256), dict(plane=plane.to(torch.int32)), dict(col=np.zeros((2, 3), np.int32))):
        with pytest.raises(ValueError):
            eng.tissue_cells(**dict(dict(plane=plane, T=3, col=col, row=row), **bad))
    for bad in (thumb[:, :, :2], thumb.to(torch.int32), thumb[:0]):
        with pytest.raises(ValueError):
            eng.tissue_blur(bad)


def test_tables_outlive_their_calls(eng):
    """The engine's contract for the host tables it hands to the stream (``Engine._hold``): eight ``tissue_cells`` /
    ``tissue_cells_union`` calls and two ``roi_plane`` calls on one stream with nothing in between that waits, every call with tables
    of its own.  The caller's are int64, so the int32 copies the stream reads are referenced by the engine alone."""
    import torch
    from tests import _focus_ref as F
    from tests import _roi_ref as R
    rng = np.random.default_rng(20)
    otsu, focus = rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 2, (24, 32), dtype=np.uint8)
    d_otsu, d_focus = torch.from_numpy(otsu).to(eng.device), torch.from_numpy(focus).to(eng.device)

    def ranges(cells, n):
        a = rng.integers(0, n, cells)
        return np.stack([a, rng.integers(a + 1, n + 1)], 1).astype(np.int64)
    cases = [(int(rng.integers(0, 256)), ranges(4, 64), ranges(3, 48)) for _ in range(8)]
    triangle = [np.array([[3, 2], [90, 20], [30, 70]])]
    samples = [(rng.integers(0, 200, 7).astype(np.int64), rng.integers(0, 160, 5).astype(np.int64)) for _ in range(2)]
    torch.cuda.synchronize(eng.device)
    got, planes = [], []
    for i, (thr, col, row) in enumerate(cases):
        got.append(eng.tissue_cells(d_otsu, thr, col, row) if i % 2 == 0 else eng.tissue_cells_union(d_otsu, thr, d_focus, col, row))
        if i in (2, 5):
            planes.append(eng.roi_plane(*samples[len(planes)], triangle))
    torch.cuda.synchronize(eng.device)
    for i, (thr, col, row) in enumerate(cases):
        want = T.cell_counts(otsu, thr, col, row) if i % 2 == 0 else F.union_counts(otsu, thr, focus, col, row)
        assert got[i].shape == (3, 4) and np.array_equal(got[i].cpu().numpy(), want), i
    for (xs, ys), plane in zip(samples, planes):
        assert plane.shape == (5, 7) and np.array_equal(plane.cpu().numpy(), R.plane(xs, ys, triangle))
    assert len({g.cpu().numpy().tobytes() for g in got}) == 8 and all(0 < int(p.sum()) < 35 for p in planes)      # (no two alike, none trivial)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _tissue_image(w=2400, h=1800):
    """Glass (near-white) with tissue -- saturated colours in 8 x 8 blocks -- over x < 1076, y < 1196: of the 4 x 3 grid of 598-pixel
    cells, (0, 0) and (0, 1) are all tissue, (1, 0) and (1, 1) a fifth glass, the other eight glass."""
    rng = np.random.default_rng(17)
    a = (255 - rng.integers(0, 3, (h, w, 3))).astype(np.uint8)
    blocks = np.stack([rng.integers(150, 256, (150, 135)), rng.integers(20, 81, (150, 135)), rng.integers(100, 201, (150, 135))], -1)
    tis = np.kron(blocks, np.ones((8, 8, 1), np.int64)) + rng.integers(-4, 5, (1200, 1080, 3))
    a[:1196, :1076] = np.clip(tis, 0, 255)[:1196, :1076]
    return a


def _deflate_slide(tmp_path):
    a = _tissue_image()
    b = np.asarray(Image.fromarray(a).resize((600, 450), Image.BILINEAR))
    raw = lambda t: zlib.compress(t.tobytes(), 1)                                            # noqa: E731
    path = tmp_path / 'tissue.svs'
    path.write_bytes(_tiff([dict(w=2400, h=1800, tw=256, th=256, comp=8, segs=_tiles_of(a, 256, 256, raw), desc='Aperio |MPP = 0.5045'),
                            dict(w=600, h=450, tw=256, th=256, comp=8, segs=_tiles_of(b, 256, 256, raw))]))
    return str(path)


def _jpeg_slide(tmp_path):
    a = _tissue_image()
    b = np.asarray(Image.fromarray(a).resize((600, 450), Image.BILINEAR))
    return J.write_slide(tmp_path / 'tissue_jpeg.svs', [J.page(a, 256, 256, 2, desc='Aperio |MPP = 0.5045'), J.page(b, 256, 256, 0)])


def _expected(path):
    """On the CPU, from the reference alone: the keep mask of the slide, its threshold, and that no cell is near the bar."""
    from biscuit_amd.wsi import WSI
    w = WSI(path)
    try:
        thumb = w.thumbnail(600)
        assert thumb.shape == (450, 600, 3) and (w.grid_h, w.grid_w) == (3, 4)
        keep, thr, frac = T.mask(thumb, w.grid_w, w.grid_h, *w.slide.dimensions, w.stride, w.extract_px)
    finally:
        w.close()
    assert ((frac < 0.3) | (frac > 0.9)).all() and (frac < 0.3).sum() >= 3 and (frac > 0.9).sum() >= 3, frac
    assert np.array_equal(keep, frac < 0.3)
    return keep, thr


def _compare(hm, full, keep, grayspace_drop=None):
    from biscuit_amd.heatmap import MASKED
    ran = keep if grayspace_drop is None else keep & ~grayspace_drop
    assert np.array_equal(hm.cell_mask, keep) and hm.cell_mask.dtype == np.bool_
    assert np.array_equal(hm.logits[ran], full.logits[ran]) and np.array_equal(hm.uncertainty[ran], full.uncertainty[ran])
    assert (hm.logits[~ran] == MASKED).all() and (hm.uncertainty[~ran] == MASKED).all() and (hm.uncertainty[ran][:, 0] > 0).all()
    assert hm.dropped == int((~ran).sum()) and hm.qc['cells_dropped'] == int((~keep).sum())
    assert sorted(map(tuple, hm.grid.tolist())) == sorted((int(x), int(y)) for y, x in zip(*np.nonzero(ran)))
    assert hm.qc['bands_skipped_rows'] == int((~keep.any(1)).sum())
    assert hm.qc['bands_read'] == int(keep.any(1).sum()) == hm.decode_stats['gpu_bands'] + hm.decode_stats['host_bands']   # canvas_bytes = 1


@pytest.fixture(scope='module')
def slide(eng, tmp_path_factory):
    """The deflate slide, its expected mask and its unmasked heatmap, computed once."""
    from biscuit_amd.heatmap import Heatmap
    path = _deflate_slide(tmp_path_factory.mktemp('tissue'))
    keep, thr = _expected(path)
    full = Heatmap.from_slide(eng, path, **KW)
    assert full.qc is None and full.cell_mask is None and full.dropped == 0 and len(full.grid) == 12
    return path, keep, thr, full


def test_otsu_mask_keeps_tissue_cells_bit_for_bit(eng, slide):
    from biscuit_amd.heatmap import Heatmap
    path, keep, thr, full = slide
    assert keep.tolist() == [[True, True, False, False], [True, True, False, False], [False] * 4]
    hm = Heatmap.from_slide(eng, path, **QC, **KW)
    _compare(hm, full, keep)
    assert hm.qc['method'] == 'otsu' and hm.qc['threshold'] == thr and set(hm.qc) == {'method', 'threshold', 'cells_dropped', 'bands_read',
                                                                                      'bands_skipped_rows'}
    assert hm.qc['bands_read'] == 2 < full.decode_stats['host_bands'] == 3
    # a fraction no cell exceeds keeps everything: the unmasked run's arrays
    every = Heatmap.from_slide(eng, path, qc='otsu', qc_width=600, qc_fraction=1.0, **KW)
    assert every.cell_mask.all() and every.dropped == 0 and np.array_equal(every.logits, full.logits) and np.array_equal(every.grid, full.grid)


def test_otsu_mask_with_device_decode(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path = _jpeg_slide(tmp_path)
    keep, thr = _expected(path)
    full = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    hm = Heatmap.from_slide(eng, path, decode='gpu', **QC, **KW)
    _compare(hm, full, keep)
    assert hm.qc['threshold'] == thr and hm.decode_stats['gpu_bands'] == 2 and hm.decode_stats['host_bands'] == 0
    assert full.decode_stats['gpu_bands'] == 3 and 0 < hm.decode_stats['segments'] < full.decode_stats['segments']


def test_cell_mask_by_hand_and_with_otsu(eng, slide):
    from biscuit_amd.heatmap import MASKED, Heatmap
    path, keep, thr, full = slide
    hand = np.ones((3, 4), bool)
    hand[0, 0] = hand[2, 3] = False
    both = Heatmap.from_slide(eng, path, cell_mask=hand, **QC, **KW)
    _compare(both, full, keep & hand)
    assert both.qc['method'] == 'otsu' and both.qc['threshold'] == thr and hand[0, 0] == 0       # (the caller's mask is not written to)
    alone = np.zeros((3, 4), bool)
    alone[0, 3] = alone[2, 1] = alone[2, 2] = True                           # glass cells the Otsu mask would drop; row 1 is skipped
    hm = Heatmap.from_slide(eng, path, cell_mask=alone, **KW)
    _compare(hm, full, alone)
    assert hm.qc['method'] is None and hm.qc['threshold'] is None and hm.qc['bands_read'] == 2
    none = Heatmap.from_slide(eng, path, cell_mask=np.zeros((3, 4), bool), **KW)                  # nothing survives: not an error
    assert (none.logits == MASKED).all() and none.grid.shape == (0, 2) and none.dropped == 12 and none.qc['bands_read'] == 0


def test_grayspace_filter_after_the_mask(eng, slide):
    from biscuit_amd import resample
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.wsi import WSI
    path, keep, thr, full = slide
    w = WSI(path)
    tiles, grid = w.tiles()
    w.close()
    frac = (resample.grayspace_count(tiles, 0.05) / (299 * 299)).reshape(3, 4)
    drop = frac > 0.1
    assert ((frac < 0.02) | (frac > 0.15)).all() and (keep & drop).sum() == 2 and (keep & ~drop).sum() == 2     # column 1: a fifth glass
    hm = Heatmap.from_slide(eng, path, grayspace_fraction=0.1, grayspace_threshold=0.05, **QC, **KW)
    _compare(hm, full, keep, grayspace_drop=drop)
    assert hm.dropped == 10 and hm.qc['cells_dropped'] == 8


def test_command_line(eng, slide, tmp_path, capsys):
    from biscuit_amd import heatmap
    path, keep, thr, full = slide
    api = heatmap.Heatmap.from_slide(eng, path, mc_n=8, seed=3, batch=16, **QC)
    out = str(tmp_path / 'qc')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd.heatmap', path, '--out', out, '--mc', '8', '--seed', '3', '--batch', '16',
                        '--qc', 'otsu', '--qc-width', '600', '--qc-fraction', '0.6'], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(os.path.join(out, 'heatmap.npz'))
    assert np.array_equal(z['cell_mask'], keep) and z['cell_mask'].dtype == np.bool_
    assert np.array_equal(z['logits'], api.logits) and np.array_equal(z['uncertainty'], api.uncertainty) and np.array_equal(z['grid'], api.grid)
    s = json.load(open(os.path.join(out, 'summary.json')))
    assert s['qc'] == api.qc and s['qc']['threshold'] == thr and s['tiles_run'] == 4 and s['tiles_dropped'] == 8
    assert json.loads(p.stdout.strip().splitlines()[-1]) == s
    # without the option (the same entry point, in this process): neither appears, and the arrays are the unmasked run's
    plain = str(tmp_path / 'plain')
    heatmap.main([path, '--out', plain, '--mc', '8', '--seed', '3', '--batch', '16'])
    capsys.readouterr()
    z = np.load(os.path.join(plain, 'heatmap.npz'))
    assert sorted(z.files) == ['grid', 'logits', 'uncertainty']
    assert np.array_equal(z['logits'], full.logits) and np.array_equal(z['uncertainty'], full.uncertainty) and np.array_equal(z['grid'], full.grid)
    s = json.load(open(os.path.join(plain, 'summary.json')))
    assert 'qc' not in s and s['tiles_run'] == 12 and s['tiles_dropped'] == 0
