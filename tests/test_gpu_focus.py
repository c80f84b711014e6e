"""The heatmap's focus mask on the device (DESIGN.md "Heatmap input", Focus mask): ``Engine.tissue_focus`` and
``Engine.tissue_cells_union`` against the numpy restatement (tests/_focus_ref.py) integer for integer, their refusals,
``Heatmap.from_slide(focus_threshold=...)`` alone and with ``qc='otsu'`` against the unmasked run bit for bit, and the command line:
``-m gpu``."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import _focus_ref as F
from tests import _tissue_ref as T
from tests import _wsi_jpeg_cases as J
from tests.test_focus import ramped_noise
from tests.test_gpu_tissue import KW, ROOT, _compare
from tests.test_wsi import _tiff, _tiles_of

pytestmark = pytest.mark.gpu

QC = dict(qc='otsu', qc_width=600)                                           # the coarse level's own width: no resize
FOCUS = dict(focus_threshold=0.02)


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


# ---- bq_tissue_focus ---------------------------------------------------------------------------------------------------------------
# (H, W): the smallest image; narrower / shorter than every halo; below the radius; one past a tile either way (the rows kernel's
# tile is 8 x 32, the columns kernel's 32 x 32); each tile exactly; several tiles with ragged edges
SIZES = [(1, 1), (1, 40), (40, 1), (7, 5), (33, 9), (9, 33), (8, 32), (32, 32), (97, 131)]


def _contents(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    corner = np.full((h, w, 3), 40, np.uint8)
    corner[h - 1, w - 1] = 255                                               # the clamped borders repeat it
    checker = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)[:, :, None].repeat(3, 2)
    return {'constant': np.full((h, w, 3), (201, 77, 140), np.uint8), 'noise': rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            'ramp': ramped_noise(h, w), 'checker': checker, 'corner': corner}


def _focus(eng, img, **kw):
    import torch
    plane, count, value = eng.tissue_focus(torch.from_numpy(img).to(eng.device), value=True, **kw)
    assert count.shape == (1,) and count.dtype == torch.int32
    return plane.cpu().numpy(), int(count.cpu().numpy()[0]), value.cpu().numpy()


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_focus_equals_reference(eng, size):
    import torch
    h, w = size
    for name, img in _contents(h, w).items():
        want_plane, want_count, want_v = F.focus(img)
        plane, count, v = _focus(eng, img)
        assert plane.dtype == np.uint8 and v.dtype == np.int32 and plane.shape == v.shape == size
        assert np.array_equal(v, want_v), (name, size, int((v != want_v).sum()), int(np.abs(v - want_v).max()))
        assert np.array_equal(plane, want_plane) and count == want_count == int((plane == 0).sum()), (name, size)
        if name == 'constant':
            assert (v == 0).all() and count == h * w                          # no edge anywhere: all out of focus
        if name == 'checker' and h > 1 and w > 1:
            assert int(F.laplace_abs(F.gray(img)).max()) > 1 << 23 and int(want_v.max()) * 65536 > 1 << 32      # beyond a 32-bit sum
    img = _contents(h, w)['ramp']
    plane, count = eng.tissue_focus(torch.from_numpy(img).to(eng.device))     # without V: the same plane
    assert np.array_equal(plane.cpu().numpy(), F.focus(img)[0]) and int(count.cpu().numpy()[0]) == F.focus(img)[1]


def test_ramp_straddles_the_threshold():
    plane, count, v = F.focus(_contents(97, 131)['ramp'])
    assert 0.1 < count / plane.size < 0.9 and plane[:, :20].max() == 0 and plane[:, -20:].min() == 1


@pytest.mark.parametrize('sigma', [0.25, 4.1], ids=['r1', 'r16'])
def test_other_radii_and_thresholds(eng, sigma):
    taps = F.taps(sigma)
    assert len(taps) == (3 if sigma == 0.25 else 33)
    for name in ('noise', 'ramp', 'checker'):
        img = _contents(40, 61)[name]
        for threshold in (0.02, 0.0, 0.3):
            want_plane, want_count, want_v = F.focus(img, F.units(threshold), taps)
            plane, count, v = _focus(eng, img, threshold=threshold, sigma=sigma)
            assert np.array_equal(v, want_v) and np.array_equal(plane, want_plane) and count == want_count, (name, sigma, threshold)


# ---- bq_tissue_cells_union ---------------------------------------------------------------------------------------------------------
def test_union_equals_reference(eng):
    import torch
    rng = np.random.default_rng(11)
    otsu = rng.integers(0, 256, (97, 131), dtype=np.uint8)
    otsu[:, 70:] //= 8                                                       # a darker half: more background at a middling T
    blobs = (rng.random((40, 61)) < 0.6).astype(np.uint8)
    blobs[10:25, 5:30] = 0
    d_otsu = torch.from_numpy(otsu).to(eng.device)
    geoms = [(7, 5, 131, 97, 2400, 1800, 299, 598),                          # stride_div = 2: cells overlap
             (131, 40, 131, 97, 131 * 598, 97 * 598, 598, 598),              # a cell is one pixel of the Otsu plane
             (1, 1, 131, 97, 131, 97, 131, 97)]                              # one cell = the whole plane
    for fname, focus in (('blobs', blobs), ('ones', np.ones((40, 61), np.uint8)), ('zeros', np.zeros((40, 61), np.uint8)),
                         ('wider', (rng.random((200, 300)) < 0.5).astype(np.uint8)), ('pixel', np.ones((1, 1), np.uint8)),
                         ('same', (rng.random((97, 131)) < 0.5).astype(np.uint8))):
        d_focus = torch.from_numpy(focus).to(eng.device)
        for g in geoms:
            col, row = T.cell_ranges(*g)
            if g[0] == 131:
                assert ((col[:, 1] - col[:, 0]) == 1).all() and ((row[:, 1] - row[:, 0]) == 1).all()
            if g[0] == 7:
                assert (col[1:, 0] < col[:-1, 1]).all()
            area = (row[:, 1] - row[:, 0])[:, None] * (col[:, 1] - col[:, 0])[None, :]
            for thr in (0, 255, 40):
                want = F.union_counts(otsu, thr, focus, col, row)
                got = eng.tissue_cells_union(d_otsu, thr, d_focus, col, row).cpu().numpy()
                assert got.dtype == np.int32 and np.array_equal(got, want), (fname, g, thr)
                if fname in ('ones', 'pixel'):                               # nothing out of focus: tissue_cells' own counts
                    assert np.array_equal(got, eng.tissue_cells(d_otsu, thr, col, row).cpu().numpy())
                    assert np.array_equal(got, T.cell_counts(otsu, thr, col, row))
                if fname == 'zeros' or thr == 255:                           # everything bad: the areas
                    assert np.array_equal(got, area)
        if fname == 'blobs':
            col, row = T.cell_ranges(*geoms[0])
            assert len(np.unique(F.union_counts(otsu, 40, focus, col, row))) > 4
            assert (F.union_counts(otsu, 0, focus, col, row) > T.cell_counts(otsu, 0, col, row)).any()


def test_bad_arguments(eng):
    """Argument checks only: every refusal is BQ_ERR_ARG (-1) from the C entry, or a ValueError before it, with nothing enqueued."""
    import torch
    from biscuit_amd import tissue
    dev = eng.device
    thumb = torch.zeros((8, 9, 3), dtype=torch.uint8, device=dev)
    plane, count = eng.tissue_focus(thumb)
    assert int(count.cpu().numpy()[0]) == 72 and not plane.any().item()
    taps = eng._tables['tissue_focus', 3.0]
    assert (taps.numel() - 1) // 2 == 12 and taps.cpu().numpy().tolist() == F.taps()
    work = torch.zeros((8, 9), dtype=torch.int32, device=dev)
    value = torch.full((8, 9), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()                                               # noqa: E731

    def focus(th=p(thumb), h=8, w=9, tp=p(taps), r=12, thr=51000, wk=p(work), v=p(value), pl=p(plane), cn=p(cnt)):
        return eng._lib.bq_tissue_focus(eng._ctx, th, h, w, tp, r, thr, wk, v, pl, cn, st)
    for kw in (dict(th=None), dict(tp=None), dict(wk=None), dict(pl=None), dict(cn=None), dict(h=0), dict(w=-1), dict(h=1 << 16, w=1 << 15),
               dict(r=0), dict(r=17), dict(r=-12), dict(thr=-1)):
        assert focus(**kw) == -1, kw
    assert b'bq_tissue_focus' in eng._lib.bq_last_error(eng._ctx)
    assert (cnt.cpu().numpy() == -7).all() and (value.cpu().numpy() == -7).all()                  # nothing was enqueued
    assert focus(v=None) == 0 and cnt.cpu().numpy().tolist() == [72] and (value.cpu().numpy() == -7).all()
    assert focus() == 0 and (value.cpu().numpy() == 0).all()
    for bad in (thumb[:, :, :2], thumb.to(torch.int32), thumb[:0], thumb[0], thumb.cpu()):        # shape, dtype, empty, dimensions, device
        with pytest.raises(ValueError):
            eng.tissue_focus(bad)
    for kw in (dict(sigma=4.2), dict(sigma=0.0), dict(threshold=-0.5), dict(threshold=float('nan'))):        # r = 17, r = 0
        with pytest.raises(ValueError):
            eng.tissue_focus(thumb, **kw)
    assert ('tissue_focus', 4.2) not in eng._tables and ('tissue_focus', 0.0) not in eng._tables

    otsu = torch.zeros((8, 9), dtype=torch.uint8, device=dev)
    fplane = torch.ones((4, 5), dtype=torch.uint8, device=dev)
    col, row = np.array([[0, 4], [4, 9]], np.int32), np.array([[0, 8]], np.int32)
    xmap, ymap = tissue.plane_map(9, 5), tissue.plane_map(8, 4)
    tables = torch.zeros(9 + 8 + 6, dtype=torch.int32, device=dev)
    out = torch.full((1, 2), -7, dtype=torch.int32, device=dev)

    def union(op=p(otsu), ho=8, wo=9, t=3, fp=p(fplane), hf=4, wf=5, xm=xmap, ym=ymap, c=col, r=row, gw=None, gh=None, tb=p(tables),
              cn=p(out)):
        h = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
        return eng._lib.bq_tissue_cells_union(eng._ctx, op, ho, wo, t, fp, hf, wf, h(xm), h(ym), h(c), len(c) if gw is None else gw,
                                              h(r), len(r) if gh is None else gh, tb, cn, st)
    a = lambda *v: np.array(v, np.int32).reshape(-1, 2)                      # noqa: E731
    m = lambda *v: np.array(v, np.int32)                                     # noqa: E731
    for kw in (dict(op=None), dict(fp=None), dict(tb=None), dict(cn=None), dict(xm=None), dict(ym=None), dict(c=None, gw=2), dict(r=None, gh=1),
               dict(t=-1), dict(t=256), dict(ho=1 << 16, wo=1 << 15), dict(hf=1 << 16, wf=1 << 15), dict(hf=0), dict(gw=0),
               dict(gw=tissue.MAX_GRID + 1), dict(gh=tissue.MAX_GRID + 1),
               dict(c=a(0, 4, 4, 4)), dict(c=a(0, 4, 4, 10)), dict(c=a(-1, 4, 4, 9)), dict(r=a(0, 9)), dict(r=a(3, 2)),
               dict(xm=m(0, 0, 1, 1, 2, 2, 3, 4, 5)), dict(xm=m(-1, 0, 1, 1, 2, 2, 3, 4, 4)), dict(xm=m(0, 1, 0, 1, 2, 2, 3, 4, 4)),
               dict(ym=m(0, 0, 1, 1, 2, 2, 3, 4)), dict(ym=m(0, 0, 1, 1, 3, 2, 3, 3))):
        assert union(**kw) == -1, kw
    assert b'bq_tissue_cells_union' in eng._lib.bq_last_error(eng._ctx)
    assert (out.cpu().numpy() == -7).all()                                   # nothing was enqueued
    assert union() == 0 and out.cpu().numpy().tolist() == [[32, 40]]         # (a black Otsu plane: 0 <= 3 everywhere)
    ok = dict(otsu_plane=otsu, T=3, focus_plane=fplane, col=col, row=row)
    for bad in (dict(col=a(0, 4, 4, 10)), dict(row=a(2, 2)), dict(T=256), dict(otsu_plane=otsu.to(torch.int32)), dict(focus_plane=fplane.cpu()),
                dict(focus_plane=fplane[0]), dict(col=np.zeros((2, 3), np.int32)), dict(xmap=xmap[:8]), dict(ymap=np.append(ymap, 3)),
                dict(xmap=m(0, 0, 1, 1, 2, 2, 3, 4, 5)), dict(ymap=m(0, 0, 1, 1, 3, 2, 3, 3))):
        with pytest.raises(ValueError):
            eng.tissue_cells_union(**dict(ok, **bad))
    assert eng.tissue_cells_union(**ok, xmap=xmap, ymap=ymap).cpu().numpy().tolist() == [[32, 40]]


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _focus_image(w=2400, h=1800):
    """One stained colour over x < 1196, y < 1196 of near-white glass: sharp texture (8 x 8 blocks of a random shade) over x < 598,
    the same texture Gaussian-blurred over 598 <= x < 1196 -- still saturated, so Otsu keeps it.  Of the 4 x 3 grid of 598-pixel
    cells, column 0 of rows 0 and 1 is sharp, column 1 of rows 0 and 1 is out of focus, the other eight are glass."""
    from scipy import ndimage
    rng = np.random.default_rng(23)
    a = (255 - rng.integers(0, 3, (h, w, 3))).astype(np.uint8)
    blocks = np.stack([rng.integers(150, 256, (150, 150)), rng.integers(20, 81, (150, 150)), rng.integers(100, 201, (150, 150))], -1)
    soft = ndimage.gaussian_filter(blocks.astype(np.float64), sigma=(5, 5, 0), mode='nearest')
    tex = np.where((np.arange(150) * 8 < 598)[None, :, None], blocks, np.rint(soft)).astype(np.int64)
    a[:1196, :1196] = np.clip(np.kron(tex, np.ones((8, 8, 1), np.int64)), 0, 255)[:1196, :1196]
    return a


def _pages(a):
    return a, np.asarray(Image.fromarray(a).resize((600, 450), Image.BILINEAR))


def _deflate_slide(tmp_path):
    a, b = _pages(_focus_image())
    raw = lambda t: zlib.compress(t.tobytes(), 1)                                            # noqa: E731
    path = tmp_path / 'focus.svs'
    path.write_bytes(_tiff([dict(w=2400, h=1800, tw=256, th=256, comp=8, segs=_tiles_of(a, 256, 256, raw), desc='Aperio |MPP = 0.5045'),
                            dict(w=600, h=450, tw=256, th=256, comp=8, segs=_tiles_of(b, 256, 256, raw))]))
    return str(path)


def _jpeg_slide(tmp_path):
    a, b = _pages(_focus_image())
    return J.write_slide(tmp_path / 'focus_jpeg.svs', [J.page(a, 256, 256, 2, desc='Aperio |MPP = 0.5045'), J.page(b, 256, 256, 0)])


SHARP = [[True, False, False, False], [True, False, False, False], [False] * 4]
STAINED = [[True, True, False, False], [True, True, False, False], [False] * 4]


def _expected(path, threshold=0.02):
    """On the CPU, from the restatements alone: the keep masks of the slide under Otsu, under focus and under both, the Otsu
    threshold and the focus report; at the default threshold no cell is near the bar under any of them."""
    from biscuit_amd.wsi import WSI
    w = WSI(path)
    try:
        othumb, fthumb = w.thumbnail(600), w.thumbnail(303)                  # 303 = round(2400 * 0.5045 / 4)
        assert othumb.shape == (450, 600, 3) and fthumb.shape == (227, 303, 3) and (w.grid_h, w.grid_w) == (3, 4)
        geom = (w.grid_w, w.grid_h, *w.slide.dimensions, w.stride, w.extract_px)
    finally:
        w.close()
    args = lambda t: geom[:2] + (t.shape[1], t.shape[0]) + geom[2:]          # noqa: E731
    otsu_keep, thr, otsu_frac = T.mask(othumb, *geom)
    fplane, fcount, _ = F.focus(fthumb, F.units(threshold))
    col, row = T.cell_ranges(*args(fthumb))
    focus_keep, focus_frac = F.keep(T.cell_counts(fplane, 0, col, row), col, row)
    oplane = T.blur(othumb)[0]
    col, row = T.cell_ranges(*args(othumb))
    both_keep, both_frac = F.keep(F.union_counts(oplane, thr, fplane, col, row), col, row)
    if threshold == 0.02:
        for frac in (otsu_frac, focus_frac, both_frac):
            assert ((frac < 0.3) | (frac > 0.75)).all(), frac
        assert otsu_keep.tolist() == STAINED and focus_keep.tolist() == SHARP and both_keep.tolist() == SHARP
    return {'otsu': otsu_keep, 'focus': focus_keep, 'both': both_keep, 'threshold': thr,
            'report': {'focus_threshold': float(threshold), 'focus_width': 303, 'focus_share': fcount / float(227 * 303)}}


QC_KEYS = {'method', 'threshold', 'cells_dropped', 'bands_read', 'bands_skipped_rows'}
FOCUS_KEYS = {'focus_threshold', 'focus_width', 'focus_share'}


@pytest.fixture(scope='module')
def slide(eng, tmp_path_factory):
    """The deflate slide, its expected masks and its unmasked heatmap, computed once."""
    from biscuit_amd.heatmap import Heatmap
    path = _deflate_slide(tmp_path_factory.mktemp('focus'))
    want = _expected(path)
    full = Heatmap.from_slide(eng, path, **KW)
    assert full.qc is None and full.cell_mask is None and full.dropped == 0 and len(full.grid) == 12
    return path, want, full


def test_focus_mask_drops_blurred_cells_bit_for_bit(eng, slide):
    from biscuit_amd.heatmap import Heatmap
    path, want, full = slide
    otsu = Heatmap.from_slide(eng, path, **QC, **KW)                          # Otsu alone keeps the blurred cells, and says nothing new
    _compare(otsu, full, want['otsu'])
    assert otsu.cell_mask.tolist() == STAINED and set(otsu.qc) == QC_KEYS
    both = Heatmap.from_slide(eng, path, **QC, **FOCUS, **KW)                 # Slideflow's qc='both'
    _compare(both, full, want['both'])
    assert both.cell_mask.tolist() == SHARP and set(both.qc) == QC_KEYS | FOCUS_KEYS
    assert both.qc['method'] == 'otsu' and both.qc['threshold'] == want['threshold'] == otsu.qc['threshold']
    assert {k: both.qc[k] for k in FOCUS_KEYS} == want['report'] and 0.7 < both.qc['focus_share'] < 0.95
    alone = Heatmap.from_slide(eng, path, **FOCUS, **KW)                      # Slideflow's qc='blur': glass has no edges either
    _compare(alone, full, want['focus'])
    assert alone.cell_mask.tolist() == SHARP and set(alone.qc) == QC_KEYS | FOCUS_KEYS
    assert alone.qc['method'] is None and alone.qc['threshold'] is None and {k: alone.qc[k] for k in FOCUS_KEYS} == want['report']
    # a threshold of 0 calls only perfectly flat pixels out of focus: the blurred cells stay, and the mask is Otsu's
    flat = _expected(path, 0.0)
    assert flat['both'].tolist() == STAINED
    none = Heatmap.from_slide(eng, path, focus_threshold=0.0, **QC, **KW)
    _compare(none, full, flat['both'])
    assert {k: none.qc[k] for k in FOCUS_KEYS} == flat['report']
    # the caller's mask still ANDs on top
    hand = np.ones((3, 4), bool)
    hand[0, 0] = False
    _compare(Heatmap.from_slide(eng, path, cell_mask=hand, **QC, **FOCUS, **KW), full, want['both'] & hand)


def test_focus_mask_with_device_decode(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path = _jpeg_slide(tmp_path)
    want = _expected(path)
    full = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    both = Heatmap.from_slide(eng, path, decode='gpu', **QC, **FOCUS, **KW)
    _compare(both, full, want['both'])
    assert both.qc['threshold'] == want['threshold'] and {k: both.qc[k] for k in FOCUS_KEYS} == want['report']
    assert both.decode_stats['gpu_bands'] == 2 and both.decode_stats['host_bands'] == 0
    assert full.decode_stats['gpu_bands'] == 3 and 0 < both.decode_stats['segments'] < full.decode_stats['segments']
    alone = Heatmap.from_slide(eng, path, decode='gpu', **FOCUS, **KW)
    _compare(alone, full, want['focus'])


def test_command_line(eng, slide, tmp_path, capsys):
    from biscuit_amd import heatmap
    path, want, full = slide
    api = heatmap.Heatmap.from_slide(eng, path, mc_n=8, seed=3, batch=16, **QC, **FOCUS)
    out = str(tmp_path / 'both')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd.heatmap', path, '--out', out, '--mc', '8', '--seed', '3', '--batch', '16',
                        '--qc', 'otsu', '--qc-width', '600', '--qc-focus'], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(os.path.join(out, 'heatmap.npz'))
    assert np.array_equal(z['cell_mask'], want['both']) and z['cell_mask'].dtype == np.bool_
    assert np.array_equal(z['logits'], api.logits) and np.array_equal(z['uncertainty'], api.uncertainty) and np.array_equal(z['grid'], api.grid)
    s = json.load(open(os.path.join(out, 'summary.json')))
    assert s['qc'] == api.qc and set(s['qc']) == QC_KEYS | FOCUS_KEYS and s['qc']['focus_threshold'] == 0.02
    assert s['tiles_run'] == 2 and s['tiles_dropped'] == 10 and json.loads(p.stdout.strip().splitlines()[-1]) == s
    # in this process: the focus mask alone with its own options; then no option at all -- the files of a run without the feature
    solo = str(tmp_path / 'solo')
    heatmap.main([path, '--out', solo, '--mc', '8', '--seed', '3', '--batch', '16', '--qc-focus', '0.02', '--qc-focus-mpp', '4',
                  '--qc-focus-sigma', '3'])
    capsys.readouterr()
    z = np.load(os.path.join(solo, 'heatmap.npz'))
    s = json.load(open(os.path.join(solo, 'summary.json')))
    assert np.array_equal(z['cell_mask'], want['focus']) and s['qc']['method'] is None and s['qc']['focus_width'] == 303
    otsu = heatmap.Heatmap.from_slide(eng, path, mc_n=8, seed=3, batch=16, **QC)
    for name, argv, ref in (('otsu', ['--qc', 'otsu', '--qc-width', '600'], otsu), ('plain', [], full)):
        d = str(tmp_path / name)
        heatmap.main([path, '--out', d, '--mc', '8', '--seed', '3', '--batch', '16'] + argv)
        capsys.readouterr()
        z = np.load(os.path.join(d, 'heatmap.npz'))
        s = json.load(open(os.path.join(d, 'summary.json')))
        assert sorted(z.files) == (['cell_mask'] if argv else []) + ['grid', 'logits', 'uncertainty']
        assert np.array_equal(z['logits'], ref.logits) and np.array_equal(z['uncertainty'], ref.uncertainty) and np.array_equal(z['grid'], ref.grid)
        assert set(s) == {'slide', 'grid_shape', 'tiles_run', 'tiles_dropped', 'seconds', 'tiles_per_s', 'decode_stats'} | ({'qc'} if argv else set())
        if argv:
            assert s['qc'] == otsu.qc and set(s['qc']) == QC_KEYS and np.array_equal(z['cell_mask'], want['otsu'])
