"""The heatmap's output stage on the device (DESIGN.md "Heatmap output"): ``Engine.heatmap_render`` against the numpy restatement
(``tests/_render_ref.py``) byte for byte, and ``Heatmap.save`` / ``python -m biscuit_amd.heatmap --render`` end to end: ``-m gpu``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from tests import _render_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# grid 5 x 7 under a thumbnail of 83 x 61 (pitch 249): tiles of 800 level-0 pixels at stride 400 (stride_div = 2), so the cells
# start 200 pixels = 4 output pixels in; the grid ends before the right edge and one output row before the bottom
MAIN = dict(slide_w0=4150, slide_h0=3050, stride=400, extract_px=800)
VMIN, VMAX = 0.125, 0.875


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


def _thumb(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _lut():
    from biscuit_amd.render import PRGN_TRUNC
    return PRGN_TRUNC


@pytest.fixture(scope='module')
def main_case():
    rng = np.random.default_rng(7)
    v = rng.uniform(0.0, 1.0, (7, 5)).astype(np.float32)
    v[1, 1], v[2, 3], v[4, 0], v[5, 4] = VMIN, VMAX, VMIN - 0.05, VMAX + 3.0        # exactly the bounds, below, above
    v[3, 2] = v[0, 0] = v[6, 3] = ref.MASKED                                       # interior, corner, bottom row
    v[2, 1] = np.nan
    v[4, 4] = np.inf
    return v, _thumb(61, 83, 1)


def _gpu(eng, values, thumb, geom, mode='none', vmin=0.0, vmax=1.0, alpha=0.6, inplace=False, lut=None):
    import torch
    from biscuit_amd import render as R
    gh, gw = values.shape
    col, row = R.render_tables(gw, gh, thumb.shape[1], thumb.shape[0], interpolation=mode, **geom)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)                     # noqa: E731
    d_thumb = up(thumb)
    out = eng.heatmap_render(up(values), up(col), up(row), up(_lut() if lut is None else lut), d_thumb, vmin=vmin, vmax=vmax,
                             alpha=alpha, interpolation=mode, out=d_thumb if inplace else None)
    assert (out.data_ptr() == d_thumb.data_ptr()) == inplace
    if not inplace:
        assert np.array_equal(d_thumb.cpu().numpy(), thumb)                         # the thumbnail is read only
    return out.cpu().numpy()


@pytest.mark.parametrize('inplace', [False, True], ids=['out', 'inplace'])
@pytest.mark.parametrize('alpha', [0.0, 0.6, 1.0])
@pytest.mark.parametrize('mode', ['none', 'bicubic'])
def test_main_case_equals_the_restatement(eng, main_case, mode, alpha, inplace):
    v, thumb = main_case
    want = ref.render(v, thumb, _lut(), vmin=VMIN, vmax=VMAX, alpha=alpha, interpolation=mode, **MAIN)
    got = _gpu(eng, v, thumb, MAIN, mode, VMIN, VMAX, alpha, inplace)
    assert got.dtype == np.uint8 and got.shape == thumb.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:5].tolist()
    # the construction: a transparent margin on all four sides, holes where the cells are masked or not finite, colour elsewhere
    drawn = (want != thumb).any(-1)
    if alpha == 0.0:
        assert not drawn.any()
        return
    assert not drawn[:4].any() and not drawn[:, :4].any() and not drawn[-1:].any() and not drawn[:, 44:].any()
    assert drawn[4:60, 4:44].mean() > 0.8 and not drawn[4 + 3 * 8:4 + 4 * 8, 4 + 2 * 8:4 + 3 * 8].any()       # cell (2, 3) is a hole
    if alpha == 1.0:
        cell = lambda gx, gy: want[4 + 8 * gy + 4, 4 + 8 * gx + 4].tolist()                   # noqa: E731
        if mode == 'none':
            assert cell(1, 1) == _lut()[0].tolist() == cell(0, 4) and cell(3, 2) == _lut()[255].tolist() == cell(4, 5)


@pytest.mark.parametrize('mode', ['none', 'bicubic'])
@pytest.mark.parametrize('w,h', [(1, 4), (3, 4), (5, 4), (7, 1), (2, 2)])
def test_narrow_thumbnails(eng, mode, w, h):
    """Widths below one thread's four pixels, rows whose run has no aligned group of four, one row."""
    v = np.random.default_rng(w * 10 + h).uniform(0, 1, (2, 3)).astype(np.float32)
    v[0, 1] = ref.MASKED
    geom = dict(slide_w0=1200, slide_h0=900, stride=377, extract_px=377)
    thumb = _thumb(h, w, 2)
    want = ref.render(v, thumb, _lut(), interpolation=mode, **geom)
    for inplace in (False, True):
        assert np.array_equal(_gpu(eng, v, thumb, geom, mode, inplace=inplace), want)


@pytest.mark.parametrize('mode', ['none', 'bicubic'])
def test_all_masked_is_the_thumbnail(eng, mode):
    v = np.full((4, 6), ref.MASKED, np.float32)
    v[1, 2] = np.nan
    thumb = _thumb(37, 50, 3)
    geom = dict(slide_w0=3600, slide_h0=2400, stride=600, extract_px=600)
    assert np.array_equal(ref.render(v, thumb, _lut(), interpolation=mode, **geom), thumb)
    assert np.array_equal(_gpu(eng, v, thumb, geom, mode, alpha=1.0), thumb)
    assert np.array_equal(_gpu(eng, v, thumb, geom, mode, alpha=1.0, inplace=True), thumb)


def test_bicubic_around_a_single_live_cell(eng):
    """One live cell among masked ones: the taps on masked cells are dropped and the rest renormalised -- the cell keeps its own
    colour --, and nothing outside the cell is coloured."""
    v = np.full((5, 5), ref.MASKED, np.float32)
    v[2, 2] = 0.3
    geom = dict(slide_w0=3000, slide_h0=3000, stride=600, extract_px=600)
    thumb = _thumb(45, 45, 4)
    want = ref.render(v, thumb, _lut(), alpha=1.0, interpolation='bicubic', **geom)
    got = _gpu(eng, v, thumb, geom, 'bicubic', alpha=1.0)
    assert np.array_equal(got, want)
    inside = np.zeros((45, 45), bool)
    inside[18:27, 18:27] = True
    q = int(ref.cell_q(v, 0.0, 1.0)[2, 2])
    assert (got[inside] == _lut()[q >> 8]).all() and np.array_equal(got[~inside], thumb[~inside])
    # the other way round, a masked cell among live ones: a clean hole, and its neighbours' colours do not use its -1
    v = np.full((5, 5), 0.3, np.float32)
    v[2, 2] = ref.MASKED
    got = _gpu(eng, v, thumb, geom, 'bicubic', alpha=1.0)
    assert np.array_equal(got, ref.render(v, thumb, _lut(), alpha=1.0, interpolation='bicubic', **geom))
    assert np.array_equal(got[inside], thumb[inside]) and (got[~inside] == _lut()[q >> 8]).all()


@pytest.mark.parametrize('mode', ['none', 'bicubic'])
def test_block_borders(eng, mode):
    """One cell under 64 x 64 pixels, then rows of 2 049 pixels: longer than one block's share of the column table."""
    one = np.array([[0.7]], np.float32)
    geom = dict(slide_w0=640, slide_h0=640, stride=600, extract_px=600)
    thumb = _thumb(64, 64, 5)
    assert np.array_equal(_gpu(eng, one, thumb, geom, mode), ref.render(one, thumb, _lut(), interpolation=mode, **geom))
    v = np.random.default_rng(6).uniform(0, 1, (2, 3)).astype(np.float32)
    v[1, 2] = ref.MASKED
    geom = dict(slide_w0=1200, slide_h0=900, stride=377, extract_px=377)
    thumb = _thumb(5, 2049, 6)
    want = ref.render(v, thumb, _lut(), interpolation=mode, **geom)
    assert np.array_equal(_gpu(eng, v, thumb, geom, mode), want) and np.array_equal(_gpu(eng, v, thumb, geom, mode, inplace=True), want)


def test_deterministic_and_independent_of_earlier_launches(eng, main_case):
    v, thumb = main_case
    first = _gpu(eng, v, thumb, MAIN, 'bicubic', VMIN, VMAX)
    other = _gpu(eng, np.full((2, 3), 0.9, np.float32), _thumb(5, 2049, 8), dict(slide_w0=1200, slide_h0=900, stride=377, extract_px=377),
                 'bicubic', lut=255 - _lut())
    assert other.shape == (5, 2049, 3)
    again = _gpu(eng, v, thumb, MAIN, 'bicubic', VMIN, VMAX)
    assert np.array_equal(first, again) and np.array_equal(again, _gpu(eng, v, thumb, MAIN, 'bicubic', VMIN, VMAX, inplace=True))


def test_refusals(eng, main_case):
    import torch
    from biscuit_amd import render as R
    from biscuit_amd.engine import BiscuitHipError
    v, thumb = main_case
    dev = eng.device
    col, row = R.render_tables(5, 7, 83, 61, **MAIN)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (v, col, row, _lut(), thumb)]
    for kw in (dict(vmin=1.0, vmax=1.0), dict(vmax=float('inf')), dict(alpha=1.5), dict(interpolation='bilinear'),
               dict(interpolation='bicubic')):                                     # (the tables are 'none' tables)
        with pytest.raises(ValueError):
            eng.heatmap_render(*d, **kw)
    with pytest.raises(ValueError):
        eng.heatmap_render(d[0], d[1], d[2], d[3][:255], d[4])
    big = torch.zeros(61 * 83 * 3 + 12, dtype=torch.uint8, device=dev)
    inside, shifted = big[:61 * 83 * 3].view(61, 83, 3), big[12:].view(61, 83, 3)
    with pytest.raises(BiscuitHipError, match='overlap'):
        eng.heatmap_render(d[0], d[1], d[2], d[3], inside, out=shifted)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = [t.data_ptr() for t in d]
    call = lambda gh, gw, mode, H, W, inv, A: eng._lib.bq_heatmap_render(eng._ctx, p[0], gh, gw, p[1], p[2], mode, p[3], p[4],       # noqa: E731
                                                                          big.data_ptr(), H, W, 0.0, inv, A, st)
    for args in ((0, 5, 0, 61, 83, 1.0, 154), (7, 5, 2, 61, 83, 1.0, 154), (7, 5, 0, 0, 83, 1.0, 154), (7, 5, 0, 61, 16385, 1.0, 154),
                 (7, 5, 0, 61, 83, 0.0, 154), (7, 5, 0, 61, 83, float('inf'), 154), (7, 5, 0, 61, 83, 1.0, 257), (7, 5, 0, 61, 83, 1.0, -1)):
        assert call(*args) == -1                                                    # BQ_ERR_ARG, nothing enqueued
    torch.cuda.synchronize()
    assert (big == 0).all()


# ---- end to end: a slide file -> from_slide -> save -> PNGs; the command line ------------------------------------------------------
def _slide(tmp_path):
    """1 200 x 900 level-0 pixels as JPEG tiles of 256 (4:2:0), a second level of 300 x 225; 0.8 um a pixel: tiles of 377 pixels,
    a 3 x 2 grid that leaves 69 pixels on the right and 146 at the bottom."""
    from tests._wsi_jpeg_cases import page, write_slide
    yy, xx = np.mgrid[0:900, 0:1200]
    a = np.stack([150 + 80 * np.sin(xx / 41.0), 120 + 70 * np.cos(yy / 33.0), 140 + 60 * np.sin((xx + yy) / 57.0)], -1)
    a = np.clip(a + np.random.default_rng(9).integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    b = np.asarray(Image.fromarray(a).resize((300, 225), Image.BILINEAR))
    return write_slide(tmp_path / 'case.svs', [page(a, 256, 256, 2, desc='Aperio |MPP = 0.8'), page(b, 256, 256, 0)])


def _png(path):
    return np.asarray(Image.open(path).convert('RGB'))


def test_save_and_command_line(eng, tmp_path):
    from biscuit_amd.heatmap import MASKED, Heatmap
    from biscuit_amd.render import PRGN_TRUNC, render_tables
    from biscuit_amd.wsi import WSI
    path = _slide(tmp_path)
    hm = Heatmap.from_slide(eng, path, mc_n=2, batch=8)
    assert hm.logits.shape == (2, 3, 2) and (hm.slide_w0, hm.slide_h0, hm.stride, hm.extract_px) == (1200, 900, 377, 377)
    host = Heatmap.from_slide(eng, path, mc_n=2, batch=8, resample='host')          # the geometry is recorded for both modes
    assert (host.slide_w0, host.slide_h0, host.stride, host.extract_px, host.slide_path) == (1200, 900, 377, 377, path)
    assert np.array_equal(host.logits, hm.logits)
    unc = hm.uncertainty[:, :, 0]
    thr = float(np.median(unc[unc >= 0]))
    mask = unc > thr
    assert mask.any() and not mask.all()
    before = hm.logits.copy()
    out = str(tmp_path / 'api')
    paths = hm.save(eng, out, tile_uq_thresh=thr, width=400)
    assert np.array_equal(hm.logits, before)                                        # save masks a copy
    names = ['case-raw.png', 'case-0.png', 'case-1.png', 'case-uncertainty.png', os.path.join('high_confidence', 'case-0.png'),
             os.path.join('high_confidence', 'case-1.png')]
    assert [os.path.relpath(p, out) for p in paths] == names and all(os.path.exists(p) for p in paths)
    w = WSI(path)
    thumb = w.thumbnail(400)
    w.close()
    assert thumb.shape == (300, 400, 3) and np.array_equal(_png(paths[0]), thumb)
    geom = dict(slide_w0=1200, slide_h0=900, stride=377, extract_px=377)
    for c in (0, 1):
        assert np.array_equal(_png(paths[1 + c]), ref.render(hm.logits[:, :, c], thumb, PRGN_TRUNC, **geom))
    assert np.array_equal(_png(paths[3]), ref.render(unc, thumb, PRGN_TRUNC, vmin=0.0, vmax=float(unc.max()), **geom))
    masked = hm.logits.copy()
    masked[mask, :] = MASKED
    col, row = render_tables(3, 2, 400, 300, **geom)
    hole = (row[:, None] >= 0) & (col[None, :] >= 0) & mask[np.maximum(row, 0)[:, None], np.maximum(col, 0)[None, :]]
    assert hole.any() and not hole.all()
    for c in (0, 1):
        full, conf = _png(paths[1 + c]), _png(paths[4 + c])
        assert np.array_equal(conf, ref.render(masked[:, :, c], thumb, PRGN_TRUNC, **geom))
        assert np.array_equal(conf[~hole], full[~hole]) and np.array_equal(conf[hole], thumb[hole]) and (conf[hole] != full[hole]).any()
    # bicubic and another alpha through the same door; a heatmap without a slide takes the thumbnail and the geometry as keywords
    img = hm.render(eng, 'uncertainty', 1, thumb=thumb, vmax=0.5, alpha=0.3, interpolation='bicubic')
    assert np.array_equal(img, ref.render(hm.uncertainty[:, :, 1], thumb, PRGN_TRUNC, vmax=0.5, alpha=0.3, interpolation='bicubic', **geom))
    bare = Heatmap.__new__(Heatmap)
    bare.logits, bare.uncertainty = hm.logits, hm.uncertainty
    with pytest.raises(ValueError, match='extract_px'):
        bare.render(eng, thumb=thumb)
    assert np.array_equal(bare.render(eng, thumb=thumb, **geom), _png(paths[1]))

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, '-m', 'biscuit_amd.heatmap', path, '--mc', '2', '--batch', '8', '--tile-uq', repr(thr)]
    cli = str(tmp_path / 'cli')
    p = subprocess.run(base + ['--out', cli, '--render', '--render-width', '400'], capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    s = json.load(open(os.path.join(cli, 'summary.json')))
    assert s['rendered'] == names and json.loads(p.stdout.strip().splitlines()[-1]) == s
    for n in names:
        assert np.array_equal(_png(os.path.join(cli, n)), _png(os.path.join(out, n))), n
    assert sorted(os.listdir(cli)) == sorted(names[:4] + ['heatmap.npz', 'high_confidence', 'summary.json'])
    z = np.load(os.path.join(cli, 'heatmap.npz'))
    assert np.array_equal(z['logits'], hm.logits) and np.array_equal(z['uq_mask'], mask) and np.array_equal(z['masked_logits'], masked)
    plain = str(tmp_path / 'plain')
    p = subprocess.run(base + ['--out', plain], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(plain)) == ['heatmap.npz', 'summary.json']             # without --render: what it always wrote
    s0 = json.load(open(os.path.join(plain, 'summary.json')))
    assert 'rendered' not in s0 and set(s0) == set(s) - {'rendered'} and json.loads(p.stdout.strip().splitlines()[-1]) == s0
    assert np.array_equal(np.load(os.path.join(plain, 'heatmap.npz'))['masked_logits'], masked)
