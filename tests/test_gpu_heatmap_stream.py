"""The streamed whole-slide heatmap on the device: ``Engine.tile_resample`` against Pillow byte for byte, ``Heatmap.from_slide(
resample='gpu')`` against the host path bit for bit, the background filter and the ``python -m biscuit_amd.heatmap`` command
line: ``-m gpu``."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import _resample_ref as R
from tests.test_wsi import _img, _slide_file, _tiff, _tiles_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = {'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, 6.0]}


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


@pytest.mark.parametrize('src', R.WIDTHS)
def test_tile_resample_equals_pillow(eng, src):
    import torch
    canvas, origin = R.case(src)
    want = R.pillow_tiles(canvas, origin, src)
    d_canvas, d_origin = torch.from_numpy(canvas).to(eng.device), torch.from_numpy(origin).to(eng.device)
    got = eng.tile_resample(d_canvas, d_origin, src).cpu().numpy()            # one batch: overlapping, partial and outside windows
    for i in range(len(origin)):
        assert np.array_equal(got[i], want[i]), (src, origin[i].tolist(), int(np.abs(got[i].astype(int) - want[i]).max()))
    # into a slice of a larger buffer (how from_slide fills a batch), tiles in another order; the neighbours stay untouched
    buf = torch.full((len(origin) + 3, R.PX, R.PX, 3), 91, dtype=torch.uint8, device=eng.device)
    rev = torch.from_numpy(origin[::-1].copy()).to(eng.device)
    out = eng.tile_resample(d_canvas, rev, src, out=buf[2:2 + len(origin)])
    assert out.data_ptr() == buf[2:].data_ptr()
    b = buf.cpu().numpy()
    assert np.array_equal(b[2:2 + len(origin)], want[::-1]) and (b[:2] == 91).all() and (b[-1:] == 91).all()
    assert eng.tile_resample(d_canvas, d_origin[:0], src).shape == (0, R.PX, R.PX, 3)      # n = 0: no launch


def test_tile_resample_refusals(eng):
    import torch
    from biscuit_amd.engine import BiscuitHipError
    canvas = torch.zeros((64, 64, 3), dtype=torch.uint8, device=eng.device)
    origin = torch.zeros((1, 2), dtype=torch.int32, device=eng.device)
    from biscuit_amd.resample import ResampleError
    with pytest.raises(ResampleError):
        eng.tile_resample(canvas, origin, 9 * 299)
    b, c = torch.zeros((299, 2), dtype=torch.int32, device=eng.device), torch.zeros((299, 9), dtype=torch.int32, device=eng.device)
    out = torch.full((1, 299, 299, 3), 7, dtype=torch.uint8, device=eng.device)
    ptr = lambda t: t.data_ptr()                                                              # noqa: E731
    st = torch.cuda.current_stream(eng.device).cuda_stream
    call = lambda n, src, px, k: eng._lib.bq_tile_resample(eng._ctx, ptr(canvas), 64, 64, ptr(origin), n, src, px, ptr(b), ptr(c), k,  # noqa: E731
                                                           ptr(out), st)
    assert call(1, 302, 299, 9) == 0
    for args in ((-1, 302, 299, 9), (1, 302, 0, 9), (1, 9 * 299, 299, 9), (1, 302, 299, 7), (1, 10, 299, 7)):
        assert call(*args) == -1                                                              # BQ_ERR_ARG, nothing enqueued
    with pytest.raises(BiscuitHipError):
        eng._check(call(1, 302, 299, 11))
    assert call(0, 302, 299, 9) == 0


@pytest.mark.parametrize('stride_div', [1, 2])
@pytest.mark.parametrize('fit', [None, FIT], ids=['plain', 'reinhard'])
def test_streamed_heatmap_equals_host_path(eng, tmp_path, stride_div, fit):
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.wsi import WSI
    path, _ = _slide_file(tmp_path)
    w = WSI(path, stride_div=stride_div)
    assert sum(1 for _ in w.bands(1)) >= 3                                  # the budget below forces at least three bands
    w.close()
    kw = dict(stride_div=stride_div, mc_n=8, seed=3, batch=16, norm_fit=fit)
    host = Heatmap.from_slide(eng, path, resample='host', **kw)
    gpu = Heatmap.from_slide(eng, path, resample='gpu', canvas_bytes=1, **kw)
    assert gpu.logits.shape == host.logits.shape == ((3, 4, 2) if stride_div == 1 else (5, 7, 2))
    assert np.array_equal(gpu.logits, host.logits) and np.array_equal(gpu.uncertainty, host.uncertainty)
    assert np.array_equal(gpu.grid, host.grid) and gpu.dropped == 0 and (gpu.uncertainty[:, :, 0] > 0).all()
    one = Heatmap.from_slide(eng, path, **kw)                                # the default: one band
    assert np.array_equal(one.logits, host.logits) and np.array_equal(one.uncertainty, host.uncertainty)


def test_streamed_heatmap_with_split_columns(eng, tmp_path, monkeypatch):
    """A slide whose grid rows are wider than one read (``WSI.READ_LIMIT``, lowered here) reaches the engine band by band, not in
    row-major order, in other batches than the host path's: every cell's values are still the host path's, bit for bit."""
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.wsi import WSI
    path, _ = _slide_file(tmp_path)
    kw = dict(stride_div=2, mc_n=8, seed=3, batch=16, norm_fit=FIT)
    host = Heatmap.from_slide(eng, path, resample='host', **kw)
    monkeypatch.setattr(WSI, 'READ_LIMIT', 1300)
    gpu = Heatmap.from_slide(eng, path, resample='gpu', **kw)
    assert np.array_equal(gpu.logits, host.logits) and np.array_equal(gpu.uncertainty, host.uncertainty)
    assert not np.array_equal(gpu.grid, host.grid) and sorted(map(tuple, gpu.grid.tolist())) == sorted(map(tuple, host.grid.tolist()))


def test_tile_resample_refuses_a_grid_beyond_the_launch_limit(eng):
    """n x strips of output rows is one grid dimension: beyond 2^31 - 1 workgroups the call is BQ_ERR_ARG, nothing enqueued."""
    import torch
    from biscuit_amd import resample
    px, src = 2048, 2050                                                     # the LDS holds one output row's taps: 2 048 strips a tile
    b, c = resample.taps(src, px)
    db, dc = torch.from_numpy(b).to(eng.device), torch.from_numpy(c).to(eng.device)
    canvas = torch.zeros((8, 8, 3), dtype=torch.uint8, device=eng.device)
    origin = torch.zeros((1, 2), dtype=torch.int32, device=eng.device)
    st = torch.cuda.current_stream(eng.device).cuda_stream
    rc = eng._lib.bq_tile_resample(eng._ctx, canvas.data_ptr(), 8, 8, origin.data_ptr(), 1 << 20, src, px, db.data_ptr(), dc.data_ptr(),
                                   int(c.shape[1]), canvas.data_ptr(), st)
    assert rc == -1 and b'workgroups' in eng._lib.bq_last_error(eng._ctx)
    rc = eng._lib.bq_tile_resample(eng._ctx, canvas.data_ptr(), 8, 8, origin.data_ptr(), 1, 4100, 4096, db.data_ptr(), dc.data_ptr(), 9,
                                   canvas.data_ptr(), st)
    assert rc == -1 and b'LDS' in eng._lib.bq_last_error(eng._ctx)          # px = 4 096: not even one row's taps fit
    torch.cuda.synchronize()


def _mixed_tiles():
    rng = np.random.default_rng(11)
    t = rng.integers(0, 256, (6, 299, 299, 3), dtype=np.uint8)              # saturated noise
    g = rng.integers(0, 256, (299, 299, 1), dtype=np.uint8)
    t[1] = np.clip(g.astype(int) + rng.integers(-3, 4, (299, 299, 3)), 0, 255)   # near-grey: saturations around the thresholds
    t[2, :150] = 0                                                           # black (mx = 0: s = 0)
    t[3, :, 100:] = 255                                                      # white
    t[4] = 255
    t[5, ::2] = np.clip(g[::2].astype(int) + rng.integers(-12, 13, (150, 299, 3)), 0, 255)
    return t


@pytest.mark.parametrize('thr', [0.05, 0.1, 0.5])
def test_grey_counts_equal_numpy(eng, thr):
    import torch
    from biscuit_amd import resample
    t = _mixed_tiles()
    want = resample.grayspace_count(t, thr)
    assert len(set(want.tolist())) >= 5 and want[4] == 299 * 299 and 0 < want[0] < want[1]
    got = eng.tile_grayspace(torch.from_numpy(t).to(eng.device), thr).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)


def _margin_slide(tmp_path):
    """The two-level test slide with everything right of x = 1196 white: grid columns 2 and 3 of the 4 x 3 grid are glass."""
    w, h = 2400, 1800
    a = _img(w, h, 5)
    a[:, 1196:] = 255
    b = np.asarray(Image.fromarray(a).resize((w // 4, h // 4), Image.BILINEAR))
    raw = lambda t: zlib.compress(t.tobytes(), 1)                                            # noqa: E731
    path = tmp_path / 'margin.svs'
    path.write_bytes(_tiff([dict(w=w, h=h, tw=256, th=256, comp=8, segs=_tiles_of(a, 256, 256, raw), desc='Aperio |MPP = 0.5045'),
                            dict(w=w // 4, h=h // 4, tw=256, th=256, comp=8, segs=_tiles_of(b, 256, 256, raw))]))
    return str(path)


def test_background_filter_keeps_tissue_cells_bit_for_bit(eng, tmp_path):
    from biscuit_amd import resample
    from biscuit_amd.heatmap import MASKED, Heatmap
    from biscuit_amd.wsi import WSI
    path = _margin_slide(tmp_path)
    # the construction, on the CPU with the numpy definition: which cells the filter must drop
    w = WSI(path)
    tiles, grid = w.tiles()
    w.close()
    frac = resample.grayspace_count(tiles, 0.05) / (299 * 299)
    drop = frac > 0.6
    assert len(grid) == 12 and drop.sum() >= 3 and (~drop).sum() >= 3        # at least a quarter dropped, at least a quarter kept
    assert (frac[drop] > 0.9).all() and (frac[~drop] < 0.3).all()             # and none of them near the bar
    kw = dict(mc_n=8, seed=3, batch=16, canvas_bytes=1)
    full = Heatmap.from_slide(eng, path, **kw)
    filt = Heatmap.from_slide(eng, path, grayspace_fraction=0.6, grayspace_threshold=0.05, **kw)
    assert filt.dropped == int(drop.sum()) and len(filt.grid) == int((~drop).sum()) and full.dropped == 0 and len(full.grid) == 12
    assert sorted(map(tuple, filt.grid.tolist())) == sorted(map(tuple, grid[~drop].tolist()))
    for (gx, gy), d in zip(grid.tolist(), drop):
        if d:
            assert (filt.logits[gy, gx] == MASKED).all() and (filt.uncertainty[gy, gx] == MASKED).all()
        else:
            assert np.array_equal(filt.logits[gy, gx], full.logits[gy, gx]) and np.array_equal(filt.uncertainty[gy, gx], full.uncertainty[gy, gx])
            assert filt.uncertainty[gy, gx, 0] > 0
    incl, excl = filt.split_by_uncertainty(float(np.median(full.uncertainty[:, :, 0])))
    assert len(incl) + len(excl) == len(filt.grid)
    with pytest.raises(ValueError):
        Heatmap.from_slide(eng, path, resample='host', grayspace_fraction=0.6)


def test_command_line(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path = _margin_slide(tmp_path)
    out = str(tmp_path / 'out')
    thr = 0.0
    api = Heatmap.from_slide(eng, path, mc_n=8, seed=3, batch=16, grayspace_fraction=0.6)
    thr = float(np.median(api.uncertainty[:, :, 0][api.uncertainty[:, :, 0] >= 0]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd.heatmap', path, '--out', out, '--mc', '8', '--seed', '3', '--batch', '16',
                        '--tile-uq', repr(thr), '--grayspace-fraction', '0.6', '--save-tiles'], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(os.path.join(out, 'heatmap.npz'))
    assert np.array_equal(z['logits'], api.logits) and np.array_equal(z['uncertainty'], api.uncertainty) and np.array_equal(z['grid'], api.grid)
    incl, excl = api.split_by_uncertainty(thr)
    mask = api.mask_uncertain(thr)
    assert np.array_equal(z['uq_mask'], mask) and np.array_equal(z['masked_logits'], api.logits) and mask.any() and not mask.all()
    s = json.load(open(os.path.join(out, 'summary.json')))
    assert s['grid_shape'] == [3, 4] and s['tiles_run'] == len(api.grid) == 6 and s['tiles_dropped'] == api.dropped == 6
    assert s['seconds'] > 0 and s['tiles_per_s'] > 0 and json.loads(p.stdout.strip().splitlines()[-1]) == s
    assert sorted(os.listdir(os.path.join(out, 'uq_incl'))) == sorted(n for _, n in incl) and len(incl) > 0
    assert sorted(os.listdir(os.path.join(out, 'uq_excl'))) == sorted(n for _, n in excl) and len(excl) > 0
    i, name = incl[0]
    gx, gy = api.grid[i]
    from biscuit_amd.wsi import WSI
    w = WSI(path)
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, 'uq_incl', name))), w._tile(int(gx), int(gy)))
    w.close()
