"""The feature map end to end (biscuit_amd/featuremap.py): three self-written PNG TFRecords of 12 tiles, synthetic weights,
``max_tiles = 10`` -- a kept tile's numbers against ``evaluate()`` over the same slides, the map, the table, the mosaic and the
command line.  ``-m gpu``."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from biscuit_amd import featuremap as fm
from biscuit_amd import inference as inf
from biscuit_amd import tfrecord as tfr
from biscuit_amd.synthetic import make_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(mc_n=8, seed=3)
COLUMNS = ['slide', 'loc_x', 'loc_y', 'x', 'y', 'cohort-y_pred1', 'cohort-uncertainty1', 'confident']


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


@pytest.fixture(scope='module')
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp('cohort')
    paths, tiles = [], []
    for i, name in enumerate(('a', 'b', 'c')):
        t = make_tiles(12, seed=40 + i, slide_bias=[(i % 2) * 60.0 - 30.0, 0.0, i * 10.0])
        loc = np.stack([np.arange(12) % 4 * 299 + 150, np.arange(12) // 4 * 299 + 150 + 1000 * i], 1).astype(np.int64)
        paths.append(str(d / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
        tiles.append(t)
    return paths, tiles


@pytest.fixture(scope='module')
def fmap(eng, cohort):
    slides = inf.slides_from_tfrecords(cohort[0], {'a': 0, 'b': 1, 'c': 1})
    return fm.generate_features(eng, slides, max_tiles=10, **KW)


def test_thirty_rows_with_the_numbers_of_evaluate(eng, cohort, fmap):
    paths, tiles = cohort
    assert len(fmap) == 30 and fmap.slide == ['a'] * 10 + ['b'] * 10 + ['c'] * 10
    assert fmap.index.tolist() == list(range(10)) * 3
    assert np.array_equal(fmap.tiles, np.concatenate([t[:10] for t in tiles]))
    assert fmap.loc[11].tolist() == [1 * 299 + 150, 150 + 1000] and fmap.loc.shape == (30, 2)
    res = inf.evaluate(eng, inf.slides_from_tfrecords(paths, {'a': 0, 'b': 1, 'c': 1}), outcome='cohort', batch=16, **KW)
    df = res.tile_df
    assert len(df) == 36
    keep = np.concatenate([np.arange(10) + 12 * i for i in range(3)])
    mean = np.stack([df['cohort-y_pred0'].to_numpy(), df['cohort-y_pred1'].to_numpy()], 1).astype(np.float32)[keep]
    std = np.stack([df['cohort-uncertainty0'].to_numpy(), df['cohort-uncertainty1'].to_numpy()], 1).astype(np.float32)[keep]
    assert np.array_equal(fmap.y_pred.view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(fmap.uncertainty.view(np.uint32), std.view(np.uint32))
    assert (fmap.uncertainty > 0).all()
    feat = torch.cat([eng.backbone_u8(torch.from_numpy(t[:10].copy()).to(eng.device)) for t in tiles]).cpu().numpy()
    assert fmap.features.shape == (30, 2048) and fmap.features.dtype == np.float32
    assert np.array_equal(fmap.features.view(np.uint32), feat.view(np.uint32))


def test_map_table_and_mosaic(eng, fmap, tmp_path):
    xy = fm.embed(eng, fmap.features, n_neighbors=15)
    assert xy.shape == (30, 2) and xy.dtype == np.float32 and np.isfinite(xy).all()
    again = fm.embed(eng, fmap.features, n_neighbors=15)
    assert np.array_equal(xy.view(np.uint32), again.view(np.uint32))
    fm.embed(eng, fmap, n_neighbors=15)
    assert np.array_equal(fmap.xy.view(np.uint32), xy.view(np.uint32))
    fmap.labels = {'a': 'wt', 'b': 'mut', 'c': 'mut'}
    image = fm.mosaic(eng, fmap, num_tiles_x=4, cell_px=40)
    cells, (ny, nx) = fm.mosaic_cells(fmap.xy, 4)
    assert nx == 4 and image.shape == (ny * 40, 4 * 40, 3) and cells == fmap.mosaic_cells and 1 <= len(cells) <= ny * nx
    assert len({p for _, _, p in cells}) == len(cells) and len({(x, y) for x, y, _ in cells}) == len(cells)
    used = np.zeros((ny, nx), bool)
    for x, y, p in cells:
        canvas = torch.from_numpy(fmap.tiles[p].copy()).to(eng.device)
        want = eng.tile_resample(canvas, torch.zeros((1, 2), dtype=torch.int32, device=eng.device), 299, 40).cpu().numpy()[0]
        assert np.array_equal(image[y * 40:(y + 1) * 40, x * 40:(x + 1) * 40], want), (x, y, p)
        used[y, x] = True
    for y, x in zip(*np.nonzero(~used)):
        assert (image[y * 40:(y + 1) * 40, x * 40:(x + 1) * 40] == 255).all()
    # the assignment: every point lies in its cell, and no point of that cell is nearer the cell's centre
    lo, hi = fmap.xy.astype(np.float64).min(0), fmap.xy.astype(np.float64).max(0)
    side = (hi[0] - lo[0]) / 4
    for x, y, p in cells:
        centre = np.array([lo[0] + (x + 0.5) * side, hi[1] - (y + 0.5) * side])
        inside = [q for q in range(30) if min(int((fmap.xy[q, 0] - lo[0]) / side), 3) == x and min(int((hi[1] - fmap.xy[q, 1]) / side), ny - 1) == y]
        assert p in inside and all(((fmap.xy[p] - centre) ** 2).sum() <= ((fmap.xy[q] - centre) ** 2).sum() for q in inside)
    paths = fmap.save(str(tmp_path), 'cohort', tile_uq=float(np.median(fmap.uncertainty[:, 1])))
    assert [os.path.basename(p) for p in paths] == ['umap.csv', 'mosaic.png']
    df = pd.read_csv(paths[0])
    assert list(df.columns) == COLUMNS + ['label'] and len(df) == 30
    assert 0 < int(df['confident'].sum()) < 30
    assert np.array_equal(df['confident'].to_numpy(), df['cohort-uncertainty1'].to_numpy() < np.median(fmap.uncertainty[:, 1]).astype(np.float64))
    assert np.array_equal(df['x'].to_numpy().astype(np.float32), fmap.xy[:, 0]) and df['label'].tolist() == ['wt'] * 10 + ['mut'] * 20
    assert np.array_equal(np.asarray(Image.open(paths[1])), image)


def test_command_line_writes_the_same_files(eng, cohort, fmap, tmp_path):
    out = str(tmp_path / 'cli')
    cmd = [sys.executable, '-m', 'biscuit_amd.featuremap', *cohort[0], '--out', out, '--mc', '8', '--seed', '3', '--n-neighbors', '15',
           '--mosaic', '4', '--cell-px', '40', '--tile-uq', '0.05']
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    info = json.loads(done.stdout.strip().splitlines()[-1])
    assert info['tiles'] == 30 and info['slides'] == 3
    df = pd.read_csv(os.path.join(out, 'umap.csv'))
    assert list(df.columns) == COLUMNS and len(df) == 30
    assert np.array_equal(df['cohort-y_pred1'].to_numpy().astype(np.float32), fmap.y_pred[:, 1])
    assert np.array_equal(df['cohort-uncertainty1'].to_numpy().astype(np.float32), fmap.uncertainty[:, 1])
    xy = fm.embed(eng, fmap.features, n_neighbors=15)
    assert np.array_equal(df[['x', 'y']].to_numpy().astype(np.float32), xy)
    img = np.asarray(Image.open(os.path.join(out, 'mosaic.png')))
    _, (ny, nx) = fm.mosaic_cells(xy, 4)
    assert img.shape == (ny * 40, nx * 40, 3)
