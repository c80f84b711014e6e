"""Tile extraction on the device (``biscuit_amd/extract.py``: slide file -> bands -> ``bq_tile_resample`` -> ``bq_jpeg_encode`` ->
TFRecord) against the host's definition of every step: ``WSI._tile`` for the pixels, ``tfrecord.encode_image`` (Pillow) for the
files, ``evaluate()`` and ``Heatmap`` for what a consumer computes from them.  ``-m gpu``."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from biscuit_amd import tfrecord as tfr
from tests import _wsi_jpeg_cases as wj
from tests.test_wsi import _img, _slide_file, _tiff, _tiles_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    return Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)


def records(path):
    return [tfr.parse_example(r) for r in tfr.read_records(path, verify='full')]


def _two_level(tmp_path, a, name):
    h, w = a.shape[:2]
    b = np.asarray(Image.fromarray(a).resize((w // 4, h // 4), Image.BILINEAR))
    raw = lambda t: zlib.compress(t.tobytes(), 1)                                            # noqa: E731
    path = tmp_path / name
    path.write_bytes(_tiff([dict(w=w, h=h, tw=256, th=256, comp=8, segs=_tiles_of(a, 256, 256, raw), desc='Aperio |MPP = 0.5045'),
                            dict(w=w // 4, h=h // 4, tw=256, th=256, comp=8, segs=_tiles_of(b, 256, 256, raw))]))
    return str(path)


def test_records_are_pillows_files_in_row_major_order_whatever_the_banding(eng, tmp_path, monkeypatch):
    """The 7 x 5 grid (stride_div = 2) of the two-level test slide: every record's image_raw is the file Pillow writes for the
    host's tile of that cell, loc is the cell's centre in level-0 pixels, the records stand in row-major order -- read as one band,
    and as several bands with every row split into column ranges (the cells then reach the device rectangle by rectangle)."""
    from biscuit_amd.extract import extract_slide
    from biscuit_amd.wsi import WSI
    path, _ = _slide_file(tmp_path)
    one = extract_slide(eng, path, str(tmp_path / 'one'), stride_div=2, batch=16)
    assert one['tfrecord'] == str(tmp_path / 'one' / 'slide.tfrecords') and one['grid_shape'] == [5, 7] and one['tiles_written'] == 35
    recs = records(one['tfrecord'])
    w = WSI(path, stride_div=2)
    try:
        assert (w.stride, w.extract_px) == (299, 598)
        for i, r in enumerate(recs):
            gy, gx = divmod(i, 7)
            assert r['slide'] == b'slide' and (r['loc_x'], r['loc_y']) == ([gx * 299 + 299], [gy * 299 + 299]), i
            assert r['image_raw'] == tfr.encode_image(w._tile(gx, gy), 'JPEG'), (gx, gy)
        monkeypatch.setattr(WSI, 'READ_LIMIT', 1300)
        rects = [b[:4] for b in w.bands(1)]
    finally:
        w.close()
    assert len({r[0] for r in rects}) >= 3 and len({r[2] for r in rects}) >= 2           # several bands, and a column split
    split = extract_slide(eng, path, str(tmp_path / 'split'), stride_div=2, batch=16, canvas_bytes=1)
    assert open(split['tfrecord'], 'rb').read() == open(one['tfrecord'], 'rb').read()
    assert split['decode_stats']['host_bands'] == len(rects) and one['decode_stats'] == {'gpu_bands': 0, 'host_bands': 1, 'segments': 0}
    s = json.load(open(str(tmp_path / 'one' / 'slide.extract.json')))
    assert s == json.loads(json.dumps(one)) and s['bytes_written'] == os.path.getsize(one['tfrecord'])
    assert (s['quality'], s['subsampling'], s['cells'], s['cells_dropped']) == (95, '4:2:0', 35, {'masks': 0, 'roi': None, 'grayspace': 0})


def test_masks_write_exactly_the_kept_cells(eng, tmp_path):
    from biscuit_amd.extract import extract_slide, tile_loc
    from biscuit_amd.slide_input import MaskSpec, otsu_mask
    from biscuit_amd.wsi import WSI
    a = _img(2400, 1800, 5)
    a[:, 1196:] = 255                                                        # grid columns 2 and 3 of the 4 x 3 grid are glass
    path = _two_level(tmp_path, a, 'margin.svs')
    full = records(extract_slide(eng, path, str(tmp_path / 'full'), batch=16)['tfrecord'])
    assert len(full) == 12

    def check(summary, keep):
        recs = records(summary['tfrecord'])
        cells = np.flatnonzero(keep.reshape(-1))
        assert summary['tiles_written'] == len(recs) == len(cells) and summary['cells_dropped']['masks'] == 12 - len(cells)
        assert [(r['loc_x'][0], r['loc_y'][0]) for r in recs] == [tuple(x) for x in tile_loc(cells, 4, 598, 598).tolist()]
        assert [r['image_raw'] for r in recs] == [full[c]['image_raw'] for c in cells]     # a kept tile does not depend on the mask

    mine = np.zeros((3, 4), bool)
    mine[0, 3] = mine[1, 0] = mine[1, 2] = mine[2, 1] = True
    check(extract_slide(eng, path, str(tmp_path / 'mine'), batch=16, cell_mask=mine, canvas_bytes=1), mine)
    w = WSI(path)
    try:
        otsu, _ = otsu_mask(eng, w, MaskSpec(qc_width=2048, qc_fraction=0.6))
    finally:
        w.close()
    assert otsu[:, :2].all() and not otsu[:, 2:].any()
    s = extract_slide(eng, path, str(tmp_path / 'otsu'), batch=16, qc='otsu')
    check(s, otsu)
    assert s['qc']['method'] == 'otsu' and s['qc']['threshold'] is not None
    check(extract_slide(eng, path, str(tmp_path / 'both'), batch=16, qc='otsu', cell_mask=mine), otsu & mine)
    grey = extract_slide(eng, path, str(tmp_path / 'grey'), batch=16, grayspace_fraction=0.6)
    assert grey['tiles_written'] == 6 and grey['cells_dropped']['grayspace'] == 6
    assert [r['image_raw'] for r in records(grey['tfrecord'])] == [full[c]['image_raw'] for c in np.flatnonzero(otsu.reshape(-1))]
    none = extract_slide(eng, path, str(tmp_path / 'none'), cell_mask=np.zeros((3, 4), bool))
    assert none['tiles_written'] == 0 and os.path.getsize(none['tfrecord']) == 0


def test_row_major_order_under_a_mask_whose_column_ranges_start_in_different_rows(eng, tmp_path, monkeypatch):
    """One band of three rows in three column ranges; the mask keeps all of the first range, row 2 of the second and row 0 of the
    third, and the first batch fills up inside the second range: the record of the third range's row 0 still precedes rows 1 and 2."""
    from biscuit_amd.extract import extract_slide, tile_loc
    from biscuit_amd.wsi import WSI
    path, _ = _slide_file(tmp_path)
    monkeypatch.setattr(WSI, 'READ_LIMIT', 1300)
    keep = np.zeros((5, 7), bool)
    keep[:3, :3] = True
    keep[2, 4] = keep[0, 6] = True
    w = WSI(path, stride_div=2)
    try:
        rects = [b[:4] for b in w.bands(keep=keep)]
    finally:
        w.close()
    assert rects == [(0, 3, 0, 3), (2, 3, 4, 5), (0, 1, 6, 7)]
    s = extract_slide(eng, path, str(tmp_path / 'm'), stride_div=2, batch=10, cell_mask=keep)
    got = [(r['loc_x'][0], r['loc_y'][0]) for r in records(s['tfrecord'])]
    assert got == [tuple(x) for x in tile_loc(np.flatnonzero(keep.reshape(-1)), 7, 299, 598).tolist()] and len(got) == 11


def test_device_decoded_bands_write_the_same_file(eng, tmp_path):
    from biscuit_amd.extract import extract_slide
    path = wj.slide_file(tmp_path, 0.5045)
    host = extract_slide(eng, path, str(tmp_path / 'host'), batch=16, canvas_bytes=1)
    dev = extract_slide(eng, path, str(tmp_path / 'dev'), batch=16, canvas_bytes=1, decode='gpu')
    assert dev['decode_stats']['gpu_bands'] >= 3 and dev['decode_stats']['host_bands'] == 0 and dev['decode_stats']['segments'] > 0
    assert host['decode_stats']['gpu_bands'] == 0 and host['tiles_written'] == 12
    assert open(dev['tfrecord'], 'rb').read() == open(host['tfrecord'], 'rb').read()


def _tile_table(res):
    df = res.tile_df
    mean = np.stack([df['cohort-y_pred0'].to_numpy(), df['cohort-y_pred1'].to_numpy()], 1).astype(np.float32)
    std = np.stack([df['cohort-uncertainty0'].to_numpy(), df['cohort-uncertainty1'].to_numpy()], 1).astype(np.float32)
    return mean, std


def test_evaluate_over_the_extracted_tfrecord(eng, tmp_path):
    """``evaluate()`` over an extracted TFRecord against the heatmap path, per tile, bit for bit, at the same seed.  Both index
    Philox alike for an unmasked slide (``evaluate``: the record's index; ``from_slide``: the row-major cell index, which is
    the record's), so ``Heatmap.from_slide`` is the reference -- on a slide whose tiles JPEG reproduces exactly: every cell of the
    598-pixel grid one grey level of its own (grey is exact through BT.601 both ways, a constant block is its DC alone, and at
    quality 95 the DC quantiser divides it without remainder), because ``from_slide`` sees the resampled pixels and ``evaluate``
    the decoded JPEG, which for a textured tile are different images.  The textured slide is held to the same equality against
    ``Heatmap`` over the DECODED records (grid and indices as ``from_slide``'s), read on the host and with ``gpu_decode``."""
    from biscuit_amd import inference as inf
    from biscuit_amd.extract import extract_slide
    from biscuit_amd.heatmap import Heatmap
    kw = dict(mc_n=8, seed=3, batch=16)
    a = np.empty((1800, 2400, 3), np.uint8)
    for gy in range(4):
        for gx in range(5):
            a[gy * 598:(gy + 1) * 598, gx * 598:(gx + 1) * 598] = 25 + 17 * (gy * 4 + gx) if gy < 3 and gx < 4 else 230      # (the strips no tile reaches)
    path = _two_level(tmp_path, a, 'grey.svs')
    s = extract_slide(eng, path, str(tmp_path / 'g'), batch=16)
    hm = Heatmap.from_slide(eng, path, **kw)
    res = inf.evaluate(eng, inf.slides_from_tfrecords([s['tfrecord']], {'grey': 1}), outcome='cohort', **kw)
    mean, std = _tile_table(res)
    assert mean.shape == (12, 2) and len({m.tobytes() for m in mean}) == 12 and (std[:, 0] > 0).all()
    assert np.array_equal(mean, hm.logits.reshape(12, 2)) and np.array_equal(std, hm.uncertainty.reshape(12, 2))

    path, _ = _slide_file(tmp_path)
    s = extract_slide(eng, path, str(tmp_path / 't'), batch=16)
    tiles = np.stack([tfr.decode_image(r['image_raw']) for r in records(s['tfrecord'])])
    grid = np.stack([np.arange(12) % 4, np.arange(12) // 4], 1)
    hm = Heatmap(eng, tiles, grid, grid_shape=(3, 4), **kw)
    for gpu_decode in (False, True):
        res = inf.evaluate(eng, inf.slides_from_tfrecords([s['tfrecord']], {'slide': 1}, gpu_decode=gpu_decode), outcome='cohort', **kw)
        mean, std = _tile_table(res)
        assert np.array_equal(mean, hm.logits.reshape(12, 2)) and np.array_equal(std, hm.uncertainty.reshape(12, 2)), gpu_decode


def test_command_line(eng, tmp_path):
    from biscuit_amd.extract import extract_slide
    path, _ = _slide_file(tmp_path)
    out = str(tmp_path / 'cli')
    api = extract_slide(eng, path, str(tmp_path / 'api'), stride_div=2, quality=90, subsampling='4:4:4', batch=16)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd.extract', path, '--out', out, '--stride-div', '2', '--quality', '90',
                        '--subsampling', '4:4:4', '--batch', '16'], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(os.path.join(out, 'slide.tfrecords'), 'rb').read() == open(api['tfrecord'], 'rb').read()
    s = json.load(open(os.path.join(out, 'slide.extract.json')))
    assert s['tiles_written'] == 35 and s['quality'] == 90 and s['subsampling'] == '4:4:4' and s['grid_shape'] == [5, 7]
    assert s['bytes_written'] == api['bytes_written'] and json.loads(p.stdout.strip().splitlines()[-1])['tiles_written'] == 35
