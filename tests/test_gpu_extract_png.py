"""Tile extraction to PNG records (``extract_slide(img_format='png')``: bands -> ``bq_tile_resample`` -> ``bq_png_encode`` ->
TFRecord) on the textured two-level test slide: the records decode to the resampled tiles bit for bit, so ``evaluate()`` over the
file equals ``Heatmap.from_slide`` exactly -- the equality the JPEG path (tests/test_gpu_extract.py) can only show on a flat slide.
``-m gpu``."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from biscuit_amd import tfrecord as tfr
from tests import _png_encode_cases as pc
from tests.test_wsi import _slide_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    return Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)


@pytest.fixture(scope='module')
def extracted(eng, tmp_path_factory):
    """The 5 x 7 grid (stride_div = 2) of the textured slide, extracted once as PNG: (slide path, summary, the batches the encoder
    was handed -- what ``Engine.tile_resample`` produced)."""
    from biscuit_amd.extract import extract_slide
    tmp = tmp_path_factory.mktemp('png')
    path, _ = _slide_file(tmp)
    seen, encode = [], eng.png_encode

    def spy(tiles, *a, **kw):
        seen.append(tiles.cpu().numpy().copy())
        return encode(tiles, *a, **kw)
    eng.png_encode = spy
    try:
        summary = extract_slide(eng, path, str(tmp / 'api'), stride_div=2, batch=16, img_format='png')
    finally:
        del eng.png_encode
    return path, summary, np.concatenate(seen)


def records(path):
    return [tfr.parse_example(r) for r in tfr.read_records(path, verify='full')]


def test_records_are_the_resampled_tiles_in_row_major_order(eng, extracted):
    from biscuit_amd.wsi import WSI
    path, s, batch = extracted
    assert s['grid_shape'] == [5, 7] and s['tiles_written'] == 35 and batch.shape == (35, 299, 299, 3)
    assert (s['img_format'], s['quality'], s['subsampling']) == ('png', None, None)
    assert json.load(open(s['tfrecord'][:-len('.tfrecords')] + '.extract.json')) == json.loads(json.dumps(s))
    recs = records(s['tfrecord'])
    assert len(recs) == 35 and s['bytes_written'] == os.path.getsize(s['tfrecord'])
    w = WSI(path, stride_div=2)
    try:
        for i, r in enumerate(recs):
            gy, gx = divmod(i, 7)
            assert r['slide'] == b'slide' and (r['loc_x'], r['loc_y']) == ([gx * 299 + 299], [gy * 299 + 299]), i
            pc.check_container(r['image_raw'], 299)
            got = tfr.decode_image(r['image_raw'])
            assert np.array_equal(got, batch[i]), i                  # one band, no mask: the batches are the cells in order
            assert np.array_equal(got, w._tile(gx, gy)), (gx, gy)
    finally:
        w.close()


def _tile_table(res):
    df = res.tile_df
    mean = np.stack([df['cohort-y_pred0'].to_numpy(), df['cohort-y_pred1'].to_numpy()], 1).astype(np.float32)
    std = np.stack([df['cohort-uncertainty0'].to_numpy(), df['cohort-uncertainty1'].to_numpy()], 1).astype(np.float32)
    return mean, std


def test_evaluate_equals_from_slide_on_the_textured_slide(eng, extracted):
    """Both index Philox by the row-major cell (an unmasked slide), both see the same pixels: equal per tile, bit for bit, with
    the records read on the host and with ``gpu_decode``."""
    from biscuit_amd import inference as inf
    from biscuit_amd.heatmap import Heatmap
    path, s, _ = extracted
    kw = dict(mc_n=8, seed=3, batch=16)
    hm = Heatmap.from_slide(eng, path, stride_div=2, **kw)
    assert len({m.tobytes() for m in hm.logits.reshape(35, 2)}) == 35
    for gpu_decode in (False, True):
        res = inf.evaluate(eng, inf.slides_from_tfrecords([s['tfrecord']], {'slide': 1}, gpu_decode=gpu_decode), outcome='cohort', **kw)
        mean, std = _tile_table(res)
        assert np.array_equal(mean, hm.logits.reshape(35, 2)) and np.array_equal(std, hm.uncertainty.reshape(35, 2)), gpu_decode


def test_command_line_writes_the_same_file(extracted, tmp_path):
    path, api, _ = extracted
    out = str(tmp_path / 'cli')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd.extract', path, '--out', out, '--stride-div', '2', '--img-format', 'png',
                        '--batch', '16'], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(os.path.join(out, 'slide.tfrecords'), 'rb').read() == open(api['tfrecord'], 'rb').read()
    s = json.load(open(os.path.join(out, 'slide.extract.json')))
    assert (s['tiles_written'], s['img_format'], s['quality'], s['subsampling']) == (35, 'png', None, None)


def test_jpeg_settings_with_png_are_refused_and_jpg_stays_the_default(eng, extracted, tmp_path, capsys):
    from biscuit_amd import extract
    path = extracted[0]
    for extra in (['--quality', '90'], ['--subsampling', '4:4:4']):
        with pytest.raises(SystemExit) as e:
            extract.main([path, '--out', str(tmp_path / 'no'), '--img-format', 'png'] + extra)
        assert e.value.code == 2 and 'jpg only' in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / 'no'))
    with pytest.raises(ValueError, match='img_format'):
        extract.extract_slide(eng, str(tmp_path / 'missing.svs'), str(tmp_path / 'no'), img_format='jpeg')      # before the slide is opened
    assert inspect.signature(extract.extract_slide).parameters['img_format'].default == 'jpg'
    s = extract.extract_slide(eng, path, str(tmp_path / 'jpg'), stride_div=2, batch=16)
    assert (s['img_format'], s['quality'], s['subsampling']) == ('jpg', 95, '4:2:0')
    assert all(r['image_raw'][:2] == b'\xff\xd8' for r in records(s['tfrecord']))
