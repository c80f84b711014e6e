"""The device JPEG decoder (csrc/kernels_jpeg.hip, ``bq_jpeg_decode``) against Pillow (libjpeg-turbo) byte for byte, against the
CPU build of the same routines (``bqio_jpeg_decode_extracted``) status for status, and through ``evaluate(gpu_decode=True)``
against the host-decoded run bit for bit: ``-m gpu``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from biscuit_amd.synthetic import make_tiles
from biscuit_amd.weights import synthetic_weights
from tests import _jpeg_cases as jc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    return Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)


def gpu(eng, scan, desc, tables, px, scratch=None):
    tiles, status = eng.jpeg_decode(torch.from_numpy(scan).cuda(), torch.from_numpy(desc.view(np.int32)).cuda(),
                                    torch.from_numpy(tables).cuda(), px, scratch=scratch)
    return tiles.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('px', jc.SIZES)
def test_same_bytes_as_libjpeg_tile_by_tile_and_packed(eng, px, tmp_path):
    """The matrix of tests/test_jpeg.py: every encoding in a call of its own, then all of one size in ONE call -- the lanes of a
    wave hold different table sets, samplings and lengths.  Every status 0, Pillow's bytes."""
    cases = jc.matrix(px)
    assert len(cases) >= 40
    raws = [r for r, _ in cases]
    want = [jc.pillow(r) for r in raws]
    path = str(tmp_path / 'm.tfrecords')
    tfr.write_slide(path, 'm', raws, np.zeros((len(raws), 2), np.int64))
    for i, (_, what) in enumerate(cases):
        got, status = gpu(eng, *jc.extract(path, i, 1, px), px)
        assert status[0] == 0 and np.array_equal(got[0], want[i]), (px, what)
    scan, desc, tables = jc.extract(path, 0, len(raws), px)
    assert tables.shape[0] >= 8 and len(set(desc[:, 2].tolist())) == 3
    got, status = gpu(eng, scan, desc, tables, px)
    assert not status.any(), status
    for i, (_, what) in enumerate(cases):
        assert np.array_equal(got[i], want[i]), (px, what)
    # the same call in rounds of 7 tiles (a scratch that holds no more): the rounds' edges fall inside 4-pixel store groups
    few = jc.extract(path, 0, 7, px)
    small = torch.empty(int(tn.lib().bqio_jpeg_coef_bytes(px)) * 7, dtype=torch.uint8, device='cuda')
    assert small.numel() == eng.jpeg_scratch(7, px).numel()
    got7, status7 = gpu(eng, *few, px, scratch=small)
    assert np.array_equal(got7, got[:7]) and not status7.any()


def test_saturated_colours(eng, tmp_path):
    raws = jc.saturated()
    for (scan, desc, tables), raw in zip(jc.extract_each(tmp_path, raws, 299, 'sat'), raws):
        got, status = gpu(eng, scan, desc, tables, 299)
        assert status[0] == 0 and np.array_equal(got[0], jc.pillow(raw))


def test_damaged_streams_get_the_cpu_builds_verdict(tmp_path):
    """300 of the byte-flipped files of tests/test_jpeg.py (fixed seed).  Order: the extractor and the CPU build of the decoder's
    routines process every stream first -- in bounds, terminating, with a verdict --; only then the same packed streams go to the
    GPU, once, in a child process under a time limit.  Statuses and bytes must be the CPU build's."""
    files = jc.byte_flipped(300)
    parts = [r for r in jc.extract_each(tmp_path, files, 299, 'flipped') if not isinstance(r, Exception)]
    assert len(parts) >= 100
    scan, desc, tables = jc.pack(parts)
    want, want_status = tn.jpeg_decode_extracted(scan, desc, tables, 299)
    assert (want_status == 0).sum() >= 50 and (want_status != 0).sum() >= 20          # both kinds are in the set
    src, dst = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(src, scan=scan, desc=desc, tables=tables, px=299)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_jpeg_gpu_worker.py'), src, dst], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(dst)
    assert np.array_equal(got['status'], want_status)
    assert np.array_equal(got['tiles'], want)


def _cohort(tmp_path):
    from biscuit_amd.synthetic import make_slides
    tiles, sidx, y = make_slides(4, 19, seed=31)
    paths, labels = [], {}

    def add(name, records, label):
        p = str(tmp_path / f'{name}.tfrecords')
        tfr.write_slide(p, name, records)
        paths.append(p); labels[name] = int(label)
    add('png0', tiles[sidx == 0], y[0])
    add('jpg444', [jc.enc(t, quality=95, subsampling=0) for t in tiles[sidx == 1]], y[1])
    add('empty', [], 0)
    add('jpg420', [jc.enc(t, quality=80, subsampling=2, optimize=True) for t in tiles[sidx == 2]], y[2])
    prog = [jc.enc(t, quality=90) for t in tiles[sidx == 3][:5]]
    prog[3] = jc.enc(tiles[sidx == 3][3], quality=90, progressive=True)
    add('prog', prog, y[3])
    add('png1', tiles[sidx == 3][5:12], 1)
    return paths, labels


@pytest.mark.parametrize('pooled', [False, True], ids=['one_engine', 'pool_with_decode_cus'])
def test_evaluate_from_jpeg_chunks_equals_the_host_decoded_run(tmp_path, pooled, monkeypatch):
    """``evaluate`` with ``gpu_decode=True`` over PNG slides, JPEG slides at two samplings, an empty slide and a slide with a
    progressive record (which stays on the host): the slide table, the per-tile mean / std and the bytes of
    tile_predictions_eval.csv are those of the host-decoded run.  Small chunks: several in flight, slides span chunks, PNG and
    JPEG chunks alternate."""
    from biscuit_amd import feed, inference as inf
    from biscuit_amd.engine import Engine, EnginePool
    monkeypatch.setattr(feed, 'CHUNK_TILES_Z', 8)
    monkeypatch.setattr(feed, 'RAMP_CHUNKS_Z', (3, 5))
    calls, read_jpeg = [], feed.TFRecordSource.read_jpeg

    def counted(self, *a):
        calls.append(os.path.basename(self.path))
        return read_jpeg(self, *a)
    monkeypatch.setattr(feed.TFRecordSource, 'read_jpeg', counted)
    paths, labels = _cohort(tmp_path)
    srcs = [s.source for s in inf.slides_from_tfrecords(paths, labels, gpu_decode=True)]
    assert [s.z_ok() for s in srcs] == [True, False, False, False, False, True]
    assert [s.jpeg_ok() for s in srcs] == [False, True, False, True, False, False]
    for s in srcs:
        s.close()
    w = synthetic_weights(1)
    if pooled:
        e = EnginePool(w, n_streams=2, reserve_cus=16, dtype='f16', max_batch=16, max_mc=5)
        assert len(e.decode_streams) == 2
    else:
        e = Engine(w, dtype='f16', max_batch=16, max_mc=5)
    da, dr = str(tmp_path / 'dev'), str(tmp_path / 'host')
    os.makedirs(da); os.makedirs(dr)
    a = inf.evaluate(e, inf.slides_from_tfrecords(paths, labels, gpu_decode=True), outcome='cohort', mc_n=5, seed=3, batch=16, save_dir=da)
    ref = inf.evaluate(e, inf.slides_from_tfrecords(paths, labels), outcome='cohort', mc_n=5, seed=3, batch=16, save_dir=dr)
    assert calls.count('jpg444.tfrecords') > 1 and calls.count('jpg420.tfrecords') > 1      # the run really was cut up: 19 tiles, several reads
    assert list(a.slide_count) == [19, 19, 0, 19, 5, 7]
    for col in ('cohort-y_pred0', 'cohort-y_pred1', 'cohort-uncertainty0', 'cohort-uncertainty1'):
        assert np.array_equal(a.tile_df[col].to_numpy(), ref.tile_df[col].to_numpy()), col
    for f in ('slide_pred', 'slide_unc', 'slide_count'):
        assert np.array_equal(getattr(a, f), getattr(ref, f), equal_nan=True), f
    assert open(a.table_path, 'rb').read() == open(ref.table_path, 'rb').read() and a.table_rows == 69
    if pooled:
        e.close()


def test_a_damaged_scan_fails_the_run_naming_slide_and_tile(tmp_path):
    """One JPEG tile whose scan the markers do not give away (the extractor takes it) but the entropy decoder refuses -- found on
    the CPU build first --: the run stops with an IOError that names the slide and the tile, never a silently wrong tile."""
    from biscuit_amd import inference as inf
    from biscuit_amd.engine import Engine
    raws = [jc.enc(t, quality=90) for t in make_tiles(6, seed=5)]
    sos = raws[4].index(b'\xff\xda')
    bad = None
    for k in range(64):                                  # the first edit of this family the CPU build refuses with a status
        b = bytearray(raws[4])
        b[sos + 3000 + k] = (b[sos + 3000 + k] ^ 0x5a) & 0x7f
        res = jc.extract_each(tmp_path, [bytes(b)], 299, f'try{k}')[0]
        if not isinstance(res, Exception) and tn.jpeg_decode_extracted(*res)[1][0] != 0:
            bad = bytes(b)
            break
    assert bad is not None
    raws[4] = bad
    path = str(tmp_path / 'd.tfrecords')
    tfr.write_slide(path, 'd', raws)
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    with pytest.raises(IOError, match=r'device JPEG decoder refused 1 tile\(s\) \(first: d, tile 4, status'):
        inf.evaluate(e, inf.slides_from_tfrecords([path], {'d': 1}, gpu_decode=True), outcome='cohort', mc_n=2, seed=3, batch=8)
