"""The training augmentation on the device (csrc/kernels_augment.hip, ``bq_augment`` through ``Engine.augment``) against the CPU
build of the same routines (``bqio_augment`` through ``augment.apply_host``) and therefore against Pillow, numpy and the integer
blur, which tests/test_augment.py holds that build to: byte for byte and status for status, in rounds, on poisoned memory, and end
to end through ``train.cache_features`` and ``train.train_head``.  ``-m gpu``."""
import numpy as np
import pytest
import torch

from biscuit_amd import augment as A
from biscuit_amd import inference as inf
from biscuit_amd import stain
from biscuit_amd import tfrecord as tfr
from biscuit_amd import train as T
from biscuit_amd.synthetic import make_tiles
from tests import _augment_ref as ref
from tests import _jpeg_encode_cases as ec
from tests import _poison as P
from tests import test_gpu_abi_homes as homes
from tests import test_gpu_poison_tools as tools

pytestmark = pytest.mark.gpu

CLASSES = {'augment_jpeg', 'augment_place', 'augment_blur_h', 'augment_blur_v'}
ST_PARAM = 2                             # augment_device.h: a parameter row out of range, seen on the device
NORM_FIT = {'target_means': [60.0, 10.0, -5.0], 'target_stds': [15.0, 8.0, 6.0]}


@pytest.fixture(scope='module')
def eng():
    e = homes._engine()
    yield e
    e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def gpu(eng, tiles, params, **kw):
    out, status = eng.augment(up(eng, tiles), params, **kw)
    return out.cpu().numpy(), status.cpu().numpy()


def _dihedral_case():
    """px 17, n = 8 twice over: all 16 (k, flips) codes with j at quality 50 and b at sigma = 2."""
    tiles = np.concatenate([ec.mixed(8, 17), ec.mixed(8, 17, seed=6)])
    params = np.array([[k, f, 50, 4] for k in range(4) for f in range(4)], np.uint8)
    return tiles, params


# ------------------------------------------------------------------------------------------------ device against host
def test_composition_table_equals_the_host(eng):
    tiles, params = ec.mixed(16, 33), ref.composition_table()
    want, want_status = A.apply_host(tiles, params)
    got, status = gpu(eng, tiles, params)
    assert np.array_equal(got, want) and np.array_equal(status, want_status) and not status.any()
    assert np.array_equal(got[3], tiles[3]) and np.array_equal(got[8], tiles[8])       # all-zero rows in the middle of the batch


def test_every_dihedral_code_with_jpeg_and_blur(eng):
    tiles, params = _dihedral_case()
    for lo in (0, 8):
        want, want_status = A.apply_host(tiles[lo:lo + 8], params[lo:lo + 8])
        got, status = gpu(eng, tiles[lo:lo + 8], params[lo:lo + 8])
        assert np.array_equal(got, want) and np.array_equal(status, want_status)


def test_tiles_of_299_one_stage_each_and_all(eng):
    tiles = np.stack([ec.tile(299, 'synthetic'), ec.tile(299, 'noise'), ec.tile(299, 'gradient'), ec.tile(299, 'synthetic')])
    params = np.array([[0, 0, 75, 0], [3, 2, 0, 0], [0, 0, 0, 4], [1, 1, 60, 2]], np.uint8)
    want, want_status = A.apply_host(tiles, params)
    got, status = gpu(eng, tiles, params)
    assert np.array_equal(got, want) and np.array_equal(status, want_status) and not status.any()
    assert np.array_equal(got[0], ec.pillow_pixels(ec.pillow(299, 'synthetic', 75, '4:2:0')))


# ------------------------------------------------------------------------------------------------ rounds
def test_rounds_do_not_change_the_result(eng):
    tiles, params = ec.mixed(16, 33), ref.composition_table()
    want, _ = A.apply_host(tiles, params)
    per_tile = eng.augment_scratch(1, 33).numel()
    assert eng.augment_scratch(16, 33).numel() == 16 * per_tile and eng.augment_scratch(300, 33).numel() == 256 * per_tile
    one, check = P.guarded(per_tile, 0xA5, eng.device)                                 # sixteen rounds of one tile
    got, status = gpu(eng, tiles, params, scratch=one)
    check()
    assert np.array_equal(got, want) and not status.any()
    got, _ = gpu(eng, tiles, params, scratch=eng.augment_scratch(16, 33))
    assert np.array_equal(got, want)
    from biscuit_amd.engine import BiscuitHipError
    with pytest.raises(BiscuitHipError, match='scratch'):
        gpu(eng, tiles, params, scratch=one[:per_tile - 1])
    # 17 px: a tile is 867 bytes, so rounds begin inside a group of four pixels; and an output that is not 4-byte aligned
    tiles, params = _dihedral_case()
    want, _ = A.apply_host(tiles, params)
    got, _ = gpu(eng, tiles, params, scratch=eng.augment_scratch(3, 17))
    assert np.array_equal(got, want)
    buf, check = P.guarded(tiles.size + 1, 0xFF, eng.device)
    out = buf[1:].view(tiles.shape)
    eng.augment(up(eng, tiles), params, out=out, scratch=eng.augment_scratch(5, 17))
    check()
    assert np.array_equal(out.cpu().numpy(), want) and int(buf[0]) == 0xFF


# ------------------------------------------------------------------------------------------------ poison
def test_no_result_depends_on_stale_bytes(eng):
    tiles, params = ec.mixed(16, 33), ref.composition_table()
    want, want_status = A.apply_host(tiles, params)
    d = up(eng, tiles)
    got, status = tools.under_every_fill(eng, lambda: tools.host(*eng.augment(d, params)))
    assert np.array_equal(got, want) and np.array_equal(status, want_status)
    assert np.array_equal(got[3], tiles[3]) and np.array_equal(got[8], tiles[8])
    per_tile = eng.augment_scratch(1, 33).numel()
    for fill in P.BYTE_FILLS:                                                          # a caller's own scratch and output, guarded
        scratch, check_s = P.guarded(2 * per_tile, fill, eng.device)
        out, check_o = P.guarded(tiles.size, fill, eng.device)
        st, check_t = P.guarded(4 * len(tiles), fill, eng.device)
        eng.augment(d, params, out=out.view(tiles.shape), status=st.view(torch.int32), scratch=scratch)
        torch.cuda.synchronize(eng.device)
        check_s(); check_o(); check_t()
        assert np.array_equal(out.view(tiles.shape).cpu().numpy(), want) and not st.view(torch.int32).any()


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments(eng):
    tiles = up(eng, ec.mixed(3, 17))
    bad = np.array([[0, 0, 0, 0], [1, 0, 101, 0], [2, 1, 0, 0]], np.uint8)
    with pytest.raises(ValueError, match='parameter'):
        eng.augment(tiles, bad)
    out, status = eng.augment(tiles, up(eng, bad))         # on the device the row cannot be read: status 2, the tile unchanged
    assert status.cpu().tolist() == [0, ST_PARAM, 0] and torch.equal(out[1], tiles[1]) and torch.equal(out[0], tiles[0])
    assert np.array_equal(out[2].cpu().numpy(), ref.dihedral(tiles[2].cpu().numpy(), 2, 1))
    with pytest.raises(ValueError, match='px'):
        eng.augment(torch.zeros((1, 7, 7, 3), dtype=torch.uint8, device=eng.device), np.zeros((1, 4), np.uint8))
    from biscuit_amd.engine import BiscuitHipError
    with pytest.raises(BiscuitHipError, match='overlaps'):
        eng.augment(tiles, np.zeros((3, 4), np.uint8), out=tiles)


def test_profiling_classes_are_exactly_the_new_ones():
    eng = homes._engine()
    try:
        eng.profile_enable(True)
        out, status = eng.augment(torch.empty((0, 33, 33, 3), dtype=torch.uint8, device=eng.device), np.zeros((0, 4), np.uint8))
        assert tuple(out.shape) == (0, 33, 33, 3) and not eng.profile_read()           # n = 0: nothing was launched
        eng.augment(up(eng, ec.mixed(16, 33)), ref.composition_table())
        prof = eng.profile_read()
        assert {p.name for p in prof} == CLASSES and all(p.launches >= 1 for p in prof)
    finally:
        eng.close()


def test_close_lets_go_of_every_device_tensor():
    eng = homes._engine()
    eng.augment(up(eng, ec.mixed(2, 17)), np.array([[1, 2, 70, 3], [0, 0, 0, 0]], np.uint8))
    assert 'augment' in {family for family, v in eng._tool_ws.items() if homes._device_tensors(v)}
    eng.close()
    assert {k: v for k, v in vars(eng).items() if homes._device_tensors(v)} == {}
    eng.close()
    assert eng._ctx is None and {k: v for k, v in vars(eng).items() if homes._device_tensors(v)} == {}


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def cohort(tmp_path_factory):
    """4 slides x 6 tiles of 299 px -> (paths, labels, all tiles in cohort order)."""
    d = tmp_path_factory.mktemp('augment')
    paths, tiles = [], []
    for i, name in enumerate('abcd'):
        t = make_tiles(6, seed=80 + i, slide_bias=[(i % 2) * 40.0 - 20.0, 0.0, 0.0])
        loc = np.stack([np.arange(6) * 299 + 150, np.full(6, 150 + 1000 * i)], 1).astype(np.int64)
        paths.append(str(d / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
        tiles.append(t)
    return paths, {'a': 0, 'b': 1, 'c': 0, 'd': 1}, np.concatenate(tiles)


@pytest.fixture(scope='module')
def caches(eng, cohort):
    paths, labels, _ = cohort
    slides = lambda: inf.slides_from_tfrecords(paths, labels)
    plain = T.cache_features(eng, slides(), norm_fit=NORM_FIT)
    views = T.cache_features(eng, slides(), norm_fit=NORM_FIT, augment='xyrjb', views=2, seed=3)
    return plain, views


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_cached_views_are_the_host_augmented_tiles_features(eng, cohort, caches):
    paths, labels, tiles = cohort
    plain, views = caches
    assert eng.max_batch == 8                              # batches cross slides (6 tiles each)
    assert plain.views is None and tuple(views.views.shape) == (2, 24, 2048) and views.views.is_cuda
    assert (views.augment, views.augment_seed, views.n_views()) == ('xyrjb', 3, 2)
    assert np.array_equal(_bits(views.feats), _bits(plain.feats))                      # feats: bit for bit the unaugmented ones
    for v in range(2):
        params = A.draw(24, 'xyrjb', 3, v)
        host, status = A.apply_host(tiles, params)
        assert not status.any()
        want = torch.cat([eng.backbone_u8(stain.normalise(eng, up(eng, host[a:a + 8]), 'reinhard_fast', NORM_FIT)) for a in range(0, 24, 8)])
        assert np.array_equal(_bits(views.views[v]), _bits(want)), v
    assert (A.draw(24, 'xyrjb', 3, 0)[:, 2] > 0).any() and not np.array_equal(_bits(views.views[0]), _bits(views.views[1]))
    five = T.cache_features(eng, inf.slides_from_tfrecords(paths, labels), norm_fit=NORM_FIT, augment='xyrjb', views=2, seed=3, batch=5)
    assert np.array_equal(_bits(five.views), _bits(views.views)) and np.array_equal(_bits(five.feats), _bits(views.feats))


def test_training_reads_the_views_and_prediction_does_not(eng, cohort, caches):
    _, labels, _ = cohort
    plain, views = caches
    rows = np.arange(24)
    y = np.array([labels[views.slides[i]] for i in views.slide_idx])
    params = T.TrainParams(batch_size=8, epochs=[2], augment='xyrjb')
    first, losses = T.train_head(eng, views, rows, y, params=params, seed=5)
    again, losses2 = T.train_head(eng, views, rows, y, params=params, seed=5)
    without, _ = T.train_head(eng, plain, rows, y, params=params, seed=5)
    assert len(losses) == 6 and np.array_equal(losses.view(np.uint32), losses2.view(np.uint32))
    for name, _ in T.HEAD_TENSORS:
        assert np.array_equal(first[name].view(np.uint32), again[name].view(np.uint32)), name
    assert any(not np.array_equal(first[name], without[name]) for name, _ in T.HEAD_TENSORS)
    a = T.predict(eng, views, rows, None, mc_n=2, seed=3, y_true=labels)
    b = T.predict(eng, plain, rows, None, mc_n=2, seed=3, y_true=labels)
    assert a.equals(b)


def test_cache_file_round_trips_with_its_views(eng, cohort, caches, tmp_path):
    paths, labels, _ = cohort
    _, views = caches
    slides = lambda: inf.slides_from_tfrecords(paths, labels)
    path = str(tmp_path / 'cache.npz')
    kw = dict(norm_fit=NORM_FIT, augment='xyrjb', views=2, seed=3)
    made = T.cached_features(eng, slides(), path, **kw)
    back = T.cached_features(eng, slides(), path, **kw)                                # the second call reads the file
    for c in (made, back):
        assert c.views.is_cuda and np.array_equal(_bits(c.views), _bits(views.views)) and np.array_equal(_bits(c.feats), _bits(views.feats))
        assert (c.augment, c.augment_seed, c.slides) == ('xyrjb', 3, views.slides)
    for other in (dict(kw, seed=4), dict(kw, views=1), dict(kw, augment='xy'), dict(norm_fit=NORM_FIT)):
        with pytest.raises(SystemExit, match='--cache'):
            T.cached_features(eng, slides(), path, **other)
    with pytest.raises(SystemExit, match='other slides'):
        T.cached_features(eng, inf.slides_from_tfrecords(paths[:3], labels), path, **kw)
