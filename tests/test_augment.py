"""The training augmentation's definition (csrc/augment_device.h) on the CPU (``bqio_augment`` through ``augment.apply_host``)
against tests/_augment_ref.py: Pillow's round-trip pixels for ``j``, numpy for ``r``, ``x``, ``y``, the integer statement and scipy
for ``b``, byte for byte; then ``augment.draw``, the errors, and the rows ``train_head`` reads from a cache with views.  The GPU
kernels are compiled from the same header and held to this build in tests/test_gpu_augment.py."""
import numpy as np
import pytest

from biscuit_amd import augment as A
from biscuit_amd import tfrecord_native as tn
from tests import _augment_ref as ref
from tests import _jpeg_encode_cases as ec

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


def _rows(n, k=0, flips=0, quality=0, blur=0):
    return np.tile(np.array([[k, flips, quality, blur]], np.uint8), (n, 1))


def _stack(px):
    return np.stack([ec.tile(px, what) for what in ec.CONTENTS])


@pytest.mark.parametrize('px', [8, 15, 16, 17, 33])
def test_jpeg_is_pillows_round_trip(px):
    """8: dummy blocks; 15: odd chroma width; 16: one MCU; 17: a dummy row and column; 33: odd chroma width 17."""
    tiles = _stack(px)
    for q in (1, 25, 50, 75, 95, 100):
        got, status = A.apply_host(tiles, _rows(len(tiles), quality=q))
        assert not status.any(), (px, q, status)
        for i, what in enumerate(ec.CONTENTS):
            assert np.array_equal(got[i], ec.pillow_pixels(ec.pillow(px, what, q, '4:2:0'))), (px, what, q)


@pytest.mark.parametrize('q', [50, 75, 100])
def test_jpeg_is_pillows_round_trip_at_299(q):
    tiles = _stack(299)
    got, status = A.apply_host(tiles, _rows(len(tiles), quality=q))
    assert not status.any()
    for i, what in enumerate(ec.CONTENTS):
        assert np.array_equal(got[i], ec.pillow_pixels(ec.pillow(299, what, q, '4:2:0'))), (what, q)


def test_turns_and_flips_are_numpys():
    tile = ec.tile(17, 'noise')
    codes = [(k, f) for k in range(4) for f in range(4)]
    params = np.array([[k, f, 0, 0] for k, f in codes], np.uint8)
    got, status = A.apply_host(np.stack([tile] * 16), params)
    assert not status.any()
    for i, (k, f) in enumerate(codes):
        assert np.array_equal(got[i], ref.dihedral(tile, k, f)), (k, f)
    assert got[0].tobytes() == tile.tobytes()             # the all-zero row returns the input bytes
    assert len({g.tobytes() for g in got}) == 8            # the dihedral group of a tile without symmetry, each element twice


def test_blur_weights_sum_to_65536():
    assert A.blur_weights(1).tolist() == [17, 6976, 51550, 6976, 17]
    for b, r in zip((1, 2, 3, 4), (2, 3, 5, 6)):
        w = A.blur_weights(b)
        assert len(w) == 2 * r + 1 and int(w.sum()) == 65536 and np.array_equal(w, w[::-1]) and np.array_equal(w, ref.weights(b))


@pytest.mark.parametrize('px', [8, 17, 33])
def test_blur_is_the_integer_statement(px):
    tiles = _stack(px)
    for b in (1, 2, 3, 4):
        got, status = A.apply_host(tiles, _rows(len(tiles), blur=b))
        assert not status.any()
        for i, what in enumerate(ec.CONTENTS):
            assert np.array_equal(got[i], ref.blur_int(tiles[i], b)), (px, what, b)


@pytest.mark.parametrize('px', [8, 17, 33, 299])
def test_blur_is_within_one_level_of_scipy(px):
    """Against numpy.rint of the float64 filter: no sample more than one level away, at most 2 % of a tile's samples differing
    (0.92 % at worst when the definition was written)."""
    tiles = _stack(px)
    worst = 0.0
    for b in (1, 2, 3, 4):
        got, _ = A.apply_host(tiles, _rows(len(tiles), blur=b))
        for i, what in enumerate(ec.CONTENTS):
            d = np.abs(got[i].astype(np.int16) - ref.blur_scipy(tiles[i], b))
            share = float((d != 0).mean())
            worst = max(worst, share)
            assert d.max() <= 1 and share <= 0.02, (px, what, b, int(d.max()), share)
    print(f'px {px}: at most {100 * worst:.2f} % of a tile\'s samples differ from rounded scipy')


def test_composition_equals_the_oracles():
    tiles, params = ec.mixed(16, 33), ref.composition_table()
    assert ((params != 0).sum(0) >= 1).all() and (params[5] != 0).all() and not params[3].any()
    got, status = A.apply_host(tiles, params)
    assert not status.any()
    want = ref.compose(tiles, params)
    for i in range(16):
        assert np.array_equal(got[i], want[i]), (i, params[i])
    assert got[3].tobytes() == tiles[3].tobytes() and got[8].tobytes() == tiles[8].tobytes()
    one, _ = A.apply_host(tiles, params, threads=1)        # the result does not depend on the threads
    assert np.array_equal(one, got)


def test_draw():
    a = A.draw(1000, 'xyrjb', 7, 2)
    assert a.dtype == np.uint8 and a.shape == (1000, 4)
    assert np.array_equal(a, A.draw(1000, 'bjryx', 7, 2))                              # fixed for fixed (seed, view); order-free
    assert not np.array_equal(a, A.draw(1000, 'xyrjb', 7, 3)) and not np.array_equal(a, A.draw(1000, 'xyrjb', 8, 2))
    assert np.array_equal(A.draw(20000, 'xyrjb', 7, 2)[:1000], a)                      # row i does not depend on n
    assert np.array_equal(A.draw(1000, 'xj', 7, 2)[:, 2], a[:, 2])                     # nor on the other letters
    xj = A.draw(1000, 'xj', 7, 2)
    assert not xj[:, 0].any() and not xj[:, 3].any() and (xj[:, 1] <= 1).all() and np.array_equal(xj[:, 1], a[:, 1] & 1)
    assert not A.draw(50, '', 7, 2).any() and not A.draw(50, None, 7, 2).any() and A.draw(0, 'xyrjb', 1, 0).shape == (0, 4)
    big = A.draw(20000, 'xyrjb', 11, 0)
    j, b = big[:, 2] > 0, big[:, 3] > 0
    assert abs(j.mean() - 0.5) <= 0.02 and abs(b.mean() - 0.1) <= 0.02
    assert sorted(set(big[j, 2].tolist())) == list(range(50, 101))                     # qualities span exactly 50..100
    assert set(big[b, 3].tolist()) == {1, 2, 3, 4} and set(big[:, 0].tolist()) == {0, 1, 2, 3} and set(big[:, 1].tolist()) == {0, 1, 2, 3}
    shares = np.bincount(big[b, 3], minlength=5)[1:] / b.sum()
    assert np.abs(shares - (0.5, 0.25, 0.125, 0.125)).max() <= 0.04
    A.check_params(big)


def test_errors():
    assert A.parse('bjryx') == 'xyrjb' and A.parse('') == '' and A.parse(None) == '' and A.parse('jj') == 'j'
    with pytest.raises(ValueError, match='unknown letter'):
        A.parse('xz')
    with pytest.raises(ValueError):
        A.draw(4, 'n', 0, 0)
    tile = np.zeros((1, 8, 8, 3), np.uint8)
    for bad in ([4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 101, 0], [0, 0, 0, 5]):
        with pytest.raises(ValueError, match='parameter'):
            A.apply_host(tile, np.array([bad], np.uint8))
        with pytest.raises(ValueError):
            A.check_params(np.array([bad], np.uint8))
    with pytest.raises(ValueError, match='8 <= px'):
        A.apply_host(np.zeros((1, 7, 7, 3), np.uint8), np.zeros((1, 4), np.uint8))
    out, status = np.zeros_like(tile), np.zeros(1, np.int32)
    prm = np.zeros((1, 4), np.uint8)
    assert tn.lib().bqio_augment(tile.ctypes.data, 1, 8, prm.ctypes.data, tile.ctypes.data, status.ctypes.data, 1) == -1
    assert b'overlaps' in tn.lib().bqio_augment_last_error()
    assert tn.lib().bqio_augment(None, 1, 8, prm.ctypes.data, out.ctypes.data, status.ctypes.data, 1) == -1
    assert tn.lib().bqio_augment(None, 0, 8, None, None, None, 1) == 0                 # n = 0 touches nothing
    with pytest.raises(ValueError):
        A.blur_weights(5)
    got, status = A.apply_host(np.zeros((0, 8, 8, 3), np.uint8), np.zeros((0, 4), np.uint8))
    assert got.shape == (0, 8, 8, 3) and status.shape == (0,)


def test_train_head_reads_view_e_mod_v():
    """The row arithmetic only: a host-made cache with V = 2 views and a stub in place of ``Engine.head_train_steps``."""
    import torch
    from biscuit_amd import train as T

    class Stub:
        device = torch.device('cpu')
        weights = T.glorot_head(0)

        def __init__(self):
            self.calls = []

        def head_train_steps(self, w, m, v, feats, rows, labels, batch, step, seed, lr, **kw):
            self.calls.append((feats, rows.numpy().copy(), labels.numpy().copy(), step))
            return torch.zeros(len(lr))

    N, V = 10, 2
    feats = np.zeros((N, 2048), np.float32)
    views = np.arange(V * N * 2048, dtype=np.float32).reshape(V, N, 2048)
    rows, labels = np.array([1, 4, 5, 8, 9]), np.array([0, 1, 1, 0, 1])
    params = T.TrainParams(batch_size=2, epochs=[3], augment='xyrjb')
    cache = T.FeatureCache(feats, np.zeros(N, np.int64), np.zeros((N, 2), np.int64), ['s'], views, 'xyrjb', 0)
    eng = Stub()
    T.train_head(eng, cache, rows, labels, init='model', params=params, seed=5)
    assert len(eng.calls) == 3
    for e, (f, r, y, step) in enumerate(eng.calls):
        order = np.random.default_rng([5, e]).permutation(len(rows))
        assert f.shape == (V * N, 2048) and np.array_equal(np.asarray(f), views.reshape(V * N, 2048))
        assert np.array_equal(r, rows[order] + (e % V) * N) and np.array_equal(y, labels[order]) and step == 3 * e
        assert np.array_equal(np.asarray(f)[r], views[e % V][rows[order]])
    plain = Stub()
    T.train_head(plain, T.FeatureCache(feats, cache.slide_idx, cache.loc, ['s']), rows, labels, init='model', params=params, seed=5)
    for e, (f, r, y, step) in enumerate(plain.calls):                                  # without views nothing changes
        assert f is feats and np.array_equal(r, rows[np.random.default_rng([5, e]).permutation(len(rows))])
    with pytest.raises(ValueError):
        T.TrainParams(augment='q').validate()


def test_cache_file_carries_views(tmp_path):
    from biscuit_amd import train as T
    base = dict(feats=np.ones((3, 2048), np.float32), slide_idx=np.zeros(3, np.int64), loc=np.zeros((3, 2), np.int64), slides=['s'])
    plain = T.FeatureCache(**base)
    plain.save(tmp_path / 'plain.npz')
    back = T.FeatureCache.load(tmp_path / 'plain.npz')
    assert back.views is None and back.n_views() == 0 and back.augment == '' and np.array_equal(back.feats, base['feats'])
    views = np.arange(2 * 3 * 2048, dtype=np.float32).reshape(2, 3, 2048)
    T.FeatureCache(**base, views=views, augment='xj', augment_seed=9).save(tmp_path / 'views.npz')
    back = T.FeatureCache.load(tmp_path / 'views.npz')
    assert np.array_equal(back.views, views) and back.n_views() == 2 and (back.augment, back.augment_seed) == ('xj', 9)


def test_command_line_refuses_a_bad_augmentation(tmp_path):
    from biscuit_amd import train as T
    base = ['a.tfrecords', '--labels', 'l.csv', '--model', str(tmp_path), '--out', str(tmp_path / 'out')]
    with pytest.raises(SystemExit, match='--augment'):
        T.main(base + ['--augment', 'xz'])
    with pytest.raises(SystemExit, match='--views'):
        T.main(base + ['--augment', 'xyrjb', '--views', '0'])
    assert not (tmp_path / 'out').exists()
