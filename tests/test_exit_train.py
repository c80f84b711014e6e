"""Exit-flow fine-tuning without a GPU (DESIGN.md section 7 "Exit-flow fine-tuning"): the float64 restatement against central
differences, its float32 twin on the GPU cases, and the host side of ``biscuit_amd.train`` -- the exit vector, ``--trainable``, the
memory guard, the activation cache's file."""
import numpy as np
import pytest

from biscuit_amd import train as T
from tests import _exit_train_ref as X
from tests import _train_ref as R


# ------------------------------------------------------------------------------------------------ 1. the yardstick itself
def _toy(seed=4, H=4, W=4, C=(8, 12, 16), head=(16, 12, 8), n=3):
    """Block 14 at H = W = 4 and 8 / 12 / 16 channels in front of a head 16 -> 12 -> 8 -> 2, float64; a dead channel in each layer."""
    rng = np.random.default_rng(seed)
    e = {}
    for l, (cin, cout) in (('1', C[:2]), ('2', C[1:])):
        e['D' + l] = rng.normal(0, 1 / 3.0, (3, 3, cin))
        e['P' + l] = rng.normal(0, np.sqrt(2.0 / cin), (cin, cout))
        e['gamma' + l] = rng.uniform(0.5, 1.5, cout)
        e['beta' + l] = rng.normal(0.3, 0.3, cout)
        e['mean' + l] = rng.normal(0, 0.3, cout)
        e['var' + l] = np.exp(rng.uniform(np.log(0.25), np.log(4.0), cout))
        e['beta' + l][-1] = -50.0
    w = {}
    for name, (cin, cout) in zip(R.HEAD, ((head[0], head[1]), (head[1], head[2]), (head[2], 2))):
        w[name + '/kernel'] = rng.normal(0, np.sqrt(2.0 / cin), (cin, cout))
        w[name + '/bias'] = rng.normal(0, 0.1, cout)
    x = np.abs(rng.standard_normal((n, H, W, C[0])))
    x[1, 0, 0] = 0
    return x, e, w, head


def test_float64_gradients_match_central_differences():
    """20 random elements of each of the fourteen tensors (fewer where a tensor has fewer) at rate 0.1 with fixed masks, n = 3, h =
    1e-6: the central difference of the float64 loss agrees with the float64 gradient within 1e-6 of the tensor's largest gradient
    entry -- ``_train_ref``'s rule and figures.  D1 and D2 also at their four corner taps, where a wrong padding rule would show."""
    rng = np.random.default_rng(8)
    x, e, w, head = _toy()
    labels = np.array([0, 1, 1])
    keeps = X.keep_masks(R.SEED, np.array([3, 7, 11]), 2, 0.1, head)
    loss, g, _ = X.loss_and_grad(x, labels, e, w, keeps, 0.1)
    assert np.isfinite(loss)
    h = 1e-6
    for d, names in ((e, X.EXIT), (w, R.TENSORS)):
        for name in names:
            scale = np.abs(g[name]).max()
            assert scale > 0 and g[name].shape == d[name].shape
            flat = d[name].reshape(-1)                          # a view: the perturbation reaches the dict
            picks = list(rng.choice(flat.size, min(20, flat.size), replace=False))
            if name in ('D1', 'D2'):
                C = d[name].shape[2]
                picks += [(ky * 3 + kx) * C + int(rng.integers(C - 1)) for ky in (0, 2) for kx in (0, 2)]
            for i in picks:
                keep = flat[i]
                flat[i] = keep + h
                up = X.loss_and_grad(x, labels, e, w, keeps, 0.1)[0]
                flat[i] = keep - h
                down = X.loss_and_grad(x, labels, e, w, keeps, 0.1)[0]
                flat[i] = keep
                fd = (up - down) / (2 * h)
                assert abs(fd - g[name].reshape(-1)[i]) <= 1e-6 * scale, (name, int(i), fd, g[name].reshape(-1)[i])
    assert not g['gamma1'][-1] and not g['beta2'][-1] and not g['P2'][:, -1].any()          # the dead channels


def test_head_part_is_train_refs_own_and_the_input_gradient_is_right():
    """``head_loss_grad`` returns ``_train_ref.loss_and_grad``'s loss and gradients as they are, and its input gradient agrees with
    central differences over the features."""
    rng = np.random.default_rng(3)
    _, _, w, head = _toy()
    f = np.abs(rng.standard_normal((3, head[0])))
    labels = np.array([1, 0, 1])
    keeps = X.keep_masks(R.SEED, np.array([0, 5, 9]), 1, 0.1, head)
    loss, g, df = X.head_loss_grad(f, labels, w, keeps, 0.1)
    want_loss, want = R.loss_and_grad(f, labels, w, keeps, 0.1)
    assert loss == want_loss and all(np.array_equal(g[k], want[k]) for k in R.TENSORS)
    assert (df[~keeps[0]] == 0).all() and np.abs(df).max() > 0
    for i in range(f.size):
        flat = f.reshape(-1)
        keep = flat[i]
        flat[i] = keep + 1e-6
        up = R.loss_and_grad(f, labels, w, keeps, 0.1, want_grad=False)[0]
        flat[i] = keep - 1e-6
        down = R.loss_and_grad(f, labels, w, keeps, 0.1, want_grad=False)[0]
        flat[i] = keep
        assert abs((up - down) / 2e-6 - df.reshape(-1)[i]) <= 1e-6 * np.abs(df).max()


def test_depthwise_transposes_are_transposes():
    """<dw(x, D), y> = <x, dw_input_grad(y, D)> = <D, dw_weight_grad(x, y)>, and a one-hot corner input meets only the taps that
    zero padding leaves it."""
    rng = np.random.default_rng(1)
    x, y, D = rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((3, 3, 3))
    lhs = (X.dw(x, D) * y).sum()
    assert abs(lhs - (x * X.dw_input_grad(y, D)).sum()) < 1e-12 and abs(lhs - (D * X.dw_weight_grad(x, y)).sum()) < 1e-12
    one = np.zeros((1, 4, 5, 1))
    one[0, 0, 0, 0] = 1
    out = X.dw(one, np.arange(9.0).reshape(3, 3, 1))
    assert out[0, 0, 0, 0] == 4 and out[0, 1, 1, 0] == 0 and out[0, 0, 1, 0] == 3 and out[0, 1, 0, 0] == 1 and out.sum() == 0 + 1 + 3 + 4


@pytest.mark.parametrize('n', X.GRAD_N)
def test_float32_twin_error_on_the_gpu_cases(n):
    """Per tensor max|g32 - g64| / max|g64| of the GPU gradient cases: computed, never stored -- tests/test_gpu_exit_train.py allows
    the device 8 x this number and adds nothing to it.  Here: a rounding-level number, no less than float32's unit roundoff -- the
    rule the cases are chosen by, so that the loss's one figure and ``logits/bias``'s two are not float64's by luck -- and not large
    (both rates, both label kinds)."""
    for rate in X.GRAD_RATES:
        for kind in X.GRAD_LABELS:
            rows, labels, l64, g64, f64, twin = X.grad_reference(n, rate, kind)
            assert np.isfinite(l64) and len(rows) == n and f64.shape == (n, 2048)
            assert np.array_equal(rows, X.grad_case(n, kind, rate)[0]) and (n < 3 or (rows[1] == 1 and rows[2] == rows[0]))
            assert set(twin) == set(X.EXIT + R.TENSORS + ('loss', 'feat'))
            for name in X.EXIT + R.TENSORS + ('loss', 'feat'):
                print(f'n={n} rate={rate} {kind} {name}: {twin[name]:.3e}')
                assert 2.0 ** -24 <= twin[name] < 1e-4, (n, rate, kind, name, twin[name])
            assert (g64['gamma1'][-8:] == 0).all() and (g64['P1'][:, -8:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_exit_vector_round_trip():
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    vec = T.flatten_exit(w)
    assert vec.shape == (T.EXIT_PARAMS,) == (4748800,) and vec.dtype == np.float32 and T.EXIT_PARAMS + T.HEAD_PARAMS == 7898626
    back = T.unflatten_exit(vec)
    assert [k for k, _ in T.EXIT_TENSORS] == list(back) and all(np.array_equal(back[k], w[k]) and back[k].shape == s for k, s in T.EXIT_TENSORS)
    # the order: D1 [3][3][1024], P1 [1024][1536], gamma1, beta1, D2, P2, gamma2, beta2
    assert vec[1024 + 5] == w['block14_sepconv1/depthwise_kernel'][0, 1, 5, 0]
    assert vec[9216 + 1536 * 2 + 7] == w['block14_sepconv1/pointwise_kernel'][0, 0, 2, 7]
    assert vec[1582080 + 3] == w['block14_sepconv1_bn/gamma'][3] and vec[1583616 + 3] == w['block14_sepconv1_bn/beta'][3]
    assert vec[1585152] == w['block14_sepconv2/depthwise_kernel'][0, 0, 0, 0] and vec[1598976 + 2048] == w['block14_sepconv2/pointwise_kernel'][0, 0, 1, 0]
    assert vec[4744704] == w['block14_sepconv2_bn/gamma'][0] and vec[-1] == w['block14_sepconv2_bn/beta'][-1]
    stats = T.exit_bn_stats(w)
    assert stats.shape == (7168,) and stats[1536] == w['block14_sepconv1_bn/moving_variance'][0] and stats[-1] == w['block14_sepconv2_bn/moving_variance'][-1]
    # the test reference flattens to the same vector
    e = X.from_keras(w)
    ref_vec, ref_stats = X.flatten(e)
    assert np.array_equal(ref_vec, vec) and np.array_equal(ref_stats, stats)
    with pytest.raises(ValueError):
        T.unflatten_exit(vec[:-1])
    with pytest.raises(ValueError):
        T.flatten_exit({**w, 'block14_sepconv1_bn/gamma': np.zeros(3, np.float32)})


def test_pack_blob_carries_the_trunk_multiplier():
    """``act/trunk_mul`` = 2^k of ``block13_out``'s activation exponent, which ``bq_trunk_u8`` multiplies by: present in an f16 blob
    exactly when k is not 0, and nothing else in the blob knows of it."""
    import struct
    from biscuit_amd import weights as W

    def entries(blob):
        magic, ver, cnt, dt = struct.unpack('<4sIII', blob[:16])
        out = {}
        for i in range(cnt):
            nm, off, ln = struct.unpack('<48sQQ', blob[16 + 64 * i:16 + 64 * (i + 1)])
            out[nm.rstrip(b'\0').decode()] = blob[off:off + ln]
        return out
    w = W.synthetic_weights(2, hard=True)
    assert W.TRUNK_TENSOR == 'block13_out' and W.TRUNK_TENSOR in {o for _, _, o in W.tensor_plan()}
    plain = entries(W.pack_blob(w, 'f16', {'block4_out': 6}))
    assert 'act/trunk_mul' not in plain
    for k, mul in ((3, 8.0), (-2, 0.25)):
        b = entries(W.pack_blob(w, 'f16', {'block4_out': 6, W.TRUNK_TENSOR: k}))
        assert set(b) == set(plain) | {'act/trunk_mul'} and np.frombuffer(b['act/trunk_mul'], np.float32).tolist() == [mul]
        moved = {name for name in plain if plain[name] != b[name]}
        assert moved and all(name.startswith(('block13_', 'block14_sepconv1/')) and name.endswith(('/scale', '/bias')) for name in moved), moved


def test_exit_file_round_trip(tmp_path):
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    T.save_exit(str(tmp_path / T.EXIT_FILE), w)
    back = T.load_exit(str(tmp_path / T.EXIT_FILE))
    assert T.EXIT_FILE == 'exit.npz' and all(np.array_equal(back[k], w[k]) for k, _ in T.EXIT_TENSORS) and len(back) == 8


def test_trainable_is_validated_before_anything_loads(tmp_path, capsys):
    assert T.TrainParams().trainable == 'head' and T.TrainParams(trainable='exit').validate().trainable == 'exit'
    with pytest.raises(ValueError, match='trainable'):
        T.TrainParams(trainable='block13').validate()
    with pytest.raises(ValueError, match='256'):
        T.TrainParams(trainable='exit', batch_size=257).validate()
    with pytest.raises(ValueError):
        T.TrainParams(trainable='exit', validation_dropout=True).validate()
    # the command line refuses the value while parsing: no file named here exists, and none is looked for
    with pytest.raises(SystemExit) as err:
        T.main([str(tmp_path / 'none.tfrecords'), '--labels', str(tmp_path / 'none.csv'), '--model', str(tmp_path / 'none'), '--out',
                str(tmp_path / 'out'), '--trainable', 'everything'])
    assert err.value.code == 2 and '--trainable' in capsys.readouterr().err and not (tmp_path / 'out').exists()


def test_memory_guard_names_both_figures():
    assert T.ACT_BYTES == 409600 and T.activation_cache_bytes(1000, 2) == 1000 * 409600 * 3
    assert T.check_activation_memory(1000, 0, 409600000) == 409600000
    with pytest.raises(ValueError) as err:
        T.check_activation_memory(1000, 1, 500000000)
    assert '819200000' in str(err.value) and '500000000' in str(err.value)


def test_fit_head_refuses_a_feature_cache_for_exit():
    class _Engine:
        class hp:
            seed = 1
        weights = {}
        device = 'cpu'
    cache = T.FeatureCache(np.zeros((4, 2048), np.float32), np.zeros(4, np.int64), np.zeros((4, 2), np.int64), ['s'])
    with pytest.raises(ValueError, match='ActivationCache'):
        T.fit_head(_Engine(), cache, [0, 1], [0, 1], init={}, params=T.TrainParams(trainable='exit'))


def test_activation_cache_file(tmp_path):
    rng = np.random.default_rng(2)
    c = T.ActivationCache(rng.random((3, 2048), dtype=np.float32), np.array([0, 0, 1], np.int64), np.arange(6, dtype=np.int64).reshape(3, 2),
                          ['a', 'b'], rng.random((2, 3, 2048), dtype=np.float32), 'xy', 9, acts=rng.random((3, 10, 10, 1024), dtype=np.float32),
                          act_views=rng.random((2, 3, 10, 10, 1024), dtype=np.float32))
    path = str(tmp_path / 'acts.npz')
    c.save(path)
    back = T.ActivationCache.load(path)
    assert isinstance(back, T.FeatureCache) and len(back) == 3 and back.n_views() == 2 and (back.augment, back.augment_seed) == ('xy', 9)
    assert all(np.array_equal(getattr(back, k), getattr(c, k)) for k in ('feats', 'views', 'acts', 'act_views', 'slide_idx', 'loc'))
    assert np.array_equal(back.rows_of(['b']), [2])
    # a FeatureCache reads the same file; an ActivationCache refuses a feature cache's
    assert np.array_equal(T.FeatureCache.load(path).feats, c.feats)
    T.FeatureCache(c.feats, c.slide_idx, c.loc, c.slides).save(str(tmp_path / 'feats.npz'))
    with pytest.raises(ValueError, match='activation'):
        T.ActivationCache.load(str(tmp_path / 'feats.npz'))
