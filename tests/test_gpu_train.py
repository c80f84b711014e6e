"""Head training on the GPU (csrc/kernels_train.hip, biscuit_amd/train.py; DESIGN.md section 7 "Head training") against the float64
restatement of tests/_train_ref.py: a cache of 40 half-normal feature rows (one all zeros) and ``synthetic_weights(1)``'s head with
eight dead units.  The gradient tolerance is 8 x the float32 twin's own distance from float64 for the same case (the factor covers
a different summation order over K <= 2048).  ``-m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from biscuit_amd import inference as inf
from biscuit_amd import predictions, threshold
from biscuit_amd import tfrecord as tfr
from biscuit_amd import train as T
from biscuit_amd.synthetic import make_tiles
from tests import _poison as P
from tests import _train_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


@pytest.fixture(scope='module')
def feats(eng):
    return torch.from_numpy(R.cache()).to(eng.device)


@pytest.fixture(scope='module')
def params(eng):
    return torch.from_numpy(T.flatten_head(R.head())).to(eng.device)


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# ------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize('n', R.GRAD_N)
def test_gradients_within_eight_twin_errors(eng, feats, params, n):
    for rate in R.GRAD_RATES:
        for kind in R.GRAD_LABELS:
            rows, labels, l64, g64, twin = R.grad_reference(n, rate, kind)
            g, loss = eng.head_grad(params, feats, up(eng, rows), up(eng, labels), 3, R.SEED, rate=rate)
            gd = T.unflatten_head(g.cpu().numpy())
            err = {k: R.rel_err(gd[k], g64[k]) for k in R.TENSORS}
            err['loss'] = R.rel_err(float(loss[0]), l64)
            for k, e in err.items():
                print(f'n={n} rate={rate} {kind} {k}: device {e:.3e} twin {twin[k]:.3e} ratio {e / twin[k]:.2f}')
            for k, e in err.items():
                assert e <= 8 * twin[k], (n, rate, kind, k, e, twin[k])
            assert (gd['hidden_0/kernel'][:, -8:] == 0).all() and (gd['hidden_0/bias'][-8:] == 0).all()
            assert (gd['hidden_1/kernel'][-8:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. Adam, isolated
def test_adam_against_float64_at_step_0_and_1000(eng, feats, params):
    rows, labels, _, _, _ = R.grad_reference(33, 0.1, 'mixed')
    g, _ = eng.head_grad(params, feats, up(eng, rows), up(eng, labels), 3, R.SEED, rate=0.1)
    gh = g.cpu().numpy()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    for step in (0, 1000):
        w0, m0, v0 = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        eng.head_adam(w, m, v, g, step, 1e-3)
        w64, m64, v64 = R.adam(w0, m0, v0, gh, step, 1e-3)
        w1, m1, v1 = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        assert (np.abs(m1 - m64) <= 2.0 ** -22 * np.abs(m64)).all() and (np.abs(v1 - v64) <= 2.0 ** -22 * np.abs(v64)).all()
        want = w64.astype(np.float32)
        assert (np.abs(w1.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
        still = (gh == 0) & (m0 == 0) & (v0 == 0)
        assert still.sum() >= 8 * 2048 and np.array_equal(w1[still].view(np.uint32), w0[still].view(np.uint32))
        assert not np.array_equal(w1, w0)


# ------------------------------------------------------------------------------------------------ 3. steps == single calls
def _seven_steps():
    rng = np.random.default_rng(3)
    rows = np.concatenate([rng.permutation(R.CACHE_ROWS) for _ in range(3)])[:6 * 16 + 8].astype(np.int64)
    return rows, rng.integers(0, 2, len(rows)).astype(np.uint8), [1e-3 * 0.98 ** i for i in range(7)]


def _run_steps(eng, feats, params, scratch=None):
    rows, labels, lr = _seven_steps()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    losses = eng.head_train_steps(w, m, v, feats, up(eng, rows), up(eng, labels), 16, 0, 9, lr, rate=0.1, scratch=scratch)
    assert losses.shape == (7,)
    return [t.cpu().numpy() for t in (w, m, v, losses)]


@pytest.fixture(scope='module')
def seven(eng, feats, params):
    return _run_steps(eng, feats, params)


def test_train_steps_equal_the_single_calls_bit_for_bit(eng, feats, params, seven):
    rows, labels, lr = _seven_steps()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    losses = []
    for i in range(7):
        r, y = up(eng, rows[i * 16:(i + 1) * 16]), up(eng, labels[i * 16:(i + 1) * 16])
        assert r.numel() == (16 if i < 6 else 8)
        g, loss = eng.head_grad(w, feats, r, y, i, 9, rate=0.1)
        eng.head_adam(w, m, v, g, i, lr[i])
        losses.append(loss.cpu().numpy()[0])
    single = [w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), np.array(losses, np.float32)]
    for a, b in zip(seven, single):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(seven, _run_steps(eng, feats, params)):                # a second run: the same bits
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(seven[3]).all() and not np.array_equal(seven[0], params.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 4. trajectory
def test_trajectory_follows_float64():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    rng = np.random.default_rng(21)
    f = np.abs(rng.standard_normal((40, 2048))).astype(np.float32)
    f[20:] += np.float32(0.25) * (np.arange(2048) % 2 == 0)                # the classes differ in mean
    y = (np.arange(40) >= 20).astype(np.uint8)
    idx = np.concatenate([np.random.default_rng([4, e]).permutation(40) for e in range(16)])[:640]
    lr = [1e-3] * 40
    _, l64 = R.train_steps(f, idx, y[idx], R.head(), 16, 9, 0.1, lr)
    _, l32 = R.train_steps(f, idx, y[idx], R.head(), 16, 9, 0.1, lr, dtype=np.float32)
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    try:
        w = up(eng, T.flatten_head(R.head()))
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        dev = eng.head_train_steps(w, m, v, up(eng, f), up(eng, idx), up(eng, y[idx]), 16, 0, 9, lr, rate=0.1).cpu().numpy().astype(np.float64)
    finally:
        eng.close()
    twin = abs(l32[-10:].astype(np.float64).mean() - l64[-10:].mean())
    mine = abs(dev[-10:].mean() - l64[-10:].mean())
    print(f'last-10 mean loss: float64 {l64[-10:].mean():.6e}, device off by {mine:.3e}, float32 twin off by {twin:.3e}; first {dev[0]:.4f}')
    assert mine <= 8 * twin and dev[-10:].mean() < dev[0]


# ------------------------------------------------------------------------------------------------ 5. the new path joins the old one
def test_cache_predict_equals_evaluate_and_a_trained_head_a_fresh_engine(eng, tmp_path):
    from biscuit_amd.engine import Engine
    paths = []
    for i, name in enumerate(('a', 'b')):
        t = make_tiles(5, seed=60 + i, slide_bias=[i * 40.0 - 20.0, 0.0, 0.0])
        loc = np.stack([np.arange(5) * 299 + 150, np.full(5, 150 + 1000 * i)], 1).astype(np.int64)
        paths.append(str(tmp_path / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
    labels = {'a': 0, 'b': 1}
    cache = T.cache_features(eng, inf.slides_from_tfrecords(paths, labels), batch=4)
    assert len(cache) == 10 and cache.slides == ['a', 'b'] and tuple(cache.feats.shape) == (10, 2048) and cache.feats.is_cuda
    assert cache.slide_idx.tolist() == [0] * 5 + [1] * 5 and cache.loc[6].tolist() == [299 + 150, 1150]
    rows = np.arange(10)
    table = T.predict(eng, cache, rows, None, mc_n=8, seed=3, y_true=labels)
    want = inf.evaluate(eng, inf.slides_from_tfrecords(paths, labels), outcome='cohort', batch=16, mc_n=8, seed=3).tile_df
    assert [c for c in table.columns if not c.startswith('loc_')] == list(want.columns) and len(table) == 10 == len(want)
    for col in want.columns:
        assert np.array_equal(table[col].to_numpy(), want[col].to_numpy()), col

    head, losses = T.train_head(eng, cache, rows, np.array([0] * 5 + [1] * 5), init='model',
                                params=T.TrainParams(batch_size=4, learning_rate=1e-3), seed=5)
    assert losses.shape == (3,) and np.isfinite(losses).all()
    assert not np.array_equal(head['logits/kernel'], np.asarray(eng.weights['logits/kernel'], np.float32))
    table = T.predict(eng, cache, rows, head, mc_n=8, seed=3, y_true=labels)
    fresh = Engine({**eng.weights, **head}, dtype='f16', max_batch=16, max_mc=8)
    try:
        mean, std = fresh.mc_head(cache.feats, 8, 3, tile_idx0=0, tile_idx=up(eng, rows.astype(np.int64)))
        mean, std = mean.cpu().numpy(), std.cpu().numpy()
    finally:
        fresh.close()
    assert np.array_equal(table['cohort-y_pred1'].to_numpy(), mean[:, 1].astype(np.float64))
    assert np.array_equal(table['cohort-uncertainty1'].to_numpy(), std[:, 1].astype(np.float64))
    assert not np.array_equal(table['cohort-y_pred1'].to_numpy(), want['cohort-y_pred1'].to_numpy())


# ------------------------------------------------------------------------------------------------ 6. non-finite input
def test_nan_in_a_gathered_row_gives_nan_and_elsewhere_changes_nothing(eng, feats, params):
    rows, labels, _, _, _ = R.grad_reference(32, 0.1, 'mixed')
    spare = next(r for r in range(R.CACHE_ROWS) if r not in set(rows.tolist()))
    g0, l0 = eng.head_grad(params, feats, up(eng, rows), up(eng, labels), 3, R.SEED, rate=0.1)
    for value in (float('nan'), float('inf')):
        bad = feats.clone()
        bad[spare, 100] = value
        g1, l1 = eng.head_grad(params, bad, up(eng, rows), up(eng, labels), 3, R.SEED, rate=0.1)
        assert torch.equal(g1, g0) and torch.equal(l1, l0) and bool(torch.isfinite(l0).all())
        for unit in range(4):                       # kept or dropped: every unit of a Philox group
            bad = feats.clone()
            bad[int(rows[5]), 100 + unit] = value
            _, l2 = eng.head_grad(params, bad, up(eng, rows), up(eng, labels), 3, R.SEED, rate=0.1)
            assert bool(torch.isnan(l2).all()), (value, unit)
    far = up(eng, np.where(np.arange(32) == 4, R.CACHE_ROWS, rows))              # an index outside the cache: never read, NaN
    assert bool(torch.isnan(eng.head_grad(params, feats, far, up(eng, labels), 3, R.SEED, rate=0.1)[1]).all())
    with pytest.raises(ValueError):
        eng.head_grad(params, feats, up(eng, rows).int(), up(eng, labels), 3, R.SEED)
    with pytest.raises(ValueError):
        eng.head_grad(params[:-1], feats, up(eng, rows), up(eng, labels), 3, R.SEED)


# ------------------------------------------------------------------------------------------------ 7. poisoned scratch
def test_poisoned_workspace_same_bits_guards_intact(eng, feats, params, seven):
    need = int(eng._lib.bq_head_train_workspace_bytes(16))
    assert need > 0 and eng._lib.bq_head_train_workspace_bytes(0) == 0 and eng._lib.bq_head_train_workspace_bytes(1025) == 0
    for fill in P.BYTE_FILLS:
        scratch, check = P.guarded(need, fill, eng.device)             # (a caller's own: what ``eng.train_scratch(16)`` sizes)
        got = _run_steps(eng, feats, params, scratch=scratch)
        torch.cuda.synchronize(eng.device)
        check()
        for a, b in zip(seven, got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), hex(fill)
    eng.drop_scratch()
    _run_steps(eng, feats, params)
    assert 'train' in eng._tool_ws and eng._tool_ws['train'].numel() >= need
    from biscuit_amd.engine import BiscuitHipError
    assert eng.train_scratch(16).numel() == need
    with pytest.raises(BiscuitHipError, match='workspace'):
        eng.head_train_steps(params.clone(), torch.zeros_like(params), torch.zeros_like(params), feats, up(eng, np.zeros(16, np.int64)),
                             up(eng, np.zeros(16, np.uint8)), 16, 0, 9, [1e-3], scratch=eng._bytes(need - 256))


def test_sizes_and_refusals(eng, feats, params):
    """The workspace's size is the layout of include/biscuit_hip.h, and every branch of the three entries' argument checks refuses
    with its code and its text (``bq_last_error``); nothing is enqueued."""
    lib = eng._lib
    import inspect                                  # the constants that engine.py and train.py each hold a copy of
    assert (eng.HEAD_PARAMS, eng.HEAD_TRAIN_MAX_ROWS, eng.HEAD_VALIDATE_MAX_ROWS) == (T.HEAD_PARAMS, T.HEAD_TRAIN_MAX_ROWS, T.HEAD_VALIDATE_MAX_ROWS)
    for call in (eng.head_adam, eng.head_train_steps):
        d = inspect.signature(call).parameters
        assert (d['b1'].default, d['b2'].default, d['eps'].default) == (T.ADAM_BETA_1, T.ADAM_BETA_2, T.ADAM_EPSILON)
    al = lambda b: (b + 255) & ~255                 # h0 | h1 | dz1 | dz0, each [n][1024] f32 | dlog [n][2] f32 | rowloss f64 [n]
    for n in (1, 63, 64, 65, 1024):
        assert lib.bq_head_train_workspace_bytes(n) == 4 * al(n * 1024 * 4) + al(n * 2 * 4) + al(n * 8), n
    assert lib.bq_head_train_workspace_bytes(0) == 0 and lib.bq_head_train_workspace_bytes(1025) == 0
    rows, labels = up(eng, np.zeros(32, np.int64)), up(eng, np.zeros(32, np.uint8))
    w, m, v, g = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.full_like(params, 7.0)
    loss = torch.full((2,), 7.0, dtype=torch.float32, device=eng.device)
    ws, need = eng.train_scratch(16), int(lib.bq_head_train_workspace_bytes(16))
    lr = (C.c_double * 2)(1e-3, 1e-3)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def grad(code, text, w_off=0, n_feat=int(feats.shape[0]), n=16, step=0, rate=0.1, nbytes=need):
        rc = lib.bq_head_grad(eng._ctx, vp(w, w_off), vp(feats), n_feat, vp(rows), vp(labels), n, step, 9, rate, vp(g), vp(loss), vp(ws), nbytes,
                              eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_head_grad: ' + text)

    def adam(code, text, w_off=0, step=0, b1=0.9):
        rc = lib.bq_head_adam(eng._ctx, vp(w, w_off), vp(m), vp(v), vp(g), step, 1e-3, b1, 0.999, 1e-7, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_head_adam: ' + text)

    def steps(code, text, w_off=0, n_feat=int(feats.shape[0]), steps=2, batch=16, last_n=16, step0=0, rate=0.1, b1=0.9, nbytes=need):
        rc = lib.bq_head_train_steps(eng._ctx, vp(w, w_off), vp(m), vp(v), vp(g), vp(feats), n_feat, vp(rows), vp(labels), steps, batch, last_n,
                                     step0, 9, rate, lr, b1, 0.999, 1e-7, vp(loss), vp(ws), nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_head_train_steps: ' + text)

    cache_or_step = 'an empty feature cache, or a step outside 0 .. 2^32 - 1'
    pointers = 'bad argument (null pointer, params, feats or grad not 16-byte, rows not 8-byte or the workspace not 256-byte aligned)'
    adam_values = 'a step outside 0 .. 2^32 - 1, a learning rate that is not finite, b1 or b2 outside [0, 1), or eps <= 0'
    grad(-1, '1 <= n <= 1024', n=0)
    grad(-1, '1 <= n <= 1024', n=1025)
    grad(-1, cache_or_step, n_feat=0)
    grad(-1, cache_or_step, step=1 << 32)
    grad(-1, 'the rate must lie in [0, 1)', rate=1.0)
    grad(-1, pointers, w_off=4)
    grad(-4, 'workspace below bq_head_train_workspace_bytes(n)', nbytes=need - 1)
    adam(-1, 'bad argument (null or misaligned pointer)', w_off=2)
    adam(-1, adam_values, step=1 << 32)
    adam(-1, adam_values, b1=1.0)
    steps(-1, '1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step', steps=0)
    steps(-1, '1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step', last_n=17)
    steps(-1, '1 <= n <= 1024', batch=1025)
    steps(-1, cache_or_step, n_feat=0)
    steps(-1, cache_or_step, step0=1 << 32)
    steps(-1, 'the steps pass 2^32', step0=(1 << 32) - 1)
    steps(-1, 'the rate must lie in [0, 1)', rate=1.0)
    steps(-1, pointers, w_off=4)
    steps(-1, adam_values, b1=1.0)
    steps(-4, 'workspace below bq_head_train_workspace_bytes(batch)', nbytes=need - 1)
    torch.cuda.synchronize(eng.device)
    assert torch.equal(w, params) and not m.any() and not v.any() and bool((g == 7.0).all()) and loss.tolist() == [7.0, 7.0]


# ------------------------------------------------------------------------------------------------ 8. end to end at toy size
# Chosen, among a few seeds, shifts and learning rates tried, as one where ``threshold.from_cv`` raises in no outer fold.  With four
# validation slides per inner fold Youden's cut often lies at the ROC curve's first point, whose threshold sklearn states as inf: that
# is from_cv's decision too, and the means carry it; outer fold 2 of this cohort yields finite thresholds throughout.
TOY_SEED, TOY_SHIFT, TOY_LR, TOY_EPOCHS = 12, 0.04, 1e-4, 4


def _toy_nested_cv(eng, out, data_seed=TOY_SEED, shift=TOY_SHIFT, lr=TOY_LR, epochs=TOY_EPOCHS):
    """12 synthetic slides x 6 tiles, two classes whose features differ in mean by ``shift`` on every other unit, through
    ``train_nested_cv(outer_k=3, inner_k=2)`` with a Glorot start -> ``(slides, directories, trainer)``."""
    rng = np.random.default_rng(data_seed)
    slides = [f's{i:02d}' for i in range(12)]
    labels = {s: i % 2 for i, s in enumerate(slides)}
    f = np.abs(rng.standard_normal((72, 2048))).astype(np.float32)
    sidx = np.repeat(np.arange(12), 6).astype(np.int64)
    f[sidx % 2 == 1] += np.float32(shift) * (np.arange(2048) % 2 == 0)
    cache = T.FeatureCache(up(eng, f), sidx, np.stack([np.arange(72), np.zeros(72, np.int64)], 1).astype(np.int64), slides)
    trainer = T.HeadTrainer(eng, cache, labels, params=T.TrainParams(batch_size=16, learning_rate=lr, epochs=[epochs]), init='glorot', mc_n=4)
    return slides, T.train_nested_cv(cache, labels, out, 'EXP', trainer, outer_k=3, inner_k=2, seed=2), trainer


def _from_cv_by_hand(out, slides, outer):
    """What ``threshold.from_cv`` decides over the inner folds of outer fold ``outer``: its thresholds, or the exception it raises."""
    pmap = {s: s for s in slides}
    dfs = T._cv_frames(out, f'EXP-k{outer}', 2, 'cohort', pmap)
    kw = dict(tile_pred='detect', slide_pred='detect', plot=False, patients=pmap)
    try:
        tile_uq = threshold.from_cv(dfs, tile_uq='detect', slide_uq=None, **kw)['tile_uq']
        return threshold.from_cv(dfs, tile_uq=tile_uq, slide_uq='detect', **kw)
    except Exception as e:                                      # noqa: BLE001 -- the outcome itself is what is compared
        return e


def test_nested_cv_end_to_end_at_toy_size(eng, tmp_path):
    out = str(tmp_path / 'cv')
    slides, dirs, trainer = _toy_nested_cv(eng, out)
    assert [os.path.basename(d) for d in dirs] == [f'EXP-kfold{k}' for k in (1, 2, 3)] + [f'EXP-k{k}-kfold{j}' for k in (1, 2, 3) for j in (1, 2)]
    assert len(trainer.losses) == 9 and all(np.isfinite(x).all() for x in trainer.losses)
    for d in dirs:
        df = predictions.load_tile_predictions(os.path.join(d, predictions.VAL_NAME), 'cohort')
        assert {'slide', 'y_true', 'y_pred', 'uncertainty'} <= set(df.columns) and len(df) % 6 == 0 and len(df) > 0
        assert np.isfinite(df['y_pred']).all() and (df['uncertainty'] >= 0).all()
        head = T.load_head(os.path.join(d, T.HEAD_FILE))
        assert head['hidden_0/kernel'].shape == (2048, 1024) and head['hidden_0/bias'].any()
    hand = [_from_cv_by_hand(out, slides, k) for k in (1, 2, 3)]
    print('from_cv by hand:', hand)
    refused = [h for h in hand if isinstance(h, Exception)]
    if refused:                                                 # the same refusal, as the reference lets it through
        with pytest.raises(type(refused[0])):
            T.thresholds_from_nested_cv(out, 'EXP', outer_k=3, inner_k=2)
    assert not refused, 'the toy cohort is chosen so that from_cv finds thresholds in every outer fold'
    frame, th = T.thresholds_from_nested_cv(out, 'EXP', outer_k=3, inner_k=2)
    assert frame['fold'].tolist() == [1, 2, 3] and frame['n_slides'].tolist() == [12, 12, 12]
    assert th == {'tile_uq': np.mean([h['tile_uq'] for h in hand]), 'slide_uq': np.mean([h['slide_uq'] for h in hand]),
                  'slide_pred': np.mean([h['slide_pred'] for h in hand])}
    assert not any(np.isnan(v) for v in th.values()) and all(np.isfinite(v) for v in hand[1].values())
    assert list(frame.columns) == ['id', 'n_slides', 'fold', 'uq', 'patient_auc', 'patient_uq_perc', 'slide_auc', 'slide_uq_perc']
