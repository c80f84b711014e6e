"""Training-mode batch norm of the exit flow on the GPU (csrc/kernels_train.hip: ``bq_exit_grad_bn``, ``bq_exit_bn_move``,
``bq_exit_train_steps_bn``; DESIGN.md section 7 "Exit-flow fine-tuning", Two modes) against the float64 restatement of
tests/_exit_bn_ref.py: the channel counts are the network's own, the small dimension is n in {1, 2, 3, 5} -- 100 .. 500 rows of a
layer's statistics, one to five per-tile partial sums.  The gradient tolerance is 8 x the float32 twin's own distance from float64
for the same case, with nothing added.  ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import _lib as L
from biscuit_amd import inference as inf
from biscuit_amd import tfrecord as tfr
from biscuit_amd import train as T
from biscuit_amd.synthetic import make_tiles
from tests import _exit_bn_ref as B
from tests import _exit_train_ref as X
from tests import _poison as P
from tests import _train_ref as R

pytestmark = pytest.mark.gpu

E_G2 = T.EXIT_PARAMS - 2 * 2048                                 # dgamma2 | dbeta2 close the exit vector
SLICES = {}                                                     # tensor -> its slice of the exit vector
_at = 0
for _name, _shape in T.EXIT_TENSORS:
    SLICES[_name] = slice(_at, _at + int(np.prod(_shape)))
    _at += int(np.prod(_shape))


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=8)
    yield e
    e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


@pytest.fixture(scope='module')
def dev(eng):
    """``(acts [12, 10, 10, 1024], params [P_ALL], the imported moving statistics [7168])`` on the device."""
    x, e, w = B.inputs()
    vec, stats = X.flatten(e, w)
    return up(eng, x), up(eng, vec), up(eng, stats)


# fixed batches for the bit-for-bit tests: one tile; two; three with the all-zero tile and one tile twice
CASES = {1: (np.array([2], np.int64), np.array([1], np.uint8)), 2: (np.array([5, 0], np.int64), np.array([0, 1], np.uint8)),
         3: (np.array([4, 1, 4], np.int64), np.array([0, 1, 1], np.uint8))}


def bits(t):
    return t.detach().cpu().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def same(a, b):
    return all(np.array_equal(bits(s), bits(t)) for s, t in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. gradients against float64
@pytest.mark.parametrize('n', X.GRAD_N)
def test_gradients_and_statistics_within_eight_twin_errors(eng, dev, n):
    """Worst ratios device / twin measured on an MI355X, per group (the bound is 8): see DESIGN.md section 7, Two modes, Accuracy."""
    acts, _, _ = dev
    _, _, w = B.inputs()
    for rate in X.GRAD_RATES:
        for kind in X.GRAD_LABELS:
            rows, labels, e, l64, g64, s64, twin = B.grad_reference(n, rate, kind)
            params = up(eng, X.flatten(e, w)[0])
            g, loss, bs = eng.exit_grad(params, None, acts, up(eng, rows), up(eng, labels), 3, X.SEED, rate=rate, bn='batch')
            gd = X.split_grad(g.cpu().numpy(), e, w)
            err = {k: R.rel_err(gd[k], g64[k]) for k in X.EXIT + R.TENSORS}
            err['loss'] = R.rel_err(float(loss[0]), l64)
            got = bs.cpu().numpy()
            at = 0
            for s in B.BATCH_STATS:
                err[s] = R.rel_err(got[at:at + s64[s].size], s64[s])
                at += s64[s].size
            assert at == got.size == eng.EXIT_BN_STATS
            for k, v in err.items():
                print(f'n={n} rate={rate} {kind} {k}: device {v:.3e} twin {twin[k]:.3e} ratio {v / twin[k]:.2f}')
            for k, v in err.items():
                assert v <= 8 * twin[k], (n, rate, kind, k, v, twin[k])
            assert (gd['gamma1'][-8:] == 0).all() and (gd['beta1'][-8:] == 0).all() and (gd['P1'][:, -8:] == 0).all()   # the dead channels
            assert (gd['D2'][:, :, -8:] == 0).all() and (gd['P2'][-8:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. what the two modes share
@pytest.mark.parametrize('rate', X.GRAD_RATES)
def test_frozen_call_on_the_reported_statistics_shares_the_forward_bit_for_bit(eng, dev, rate):
    acts, params, _ = dev
    for rows, labels in CASES[1], CASES[3]:
        r, y = up(eng, rows), up(eng, labels)
        g, loss, bs = eng.exit_grad(params, None, acts, r, y, 3, X.SEED, rate=rate, bn='batch')
        gf, lossf = eng.exit_grad(params, bs, acts, r, y, 3, X.SEED, rate=rate)
        assert torch.equal(loss, lossf) and bool(torch.isfinite(loss).all())
        assert torch.equal(g[eng.EXIT_PARAMS:], gf[eng.EXIT_PARAMS:]) and torch.equal(g[E_G2:eng.EXIT_PARAMS], gf[E_G2:eng.EXIT_PARAMS])
        for name, s in SLICES.items():
            if not name.startswith('block14_sepconv2_bn'):
                assert not torch.equal(g[s], gf[s]), name           # dP2 and everything upstream


# ------------------------------------------------------------------------------------------------ 3. two passes
def test_variance_of_a_channel_far_from_zero_takes_two_passes(eng, dev):
    """tests/_exit_bn_ref.py ``two_pass_case`` (noise 1e-2; tests/test_exit_bn.py shows on the CPU that a float32 E[z^2] - mu^2 misses
    this bound by four orders of magnitude): the channel's z1 is exact, so the distance is the statistics' own."""
    x, e = B.two_pass_case()
    _, _, w = B.inputs()
    c = B.TWO_PASS_CHANNEL
    k64, k32 = B.forward(x, e, np.float64)[1], B.forward(x, e, np.float32)[1]
    rows = up(eng, np.arange(B.TWO_PASS_N, dtype=np.int64))
    _, loss, bs = eng.exit_grad(up(eng, X.flatten(e, w)[0]), None, up(eng, x), rows, up(eng, np.array([0, 1, 1], np.uint8)), 3, X.SEED,
                                rate=0.0, bn='batch')
    got_mu, got_var = float(bs[c]), float(bs[1536 + c])
    twin_mu, twin_var = abs(float(k32['mu1'][c]) - k64['mu1'][c]), abs(float(k32['var1'][c]) - k64['var1'][c])
    d_mu, d_var = abs(got_mu - k64['mu1'][c]), abs(got_var - k64['var1'][c])
    print(f'var {k64["var1"][c]:.6e}: device off by {d_var:.3e}, twin by {twin_var:.3e}; mu: device off by {d_mu:.3e}, twin by {twin_mu:.3e}')
    assert bool(torch.isfinite(loss).all()) and twin_var > 0
    assert d_var <= 8 * twin_var


# ------------------------------------------------------------------------------------------------ 4. the same bits every time
def test_repeated_and_poisoned_workspace_same_bits_guards_intact(eng, dev):
    acts, params, _ = dev
    rows, labels = CASES[3]
    r, y = up(eng, rows), up(eng, labels)
    first = eng.exit_grad(params, None, acts, r, y, 3, X.SEED, rate=0.1, bn='batch')
    assert same(first, eng.exit_grad(params, None, acts, r, y, 3, X.SEED, rate=0.1, bn='batch'))
    need = int(eng._lib.bq_exit_bn_workspace_bytes(3, L.BQ_DTYPE_F32, L.BQ_ACT_DEVICE))
    assert need == eng.exit_bn_scratch(3).numel() > int(eng._lib.bq_exit_train_workspace_bytes(3))
    for fill in P.BYTE_FILLS:
        scratch, check = P.guarded(need, fill, eng.device)
        grad = torch.empty_like(params)
        P.fill_bytes(grad.view(torch.uint8), P.pattern(fill))
        again = eng.exit_grad(params, None, acts, r, y, 3, X.SEED, rate=0.1, grad=grad, scratch=scratch, bn='batch')
        torch.cuda.synchronize(eng.device)
        check()
        assert same(first, again), hex(fill)
    assert 'exit_bn' in eng._tool_ws


# ------------------------------------------------------------------------------------------------ 5., 6. the moving statistics, the loop
def _three_steps():
    rng = np.random.default_rng(3)
    rows = rng.permutation(np.array([0, 2, 3, 4, 5]))[:2 * 2 + 1].astype(np.int64)
    return rows, np.array([0, 1, 1, 0, 1], np.uint8), [1e-3 * 0.98 ** i for i in range(3)]


@pytest.fixture(scope='module')
def single(eng, dev):
    """Three steps at n = 2, 2, 1 as single calls -> ``(w, m, v, moving, losses, [(batch statistics, moving after) per step])``."""
    acts, params, stats = dev
    rows, labels, lr = _three_steps()
    w, m, v, moving = params.clone(), torch.zeros_like(params), torch.zeros_like(params), stats.clone()
    losses, trail = [], []
    for i in range(3):
        r, y = up(eng, rows[i * 2:(i + 1) * 2]), up(eng, labels[i * 2:(i + 1) * 2])
        assert r.numel() == (2 if i < 2 else 1)
        g, loss, bs = eng.exit_grad(w, None, acts, r, y, i, 9, rate=0.1, bn='batch')
        eng.adam_n(w, m, v, g, i, lr[i])
        eng.exit_bn_move(moving, bs, r.numel())
        losses.append(loss.clone())
        trail.append((bs.cpu().numpy(), moving.cpu().numpy()))
    return w, m, v, moving, torch.cat(losses), trail


def test_moving_statistics_follow_the_float64_recurrence_within_four_ulps(eng, dev, single):
    _, _, stats = dev
    before = stats.cpu().numpy()
    for i, (bs, after) in enumerate(single[5]):
        M = 200 if i < 2 else 100                               # the last, shorter step's own M
        want = B.moving_update(before, bs, M, 1536)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        off = np.abs(after.astype(np.float64) - want) / ulp
        print(f'step {i}: moving statistics off the float64 recurrence by at most {off.max():.2f} ulp')
        assert off.max() <= 4 and not np.array_equal(after, before)
        wrong_m = B.moving_update(before, bs, 300 - M, 1536)    # the other step's M shows: the variances then miss by many ulps
        assert (np.abs(after.astype(np.float64) - wrong_m) / ulp).max() > 4
        before = after


def test_train_steps_equal_the_single_calls_bit_for_bit(eng, dev, single):
    acts, params, stats = dev
    rows, labels, lr = _three_steps()
    for scratch in (None, 0xFF):
        check = lambda: None
        if scratch is not None:
            scratch, check = P.guarded(int(eng._lib.bq_exit_bn_workspace_bytes(2, L.BQ_DTYPE_F32, L.BQ_ACT_DEVICE)), scratch, eng.device)
        w, m, v, moving = params.clone(), torch.zeros_like(params), torch.zeros_like(params), stats.clone()
        losses = eng.exit_train_steps(w, m, v, moving, acts, up(eng, rows), up(eng, labels), 2, 0, 9, lr, rate=0.1, bn='batch', scratch=scratch)
        torch.cuda.synchronize(eng.device)
        check()
        assert losses.shape == (3,) and bool(torch.isfinite(losses).all())
        for a, b in zip((w, m, v, moving, losses), single[:5]):
            assert torch.equal(a, b)
    assert not torch.equal(moving, stats) and not torch.equal(w[:eng.EXIT_PARAMS], params[:eng.EXIT_PARAMS])


# ------------------------------------------------------------------------------------------------ 7. stores
def test_packed_and_host_caches_give_the_float32_caches_bits(eng, dev):
    _, params, _ = dev
    a16 = torch.from_numpy(X.cache()).to(torch.float16)
    mul = 2.0 ** -3
    a32 = a16.float() * mul
    pinned = lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)
    r, y = up(eng, np.array([4, 2], np.int64)), up(eng, np.array([0, 1], np.uint8))
    want = eng.exit_grad(params, None, a32.to(eng.device), r, y, 3, X.SEED, rate=0.1, bn='batch')
    assert bool(torch.isfinite(want[1]).all())
    for name, acts, m in (('packed', a16.to(eng.device), mul), ('host16', pinned(a16), mul), ('host32', pinned(a32), 1.0)):
        got = eng.exit_grad(params, None, acts, r, y, 3, X.SEED, rate=0.1, act_mul=m, bn='batch')
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
    assert {'exit_bn', 'exit_bn_staged'} <= set(eng._tool_ws)
    host = int(eng._lib.bq_exit_bn_workspace_bytes(2, L.BQ_DTYPE_F16, L.BQ_ACT_HOST))
    assert host == int(eng._lib.bq_exit_bn_workspace_bytes(2, L.BQ_DTYPE_F16, L.BQ_ACT_DEVICE)) + 2 * 204800 == eng.exit_bn_scratch(2, torch.float16).numel()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_sizes_and_refusals(eng, dev):
    """The refusals return their code and their text, and nothing is enqueued."""
    acts, params, stats = dev
    lib = eng._lib
    size = lambda n, t=0, wh=0: int(lib.bq_exit_bn_workspace_bytes(n, t, wh))
    assert size(0) == 0 == size(257) and size(2, 3) == 0 == size(2, -1) and size(2, 0, 2) == 0 == size(2, 0, -1)
    for n in (1, 4, 256):
        assert size(n) == int(lib.bq_exit_train_workspace_bytes(n)) + 7168 * 4 == size(n, 2)
        assert size(n, 2, 1) == int(lib.bq_exit_staged_workspace_bytes(n, 2)) + 7168 * 4
    rows, labels = up(eng, np.zeros(8, np.int64)), up(eng, np.zeros(8, np.uint8))
    w, m, v, g = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.full_like(params, 7.0)
    loss = torch.full((2,), 7.0, dtype=torch.float32, device=eng.device)
    bs = torch.full((7168 + 4,), 7.0, dtype=torch.float32, device=eng.device)
    moving = torch.cat([stats, stats[:4]])
    need = size(4)
    ws = eng.exit_bn_scratch(4)
    lr = (C.c_double * 2)(1e-3, 1e-3)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    cache = L.BqActCache(acts.data_ptr(), int(acts.shape[0]), L.BQ_DTYPE_F32, 1.0, L.BQ_ACT_DEVICE)

    def grad(code, text, n=4, s_off=0, nbytes=need):
        rc = lib.bq_exit_grad_bn(eng._ctx, vp(w), C.byref(cache), vp(rows), vp(labels), n, 0, 9, 0.1, vp(g), vp(loss), vp(bs, s_off), vp(ws),
                                 nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_exit_grad_bn: ' + text)

    def steps(code, text, batch=4, last_n=4, s_off=0, nbytes=need):
        rc = lib.bq_exit_train_steps_bn(eng._ctx, vp(w), vp(m), vp(v), vp(g), vp(moving, s_off), C.byref(cache), vp(rows), vp(labels), 2, batch,
                                        last_n, 0, 9, 0.1, lr, 0.9, 0.999, 1e-7, vp(loss), vp(ws), nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_exit_train_steps_bn: ' + text)

    pointers = 'bad argument (null pointer, params, stats, acts or an output not 16-byte, rows not 8-byte or the workspace not 256-byte aligned)'
    grad(-1, '1 <= n <= 256', n=0)
    grad(-1, '1 <= n <= 256', n=257)
    grad(-1, pointers, s_off=4)
    grad(-4, 'workspace below bq_exit_bn_workspace_bytes(n, type, where)', nbytes=need - 1)
    steps(-1, '1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step', batch=0, last_n=0)
    steps(-1, '1 <= n <= 256', batch=257, last_n=1)
    steps(-1, pointers, s_off=4)
    steps(-4, 'workspace below bq_exit_bn_workspace_bytes(batch, type, where)', nbytes=need - 1)
    for n in (0, 257):
        assert lib.bq_exit_bn_move(eng._ctx, vp(moving), vp(bs), n, eng._stream()) == -1
    assert lib.bq_exit_bn_move(eng._ctx, vp(moving, 4), vp(bs), 2, eng._stream()) == -1
    torch.cuda.synchronize(eng.device)
    assert torch.equal(w, params) and not m.any() and not v.any() and bool((g == 7.0).all()) and loss.tolist() == [7.0, 7.0]
    assert bool((bs == 7.0).all()) and torch.equal(moving[:7168], stats)
    with pytest.raises(ValueError, match='bn'):
        eng.exit_grad(params, stats, acts, rows[:2], labels[:2], 0, 9, bn='moving')
    with pytest.raises(ValueError, match='bn_stats'):
        eng.exit_grad(params, None, acts, rows[:2], labels[:2], 0, 9)


def test_a_nan_activation_a_row_outside_and_a_bad_label_give_a_nan_loss(eng, dev):
    acts, params, _ = dev
    rows, labels = CASES[3]
    y = up(eng, labels)
    loss = lambda a, r, lab: eng.exit_grad(params, None, a, up(eng, r), lab, 3, X.SEED, rate=0.1, bn='batch')[1]
    assert bool(torch.isfinite(loss(acts, rows, y)).all())
    assert bool(torch.isnan(loss(acts, np.where(np.arange(3) == 1, B.CACHE_ROWS, rows), y)).all())
    bad = acts.clone()
    bad[int(rows[0]), 9, 9, 1023] = float('inf')
    assert bool(torch.isnan(loss(bad, rows, y)).all())
    assert bool(torch.isnan(loss(acts, rows, up(eng, np.array([0, 2, 1], np.uint8)))).all())


def test_profiling_classes_of_a_training_mode_step(eng, dev):
    acts, params, stats = dev
    rows, labels = CASES[2]
    moving = stats.clone()
    eng.profile_enable(True)
    try:
        w = params.clone()
        eng.exit_train_steps(w, torch.zeros_like(w), torch.zeros_like(w), moving, acts, up(eng, rows), up(eng, labels), 2, 0, 9, [1e-3], bn='batch')
        prof = {p.name: p for p in eng.profile_read()}
    finally:
        eng.profile_enable(False)
    fwd = ('dw1', 'pw1', 'stat1', 'dw2', 'pw2', 'stat2', 'pool')                   # no coef class: the coefficients follow the statistics
    back = ('dfeat', 'bn2', 'bnfix2', 'dp2', 'du2', 'dd2', 'dh1', 'bn1', 'bnfix1', 'dp1', 'du1', 'dd1', 'adam', 'bnmove')
    head = ('fwd0', 'fwd1', 'logits', 'dx1', 'dw1', 'dw0', 'sums')
    want = {'exit_train_' + k for k in fwd + back} | {'head_train_' + k for k in head}
    assert set(prof) == want, set(prof) ^ want
    assert all(p.launches == 1 for p in prof.values())


# ------------------------------------------------------------------------------------------------ 9. end to end, toy
def _six_slides(tmp_path, per=16):
    paths, labels = [], {}
    for i in range(6):
        name = f's{i}'
        t = make_tiles(per, seed=70 + i, slide_bias=[(i % 2) * 40.0 - 20.0, 0.0, 0.0])
        loc = np.stack([np.arange(per) * 299 + 150, np.full(per, 150 + 1000 * i)], 1).astype(np.int64)
        paths.append(str(tmp_path / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
        labels[name] = i % 2
    return paths, labels


def test_toy_training_in_both_modes_end_to_end(eng, tmp_path):
    paths, labels = _six_slides(tmp_path)
    slides = lambda: inf.slides_from_tfrecords(paths, labels)
    cache = T.cache_activations(eng, slides(), batch=8)
    assert len(cache) == 96
    rows = np.arange(96)
    y = np.array([labels[cache.slides[i]] for i in cache.slide_idx], np.int64)
    imported = T.exit_bn_stats(eng.weights)

    # training mode: six steps of sixteen tiles
    params = T.TrainParams(batch_size=16, learning_rate=1e-4, epochs=[1], trainable='exit', bn='batch')
    fit = T.fit_head(eng, cache, rows, y, params=params, seed=5)
    assert fit.steps == 6 and np.isfinite(fit.losses).all()
    assert set(fit.exit) == {k for k, _ in T.EXIT_TENSORS + T.EXIT_STATS}
    T.save_exit(str(tmp_path / T.EXIT_FILE), fit.exit)
    back = T.load_exit(str(tmp_path / T.EXIT_FILE))
    assert all(np.array_equal(back[k], fit.exit[k]) for k in fit.exit)
    moved = T.exit_bn_stats(back)
    assert np.isfinite(moved).all() and not np.array_equal(moved, imported)
    for k, _ in T.EXIT_STATS:
        assert not np.array_equal(back[k], np.asarray(eng.weights[k], np.float32)), k
    assert bool((moved[1536:3072] > 0).all()) and bool((moved[5120:] > 0).all())      # variances stay variances
    fc = T.exit_feature_cache(eng, cache, back, rows)
    own = eng.exit_features_all(up(eng, T.flatten_exit(back)), up(eng, moved), cache.acts, up(eng, rows))
    assert torch.equal(fc.feats, own)                                                 # the result's statistics, not the engine's
    table = T.predict(eng, fc, rows, fit.head, mc_n=8, seed=3, y_true=labels)
    fresh = T.exit_engine(eng, back, fit.head)
    try:
        assert np.array_equal(T.exit_bn_stats(fresh.weights), moved)
        want = inf.evaluate(fresh, slides(), outcome='cohort', batch=8, mc_n=8, seed=3).tile_df
    finally:
        fresh.close()
    assert len(table) == 96 == len(want) and table['slide'].tolist() == want['slide'].tolist()
    for col in ('cohort-y_pred0', 'cohort-y_pred1', 'cohort-uncertainty0', 'cohort-uncertainty1'):
        d = float(np.abs(table[col].to_numpy() - want[col].to_numpy()).max())
        print(f'{col}: exit_engine off predict on exit_feature_cache by {d:.3e}')
        assert d <= 1e-3, (col, d)

    # frozen: what the code wrote before there were two modes -- the same calls, made here by hand
    frozen = T.fit_head(eng, cache, rows, y, params=T.TrainParams(batch_size=16, learning_rate=1e-4, epochs=[1], trainable='exit'), seed=5)
    at, lab = T._plan_epoch(params, cache, rows, y, None, None, 5, 0, {})
    stats = up(eng, imported)
    w = up(eng, np.concatenate([T.flatten_exit(eng.weights), T.flatten_head(eng.weights)]))
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    losses = eng.exit_train_steps(w, m, v, stats, cache.acts, up(eng, at), up(eng, lab), 16, 0, 5, [params.learning_rate_at(i) for i in range(6)],
                                  rate=params.dropout, b1=T.ADAM_BETA_1, b2=T.ADAM_BETA_2, eps=T.ADAM_EPSILON, act_mul=cache.act_mul)
    host = w.cpu().numpy()
    by_hand = T.unflatten_exit(host[:T.EXIT_PARAMS])
    assert set(frozen.exit) == {k for k, _ in T.EXIT_TENSORS} == set(by_hand)
    assert all(np.array_equal(frozen.exit[k], by_hand[k]) for k in by_hand) and np.array_equal(frozen.losses, losses.cpu().numpy())
    assert torch.equal(stats, up(eng, imported))
    T.save_exit(str(tmp_path / 'frozen.npz'), frozen.exit)
    with np.load(str(tmp_path / 'frozen.npz')) as z:
        assert sorted(z.files) == sorted(k for k, _ in T.EXIT_TENSORS)
    feats = cache.feats.clone()
    feats.index_copy_(0, up(eng, rows), eng.exit_features_all(up(eng, T.flatten_exit(by_hand)), stats, cache.acts, up(eng, rows)))
    hand_table = T.predict(eng, T.FeatureCache(feats, cache.slide_idx, cache.loc, cache.slides), rows, T.unflatten_head(host[T.EXIT_PARAMS:]),
                           mc_n=8, seed=3, y_true=labels)
    frozen_table = T.predict(eng, T.exit_feature_cache(eng, cache, frozen.exit, rows), rows, frozen.head, mc_n=8, seed=3, y_true=labels)
    assert frozen_table.equals(hand_table) and not frozen_table.equals(table)
