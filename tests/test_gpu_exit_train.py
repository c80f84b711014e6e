"""Exit-flow fine-tuning on the GPU (csrc/kernels_train.hip, biscuit_amd/train.py; DESIGN.md section 7 "Exit-flow fine-tuning")
against the float64 restatement of tests/_exit_train_ref.py: a cache of six half-normal ``block13_out`` tiles (one all zeros), the
stress set's block 14 with eight dead channels, ``_train_ref``'s head.  The spatial size and the channel counts are the network's
own; the small dimension is n in {1, 2, 3, 5}: 100 .. 500 rows of the pointwise products, no multiple of their 64-row tile, and
K = 100 n of dP no multiple of 32.  The gradient tolerance is 8 x the float32 twin's own distance from float64 for the same case.
``-m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from biscuit_amd import inference as inf
from biscuit_amd import tfrecord as tfr
from biscuit_amd import train as T
from biscuit_amd.synthetic import make_tiles
from tests import _exit_train_ref as X
from tests import _poison as P
from tests import _train_ref as R

pytestmark = pytest.mark.gpu


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
    """The reference's inputs on the device: ``(acts [6, 10, 10, 1024], params [P_ALL], bn_stats [7168])``."""
    x, e, w = X.inputs()
    vec, stats = X.flatten(e, w)
    assert vec.shape == (eng.ALL_PARAMS,) == (T.EXIT_PARAMS + T.HEAD_PARAMS,) and stats.shape == (eng.EXIT_BN_STATS,)
    assert (eng.EXIT_PARAMS, eng.EXIT_MAX_ROWS, eng.EXIT_ACT_SHAPE) == (T.EXIT_PARAMS, T.EXIT_MAX_ROWS, T.ACT_SHAPE)
    return up(eng, x), up(eng, vec), up(eng, stats)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).numpy()


# ------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize('n', X.GRAD_N)
def test_gradients_within_eight_twin_errors(eng, dev, n):
    acts, params, stats = dev
    x, e, w = X.inputs()
    for rate in X.GRAD_RATES:
        for kind in X.GRAD_LABELS:
            rows, labels, l64, g64, f64, twin = X.grad_reference(n, rate, kind)      # a case whose twin is off float64 in every figure
            g, loss = eng.exit_grad(params, stats, acts, up(eng, rows), up(eng, labels), 3, X.SEED, rate=rate)
            gd = X.split_grad(g.cpu().numpy(), e, w)
            err = {k: R.rel_err(gd[k], g64[k]) for k in X.EXIT + R.TENSORS}
            err['loss'] = R.rel_err(float(loss[0]), l64)
            err['feat'] = R.rel_err(eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, up(eng, rows)).cpu().numpy(), f64)
            for k, v in err.items():
                print(f'n={n} rate={rate} {kind} {k}: device {v:.3e} twin {twin[k]:.3e} ratio {v / twin[k]:.2f}')
            for k, v in err.items():
                assert v <= 8 * twin[k], (n, rate, kind, k, v, twin[k])
            assert (gd['gamma1'][-8:] == 0).all() and (gd['beta1'][-8:] == 0).all() and (gd['P1'][:, -8:] == 0).all()   # the dead channels
            assert (gd['D2'][:, :, -8:] == 0).all() and (gd['P2'][-8:] == 0).all()


def test_a_unit_at_zero_has_derivative_zero(eng, dev):
    """gamma = 0 and beta = 0 put a channel's unit at h = 0 exactly at every position (a = 0, b = beta: fma(0, z, 0)); ReLU's derivative
    there is 0 by definition, so dbeta and dgamma are 0 exactly.  With beta = 1e-30 the same unit is live and dbeta is not 0."""
    acts, _, stats = dev
    _, e, w = X.inputs()
    rows, labels = X.grad_case(2, 'mixed')
    assert 1 not in rows.tolist()                               # two tiles with content
    at = {'1': 5, '2': 7}

    def grad(beta):
        t = dict(e)
        for l, c in at.items():
            t['gamma' + l], t['beta' + l] = e['gamma' + l].copy(), e['beta' + l].copy()
            t['gamma' + l][c], t['beta' + l][c] = 0, beta
        g, loss = eng.exit_grad(up(eng, X.flatten(t, w)[0]), stats, acts, up(eng, rows), up(eng, labels), 3, X.SEED, rate=0.0)
        assert bool(torch.isfinite(loss).all())
        return X.split_grad(g.cpu().numpy(), e, w)
    zero, live = grad(np.float32(0)), grad(np.float32(1e-30))
    for l, c in at.items():
        assert zero['beta' + l][c] == 0 and zero['gamma' + l][c] == 0 and not zero['P' + l][:, c].any(), l
        assert live['beta' + l][c] != 0 and zero['beta' + l][c + 1] != 0, l


# ------------------------------------------------------------------------------------------------ 2. the head part is bq_head_grad's
@pytest.mark.parametrize('rate', X.GRAD_RATES)
def test_head_part_is_head_grad_on_exit_features_bit_for_bit(eng, dev, rate):
    acts, params, stats = dev
    for n in X.GRAD_N:
        rows, labels = X.grad_case(n, 'mixed')
        r, y = up(eng, rows), up(eng, labels)
        g, loss = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=rate)
        f = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r)
        table = torch.zeros((X.CACHE_ROWS, 2048), dtype=torch.float32, device=eng.device)
        table[r] = f                                            # a feature cache with the features at their rows (a tile twice: the same row twice)
        gh, lh = eng.head_grad(params[eng.EXIT_PARAMS:], table, r, y, 3, X.SEED, rate=rate)
        assert np.array_equal(bits(g[eng.EXIT_PARAMS:]), bits(gh)) and np.array_equal(bits(loss), bits(lh)), (n, rate)
        assert bool(torch.isfinite(loss).all()) and bool(g[:eng.EXIT_PARAMS].any())


# ------------------------------------------------------------------------------------------------ 3. a row depends on its tile only
def test_exit_features_do_not_depend_on_the_batch(eng, dev):
    acts, params, stats = dev
    e = params[:eng.EXIT_PARAMS]
    whole = eng.exit_features(e, stats, acts, up(eng, np.arange(5, dtype=np.int64)))
    for i in range(5):
        assert np.array_equal(bits(eng.exit_features(e, stats, acts, up(eng, np.array([i], np.int64)))[0]), bits(whole[i])), i
    a = eng.exit_features(e, stats, acts, up(eng, np.array([4, 0, 2], np.int64)))
    b = eng.exit_features(e, stats, acts, up(eng, np.array([3, 1], np.int64)))
    assert np.array_equal(bits(torch.stack([a[1], b[1], a[2], b[0], a[0]])), bits(whole))
    assert np.array_equal(bits(eng.exit_features_all(e, stats, acts, up(eng, np.arange(5, dtype=np.int64)))), bits(whole))
    assert bool(torch.isfinite(whole).all()) and bool((whole >= 0).all()) and bool(whole.any())


# ------------------------------------------------------------------------------------------------ 4. the same bits every time
def _three_steps():
    rng = np.random.default_rng(3)
    rows = np.concatenate([rng.permutation(X.CACHE_ROWS) for _ in range(2)])[:2 * 4 + 3].astype(np.int64)
    return rows, rng.integers(0, 2, len(rows)).astype(np.uint8), [1e-3 * 0.98 ** i for i in range(3)]


def _run_steps(eng, dev, scratch=None):
    acts, params, stats = dev
    rows, labels, lr = _three_steps()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    losses = eng.exit_train_steps(w, m, v, stats, acts, up(eng, rows), up(eng, labels), 4, 0, 9, lr, rate=0.1, scratch=scratch)
    assert losses.shape == (3,)
    return [t.cpu().numpy() for t in (w, m, v, losses)]


@pytest.fixture(scope='module')
def three(eng, dev):
    return _run_steps(eng, dev)


def test_train_steps_equal_the_single_calls_bit_for_bit(eng, dev, three):
    acts, params, stats = dev
    rows, labels, lr = _three_steps()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    losses = []
    for i in range(3):
        r, y = up(eng, rows[i * 4:(i + 1) * 4]), up(eng, labels[i * 4:(i + 1) * 4])
        assert r.numel() == (4 if i < 2 else 3)
        g, loss = eng.exit_grad(w, stats, acts, r, y, i, 9, rate=0.1)
        eng.adam_n(w, m, v, g, i, lr[i])
        losses.append(loss.cpu().numpy()[0])
    single = [w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), np.array(losses, np.float32)]
    for a, b in zip(three, single):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(three[3]).all() and not np.array_equal(three[0][:T.EXIT_PARAMS], params.cpu().numpy()[:T.EXIT_PARAMS])


def test_adam_n_is_head_adam_over_any_count(eng, dev):
    _, params, _ = dev
    head = params[eng.EXIT_PARAMS:]
    g = torch.sin(torch.arange(eng.HEAD_PARAMS, device=eng.device, dtype=torch.float32))
    a = [head.clone(), torch.zeros_like(head), torch.zeros_like(head)]
    b = [t.clone() for t in a]
    for step in (0, 7):
        eng.head_adam(*a, g, step, 1e-3)
        eng.adam_n(*b, g, step, 1e-3)
    assert all(np.array_equal(bits(s), bits(t)) for s, t in zip(a, b))
    short = [t[:1001].clone() for t in (head, torch.zeros_like(head), torch.zeros_like(head))]
    eng.adam_n(*short, g[:1001].clone(), 0, 1e-3)
    eng.adam_n(*short, g[:1001].clone(), 7, 1e-3)
    assert all(np.array_equal(bits(s), bits(t[:1001])) for s, t in zip(short, a))


def test_repeated_and_poisoned_workspace_same_bits_guards_intact(eng, dev, three):
    acts, params, stats = dev
    rows, labels = X.grad_case(3, 'mixed')
    r, y = up(eng, rows), up(eng, labels)
    g0, l0 = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=0.1)
    g0, l0 = bits(g0), bits(l0)
    g1, l1 = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=0.1)
    assert np.array_equal(bits(g1), g0) and np.array_equal(bits(l1), l0)
    need = int(eng._lib.bq_exit_train_workspace_bytes(3))
    need_f = int(eng._lib.bq_exit_features_workspace_bytes(3))
    f0 = bits(eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r))
    for fill in P.BYTE_FILLS:
        scratch, check = P.guarded(need, fill, eng.device)
        grad = torch.empty_like(params)
        P.fill_bytes(grad.view(torch.uint8), P.pattern(fill))
        g2, l2 = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=0.1, grad=grad, scratch=scratch)
        scratch_f, check_f = P.guarded(need_f, fill, eng.device)
        f2 = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r, scratch=scratch_f)
        torch.cuda.synchronize(eng.device)
        check()
        check_f()
        assert np.array_equal(bits(g2), g0) and np.array_equal(bits(l2), l0) and np.array_equal(bits(f2), f0), hex(fill)
    scratch, check = P.guarded(int(eng._lib.bq_exit_train_workspace_bytes(4)), 0xFF, eng.device)
    got = _run_steps(eng, dev, scratch=scratch)
    torch.cuda.synchronize(eng.device)
    check()
    for a, b in zip(three, got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert 'exit_train' in eng._tool_ws and 'exit_features' in eng._tool_ws and eng.exit_train_scratch(3).numel() == need


# ------------------------------------------------------------------------------------------------ 5. 64-bit offsets
def test_rows_past_the_32_bit_offsets(eng, dev):
    """A cache of 21 000 rows, 8.6 GB, allocated and not initialised: byte offsets pass 2^32 at row 10 486, element offsets 2^31 at
    row 20 972.  Rows 10 490 and 20 990 hold tiles 0 and 2 of the small cache: the gradient through them is the gradient through rows
    0 and 2 there, bit for bit (rate 0: the Philox counters, the rows, differ)."""
    acts, params, stats = dev
    free = torch.cuda.mem_get_info(eng.device)[0]
    if free < 12 << 30:
        pytest.skip(f'{free >> 30} GiB free on the device: the 8.6 GB cache of this test wants 12')
    big = torch.empty((21000,) + eng.EXIT_ACT_SHAPE, dtype=torch.float32, device=eng.device)
    try:
        assert 10490 * 409600 > 1 << 32 and 20990 * 102400 > 1 << 31
        big[10490], big[20990] = acts[0], acts[2]
        y = up(eng, np.array([0, 1], np.uint8))
        g0, l0 = eng.exit_grad(params, stats, acts, up(eng, np.array([0, 2], np.int64)), y, 3, X.SEED, rate=0.0)
        g1, l1 = eng.exit_grad(params, stats, big, up(eng, np.array([10490, 20990], np.int64)), y, 3, X.SEED, rate=0.0)
        assert np.array_equal(bits(g1), bits(g0)) and np.array_equal(bits(l1), bits(l0)) and bool(torch.isfinite(l1).all())
        e = params[:eng.EXIT_PARAMS]
        f0 = eng.exit_features(e, stats, acts, up(eng, np.array([2, 0], np.int64)))
        f1 = eng.exit_features(e, stats, big, up(eng, np.array([20990, 10490], np.int64)))
        assert np.array_equal(bits(f1), bits(f0))
    finally:
        del big


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_invalid_input_gives_a_nan_loss(eng, dev):
    acts, params, stats = dev
    rows, labels = X.grad_case(3, 'mixed')
    y = up(eng, labels)
    loss = lambda a, r, lab: eng.exit_grad(params, stats, a, up(eng, r), lab, 3, X.SEED, rate=0.1)[1]
    assert bool(torch.isfinite(loss(acts, rows, y)).all())
    for outside in (-1, X.CACHE_ROWS):                                      # never read: a NaN
        assert bool(torch.isnan(loss(acts, np.where(np.arange(3) == 1, outside, rows), y)).all()), outside
        f = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, up(eng, np.where(np.arange(3) == 1, outside, rows)))
        assert bool(torch.isnan(f[1]).all()) and bool(torch.isfinite(f[0]).all()) and bool(torch.isfinite(f[2]).all())
    for value in (float('nan'), float('inf'), float('-inf')):
        bad = acts.clone()
        bad[int(rows[0]), 9, 9, 1023] = value
        assert bool(torch.isnan(loss(bad, rows, y)).all()), value
        spare = next(t for t in range(X.CACHE_ROWS) if t not in set(rows.tolist()))
        bad = acts.clone()
        bad[spare, 0, 0, 0] = value                                         # a tile outside the batch: nothing changes
        assert torch.equal(loss(bad, rows, y), loss(acts, rows, y))
    assert bool(torch.isnan(loss(acts, rows, up(eng, np.array([0, 2, 1], np.uint8)))).all())
    with pytest.raises(ValueError):
        eng.exit_grad(params, stats, acts, up(eng, rows).int(), y, 3, X.SEED)
    with pytest.raises(ValueError):
        eng.exit_grad(params[:-1], stats, acts, up(eng, rows), y, 3, X.SEED)
    with pytest.raises(ValueError):
        eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts.reshape(-1, 100, 1024), up(eng, rows))
    with pytest.raises(ValueError):
        eng.exit_grad(params, stats, acts, up(eng, np.zeros(257, np.int64)), up(eng, np.zeros(257, np.uint8)), 3, X.SEED)


def test_sizes_and_refusals(eng, dev):
    """Every branch of the entries' argument checks refuses with its code and its text; nothing is enqueued."""
    acts, params, stats = dev
    lib = eng._lib
    assert lib.bq_exit_train_workspace_bytes(0) == 0 == lib.bq_exit_train_workspace_bytes(257) and lib.bq_exit_train_workspace_bytes(256) > 0
    assert lib.bq_exit_features_workspace_bytes(0) == 0 == lib.bq_exit_features_workspace_bytes(257)
    al = lambda b: (b + 255) & ~255
    for n in (1, 3, 256):
        fwd = 3 * al(1536 * 4) + 3 * al(2048 * 4) + al(n * 100 * 1024 * 4) + 2 * al(n * 100 * 1536 * 4) + al(n * 100 * 2048 * 4) + al(n * 2048 * 4)
        assert lib.bq_exit_features_workspace_bytes(n) == fwd, n
        back = al(n * 2048 * 4) + al(n * 100 * 2048 * 4) + 2 * al(n * 100 * 1536 * 4) + al(n * 9 * 1536 * 4)
        assert lib.bq_exit_train_workspace_bytes(n) == fwd + back + lib.bq_head_train_workspace_bytes(n), n
    rows, labels = up(eng, np.zeros(8, np.int64)), up(eng, np.zeros(8, np.uint8))
    w, m, v, g = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.full_like(params, 7.0)
    loss = torch.full((2,), 7.0, dtype=torch.float32, device=eng.device)
    feat = torch.full((4, 2048), 7.0, dtype=torch.float32, device=eng.device)
    need, need_f = int(lib.bq_exit_train_workspace_bytes(4)), int(lib.bq_exit_features_workspace_bytes(4))
    ws = eng.exit_train_scratch(4)
    lr = (C.c_double * 2)(1e-3, 1e-3)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def grad(code, text, w_off=0, n_act=6, n=4, step=0, rate=0.1, nbytes=need):
        rc = lib.bq_exit_grad(eng._ctx, vp(w, w_off), vp(stats), vp(acts), n_act, vp(rows), vp(labels), n, step, 9, rate, vp(g), vp(loss), vp(ws),
                              nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_exit_grad: ' + text)

    def features(code, text, w_off=0, n_act=6, n=4, nbytes=need_f):
        rc = lib.bq_exit_features(eng._ctx, vp(w, w_off), vp(stats), vp(acts), n_act, vp(rows), n, vp(feat), vp(ws), nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_exit_features: ' + text)

    def steps(code, text, w_off=0, steps=2, batch=4, last_n=4, step0=0, rate=0.1, b1=0.9, nbytes=need):
        rc = lib.bq_exit_train_steps(eng._ctx, vp(w, w_off), vp(m), vp(v), vp(g), vp(stats), vp(acts), 6, vp(rows), vp(labels), steps, batch,
                                     last_n, step0, 9, rate, lr, b1, 0.999, 1e-7, vp(loss), vp(ws), nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_exit_train_steps: ' + text)

    def adam(code, text, count=eng.ALL_PARAMS, w_off=0, step=0, b1=0.9):
        rc = lib.bq_adam_n(eng._ctx, vp(w, w_off), vp(m), vp(v), vp(g), count, step, 1e-3, b1, 0.999, 1e-7, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_adam_n: ' + text)

    pointers = 'bad argument (null pointer, params, stats, acts or an output not 16-byte, rows not 8-byte or the workspace not 256-byte aligned)'
    values = 'a step outside 0 .. 2^32 - 1, or a rate outside [0, 1)'
    adam_values = 'a step outside 0 .. 2^32 - 1, a learning rate that is not finite, b1 or b2 outside [0, 1), or eps <= 0'
    for call in (grad, features):
        call(-1, '1 <= n <= 256', n=0)
        call(-1, '1 <= n <= 256', n=257)
        call(-1, 'an empty activation cache', n_act=0)
        call(-1, pointers, w_off=4)
    grad(-1, values, step=1 << 32)
    grad(-1, values, rate=1.0)
    grad(-4, 'workspace below bq_exit_train_workspace_bytes(n)', nbytes=need - 1)
    features(-4, 'workspace below bq_exit_features_workspace_bytes(n)', nbytes=need_f - 1)
    steps(-1, '1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step', steps=0)
    steps(-1, '1 <= steps <= 2^24, 1 <= last_n <= batch and a learning rate per step', last_n=5)
    steps(-1, '1 <= n <= 256', batch=257, last_n=1)
    steps(-1, values, rate=1.0)
    steps(-1, 'the steps pass 2^32', step0=(1 << 32) - 1)
    steps(-1, pointers, w_off=4)
    steps(-1, adam_values, b1=1.0)
    steps(-4, 'workspace below bq_exit_train_workspace_bytes(batch)', nbytes=need - 1)
    adam(-1, '1 <= count <= 256 (2^32 - 1)', count=0)
    adam(-1, 'bad argument (null or misaligned pointer)', w_off=2)
    adam(-1, adam_values, step=1 << 32)
    torch.cuda.synchronize(eng.device)
    assert torch.equal(w, params) and not m.any() and not v.any() and bool((g == 7.0).all()) and loss.tolist() == [7.0, 7.0]
    assert bool((feat == 7.0).all())


def test_profiling_classes_and_their_flop_counts(eng, dev):
    """One gradient opens exactly its own classes and the head's seven, and the products' classes carry a GEMM's flop count.  The
    counts are the launch code's constants: they say which class a launch is filed under, not which kernel ran.  That the products
    and their transposes (``A_MAT_K`` / ``A_MAT_T`` of ``train_gemm_kernel``) compute the right thing is held by the accuracy test
    above, tensor by tensor, and for ``fwd0`` / ``dw0`` by the bit-for-bit test against ``bq_head_grad``."""
    acts, params, stats = dev
    rows, labels = X.grad_case(2, 'mixed')
    eng.profile_enable(True)
    try:
        eng.exit_grad(params, stats, acts, up(eng, rows), up(eng, labels), 3, X.SEED, rate=0.1)
        eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, up(eng, rows))
        prof = {p.name: p for p in eng.profile_read()}
    finally:
        eng.profile_enable(False)
    fwd = ('coef', 'dw1', 'pw1', 'dw2', 'pw2', 'pool')
    back = ('dfeat', 'bn2', 'dp2', 'du2', 'dd2', 'dh1', 'bn1', 'dp1', 'du1', 'dd1')
    head = ('fwd0', 'fwd1', 'logits', 'dx1', 'dw1', 'dw0', 'sums')
    want = {'exit_train_' + k for k in fwd + back} | {'exit_feat_' + k for k in fwd} | {'head_train_' + k for k in head}
    assert set(prof) == want, set(prof) ^ want
    assert all(p.launches == 1 for p in prof.values())
    M = 200.0
    for k, flops in (('pw1', 2 * M * 1024 * 1536), ('pw2', 2 * M * 1536 * 2048), ('dp1', 2 * M * 1024 * 1536), ('du1', 2 * M * 1024 * 1536),
                     ('dp2', 2 * M * 1536 * 2048), ('du2', 2 * M * 1536 * 2048), ('dfeat', 2 * 2.0 * 2048 * 1024)):
        assert prof['exit_train_' + k].flops == flops, k


# ------------------------------------------------------------------------------------------------ 7. the trunk joins the network
def _two_slides(tmp_path, per=3):
    paths = []
    for i, name in enumerate(('a', 'b')):
        t = make_tiles(per, seed=60 + i, slide_bias=[i * 40.0 - 20.0, 0.0, 0.0])
        loc = np.stack([np.arange(per) * 299 + 150, np.full(per, 150 + 1000 * i)], 1).astype(np.int64)
        paths.append(str(tmp_path / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
    return paths, {'a': 0, 'b': 1}


def test_trunk_exit_features_and_head_give_evaluates_tile_predictions(eng, tmp_path):
    paths, labels = _two_slides(tmp_path)
    cache = T.cache_activations(eng, inf.slides_from_tfrecords(paths, labels), batch=4)
    assert isinstance(cache, T.FeatureCache) and len(cache) == 6 and tuple(cache.acts.shape) == (6, 10, 10, 1024) and cache.acts.is_cuda
    assert tuple(cache.feats.shape) == (6, 2048) and cache.act_views is None and cache.views is None
    table = T.predict(eng, cache, np.arange(6), None, mc_n=8, seed=3, y_true=labels)
    want = inf.evaluate(eng, inf.slides_from_tfrecords(paths, labels), outcome='cohort', batch=16, mc_n=8, seed=3).tile_df
    assert len(table) == 6 == len(want) and table['slide'].tolist() == want['slide'].tolist()
    for col in ('cohort-y_pred0', 'cohort-y_pred1', 'cohort-uncertainty0', 'cohort-uncertainty1'):
        d = float(np.abs(table[col].to_numpy() - want[col].to_numpy()).max())
        print(f'{col}: trunk + exit_features + mc_head off evaluate() by {d:.3e}')
        assert d <= 1e-3, (col, d)
    # the cached tensor is the debug tap's, at true scale
    tiles = up(eng, make_tiles(3, seed=64))
    assert torch.equal(eng.trunk(tiles), eng.debug_activation_u8('block13_out', tiles, (10, 10, 1024)))
    path = str(tmp_path / 'acts.npz')
    cache.save(path)
    back = T.ActivationCache.load(path, eng.device)
    assert torch.equal(back.acts, cache.acts) and torch.equal(back.feats, cache.feats)


@pytest.mark.parametrize('k', (3, -2))
def test_trunk_removes_the_activation_exponent(eng, k):
    """An f16 engine that stores ``block13_out`` with exponent k (``act/trunk_mul`` = 2^k in its blob, as every calibrated engine
    has): ``trunk`` is the stored tensor times 2^k exactly, the debug tap's at true scale, and the network's values -- those of the
    engine without exponents up to what f16 rounds differently (the exponent moves no significand: nothing, away from the subnormals)."""
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import TRUNK_TENSOR
    tiles = up(eng, make_tiles(2, seed=64))
    want = eng.trunk(tiles)
    assert not eng.act_exp.get(TRUNK_TENSOR, 0)
    scaled = Engine(eng.weights, dtype='f16', max_batch=2, max_mc=2, act_exp={TRUNK_TENSOR: k})
    try:
        assert scaled.act_exp == {TRUNK_TENSOR: k}
        got = scaled.trunk(tiles)
        stored = scaled.debug_activation_u8(TRUNK_TENSOR, tiles, (10, 10, 1024), true_scale=False)
        assert torch.equal(got, stored * 2.0 ** k) and torch.equal(got, scaled.debug_activation_u8(TRUNK_TENSOR, tiles, (10, 10, 1024)))
    finally:
        scaled.close()
    top = float(want.abs().max())
    d = float((got - want).abs().max())
    print(f'k={k}: trunk off the engine without exponents by {d:.3e} of a peak of {top:.3e}')
    assert top > 0 and d <= 2.0 ** -10 * top


def test_exit_features_on_an_f32_engine_against_float64(tmp_path):
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    eng = Engine(w, dtype='f32', max_batch=2, max_mc=2)
    try:
        x = eng.trunk(up(eng, make_tiles(2, seed=61)))
        e = up(eng, T.flatten_exit(w))
        stats = up(eng, T.exit_bn_stats(w))
        f = eng.exit_features(e, stats, x, up(eng, np.arange(2, dtype=np.int64))).cpu().numpy()
        want = eng.backbone_u8(up(eng, make_tiles(2, seed=61))).cpu().numpy()
    finally:
        eng.close()
    xh = x.cpu().numpy()
    f64, _ = X.forward(xh, X.from_keras(w), np.float64)
    f32, _ = X.forward(xh, X.from_keras(w), np.float32)
    twin, mine = R.rel_err(f32, f64), R.rel_err(f, f64)
    print(f'exit_features on the f32 trunk: device {mine:.3e} twin {twin:.3e} ratio {mine / twin:.2f}; off the f32 backbone by {R.rel_err(f, want):.3e}')
    assert np.isfinite(xh).all() and xh.any() and mine <= 8 * twin
    assert R.rel_err(f, want) <= 1e-4                          # the engine's own block 14 (other kernels, folded BN) on the same tensor


# ------------------------------------------------------------------------------------------------ 8. toy training
def test_toy_training_follows_float64_and_packs_into_an_engine():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    x, e, w = X.inputs()
    rng = np.random.default_rng(21)
    acts = x.copy()
    acts[1] = np.abs(rng.standard_normal(acts[1].shape)).astype(np.float32)
    # The classes differ in mean, by a lot: at this rate each of twelve Adam steps moves all 7.9 M parameters by about 1e-3, every
    # pre-activation by about 1, and the losses jump between 0 and 3.4 on the way; only a coarse problem is learnt by step 12
    # (float64: first loss 0.613, last four 0.317 in the mean).
    acts[3:] += np.float32(3.0) * (np.arange(1024) % 2 == 0)
    y = (np.arange(6) >= 3).astype(np.uint8)
    idx = np.concatenate([np.random.default_rng([4, k]).permutation(6) for k in range(8)])[:48]
    lr = [1e-3] * 12
    _, _, l64 = X.train_steps(acts, idx, y[idx], e, w, 4, 9, 0.1, lr)
    _, _, l32 = X.train_steps(acts, idx, y[idx], e, w, 4, 9, 0.1, lr, dtype=np.float32)
    weights = synthetic_weights(1, hard=True)
    eng = Engine(weights, dtype='f16', max_batch=8, max_mc=4)
    try:
        vec, stats = X.flatten(e, w)
        assert np.array_equal(stats, T.exit_bn_stats(weights))
        p, stats = up(eng, vec), up(eng, stats)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        dev = eng.exit_train_steps(p, m, v, stats, up(eng, acts), up(eng, idx), up(eng, y[idx]), 4, 0, 9, lr, rate=0.1).cpu().numpy().astype(np.float64)
        twin = abs(l32[-4:].astype(np.float64).mean() - l64[-4:].mean())
        mine = abs(dev[-4:].mean() - l64[-4:].mean())
        print(f'last-4 mean loss: float64 {l64[-4:].mean():.6e}, device off by {mine:.3e}, float32 twin off by {twin:.3e}; first {dev[0]:.4f}')
        assert mine <= 8 * twin and dev[-4:].mean() < dev[0]
        # the trained block 14 and head as an engine of their own
        host = p.cpu().numpy()
        trained, head = T.unflatten_exit(host[:T.EXIT_PARAMS]), T.unflatten_head(host[T.EXIT_PARAMS:])
        tiles = up(eng, make_tiles(4, seed=62))
        fresh = T.exit_engine(eng, trained, head, tiles=tiles)
        try:
            assert fresh.act_exp == eng.act_exp and fresh.dtype == 'f16'
            got_mean, got_std = fresh.mc_infer(tiles, 4, 3)
            f = eng.exit_features(p[:T.EXIT_PARAMS], stats, eng.trunk(tiles), up(eng, np.arange(4, dtype=np.int64)))
            want_mean, want_std = fresh.mc_head(f, 4, 3)
            d = max(float((got_mean - want_mean).abs().max()), float((got_std - want_std).abs().max()))
            print(f'exit_engine off exit_features + head by {d:.3e}')
            assert d <= 1e-3
            assert not torch.equal(got_mean, eng.mc_infer(tiles, 4, 3)[0])
        finally:
            fresh.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 9. trainable='head' is what it was
def test_head_training_reads_an_activation_cache_as_a_feature_cache(eng, tmp_path):
    rng = np.random.default_rng(12)
    slides = [f's{i:02d}' for i in range(6)]
    labels = {s: i % 2 for i, s in enumerate(slides)}
    f = np.abs(rng.standard_normal((24, 2048))).astype(np.float32)
    sidx = np.repeat(np.arange(6), 4).astype(np.int64)
    f[sidx % 2 == 1] += np.float32(0.04) * (np.arange(2048) % 2 == 0)
    loc = np.stack([np.arange(24), np.zeros(24, np.int64)], 1).astype(np.int64)
    plain = T.FeatureCache(up(eng, f), sidx, loc, slides)
    acts = torch.rand((24, 10, 10, 1024), dtype=torch.float32, device=eng.device)
    standing_in = T.ActivationCache(up(eng, f), sidx, loc, slides, acts=acts)
    params = T.TrainParams(batch_size=8, learning_rate=1e-4, epochs=[2])
    assert params.trainable == 'head'
    fits = [T.fit_head(eng, c, np.arange(24), sidx % 2, init='glorot', params=params, seed=5) for c in (plain, standing_in)]
    assert fits[0].exit is None and fits[1].exit is None and np.array_equal(fits[0].losses.view(np.uint32), fits[1].losses.view(np.uint32))
    assert all(np.array_equal(fits[0].head[k], fits[1].head[k]) for k in R.TENSORS)
    outs = []
    for name, c in (('plain', plain), ('acts', standing_in)):
        trainer = T.HeadTrainer(eng, c, labels, params=params, init='glorot', mc_n=4)
        outs.append(T.train_cv(c, labels, str(tmp_path / name), 'EXP', 3, trainer, seed=2))
    for a, b in zip(*outs):
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and T.EXIT_FILE not in os.listdir(b) and T.HEAD_FILE in os.listdir(b)
        for name in os.listdir(a):
            with open(os.path.join(a, name), 'rb') as fa, open(os.path.join(b, name), 'rb') as fb:
                assert fa.read() == fb.read(), name


def test_exit_training_through_fit_head_and_train_cv(eng, tmp_path):
    """``trainable='exit'`` end to end at toy size: the folds' tables, ``head.npz`` and ``exit.npz``; validation checks through
    ``exit_validate``; the prediction reads the trained block 14's features."""
    paths, labels = _two_slides(tmp_path, per=4)
    cache = T.cache_activations(eng, inf.slides_from_tfrecords(paths, labels), batch=4, augment='xy', views=2, seed=1)
    assert tuple(cache.act_views.shape) == (2, 8, 10, 10, 1024) and tuple(cache.views.shape) == (2, 8, 2048)
    params = T.TrainParams(batch_size=4, learning_rate=1e-4, epochs=[2], trainable='exit', validate_on_batch=1, validation_steps=1)
    rows, y = np.arange(8), (np.arange(8) >= 4).astype(np.int64)
    fit = T.fit_head(eng, cache, rows, y, val_rows=rows, val_labels=y, params=params, seed=5)
    assert fit.steps == 4 and len(fit.checks) == 4 and np.isfinite(fit.losses).all() and all(np.isfinite(c[1]) and 0 <= c[2] <= 1 for c in fit.checks)
    assert set(fit.exit) == {k for k, _ in T.EXIT_TENSORS}
    assert not np.array_equal(fit.exit['block14_sepconv2/pointwise_kernel'], np.asarray(eng.weights['block14_sepconv2/pointwise_kernel'], np.float32))
    assert not np.array_equal(fit.exit['block14_sepconv1_bn/gamma'], np.asarray(eng.weights['block14_sepconv1_bn/gamma'], np.float32))
    # the first check's loss is exit_validate's, which is head_validate on exit_features
    fit2 = T.fit_head(eng, cache, rows, y, val_rows=rows, val_labels=y, params=params, seed=5)
    assert np.array_equal(fit.losses.view(np.uint32), fit2.losses.view(np.uint32)) and fit.checks == fit2.checks
    moved = T.exit_feature_cache(eng, cache, fit.exit, np.array([1, 6]))
    same = torch.ones(8, dtype=torch.bool)
    same[[1, 6]] = False
    assert torch.equal(moved.feats[same], cache.feats[same]) and not torch.equal(moved.feats[~same], cache.feats[~same])
    with pytest.raises(ValueError, match='ActivationCache'):
        T.fit_head(eng, T.FeatureCache(cache.feats, cache.slide_idx, cache.loc, cache.slides), rows, y, params=params, seed=5)

    # four "slides" out of the two files' tiles: two per class for a 2-fold
    four =T.ActivationCache(cache.feats, np.repeat(np.arange(4), 2).astype(np.int64), cache.loc, ['a0', 'a1', 'b0', 'b1'], cache.views, 'xy', 1,
                             acts=cache.acts, act_views=cache.act_views)
    lab = {'a0': 0, 'a1': 0, 'b0': 1, 'b1': 1}
    trainer = T.HeadTrainer(eng, four, lab, params=params, mc_n=4)
    dirs = T.train_cv(four, lab, str(tmp_path / 'cv'), 'EXP', 2, trainer, seed=2)
    for d in dirs:
        assert {T.HEAD_FILE, T.EXIT_FILE, T.MANIFEST_FILE, T.RESULTS_FILE} <= set(os.listdir(d))
        assert T.load_exit(os.path.join(d, T.EXIT_FILE))['block14_sepconv1/depthwise_kernel'].shape == (3, 3, 1024, 1)
