"""The activation cache's stores on the GPU (csrc/kernels_train.hip, biscuit_amd/train.py; DESIGN.md section 7 "Exit-flow
fine-tuning", Sizes): the engine's own 16-bit tensor on the device (``packed``) and either form in pinned host memory, gathered per
step (``host``), against the float32 device cache of the same numbers.  The 16-bit cache is made first and the float32 one derived
from it, ``a16.float() * mul``, so both hold the same values by construction and every comparison is bit equality: there is no
tolerance in this file.  The kernels' shapes are fixed at 10 x 10 x 1024; the small dimension is the row count.  ``-m gpu``."""
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

pytestmark = pytest.mark.gpu

TORCH = {'f16': torch.float16, 'bf16': torch.bfloat16}
MULS = (1.0, 2.0 ** -3, 2.0 ** 5)
STORES = ('packed', 'host16', 'host32')
ROW16, ROW32 = 204800, 409600


@pytest.fixture(scope='module')
def engines():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    made = {d: Engine(synthetic_weights(1), dtype=d, max_batch=8, max_mc=4) for d in ('f16', 'bf16')}
    yield made
    for e in made.values():
        e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def pinned(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)


def bits(t):
    return t.detach().cpu().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def same(a, b):
    return all(np.array_equal(bits(s), bits(t)) for s, t in zip(a, b)) if isinstance(a, (tuple, list)) else np.array_equal(bits(a), bits(b))


def host16(dtype):
    """The 16-bit test cache on the host, [6, 10, 10, 1024]: ``_exit_train_ref.cache()`` rounded to ``dtype`` (tile 1 all zeros), and in
    tile 4 the type's extremes: the largest finite values of either sign (f16's +-65504; bfloat16's neighbour below, +-65280), f16's
    smallest subnormal 2^-24 (a normal bfloat16) and both zeros."""
    a = torch.from_numpy(X.cache()).to(TORCH[dtype])
    top = 65504.0 if dtype == 'f16' else 65280.0
    a[4, 0, 0, :6] = torch.tensor([top, -top, 2.0 ** -24, -2.0 ** -24, 0.0, -0.0]).to(TORCH[dtype])
    a[4, 9, 9, 1020:] = torch.tensor([-top, 2.0 ** -24, -0.0, top]).to(TORCH[dtype])
    assert float(a.float().abs().max()) == top and bool((a.float() == 2.0 ** -24).any()) and bool(torch.signbit(a[4, 0, 0, 5]))
    return a


_CACHES = {}


def caches(eng, dtype, mul):
    """{store: (acts, act_mul)} of one type and one mul, made once: 'f32' the derived float32 device cache (the reference), 'packed'
    the 16-bit tensor on the device, 'host16' the same in pinned host memory, 'host32' the derived float32 one there."""
    key = (dtype, mul)
    if key not in _CACHES:
        a16 = host16(dtype)
        a32 = a16.float() * mul
        assert bool(torch.isfinite(a32).all())
        _CACHES[key] = {'f32': (a32.to(eng.device), 1.0), 'packed': (a16.to(eng.device), mul), 'host16': (pinned(a16), mul),
                        'host32': (pinned(a32), 1.0)}
    return _CACHES[key]


@pytest.fixture(scope='module')
def model(engines):
    """``(params [P_ALL], bn_stats [7168])`` of the reference on the device (both engines share device 0)."""
    _, e, w = X.inputs()
    vec, stats = X.flatten(e, w)
    eng = engines['f16']
    return up(eng, vec), up(eng, stats)


# ------------------------------------------------------------------------------------------------ 1. the trunk
def _check_packed_trunk(eng, tiles, k):
    t16, mul = eng.trunk(tiles, packed=True)
    assert mul == 2.0 ** k and t16.dtype == eng._elt and tuple(t16.shape) == (3, 10, 10, 1024) and t16.is_contiguous()
    want = eng.trunk(tiles)
    assert torch.equal(t16.float() * mul, want) and same(t16.float() * mul, want) and bool(want.any())


@pytest.mark.parametrize('dtype', ('f16', 'bf16'))
def test_packed_trunk_is_the_trunk_unwidened(engines, dtype):
    eng = engines[dtype]
    _check_packed_trunk(eng, up(eng, make_tiles(3, seed=64)), 0)


@pytest.mark.parametrize('k', (3, -2))
def test_packed_trunk_returns_the_activation_exponent(engines, k):
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import TRUNK_TENSOR
    eng = engines['f16']
    scaled = Engine(eng.weights, dtype='f16', max_batch=3, max_mc=2, act_exp={TRUNK_TENSOR: k})
    try:
        assert scaled.act_exp == {TRUNK_TENSOR: k}
        _check_packed_trunk(scaled, up(eng, make_tiles(3, seed=64)), k)
    finally:
        scaled.close()


def test_packed_trunk_is_refused_on_an_f32_engine(engines):
    from biscuit_amd.engine import Engine
    eng = Engine(engines['f16'].weights, dtype='f32', max_batch=2, max_mc=2)
    try:
        tiles = up(eng, make_tiles(2, seed=64))
        with pytest.raises(ValueError, match='lossless'):
            eng.trunk(tiles, packed=True)
        out = torch.zeros((2, 10, 10, 1024), dtype=torch.float16, device=eng.device)
        import ctypes as C
        mul = C.c_float(0.0)
        ws = eng._ws_for(2, 1)
        rc = eng._lib.bq_trunk_u8_packed(eng._ctx, C.c_void_p(tiles.data_ptr()), 2, C.c_void_p(out.data_ptr()), C.byref(mul),
                                         C.c_void_p(ws.data_ptr()), ws.numel(), eng._stream())
        assert rc == -1 and 'lossless' in eng._lib.bq_last_error(eng._ctx).decode()
        torch.cuda.synchronize(eng.device)
        assert not bool(out.any())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. bit identity
def _three_steps():
    rng = np.random.default_rng(3)
    rows = np.concatenate([rng.permutation(X.CACHE_ROWS) for _ in range(2)])[:3 + 3 + 2].astype(np.int64)
    return rows, rng.integers(0, 2, len(rows)).astype(np.uint8), [1e-3 * 0.98 ** i for i in range(3)]


def _calls(eng, model, acts, mul, n, rate):
    """Every call of the cache at one case -> a flat list of device tensors."""
    params, stats = model
    rows, labels = X.grad_case(n, 'mixed')
    r, y = up(eng, rows), up(eng, labels)
    f = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r, act_mul=mul)
    g, loss = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=rate, act_mul=mul)
    vstats, vloss, vhit = eng.exit_validate(params, stats, acts, r, y, 3, X.SEED, rowloss=True, hit=True, act_mul=mul)
    return [f, g, loss, vstats, vloss, vhit]


def _steps(eng, model, acts, mul, rate, scratch=None):
    params, stats = model
    rows, labels, lr = _three_steps()
    w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    losses = eng.exit_train_steps(w, m, v, stats, acts, up(eng, rows), up(eng, labels), 3, 0, 9, lr, rate=rate, act_mul=mul, scratch=scratch)
    assert losses.shape == (3,)
    return [w, m, v, losses]


@pytest.mark.parametrize('mul', MULS)
@pytest.mark.parametrize('dtype', ('f16', 'bf16'))
def test_every_store_gives_the_float32_caches_bits(engines, model, dtype, mul):
    eng = engines[dtype]
    c = caches(eng, dtype, mul)
    for rate in (0.0, 0.1):
        for n in (1, 3, 5):
            want = _calls(eng, model, *c['f32'], n, rate)
            assert all(bool(torch.isfinite(t).all()) for t in want), (n, rate)
            for store in STORES:
                assert same(_calls(eng, model, *c[store], n, rate), want), (store, n, rate)
        want = _steps(eng, model, *c['f32'], rate)
        assert bool(torch.isfinite(want[3]).all()) and not torch.equal(want[0], model[0])
        for store in STORES:
            assert same(_steps(eng, model, *c[store], rate), want), (store, rate)


# ------------------------------------------------------------------------------------------------ 3. the NaN rules
def _with(acts, at, value):
    """``acts`` with ``value`` at index ``at``, in the same place (a pinned copy of a pinned tensor)."""
    bad = acts.clone() if acts.is_cuda else pinned(acts)
    bad[at] = value
    return bad


@pytest.mark.parametrize('store', STORES)
@pytest.mark.parametrize('dtype', ('f16', 'bf16'))
def test_the_nan_rules_hold_in_every_store(engines, model, dtype, store):
    eng = engines[dtype]
    params, stats = model
    acts, mul = caches(eng, dtype, 2.0 ** -3)[store]
    rows, labels = X.grad_case(3, 'mixed')
    y = up(eng, labels)
    loss = lambda a, r: eng.exit_grad(params, stats, a, up(eng, r), y, 3, X.SEED, rate=0.1, act_mul=mul)[1]
    base = loss(acts, rows)
    assert bool(torch.isfinite(base).all())
    for outside in (-1, X.CACHE_ROWS):                                      # never read: a NaN
        r = np.where(np.arange(3) == 1, outside, rows)
        assert bool(torch.isnan(loss(acts, r)).all()), outside
        f = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, up(eng, r), act_mul=mul)
        assert bool(torch.isnan(f[1]).all()) and bool(torch.isfinite(f[0]).all()) and bool(torch.isfinite(f[2]).all())
    spare = next(t for t in range(X.CACHE_ROWS) if t not in set(rows.tolist()))
    for value in (float('nan'), float('inf'), float('-inf')):
        assert bool(torch.isnan(loss(_with(acts, (int(rows[0]), 9, 9, 1023), value), rows)).all()), value
        assert torch.equal(loss(_with(acts, (spare, 0, 0, 0), value), rows), base), value        # a tile outside the batch: nothing changes


# ------------------------------------------------------------------------------------------------ 4. 64-bit offsets
def _through_far_rows(eng, model, small, big, mul, far):
    """The gradient and the features through ``big``'s rows ``far``, which hold tiles 0 and 2 of ``small``, are those through rows 0
    and 2 there (rate 0: the Philox counters, the rows, differ)."""
    params, stats = model
    y = up(eng, np.array([0, 1], np.uint8))
    near = up(eng, np.array([0, 2], np.int64))
    g0, l0 = eng.exit_grad(params, stats, small, near, y, 3, X.SEED, rate=0.0, act_mul=mul)
    g1, l1 = eng.exit_grad(params, stats, big, up(eng, np.array(far, np.int64)), y, 3, X.SEED, rate=0.0, act_mul=mul)
    assert same((g1, l1), (g0, l0)) and bool(torch.isfinite(l1).all())
    e = params[:eng.EXIT_PARAMS]
    f0 = eng.exit_features(e, stats, small, near.flip(0).contiguous(), act_mul=mul)
    f1 = eng.exit_features(e, stats, big, up(eng, np.array(far[::-1], np.int64)), act_mul=mul)
    assert same(f1, f0)


def test_packed_rows_past_the_32_bit_offsets(engines, model):
    """A packed cache of 21 000 rows, 4.3 GB, allocated and not initialised: a row is 102 400 elements and 204 800 bytes, so element
    offsets pass 2^31 and byte offsets 2^32 at row 20 972."""
    eng = engines['f16']
    free = torch.cuda.mem_get_info(eng.device)[0]
    if free < 6 << 30:
        pytest.skip(f'{free >> 30} GiB free on the device: the 4.3 GB cache of this test wants 6')
    small, mul = caches(eng, 'f16', 2.0 ** -3)['packed']
    assert 20971 * 102400 < 1 << 31 <= 20972 * 102400 and 20971 * ROW16 < 1 << 32 <= 20972 * ROW16
    big = torch.empty((21000,) + eng.EXIT_ACT_SHAPE, dtype=torch.float16, device=eng.device)
    try:
        big[10490], big[20990] = small[0], small[2]
        _through_far_rows(eng, model, small, big, mul, [10490, 20990])
    finally:
        del big


def test_host_rows_past_the_32_bit_offsets(engines, model):
    """The gather's offsets: a pinned 16-bit cache of 20 973 rows, the fewest whose last row starts at or behind byte 2^32."""
    eng = engines['f16']
    n_rows = -(-(1 << 32) // ROW16) + 1
    need, free = n_rows * ROW16, T.host_free_bytes()
    assert (n_rows - 1) * ROW16 >= 1 << 32 > (n_rows - 2) * ROW16
    if free is None or free < need + (2 << 30):
        print(f'host_rows_past_the_32_bit_offsets: {need} bytes of pinned memory wanted, {free} bytes of host memory available')
        pytest.skip(f'{need} bytes of pinned host memory and 2 GiB beside them are not available ({free} free)')
    small, mul = caches(eng, 'f16', 2.0 ** -3)['host16']
    try:
        big = torch.empty((n_rows,) + eng.EXIT_ACT_SHAPE, dtype=torch.float16, pin_memory=True)
    except RuntimeError as e:
        print(f'host_rows_past_the_32_bit_offsets: {need} bytes could not be pinned: {e}')
        pytest.skip(f'{need} bytes could not be pinned')
    try:
        big[n_rows // 2], big[n_rows - 1] = small[0], small[2]
        _through_far_rows(eng, model, small, big, mul, [n_rows // 2, n_rows - 1])
        torch.cuda.synchronize(eng.device)
    finally:
        del big
        getattr(torch._C, '_host_emptyCache', lambda: None)()


# ------------------------------------------------------------------------------------------------ 5. scratch
@pytest.mark.parametrize('store', ('host16', 'host32'))
def test_staged_calls_on_a_poisoned_workspace_of_exactly_their_size(engines, model, store):
    eng = engines['f16']
    params, stats = model
    lib = eng._lib
    acts, mul = caches(eng, 'f16', 2.0 ** 5)[store]
    code, row = eng.ACT_TYPES[acts.dtype], acts.element_size() * 102400
    for n in (1, 3, 256):                                                   # the device tier's bytes and n staged rows behind them
        assert lib.bq_exit_staged_workspace_bytes(n, code) == lib.bq_exit_train_workspace_bytes(n) + n * row
        assert lib.bq_exit_features_staged_workspace_bytes(n, code) == lib.bq_exit_features_workspace_bytes(n) + n * row
    assert lib.bq_exit_staged_workspace_bytes(0, code) == 0 == lib.bq_exit_staged_workspace_bytes(257, code)
    assert lib.bq_exit_staged_workspace_bytes(3, 3) == 0 == lib.bq_exit_features_staged_workspace_bytes(3, -1)
    rows, labels = X.grad_case(3, 'mixed')
    r, y = up(eng, rows), up(eng, labels)
    g0, l0 = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=0.1, act_mul=mul)
    f0 = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r, act_mul=mul)
    s0 = _steps(eng, model, acts, mul, 0.1)
    need, need_f = int(lib.bq_exit_staged_workspace_bytes(3, code)), int(lib.bq_exit_features_staged_workspace_bytes(3, code))
    assert eng.exit_train_scratch(3, staged=acts.dtype).numel() == need and eng.exit_features_scratch(3, staged=acts.dtype).numel() == need_f
    for fill in P.BYTE_FILLS:
        scratch, check = P.guarded(need, fill, eng.device)
        scratch_f, check_f = P.guarded(need_f, fill, eng.device)
        g1, l1 = eng.exit_grad(params, stats, acts, r, y, 3, X.SEED, rate=0.1, act_mul=mul, scratch=scratch)
        f1 = eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, r, act_mul=mul, scratch=scratch_f)
        s1 = _steps(eng, model, acts, mul, 0.1, scratch=scratch)            # batch 3: the same bytes
        torch.cuda.synchronize(eng.device)
        check()
        check_f()
        assert same((g1, l1, f1), (g0, l0, f0)) and same(s1, s0), hex(fill)
    # one byte less is refused, by the library and with its own text, and nothing is enqueued
    import ctypes as C
    vp = lambda t: C.c_void_p(t.data_ptr())
    from biscuit_amd import _lib
    dev_p = C.c_void_p(0)
    assert lib.bq_host_device_pointer(vp(acts), C.byref(dev_p)) == 0 and dev_p.value
    desc = _lib.BqActCache(dev_p.value, int(acts.shape[0]), code, mul, _lib.BQ_ACT_HOST)
    feat = torch.full((3, 2048), 7.0, dtype=torch.float32, device=eng.device)
    rc = lib.bq_exit_features_c(eng._ctx, vp(params), vp(stats), C.byref(desc), vp(r), 3, vp(feat), vp(scratch_f), need_f - 1, eng._stream())
    assert (rc, lib.bq_last_error(eng._ctx).decode()) == (-4, 'bq_exit_features: workspace below bq_exit_features_staged_workspace_bytes(n, type)')
    torch.cuda.synchronize(eng.device)
    assert bool((feat == 7.0).all())
    assert {'exit_train_staged', 'exit_features_staged'} <= set(eng._tool_ws)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_launch(engines, model):
    eng, other = engines['f16'], engines['bf16']
    params, stats = model
    acts16, mul = caches(eng, 'f16', 2.0 ** -3)['packed']
    rows, labels = X.grad_case(3, 'mixed')
    r, y = up(eng, rows), up(eng, labels)
    e = params[:eng.EXIT_PARAMS]
    out = torch.full((3, 2048), 7.0, dtype=torch.float32, device=eng.device)
    grad = torch.full_like(params, 7.0)
    pageable = acts16.cpu()
    assert not pageable.is_pinned()
    wide = torch.zeros((6, 10, 10, 2048), dtype=torch.float16, device=eng.device)
    cases = [
        ('pinned', pageable, mul),                                          # a pageable host tensor
        ("engine's own type", acts16, mul, other),                          # an f16 cache on a bf16 engine
        ("engine's own type", acts16.to(torch.bfloat16), mul),              # and a bf16 one on an f16 engine
        ('power of two', acts16, 3.0),
        ('power of two', acts16, 0.0),
        ('power of two', acts16, float('inf')),
        ('power of two', acts16, -2.0),
        ('act_mul must be 1', acts16.float(), 2.0),                         # float32 is read as it is
        ('contiguous', wide[..., ::2], mul),                                # the right shape, not contiguous
        ('contiguous', acts16.reshape(-1, 100, 1024), mul),                 # a wrong shape
        ('contiguous', acts16.double(), 1.0),                               # a type the cache does not come in
    ]
    for case in cases:
        text, a, m = case[:3]
        on = case[3] if len(case) > 3 else eng
        with pytest.raises(ValueError, match=text):
            on.exit_features(e, stats, a, r, out=out, act_mul=m)
        with pytest.raises(ValueError, match=text):
            on.exit_grad(params, stats, a, r, y, 3, X.SEED, grad=grad, act_mul=m)
        with pytest.raises(ValueError, match=text):
            on.exit_train_steps(params, grad, grad, stats, a, r, y, 3, 0, 9, [1e-3], act_mul=m)
        with pytest.raises(ValueError, match=text):
            on.exit_validate(params, stats, a, r, y, 3, X.SEED, act_mul=m)
    torch.cuda.synchronize(eng.device)
    assert bool((out == 7.0).all()) and bool((grad == 7.0).all())
    # the library's own question, asked of the runtime without touching the memory
    import ctypes as C
    dev_p = C.c_void_p(1)
    assert eng._lib.bq_host_device_pointer(C.c_void_p(pageable.data_ptr()), C.byref(dev_p)) == -1 and not dev_p.value
    assert 'not mapped pinned host memory' in eng._lib.bq_last_error(None).decode()
    assert eng._lib.bq_host_device_pointer(C.c_void_p(pinned(pageable).data_ptr()), C.byref(dev_p)) == 0 and dev_p.value
    # and the next launch finds no error pending
    assert bool(torch.isfinite(eng.exit_features(e, stats, acts16, r, act_mul=mul)).all())


# ------------------------------------------------------------------------------------------------ 7. end to end
def _four_slides(tmp_path, per=8):
    paths, labels = [], {}
    for i in range(4):
        name = f's{i}'
        t = make_tiles(per, seed=70 + i, slide_bias=[(i % 2) * 40.0 - 20.0, 0.0, 0.0])
        loc = np.stack([np.arange(per) * 299 + 150, np.full(per, 150 + 1000 * i)], 1).astype(np.int64)
        paths.append(str(tmp_path / f'{name}.tfrecords'))
        tfr.write_slide(paths[-1], name, t, loc)
        labels[name] = i % 2
    return paths, labels


EXIT = T.TrainParams(batch_size=4, learning_rate=1e-4, epochs=[1], trainable='exit', augment='xy')


@pytest.fixture(scope='module')
def folds(engines, tmp_path_factory):
    """``run(store) -> (cache, fold directories)``: the two-fold ``train_cv`` with ``trainable='exit'`` on four slides of eight tiles
    under one store, each made once."""
    eng = engines['f16']
    root = tmp_path_factory.mktemp('stores')
    paths, labels = _four_slides(root)
    done = {}

    def run(store):
        if store not in done:
            cache = T.cache_activations(eng, inf.slides_from_tfrecords(paths, labels), batch=8, augment='xy', views=1, seed=1, store=store)
            trainer = T.HeadTrainer(eng, cache, labels, params=EXIT, mc_n=4)
            done[store] = (cache, T.train_cv(cache, labels, str(root / store), 'EXP', 2, trainer, seed=2))
        return done[store]
    return run


def _same_files(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in os.listdir(a):
        with open(os.path.join(a, name), 'rb') as fa, open(os.path.join(b, name), 'rb') as fb:
            assert fa.read() == fb.read(), name


@pytest.mark.parametrize('store', ('packed', 'host', 'auto'))
def test_train_cv_writes_the_same_bytes_under_every_store(engines, folds, store):
    eng = engines['f16']
    ref, ref_dirs = folds('f32')
    cache, dirs = folds(store)
    assert ref.acts.dtype == torch.float32 and ref.acts.is_cuda and ref.act_mul == 1.0 and tuple(ref.act_views.shape) == (1, 32, 10, 10, 1024)
    if store == 'auto':                                                     # 26 MB fit the device as they are
        assert cache.acts.dtype == torch.float32 and cache.acts.is_cuda
    else:
        assert cache.acts.dtype == torch.float16 and cache.act_views.dtype == torch.float16 and cache.act_mul == 1.0
        assert cache.acts.is_cuda == (store == 'packed') and (store == 'packed' or (cache.acts.is_pinned() and cache.act_views.is_pinned()))
        assert torch.equal(cache.acts.to(eng.device).float() * cache.act_mul, ref.acts)
        assert torch.equal(cache.act_views.to(eng.device).float() * cache.act_mul, ref.act_views)
    assert same(cache.feats, ref.feats) and same(cache.views, ref.views) and bool(ref.feats.any())
    assert len(dirs) == len(ref_dirs) == 2
    for a, b in zip(ref_dirs, dirs):
        assert {T.HEAD_FILE, T.EXIT_FILE, T.MANIFEST_FILE, T.RESULTS_FILE} <= set(os.listdir(a))
        _same_files(a, b)


def test_head_training_on_a_packed_cache_is_head_training_on_a_feature_cache(engines, folds, tmp_path):
    eng = engines['f16']
    cache, _ = folds('packed')
    plain = T.FeatureCache(cache.feats, cache.slide_idx, cache.loc, cache.slides, cache.views, cache.augment, cache.augment_seed)
    labels = {s: i % 2 for i, s in enumerate(cache.slides)}
    params = T.TrainParams(batch_size=8, learning_rate=1e-4, epochs=[2], augment='xy')
    assert params.trainable == 'head'
    outs = []
    for name, c in (('plain', plain), ('packed', cache)):
        trainer = T.HeadTrainer(eng, c, labels, params=params, init='glorot', mc_n=4)
        outs.append(T.train_cv(c, labels, str(tmp_path / name), 'EXP', 2, trainer, seed=2))
    for a, b in zip(*outs):
        assert T.EXIT_FILE not in os.listdir(b) and T.HEAD_FILE in os.listdir(b)
        _same_files(a, b)


def test_a_saved_packed_cache_comes_back_in_either_place(engines, folds, tmp_path):
    eng = engines['f16']
    cache, _ = folds('packed')
    path = str(tmp_path / 'packed.npz')
    cache.save(path)
    on_device, on_host = T.ActivationCache.load(path, eng.device), T.ActivationCache.load(path, eng.device, host=True)
    assert on_device.acts.is_cuda and on_host.acts.is_pinned() and on_host.act_views.is_pinned() and on_host.feats.is_cuda
    for back in (on_device, on_host):
        assert back.acts.dtype == torch.float16 and back.act_mul == cache.act_mul and same(back.acts, cache.acts) and same(back.act_views, cache.act_views)
    assert on_host.to(eng.device).acts.is_pinned()                          # to() keeps the place


# ------------------------------------------------------------------------------------------------ 8. profiling
def test_the_host_tier_opens_exit_gather_once_per_step_and_the_device_stores_nothing_new(engines, model):
    eng = engines['f16']
    params, stats = model
    rows, labels, lr = _three_steps()
    fwd = ('coef', 'dw1', 'pw1', 'dw2', 'pw2', 'pool')
    back = ('dfeat', 'bn2', 'dp2', 'du2', 'dd2', 'dh1', 'bn1', 'dp1', 'du1', 'dd1', 'adam')
    head = ('fwd0', 'fwd1', 'logits', 'dx1', 'dw1', 'dw0', 'sums')
    known = {'exit_train_' + k for k in fwd + back} | {'exit_feat_' + k for k in fwd} | {'head_train_' + k for k in head}
    seen = {}
    for store, (acts, mul) in caches(eng, 'f16', 2.0 ** -3).items():
        eng.profile_enable(True)
        try:
            _steps(eng, model, acts, mul, 0.1)
            eng.exit_features(params[:eng.EXIT_PARAMS], stats, acts, up(eng, rows[:3]), act_mul=mul)
            seen[store] = {p.name: p for p in eng.profile_read()}
        finally:
            eng.profile_enable(False)
    assert set(seen['f32']) == known == set(seen['packed'])
    for store in ('host16', 'host32'):
        assert set(seen[store]) == known | {'exit_gather'}, set(seen[store]) ^ known
        assert seen[store]['exit_gather'].launches == 3 + 1                 # three steps and one features call
        row = ROW16 if store == 'host16' else ROW32
        assert seen[store]['exit_gather'].bytes == 2.0 * (3 + 3 + 2 + 3) * row / 4         # (a class reports its launches' mean)
    assert all(seen[s]['exit_train_dw1'].launches == 3 and seen[s]['exit_train_dd1'].launches == 3 for s in seen)
    # the readers' byte counts say what they read: 4 bytes written per element, and 4 or 2 read
    assert seen['f32']['exit_feat_dw1'].bytes == 8.0 * 300 * 1024 == seen['host32']['exit_feat_dw1'].bytes
    assert seen['packed']['exit_feat_dw1'].bytes == 6.0 * 300 * 1024 == seen['host16']['exit_feat_dw1'].bytes
