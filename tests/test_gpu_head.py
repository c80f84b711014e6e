"""The MC-dropout head (kernels_head.hip: the two Dense(1024) layers; head_final_kernel: the last dropout, softmax and Welford
fold) against the float64 reference of tests/_head_ref.py, across dropout rates, pass and row counts, Philox counters and the
number range of its operands.  Run on the MI355X box with ``-m gpu``.

Every comparison holds mean and std within 2e-6 absolute (the bound test_gpu_parity.py::test_head_shapes_against_oracle holds
against the fp32 oracle) and prints the worst difference it met.  The head is the same fp32 code for every storage type, so the
tests run f32 engines, and one f16 engine shows the sharing.
"""
import contextlib

import numpy as np
import pytest
import torch

import _head_ref as R
from biscuit_amd.hp import ModelParams
from biscuit_amd.weights import synthetic_weights
from oracle import philox

pytestmark = pytest.mark.gpu

TOL = 2e-6
RATES = (0.0, 0.05, 0.1, 0.2, 0.25, 0.3, 0.5, 0.75, 0.9, 0.99)
SCALES = (-40, -24, -16, -8, 0, 8, 15, 16, 20, 40)


@pytest.fixture(scope='module')
def weights():
    return synthetic_weights(1)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def o1_features(n, seed, signed=False):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 1.0, (n, 2048)) if signed else np.abs(rng.normal(0.8, 0.5, (n, 2048)))
    return f.astype(np.float32)


@contextlib.contextmanager
def engine(weights, rate=0.1, dtype='f32', max_batch=16, max_mc=50):
    from biscuit_amd.engine import Engine
    eng = Engine(weights, hp=ModelParams(dropout=rate), dtype=dtype, max_batch=max_batch, max_mc=max_mc)
    try:
        yield eng
    finally:
        eng.close()


def run(eng, feat, mc_n, seed, tile_idx0=0, tile_idx=None):
    idx = None if tile_idx is None else dev(np.asarray(tile_idx, np.int64))
    m, s = eng.mc_head(dev(np.asarray(feat, np.float32)), mc_n, seed, tile_idx0=tile_idx0, tile_idx=idx)
    torch.cuda.synchronize()
    return m.cpu().numpy(), s.cpu().numpy()


def check(label, got, ref, tol=TOL):
    """got: (mean, std) float32 of the device, ref: float64 of the reference; returns the worst absolute difference."""
    d = max(float(np.abs(got[0] - ref[0]).max()), float(np.abs(got[1] - ref[1]).max()))
    print(f'{label}: worst |device - float64| = {d:.3e}')
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), label
    assert d < tol, (label, d)
    return d


def test_dropout_rates(weights):
    """One engine per rate, the rate going params.json -> ModelParams -> the device as a double.  0.99 is also the operand-range
    case of O(1) features at dscale = 100."""
    feat = o1_features(16, 1)
    idx = 500 + np.arange(16)
    for rate in RATES:
        with engine(weights, rate) as eng:
            got = run(eng, feat, 12, 1234, tile_idx0=500)
        check(f'rate {rate}', got, R.mc(feat, weights, rate, 1234, idx, 12))
        if rate == 0.0:
            assert (got[1] == 0).all()                                  # no dropout: every pass is the same


def test_rates_outside_the_unit_interval_are_refused(weights):
    from biscuit_amd.engine import BiscuitHipError, Engine
    for bad in (-0.1, 1.0, 1.5, float('nan'), float('inf')):
        with pytest.raises(BiscuitHipError):
            Engine(weights, hp=ModelParams(dropout=bad), dtype='f32', max_batch=1, max_mc=1)
    feat = o1_features(4, 2)
    with engine(weights, 0.1, max_batch=4, max_mc=8) as eng:
        before = run(eng, feat, 8, 3)
        for bad in (-0.1, -1e-300, 1.0, 1.0 + 1e-12, float('nan'), float('inf'), float('-inf')):
            assert eng._lib.bq_set_dropout(eng._ctx, bad) < 0, bad
            assert b'[0, 1)' in eng._lib.bq_last_error(eng._ctx)
        after = run(eng, feat, 8, 3)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])     # a refused rate changes nothing
        assert eng._lib.bq_set_dropout(eng._ctx, 0.3) == 0                                     # and a valid one applies
        check('bq_set_dropout(0.3) after creation', run(eng, feat, 8, 3), R.mc(feat, weights, 0.3, 3, np.arange(4), 8))


def test_threshold_window(weights):
    """Rate 0.3, seed 1234, tile 1378: the Philox word of layer 0, pass 11, unit 161 lies between floor(0.3 * 2^32) (the contract:
    keep) and floor(fp32(0.3) * 2^32) (drop); tests/test_head_ref.py pins that.  With features that are zero except at that unit,
    the mean over 12 passes tells which threshold the device used."""
    feat = np.zeros((1, 2048), np.float32)
    feat[0, 161] = 4.0
    with engine(weights, 0.3, max_batch=1, max_mc=12) as eng:
        got = run(eng, feat, 12, 1234, tile_idx0=1378)
    check('threshold window', got, R.mc(feat, weights, 0.3, 1234, [1378], 12))


def test_pass_counts(weights):
    """mc_n around the final kernel's blocks of eight waves, and the 64-row workgroups of the dense kernels cutting across tiles."""
    feat = o1_features(5, 3)
    with engine(weights, 0.1, max_batch=5, max_mc=50) as eng:
        for mc_n in (1, 2, 7, 8, 9, 30, 31, 50):
            got = run(eng, feat, mc_n, 99, tile_idx0=3000)
            check(f'mc_n {mc_n}', got, R.mc(feat, weights, 0.1, 99, 3000 + np.arange(5), mc_n))
            if mc_n == 1:
                assert (got[1] == 0).all()


def test_row_counts(weights):
    feat = o1_features(256, 4)
    with engine(weights, 0.1, max_batch=256, max_mc=50) as eng:
        for n in (1, 63, 64, 65, 256):
            got = run(eng, feat[:n], 50, 2024, tile_idx0=10)
            check(f'n {n} x mc 50', got, R.mc(feat[:n], weights, 0.1, 2024, 10 + np.arange(n), 50))


def test_seeds_with_a_high_word(weights):
    feat = o1_features(6, 5)
    idx = np.arange(6)
    with engine(weights, 0.2, max_batch=6, max_mc=9) as eng:
        low = run(eng, feat, 9, 7)
        for seed in (2 ** 32 + 7, 2 ** 63 + 11, 2 ** 64 - 1):
            got = run(eng, feat, 9, seed)
            check(f'seed {seed:#x}', got, R.mc(feat, weights, 0.2, seed, idx, 9))
            if seed == 2 ** 32 + 7:
                assert not np.array_equal(got[0], low[0])                 # the high word is part of the key


def test_tile_indices_across_2_32(weights):
    """The Philox tile counter is the low 32 bits of the tile index (oracle/philox.py), as tile_idx0 and as a per-tile array
    with repeats and out of order; indices equal modulo 2^32 draw the same masks."""
    feat = o1_features(8, 6)
    arr = np.array([2 ** 32 + 5, 3, 2 ** 32 - 1, 3, 2 ** 33 + 3, 7, 2 ** 32 + 5, 0], np.int64)
    with engine(weights, 0.25, max_batch=8, max_mc=7) as eng:
        t0 = 2 ** 32 - 3
        check('tile_idx0 = 2^32 - 3', run(eng, feat, 7, 11, tile_idx0=t0), R.mc(feat, weights, 0.25, 11, t0 + np.arange(8), 7))
        check('tile_idx array', run(eng, feat, 7, 11, tile_idx=arr), R.mc(feat, weights, 0.25, 11, arr, 7))
        t0 = 2 ** 32 + 100
        check('tile_idx0 + array', run(eng, feat, 7, 11, tile_idx0=t0, tile_idx=arr),
              R.mc(feat, weights, 0.25, 11, t0 + arr, 7))
        same = np.repeat(feat[:1], 8, axis=0)
        m, s = run(eng, same, 7, 11, tile_idx=arr)
        for i, j in ((1, 3), (1, 4), (0, 6)):                                  # 3, 3 and 2^33 + 3; 2^32 + 5 twice
            assert np.array_equal(m[i], m[j]) and np.array_equal(s[i], s[j]), (i, j)
        assert not np.array_equal(m[2], m[7])                                  # 2^32 - 1 and 0: other masks


def test_features_rescaled(weights):
    """features * 2^k with hidden_0/kernel * 2^-k is the same head in real arithmetic: every k lands within 2e-6 of the
    float64 result for k = 0, for non-negative (pooled ReLU) and signed features."""
    cases = [(signed, o1_features(8, 7 + signed, signed)) for signed in (False, True)]
    refs = [R.mc(f, weights, 0.1, 4321, 7000 + np.arange(8), 10) for _, f in cases]
    worst = {}
    for k in SCALES:
        with engine(weights=R.scale_features(weights, k), rate=0.1, max_batch=8, max_mc=10) as eng:
            for (signed, f), ref in zip(cases, refs):
                worst[(k, signed)] = check(f'features * 2^{k}{" (signed)" if signed else ""}',
                                           run(eng, np.ldexp(f, k), 10, 4321, tile_idx0=7000), ref)
    print('worst over the feature scalings:', f'{max(worst.values()):.3e}')


def test_hidden_rescaled(weights):
    """(hidden_0 kernel, bias) * 2^k with hidden_1/kernel * 2^-k: hidden_0's activations at 2^k, the same head."""
    feat = o1_features(8, 9)
    ref = R.mc(feat, weights, 0.1, 4321, 7000 + np.arange(8), 10)
    worst = 0.0
    for k in SCALES:
        with engine(weights=R.scale_hidden(weights, k), rate=0.1, max_batch=8, max_mc=10) as eng:
            worst = max(worst, check(f'hidden_0 * 2^{k}', run(eng, feat, 10, 4321, tile_idx0=7000), ref))
    print(f'worst over the hidden scalings: {worst:.3e}')


def test_rows_are_independent(weights):
    """A tile at 2^30, one with a NaN and one with an inf among ordinary tiles: the ordinary tiles give the bits they give
    alone (same Philox indices), the 2^30 tile its float64 result, and the non-finite tiles non-finite mean and std."""
    n, big, nan, inf = 12, 3, 6, 9
    feat = o1_features(n, 10)
    feat[big] = np.ldexp(feat[big], 30)
    feat[nan, 10] = np.nan
    feat[inf, 20] = np.inf
    ordinary = np.array([i for i in range(n) if i not in (big, nan, inf)])
    with engine(weights, 0.1, max_batch=n, max_mc=12) as eng:
        m, s = run(eng, feat, 12, 55, tile_idx0=900)
        m1, s1 = run(eng, feat[ordinary], 12, 55, tile_idx0=900, tile_idx=ordinary)
    assert np.array_equal(m[ordinary], m1) and np.array_equal(s[ordinary], s1)
    check('ordinary tiles', (m1, s1), R.mc(feat[ordinary], weights, 0.1, 55, 900 + ordinary, 12))
    check('tile at 2^30', (m[big:big + 1], s[big:big + 1]), R.mc(feat[big:big + 1], weights, 0.1, 55, [900 + big], 12))
    for i in (nan, inf):
        assert not np.isfinite(m[i]).any() and not np.isfinite(s[i]).any(), (i, m[i], s[i])
    # one pass: a non-finite feature that the pass drops changes nothing, one that it keeps makes the tile NaN
    keep = philox.dropout_keep(55, np.array([900 + nan]), 0, 0, 2048, 0.1)[0]
    dropped, kept = int(np.flatnonzero(~keep)[0]), int(np.flatnonzero(keep)[0])
    one = np.repeat(o1_features(1, 12), 2, axis=0)
    one[0, dropped] = np.nan
    one[1, kept] = np.inf
    with engine(weights, 0.1, max_batch=2, max_mc=1) as eng:
        m, s = run(eng, one, 1, 55, tile_idx=[900 + nan, 900 + nan])
    check('NaN feature dropped by the pass', (m[:1], s[:1]), R.mc(one[:1], weights, 0.1, 55, [900 + nan], 1))
    assert np.isnan(m[1]).all() and np.isnan(s[1]).all(), (m[1], s[1])


def test_f16_engine_runs_the_same_head(weights):
    feat = o1_features(16, 11)
    feat[0] = 0.0
    feat[0, 161] = 4.0                                   # the threshold-window row (tile 1378 = tile_idx0 + 0)
    with engine(weights, 0.3, dtype='f16', max_batch=16, max_mc=12) as e16:
        g16 = run(e16, feat, 12, 1234, tile_idx0=1378)
    with engine(weights, 0.3, dtype='f32', max_batch=16, max_mc=12) as e32:
        g32 = run(e32, feat, 12, 1234, tile_idx0=1378)
    assert np.array_equal(g16[0], g32[0]) and np.array_equal(g16[1], g32[1])
    check('f16 engine', g16, R.mc(feat, weights, 0.3, 1234, 1378 + np.arange(16), 12))
