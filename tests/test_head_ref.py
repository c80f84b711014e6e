"""CPU checks of the float64 head reference (tests/_head_ref.py), of the vehicles tests/test_gpu_head.py drives the head kernels
with, and of the host side of the head's weight exponents."""
import numpy as np
import pytest
import torch

import _head_ref as R
from biscuit_amd import weights as W
from oracle import philox

# The threshold-window vehicle of tests/test_gpu_head.py: rate 0.3, seed 1234, tile 1378, layer 0, pass 11, unit 161.
WINDOW = dict(rate=0.3, seed=1234, tile=1378, mc_pass=11, unit=161)


@pytest.fixture(scope='module')
def head():
    w = W.synthetic_weights(1)
    return {k: w[k] for k in R.head_tensors(w)}


def window_word():
    c = WINDOW
    r = philox.philox4x32_10(c['unit'] // 4, 0, c['mc_pass'], c['tile'], c['seed'] & 0xffffffff, c['seed'] >> 32)
    return int(r[c['unit'] % 4])


def test_reference_against_the_fp32_oracle(head):
    """O(1) features: the float64 head and XceptionOracle.head_pass (float32 torch) agree to fp32 rounding, pass by pass."""
    from oracle.xception_ref import XceptionOracle
    rng = np.random.default_rng(7)
    feat = np.abs(rng.normal(0.8, 0.5, (9, 2048))).astype(np.float32)
    for rate in (0.0, 0.1, 0.5):
        orc = XceptionOracle(head, dropout=rate)
        idx = np.arange(40, 49)
        pr = R.passes(feat, head, rate, 77, idx, 5)
        for p in range(5):
            ref = orc.head_pass(torch.from_numpy(feat), idx, p, 77).numpy()
            assert np.abs(pr[p] - ref).max() < 1e-6, (rate, p)
        m, s = R.mc(feat, head, rate, 77, idx, 5)
        om, os_ = orc.mc_from_features(feat, 5, 77, tile_index0=40)
        assert np.abs(m - om).max() < 1e-6 and np.abs(s - os_).max() < 1e-6
        assert (s.max() > 1e-3) if rate else (s.max() < 1e-15)     # dropout moves the probabilities; rate 0 gives std 0


def test_reference_rescaled_heads_are_the_same_function(head):
    rng = np.random.default_rng(8)
    feat = rng.normal(0.0, 1.0, (4, 2048)).astype(np.float32)
    idx = np.arange(4)
    m0, s0 = R.mc(feat, head, 0.2, 5, idx, 6)
    for k in (-40, 16, 40):
        m, s = R.mc(np.ldexp(feat, k), R.scale_features(head, k), 0.2, 5, idx, 6)
        assert np.abs(m - m0).max() < 1e-12 and np.abs(s - s0).max() < 1e-12
        m, s = R.mc(feat, R.scale_hidden(head, k), 0.2, 5, idx, 6)
        assert np.abs(m - m0).max() < 1e-12 and np.abs(s - s0).max() < 1e-12


def test_threshold_window_vehicle_does_not_rot(head):
    """The Philox word of the window case lies between the contract's threshold (the double rate) and the one a float32 rate
    gives, so a device that thresholds with fp32(0.3) drops a unit the contract keeps; and with features that are zero except at
    that unit, pass 11 -- and so the mean over 12 passes -- depends on it far beyond the 2e-6 the GPU test holds."""
    c = WINDOW
    word = window_word()
    t_contract = philox.keep_threshold(c['rate'])
    t_f32 = int(np.floor(float(np.float32(c['rate'])) * 2.0 ** 32))
    assert (t_contract, t_f32) == (1288490188, 1288490240)
    assert t_contract <= word < t_f32
    keep = philox.dropout_keep(c['seed'], np.array([c['tile']]), c['mc_pass'], 0, 2048, c['rate'])
    assert keep[0, c['unit']]
    feat = np.zeros((1, 2048), np.float32)
    feat[0, c['unit']] = 4.0
    m_keep, _ = R.mc(feat, head, c['rate'], c['seed'], [c['tile']], 12)
    # the same run with the unit dropped in pass 11: the mean over the first 11 passes plus pass 11 without the unit
    pr = R.passes(feat, head, c['rate'], c['seed'], [c['tile']], 12)
    p11_dropped = R.passes(np.zeros_like(feat), head, c['rate'], c['seed'], [c['tile']], 1, pass0=11)[0]
    m_drop = (pr[:11].sum(axis=0) + p11_dropped) / 12
    assert np.abs(m_keep - m_drop).max() > 1e-4


def test_split_f16_range():
    """split_f16 is fp32 grade in [2^-14, 2^16) and saturates -- lo included, never inf -- above 65504."""
    def back(a):
        hi, lo = W.split_f16(a)
        return hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / W.HEAD_SPLIT_SCALE
    rng = np.random.default_rng(1)
    m = rng.uniform(1.0, 2.0, 4096).astype(np.float32)
    for e in (-14, -10, 0, 8, 15):
        a = np.ldexp(m, e).astype(np.float32)
        assert (np.abs(back(a) - a) / a).max() < 2.5e-7, e
    big = np.array([1e5, -1e6, 3e38], np.float32)
    with np.errstate(over='raise'):
        v = back(big)
    assert np.all(np.isfinite(v)) and np.all(np.abs(v) <= 65504.0 + 65504.0 / 2048)


def test_head_weight_exponent_and_blob(head):
    assert W.head_weight_exponent(head['hidden_0/kernel']) == 0 and W.head_weight_exponent(head['hidden_1/kernel']) == 0
    assert W.head_weight_exponent(np.zeros((4, 4))) == 0
    for peak, s in ((2.0 ** -8, 0), (2.0 ** 14, 0), (2.0 ** 14 * 1.5, 1), (1e5, 3), (2.0 ** -9, -22), (2.0 ** -100, -64)):
        assert W.head_weight_exponent(np.array([[peak, -peak / 3]])) == s, peak
        if s:
            assert 2.0 ** 13 <= peak * 2.0 ** -s < 2.0 ** 14 or s == -64
    w = W.synthetic_weights(1)
    base = W.pack_blob(w, 'f32')
    assert b'hidden_0/wexp' not in base and b'hidden_1/wexp' not in base     # a head that fits packs as it always did
    big = R.scale_hidden(w, 20)                 # hidden_0 * 2^20 and hidden_1 * 2^-20: both leave the split's range
    blob = W.pack_blob(big, 'f32')
    assert b'hidden_0/wexp' in blob and b'hidden_1/wexp' in blob
    for name, sign in (('hidden_0', 1), ('hidden_1', -1)):
        s = W.head_weight_exponent(big[name + '/kernel'])
        assert s * sign > 0 and 2.0 ** 13 <= np.abs(big[name + '/kernel']).max() * 2.0 ** -s < 2.0 ** 14
