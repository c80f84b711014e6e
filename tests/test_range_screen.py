"""The f16 range screen without a GPU: its key and update rule restated in numpy (tests/_range_ref.py) and checked against the
long way round, the top-k rule with ties, and the argument checks of the C ABI and of the Python screen."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _range_ref as R
from biscuit_amd.synthetic import make_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constructed_tiles():
    flat = np.full((1, 299, 299, 3), 128, np.uint8)
    one = flat.copy()
    one[0, 150, 150, 1] = 255
    zeros = np.zeros_like(flat)
    full = np.full_like(flat, 255)
    dark = flat.copy()
    dark[0, 10:13, 20:23, :] = 0
    return np.concatenate([flat, one, zeros, full, dark, make_tiles(3, seed=11)])


def test_key_is_the_peak_of_per_image_standardisation():
    t = constructed_tiles()
    key = R.range_key(t)
    assert key.dtype == np.float32 and key.shape == (len(t),)
    assert key[0] == 0 and key[2] == 0 and key[3] == 0                  # one value everywhere: nothing to standardise
    # one bright value among N - 1 equal ones: (N - 1) / sqrt(N - 1) = sqrt(N - 1) standard deviations out
    assert abs(float(key[1]) - np.sqrt(R.N - 1)) < 1e-3 * np.sqrt(R.N)
    np.testing.assert_allclose(key, R.standardised_peak(t).astype(np.float32), rtol=1e-6)
    assert key[4] > key[5:].max() > 0                                    # a dark spot on a flat tile reaches far, texture does not


def test_key_of_a_nearly_flat_tile():
    """One byte one level above N - 1 equal ones: the smallest non-zero spread a tile can have, and the largest key
    (sqrt(N - 1), ~518).  The key is the float64 value rounded once to float32."""
    t = np.full((1, 299, 299, 3), 7, np.uint8)
    t[0, 0, 0, 0] = 8
    key = R.range_key(t)[0]
    assert key == np.float32(R.standardised_peak(t)[0]) or abs(float(key) - R.standardised_peak(t)[0]) < 1e-6 * float(key)
    assert abs(float(key) - np.sqrt(R.N - 1)) < 1e-3


def test_top_k_rule_with_ties_is_the_interval_top_k():
    rng = np.random.default_rng(3)
    k = 8
    entries = []
    for g in range(300):
        entries.append((float(np.float32(rng.integers(0, 6) * 0.5)), g, f'tile{g}'))       # six key values: ties everywhere
    perm = rng.permutation(300)                                           # global indices need not arrive in order
    entries = [entries[i] for i in perm]
    slots = []
    seen = []
    for b0 in range(0, 300, 37):
        batch = entries[b0:b0 + 37]
        before = {s[1]: i for i, s in enumerate(slots)}
        slots = R.screen_update(slots, batch, k)
        seen += batch
        assert sorted(slots, key=lambda x: (-x[0], x[1])) == R.top_k(seen, k)
        for i, s in enumerate(slots):                                     # survivors stayed where they were
            if s[1] in before:
                assert before[s[1]] == i
    # all tied: the smallest global indices win
    tied = [(1.0, g, None) for g in (9, 4, 7, 1, 3, 8, 2, 6, 5, 0)]
    assert [s[1] for s in R.top_k(tied, 4)] == [0, 1, 2, 3]
    assert sorted(s[1] for s in R.screen_update([], tied, 4)) == [0, 1, 2, 3]
    # the same tile twice (equal key and index): the entry already in a slot stays, the slots stay a prefix
    s1 = R.screen_update([], [(2.0, 5, 'old')], 3)
    s2 = R.screen_update(s1, [(2.0, 5, 'new'), (1.0, 6, 'x')], 3)
    assert s2[0] == (2.0, 5, 'old') and len(s2) == 3


def test_screen_update_fills_a_prefix_and_keeps_the_best():
    slots = R.screen_update([], [(1.0, 0, 'a'), (3.0, 1, 'b')], 4)
    assert slots == [(1.0, 0, 'a'), (3.0, 1, 'b')] or slots == [(3.0, 1, 'b'), (1.0, 0, 'a')]
    assert [s[2] for s in slots] == ['b', 'a']                           # rank order into the empty slots
    slots = R.screen_update(slots, [(0.5, 2, 'c'), (5.0, 3, 'd'), (2.0, 4, 'e')], 4)
    assert [s[2] for s in slots] == ['b', 'a', 'd', 'e']
    slots = R.screen_update(slots, [(4.0, 5, 'f')], 4)
    assert [s[2] for s in slots] == ['b', 'f', 'd', 'e']                 # 'a' (1.0) evicted, its slot reused


def _lib():
    try:
        from biscuit_amd import _lib
    except (ImportError, OSError) as e:
        pytest.fail(f'libbiscuit_hip.so must be built for the suite: {e}')
    return _lib


def test_c_abi_declares_the_screen_and_refuses_bad_arguments():
    L = _lib()
    lib = L.lib
    assert 'bq_range_key' in L.ABI and 'bq_range_screen' in L.ABI and 'bq_range_ws_bytes' in L.ABI
    assert lib.bq_range_ws_bytes(-1) == 0
    assert lib.bq_range_ws_bytes(256) >= 256 * 8 * 24 and lib.bq_range_ws_bytes(256) % 256 == 0
    assert lib.bq_range_ws_bytes(512) > lib.bq_range_ws_bytes(256)
    p = C.c_void_p(4096)           # never dereferenced: every call below is refused before anything is enqueued
    assert lib.bq_range_key(None, p, 4, p, p, 1 << 20, None) == -1
    assert b'bq_range_key' in lib.bq_last_error(None)
    assert lib.bq_range_screen(None, p, 4, 0, None, p, p, p, 8, 0, p, 1 << 20, None) == -1
    assert b'bq_range_screen' in lib.bq_last_error(None)


def test_python_screen_refuses_bad_arguments_before_allocating():
    from biscuit_amd.engine import RangeScreen

    class NoDevice:                 # anything that got past the checks would touch these and fail differently
        max_batch = 256
        device = None
        _lib = None

    for kw in ({'k': 0}, {'k': 65}, {'max_batch': 0}, {'max_batch': 2049}):
        with pytest.raises(ValueError):
            RangeScreen(NoDevice(), **kw)


def test_eval_result_reports_the_screen():
    from biscuit_amd.inference import EvalResult, evaluate
    import inspect
    r = EvalResult(None, [], np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    assert r.f16_screened == 0 and r.f16_screen_checks == 0 and r.f16_screen_headroom == float('inf') and r.f16_screen_max_key == 0.0
    assert inspect.signature(evaluate).parameters['range_screen'].default is False


def test_cli_offers_no_range_screen():
    r = subprocess.run([sys.executable, '-m', 'biscuit_amd', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '--range-screen' in r.stdout and '--no-range-screen' in r.stdout
