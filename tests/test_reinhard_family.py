"""The Reinhard family on the CPU: the host side (``stain.check`` / ``make_normalizer`` take 'reinhard', 'reinhard_mask' and
'reinhard_fast_mask' with a means / stds fit; ``model_hp`` the two masked names) and the numpy restatement the GPU tests compare against
(tests/_reinhard_family_ref.py; DESIGN.md "Reinhard family")."""
import numpy as np
import pytest

import _reinhard_family_ref as R
from biscuit_amd import stain
from oracle import stain as O

F = np.float32
NEW = ('reinhard', 'reinhard_mask', 'reinhard_fast_mask')
FIT = {'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, 6.0]}
MACENKO_FIT = {'stain_matrix_target': [[0.5, 0.2], [0.7, 0.8], [0.4, 0.5]], 'target_concentrations': [1.9, 1.0]}


def _tiles(px, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, px, px, 3), dtype=np.uint8)


def _half_glass(px, seed):
    """A tile whose left half is tissue-coloured noise and whose right half is glass (250..255)."""
    rng = np.random.default_rng(seed)
    t = rng.integers(40, 200, (px, px, 3), dtype=np.uint8)
    t[:, px // 2:] = rng.integers(250, 256, (px, px - px // 2, 3), dtype=np.uint8)
    return t


def test_methods_and_flags_table():
    assert set(stain.METHODS) == {'reinhard_fast', 'macenko', *NEW}
    assert stain.REINHARD_FLAGS == {'reinhard_fast': 0, 'reinhard': 1, 'reinhard_fast_mask': 2, 'reinhard_mask': 3}
    assert stain.REINHARD_MASK_THRESHOLD == 0.93 == R.MASK_THRESHOLD
    assert (stain.REINHARD_OK, stain.REINHARD_NO_TISSUE, stain.REINHARD_DARK) == (R.OK, R.NO_TISSUE, R.DARK)
    assert stain.REINHARD_BRIGHT_PCT == 100 * R.PCT


@pytest.mark.parametrize('name', NEW)
def test_check_and_make_normalizer_accept_the_family(name):
    stain.check(name, FIT)
    stain.check(name, None)
    norm = stain.make_normalizer(None, name, FIT)
    assert norm.method == name and norm.flags == stain.REINHARD_FLAGS[name]
    assert norm.get_fit() == FIT
    assert type(norm).from_params(None, {'norm_fit': FIT}).get_fit() == FIT
    assert stain.make_normalizer(None, name, None) is None
    with pytest.raises(ValueError):
        stain.check(name, MACENKO_FIT)                        # a fit of another method
    with pytest.raises(ValueError):
        stain.make_normalizer(None, name, MACENKO_FIT)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='non-finite'):
            stain.check(name, {'target_means': [65.0, bad, -8.0], 'target_stds': [14.0, 7.0, 6.0]})
        with pytest.raises(ValueError, match='non-finite'):
            stain.check(name, {'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, bad]})


def test_unknown_names_are_still_refused():
    for name in ('vahadane', 'reinhard_slow', 'Reinhard', ''):
        with pytest.raises(ValueError, match='normalizer must be one of'):
            stain.check(name, FIT)
        with pytest.raises(ValueError, match='normalizer must be one of'):
            stain.normalise(None, None, name, FIT)
    assert type(stain.make_normalizer(None, 'reinhard_fast', FIT)) is stain.ReinhardFast


def test_classes_take_any_square_tile_size_and_refuse_the_rest():
    norm = stain.ReinhardMask(type('E', (), {'device': 'cpu'})(), FIT['target_means'], FIT['target_stds'])
    for px in (1, 33, 299, 512, 1024):
        t, single = norm._as_batch(np.zeros((px, px, 3), np.uint8))
        assert tuple(t.shape) == (1, px, px, 3) and single
    for shape in ((4, 5, 3), (2, 4, 5, 3), (4, 4, 4), (1025, 1025, 3), (0, 0, 3)):
        with pytest.raises(ValueError):
            norm._as_batch(np.zeros(shape, np.uint8))
    with pytest.raises(TypeError):
        norm._as_batch(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(RuntimeError):
        stain.Reinhard(None).rgb_to_rgb(np.zeros((4, 4, 3), np.uint8))


def test_model_hp_reads_the_family_from_a_params_dict():
    from biscuit_amd.__main__ import model_hp
    for name in ('reinhard_mask', 'reinhard_fast_mask'):
        hp, fit = model_hp({'hp': {'dropout': 0.25}, 'normalizer': name, 'norm_fit': FIT, 'path': 'p'})
        assert hp.normalizer == name and fit == FIT and hp.dropout == 0.25
        with pytest.raises(SystemExit):
            model_hp({'hp': {}, 'normalizer': name, 'norm_fit': None})
        with pytest.raises(SystemExit):
            model_hp({'hp': {}, 'normalizer': name, 'norm_fit': MACENKO_FIT})
    for name in ('vahadane', 'reinhard'):                     # (plain 'reinhard': the drivers take it, the command lines do not)
        with pytest.raises(SystemExit):
            model_hp({'hp': {}, 'normalizer': name, 'norm_fit': FIT})


def test_flags_0_is_the_oracles_reinhard_fast():
    tm, ts = F(FIT['target_means']), F(FIT['target_stds'])
    for px, seed in ((1, 0), (7, 1), (33, 2)):
        tiles = _tiles(px, 3, seed)
        want = O.reinhard_fast(tiles, tm, ts)
        for i in range(3):
            got, status = R.normalise(tiles[i], 0, tm, ts)
            assert status == R.OK and np.array_equal(got, want[i])
            r = R.analyse(tiles[i], 0)
            assert r['p'] == F(100.0) and r['m'] == px * px and r['frac'] == F(1.0) and np.array_equal(r['bright'], tiles[i])


def test_brightness_leaves_white_alone_and_never_lowers_a_byte():
    white = np.full((5, 5, 3), 255, np.uint8)
    r = R.analyse(white, R.BRIGHTNESS)
    assert r['status'] == R.OK and r['p'] == F(100.0) and np.array_equal(r['bright'], white)
    assert np.array_equal(R.brightness_table(F(100.0)), np.arange(256))
    for seed in range(4):
        for t in _tiles(9, 2, seed) // (seed + 1):             # darker and darker tiles
            r = R.analyse(t, R.BRIGHTNESS)
            assert r['status'] == R.OK and 0 < r['p'] <= F(100.0)
            assert (r['bright'] >= t).all()
    # L never exceeds 100, so the table never maps a byte below itself, whatever the percentile
    for p in (F(1e-3), F(0.5), F(37.25), F(99.99999), F(100.0)):
        assert (R.brightness_table(p) >= np.arange(256)).all()
    dark = np.zeros((4, 4, 3), np.uint8)
    out, status = R.normalise(dark, R.BRIGHTNESS, F(FIT['target_means']), F(FIT['target_stds']))
    assert status == R.DARK and np.array_equal(out, dark)


def test_percentile_is_numpys_on_random_tiles():
    for px, seed in ((1, 0), (2, 1), (3, 2), (7, 3), (11, 4), (33, 5), (64, 6)):
        for t in _tiles(px, 3, seed):
            L = O.rgb_to_lab(t[None])[0]
            assert L.dtype == F
            assert R.percentile90(L) == F(np.percentile(L.astype(np.float64), 90))


def test_masked_tile_keeps_the_brightness_stages_bytes_off_tissue():
    tm, ts = F(FIT['target_means']), F(FIT['target_stds'])
    for flags in (R.MASK, R.MASK | R.BRIGHTNESS):
        t = _half_glass(16, 3)
        r = R.analyse(t, flags)
        assert r['status'] == R.OK and 0 < r['m'] < 256
        out, status = R.normalise(t, flags, tm, ts)
        glass = ~r['tissue']
        assert status == R.OK and glass[:, 8:].all() and r['tissue'][:, :8].all()
        assert np.array_equal(out[glass], r['bright'][glass])
        assert (out[r['tissue']] != r['bright'][r['tissue']]).any()
        # the statistics are the tissue's: the unmasked ones are dragged toward white
        r0 = R.analyse(t, flags & R.BRIGHTNESS)
        assert r0['mu'][0] > r['mu'][0] + 10


def test_stats_from_outside_replace_the_restatements_own():
    tm, ts = F(FIT['target_means']), F(FIT['target_stds'])
    t = _half_glass(16, 5)
    r = R.analyse(t, 3)
    same, _ = R.normalise(t, 3, tm, ts, stats=(r['mu'], r['sd']))
    own, _ = R.normalise(t, 3, tm, ts)
    assert np.array_equal(same, own)
    other, _ = R.normalise(t, 3, tm, ts, stats=(r['mu'] + F(5), r['sd']))
    assert not np.array_equal(other, own) and np.array_equal(other[~r['tissue']], own[~r['tissue']])


def test_degenerate_targets_do_not_fit():
    with pytest.raises(ValueError):
        R.fit(np.zeros((4, 4, 3), np.uint8), R.BRIGHTNESS)
    with pytest.raises(ValueError):
        R.fit(np.full((4, 4, 3), 255, np.uint8), R.MASK)
    mu, sd = R.fit(_half_glass(16, 7), 3)
    assert np.isfinite(mu).all() and (sd > 0).all()
