"""The Reinhard domain cases (tests/_stain_cases.py) really reach what they are built to reach, and the oracle's split halves
(oracle/stain.py) are what the kernel's table and branches are compared with.  CPU only."""
import warnings

import numpy as np
import pytest

import _stain_cases as sc
from oracle import stain

F = np.float32


@pytest.fixture(scope='module')
def thr():
    return stain.srgb_switch_points()


def test_switch_points_are_the_level_functions_steps(thr):
    assert thr.dtype == F and thr.shape == (255,)
    assert (np.diff(thr) > 0).all() and thr[0] > 0 and 1 < thr[-1] < 1 + 1e-6       # c = 1 encodes as 254: 1.055f - 0.055f < 1
    bits = thr.view(np.uint32)
    want = np.arange(1, 256)
    assert (stain.linear_to_level(bits.view(F)) == want).all()                  # the point itself has level v ...
    assert (stain.linear_to_level((bits - 1).view(F)) == want - 1).all()        # ... and the float just below it v - 1
    # monotone around every point (the bisection's premise), +-512 floats each, and on a coarse sweep of [-0.5, 1.5]
    near = (bits[:, None].astype(np.int64) + np.arange(-512, 513)[None]).astype(np.uint32).view(F)
    assert (np.diff(stain.linear_to_level(near).astype(int), axis=1) >= 0).all()
    sweep = np.linspace(-0.5, 1.5, 400001).astype(F)
    assert (np.diff(stain.linear_to_level(sweep).astype(int)) >= 0).all()


def test_level_edges_and_the_nan_rule():
    c = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-30, 1.0, np.nextafter(F(1), F(0)), 2.0, 3e38, np.inf], F)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                    # the rule is explicit: no cast of a NaN, no RuntimeWarning
        lv = stain.linear_to_level(c)
        nan_lab = stain.lab_to_rgb_u8(*(np.full((1, 2, 2), np.nan, F),) * 3)
    assert lv.tolist() == [0, 0, 0, 0, 0, 0, 254, 254, 255, 255, 255]         # (c = 1 is 254: 1.055f * 1 - 0.055f < 1)
    assert nan_lab.dtype == np.uint8 and not nan_lab.any()


def test_split_halves_compose_to_the_whole():
    tiles = sc.box_tiles()[[0, 4], :64, :64]
    tm, ts = sc.REGIMES['he_x5']
    whole = stain.reinhard_fast(tiles, tm, ts)
    lab = stain.normalised_lab(tiles, tm, ts)
    assert np.array_equal(stain.linear_to_level(stain.lab_to_linear(*lab)), whole)
    # stats= given the tiles' own statistics changes nothing; given others it is used
    mu, sd = stain.lab_stats(*stain.rgb_to_lab(tiles))
    assert np.array_equal(stain.reinhard_fast(tiles, tm, ts, stats=(mu, sd)), whole)
    assert not np.array_equal(stain.reinhard_fast(tiles, tm, ts, stats=(mu + F(3), sd)), whole)
    # a tile's bytes depend on its own statistics only
    assert np.array_equal(stain.reinhard_fast(tiles[1:], tm, ts, stats=(mu[1:], sd[1:])), whole[1:])


def test_switch_tiles_probe_every_switching_point_from_both_sides(thr):
    tiles = sc.switch_tiles()
    assert tiles.shape == (8, sc.PX, sc.PX, 3) and tiles.dtype == np.uint8
    tb = thr.view(np.uint32).astype(np.int64)
    on = np.zeros(255, bool)
    below = np.full(255, np.iinfo(np.int64).max)
    levels = np.zeros(256, bool)
    for t in tiles:
        tm, ts = sc.own_fit(t)
        c = sc.linear_values(t, tm, ts)
        out = stain.linear_to_level(c)
        assert np.array_equal(out, stain.reinhard_fast(t[None], tm, ts)[0])
        assert np.abs(out.astype(int) - t.astype(int)).max() <= 1               # the identity regime
        levels[np.unique(out)] = True
        cb = np.unique(c[c > 0].view(np.uint32)).astype(np.int64)                # positive floats order as their bit patterns
        i = np.searchsorted(cb, tb)                                             # first value >= the point
        on |= (i < len(cb)) & (cb[np.minimum(i, len(cb) - 1)] == tb)
        below = np.minimum(below, np.where(i > 0, tb - cb[np.maximum(i - 1, 0)], below))
    print(f'switch tiles: points hit exactly {int(on.sum())}/255, worst distance of the nearest value below: {int(below.max())} ulps')
    assert on.all(), np.flatnonzero(~on)
    assert (below >= 1).all() and (below <= 4).all(), below.max()
    assert levels.all()


def test_box_regimes_leave_the_gamut_and_take_every_branch():
    tiles = sc.box_tiles()
    assert tiles.shape == (8, sc.PX, sc.PX, 3) and len(sc.BOX_NAMES) == 8 and list(sc.REGIMES) == ['he', 'he_x5', 'std0', 'std1e-3']
    assert tiles[1].max() <= 40 and tiles[2].min() >= 215 and int(tiles[3].max()) - int(tiles[3].min()) == 5
    assert (tiles[5, ..., 0] == 255).all() and tiles[6].min() >= 100 and tiles[6].max() <= 138
    assert (np.diff(tiles[7, 0, :, 0].astype(int)) >= 0).all() and tiles[7, 0, 0, 0] == 0 and tiles[7, 0, -1, 0] == 255
    tm, ts = sc.REGIMES['he_x5']
    lab = stain.normalised_lab(tiles, tm, ts)
    v, c = stain.lab_to_f(*lab), stain.lab_to_linear(*lab)
    lo, hi = float((c < 0).mean()), float((c > 1).mean())
    print(f'he_x5: c < 0 on {100 * lo:.1f} %, c > 1 on {100 * hi:.1f} % of the channel values')
    assert lo >= 0.01 and hi >= 0.01
    for name, x, s in (('v', v, stain.V_SWITCH), ('c', c, stain.C_SWITCH)):
        frac = float((x > s).mean())
        assert 0.01 <= frac <= 0.99, (name, frac)
    # std0: every pixel of every tile becomes the one colour of the target means
    tm0, ts0 = sc.REGIMES['std0']
    out0 = stain.reinhard_fast(tiles, tm0, ts0)
    assert (out0 == out0[0, 0, 0]).all() and out0[0, 0, 0].tolist() == stain.lab_to_rgb_u8(*[np.full((1, 1, 1), m, F) for m in tm0])[0, 0, 0].tolist()
    # the forward switch at 0.008856: the dark box sits on both sides of it
    t = np.stack(stain.xyz_over_white(tiles[1]))
    assert 0.01 <= float((t > stain.T_SWITCH).mean()) <= 0.99


def test_constant_colours_straddle_the_cube_root_switch():
    cols = sc.constant_colours()
    assert cols.dtype == np.uint8 and len(np.unique(cols, axis=0)) == len(cols)
    have = {tuple(c) for c in cols.tolist()}
    assert all((g, g, g) in have for g in range(256))
    assert all((r, g, b) in have for r in range(0, 256, 51) for g in range(0, 256, 51) for b in range(0, 256, 51))
    near = sc.dark_switch_colours()
    assert near.shape == (48, 3) and near.max() <= 40 and all(tuple(c) in have for c in near.tolist())
    # against a brute-force enumeration of all 41^3 dark colours: nothing lies between the chosen ones and the switch
    g = np.arange(41, dtype=np.uint8)
    allc = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    assert len(allc) == 68921
    t_all, t_near = stain.xyz_over_white(allc), stain.xyz_over_white(near)
    for ch in range(3):
        lo, hi = t_near[ch][16 * ch:16 * ch + 8], t_near[ch][16 * ch + 8:16 * ch + 16]
        assert (lo <= stain.T_SWITCH).all() and (hi > stain.T_SWITCH).all()
        assert int(((t_all[ch] > lo.min()) & (t_all[ch] <= stain.T_SWITCH)).sum()) <= 8 - 1
        assert int(((t_all[ch] < hi.max()) & (t_all[ch] > stain.T_SWITCH)).sum()) <= 8 - 1
        print(f'channel {"XYZ"[ch]}: nearest t below {lo.max():.9g}, above {hi.min():.9g} (switch {stain.T_SWITCH:.9g})')


def test_constant_tile_statistics_read_the_conversion_back():
    """float32(float64 mean) of a constant tile is the colour's own L, a, b, and its deviation stays under the cancellation bound,
    for pairwise and for sequential accumulation (the kernel's tree is a third order)."""
    cols = np.concatenate([np.array(sc.DEGENERATE_CONSTANTS, np.uint8), sc.dark_switch_colours()[::6], sc.constant_colours()[300::40]])
    lab = sc.constant_lab(cols).astype(np.float64)
    for v in lab.reshape(-1):
        col = np.full(sc.NPIX, v)
        for s1, s2 in ((col.sum(), (col * col).sum()), (np.cumsum(col)[-1], np.cumsum(col * col)[-1])):
            mu = s1 / sc.NPIX
            assert F(mu) == F(v)
            sd = np.sqrt(max(s2 / sc.NPIX - mu * mu, 0.0))
            assert sd <= sc.CONST_SD_REL * abs(v)


def test_degenerate_tiles():
    one = sc.one_pixel_tiles()
    assert one.shape == (2, sc.PX, sc.PX, 3)
    for t in one:
        flat = t.reshape(-1, 3)
        assert len(np.unique(flat, axis=0)) == 2 and (flat != flat[0]).any(1).sum() == 1
    assert (one[1].reshape(-1, 3)[:-1] == one[1, 0, 0]).all()
    # a deviation of exactly 0 gives NaN and then black; anything else the colour of the target means
    tm, ts = sc.REGIMES['he']
    px = np.full((1, 1, 1, 3), 9, np.uint8)
    mu = sc.constant_lab(px[0, 0]).astype(F)
    black = stain.reinhard_fast(px, tm, ts, stats=(mu, np.zeros((1, 3), F)))
    mean_colour = stain.reinhard_fast(px, tm, ts, stats=(mu, np.full((1, 3), 1e-7, F)))
    assert not black.any()
    assert np.array_equal(mean_colour, stain.lab_to_rgb_u8(*[np.full((1, 1, 1), m, F) for m in tm]))


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
def test_reinhard_fit_rejects_non_finite_targets(bad):
    from biscuit_amd.stain import ReinhardFast, check, reinhard_fit
    good = {'target_means': [65.0, 20.0, -10.0], 'target_stds': [15.0, 8.0, 6.0]}
    tm, ts = reinhard_fit(good)
    assert ReinhardFast.from_params(None, {'norm_fit': good}).get_fit() == good
    assert list(tm) == good['target_means'] and list(ts) == good['target_stds']
    for key in good:
        for i in range(3):
            fit = {k: list(v) for k, v in good.items()}
            fit[key][i] = bad
            with pytest.raises(ValueError):
                reinhard_fit(fit)
            with pytest.raises(ValueError):
                check('reinhard_fast', fit)
            with pytest.raises(ValueError):
                ReinhardFast.from_params(None, {'norm_fit': fit})


def test_reinhard_fit_keeps_zero_and_negative_stds_and_rejects_bad_shapes():
    from biscuit_amd.stain import reinhard_fit
    for stds in ([0.0, 0.0, 0.0], [-1.0, 2.0, 0.0]):
        assert list(reinhard_fit({'target_means': [1.0, 2.0, 3.0], 'target_stds': stds})[1]) == stds
    for fit in ({'target_means': [1.0, 2.0], 'target_stds': [1.0, 2.0, 3.0]}, {'target_means': 'abc', 'target_stds': [1.0, 2.0, 3.0]},
                {'target_means': [1.0, 2.0, 3.0]}):
        with pytest.raises(ValueError):
            reinhard_fit(fit)
