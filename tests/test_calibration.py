"""The UQ calibration data on the host (``biscuit_amd/calibration.py``; DESIGN.md section 7 "UQ calibration"): the numpy path against
the per-point restatement of tests/_calibration_ref.py and, for the density, ``scipy.stats.gaussian_kde``; then the interface --
``threshold.plot_uncertainty``, ``apply`` / ``detect`` with ``plot=<directory>``, ``save`` / ``load`` and the command line.

Tolerances: the density 1e-12 of the curve's maximum; the fit 1e-10 absolute; l2, se and the band 1e-10 relative.  The same
restatement summed with ``numpy.sum`` against exact ``math.fsum`` differs by <= 1e-14 on the fit and <= 2.1e-13 relative on l2 at
N = 64 .. 4 099, so 1e-10 leaves about 500 x for another order of summation, contraction and a last place of ``exp``."""
import json
import math
import os

import numpy as np
import pandas as pd
import pytest

from biscuit_amd import calibration, predictions, threshold
from tests import _calibration_ref as R

SIZES = (64, 257, 1000, 4099)


def cases():
    out = {f'n{n}': R.case(n) for n in SIZES}
    out['tied257'] = R.tied_case()
    return out


CASES = cases()


@pytest.mark.parametrize('name', list(CASES))
def test_density_equals_the_restatement_and_scipy(name):
    x, c = CASES[name]
    R.check_kde(calibration.kde_host(x, c), x, c)


@pytest.mark.parametrize('name', list(CASES))
def test_curve_equals_the_restatement(name):
    x, c = CASES[name]
    got = calibration.loess_host(x, c)
    assert got['degenerate'] == 0
    R.check_loess(got, x, c)


def test_the_tied_case_has_sixty_rows_at_one_value():
    x, _ = R.tied_case()
    assert np.unique(x, return_counts=True)[1].max() == 60


def test_the_interpolant_is_segment_by_segment():
    x, c = R.case(257)
    raw = calibration.loess_host(x, c, grid=9)
    np.testing.assert_allclose(calibration.interpolate(raw['vertex'], raw['fit'], x), R.interp_ref(raw['vertex'], raw['fit'], x), rtol=0, atol=1e-15)


def test_one_group_only():
    x, c = R.one_group_case()
    R.check_kde(calibration.kde_host(x, c), x, c)
    R.check_loess(calibration.loess_host(x, c), x, c, constant_y=True)
    cal = calibration.uncertainty_calibration(pd.DataFrame({'uncertainty': x, 'correct': c, 'y_pred': x}), 'slide')
    assert list(cal.kde) == ['correct'] and cal.summary['no_density'] == ['incorrect']
    np.testing.assert_allclose(cal.loess['fit'], 1.0, atol=1e-10)


def test_a_group_of_one_has_no_density():
    x, _ = R.case(64)
    c = np.ones(64, bool)
    c[5] = False
    got = calibration.kde_host(x, c)
    assert not got['valid'][0] and got['valid'][1] and got['n'][0] == 1
    R.check_kde(got, x, c)


def test_degenerate_vertices_are_nan_and_counted():
    x, c = R.degenerate_case()
    got = calibration.loess_host(x, c)
    ref = R.loess_ref(x, c)
    assert got['h'][0] == 0.0 and np.isnan(got['fit'][0]) and 0 < got['degenerate'] == int(np.isnan(got['fit']).sum())
    R.check_loess(got, x, c, ref=ref)
    cal = calibration.uncertainty_calibration(pd.DataFrame({'uncertainty': x, 'correct': c, 'y_pred': x}), 'slide')
    assert cal.summary['degenerate_vertices'] == got['degenerate']


def test_grid_of_seven():
    x, c = R.case(257)
    R.check_kde(calibration.kde_host(x, c, grid=7), x, c, grid=7)
    R.check_loess(calibration.loess_host(x, c, grid=7), x, c, grid=7)


def test_descending_input():
    x, c = R.case(1000)
    o = np.argsort(-x, kind='stable')
    R.check_kde(calibration.kde_host(x[o], c[o]), x, c)
    R.check_loess(calibration.loess_host(x[o], c[o]), x, c)


def test_nan_raises():
    x, c = R.case(64)
    x[3] = np.nan
    with pytest.raises(ValueError):
        calibration.kde_host(x, c)
    with pytest.raises(ValueError):
        calibration.loess_host(x, c)
    with pytest.raises(ValueError):
        calibration.uncertainty_calibration(pd.DataFrame({'uncertainty': x, 'correct': c, 'y_pred': x}), 'slide')


# ---------------------------------------------------------------------------------------------------------------- interface
def tile_table(n_slides=24, per=60, seed=5):
    """A tile table in the writer's layout: slides of ``per`` tiles, the label by slide, y_pred near it, uncertainty larger where wrong."""
    rng = np.random.default_rng(seed)
    slides = np.repeat([f's{k:02d}' for k in range(n_slides)], per)
    y = np.repeat(np.arange(n_slides) % 2, per)
    shift = np.repeat(rng.normal(0, 0.25, n_slides), per)              # by slide: some slides come out wrong
    p1 = np.clip(y * 0.4 + 0.3 + shift + rng.normal(0, 0.2, len(y)), 0.01, 0.99)
    unc = np.abs(rng.normal(0.03, 0.01, len(y)) + 0.05 * np.abs(p1 - y))
    mean2 = np.stack([1 - p1, p1], 1)
    std2 = np.stack([unc, unc], 1)
    return predictions.tile_frame('cohort', slides, y, mean2, std2)


def processed(n=1500, seed=0):
    x, c = R.case(n, seed)
    return pd.DataFrame({'uncertainty': x, 'correct': c, 'y_pred': np.random.default_rng(seed).random(n)})


def assert_same(a, b):
    assert a.kind == b.kind and list(a.kde) == list(b.kde) and a.summary == b.summary
    for g in a.kde:
        for k in ('support', 'density', 'density_unit'):
            assert np.array_equal(a.kde[g][k], b.kde[g][k])
        assert a.kde[g]['bandwidth'] == b.kde[g]['bandwidth']
    for k in a.loess:
        assert np.array_equal(a.loess[k], b.loess[k], equal_nan=True)
    pd.testing.assert_frame_equal(a.scatter.reset_index(drop=True), b.scatter.reset_index(drop=True))


def test_plot_uncertainty_is_uncertainty_calibration():
    df = processed()
    a = threshold.plot_uncertainty(df, 'tile', threshold=0.06, title='CV UQ Calibration: x')
    b = calibration.uncertainty_calibration(df, 'tile', 0.06, title='CV UQ Calibration: x')
    assert_same(a, b)
    assert a.summary['title'] == 'CV UQ Calibration: x' and a.summary['path'] == 'host' and a.summary['N'] == 1500
    assert a.summary['n_correct'] + a.summary['n_incorrect'] == 1500 and a.summary['q'] == 1125
    assert set(a.loess) == {'vertex', 'fit', 'se', 'lower', 'upper', 'h'}
    # common normalisation: the two scaled densities integrate to 1 together
    total = sum(float((0.5 * (d['density'][1:] + d['density'][:-1]) * np.diff(d['support'])).sum()) for d in a.kde.values())
    assert abs(total - 1.0) < 5e-3


def test_tile_scatter_is_a_seeded_sample():
    df = processed()
    a = calibration.uncertainty_calibration(df, 'tile', 0.06, seed=7)
    b = calibration.uncertainty_calibration(df, 'tile', 0.06, seed=7)
    c = calibration.uncertainty_calibration(df, 'tile', 0.06, seed=8)
    assert len(a.scatter) == 1000 and list(a.scatter.columns) == ['y_pred', 'uncertainty', 'correct', 'above']
    pd.testing.assert_frame_equal(a.scatter, b.scatter)
    assert not a.scatter['uncertainty'].equals(c.scatter['uncertainty'])
    assert (a.scatter['above'] == (a.scatter['uncertainty'] >= 0.06)).all()
    small = calibration.uncertainty_calibration(processed(300), 'tile')
    assert len(small.scatter) == 300 and not small.scatter['above'].any()
    assert len(calibration.uncertainty_calibration(df, 'slide').scatter) == 1500


def test_apply_and_detect_save_where_the_reference_draws(tmp_path):
    base = tile_table()
    predictions.rename_cols(base, 'cohort')
    th0, auc0 = threshold.detect(base.copy(), tile_uq=0.2)          # a loose tile filter: some slides stay wrong, so slide_uq is detected
    th1, auc1 = threshold.detect(base.copy(), tile_uq=0.2, plot=tmp_path / 'detect')
    assert th0 == th1 and auc0 == auc1 and th0['slide_uq'] is not None
    for k, p in calibration.Calibration.paths(tmp_path / 'detect', 'slide').items():
        assert os.path.getsize(p) > 0, k
    with open(calibration.Calibration.paths(tmp_path / 'detect', 'slide')['summary']) as f:
        assert json.load(f)['threshold'] == th1['slide_uq']
    m0, s0 = threshold.apply(base.copy(), th0['tile_uq'], th0['slide_uq'], th0['tile_pred'], th0['slide_pred'])
    m1, s1 = threshold.apply(base.copy(), th0['tile_uq'], th0['slide_uq'], th0['tile_pred'], th0['slide_pred'], plot=str(tmp_path / 'apply'),
                             title='held out')
    assert m0 == m1
    pd.testing.assert_frame_equal(s0, s1)
    saved = calibration.Calibration.load(tmp_path / 'apply', 'slide')
    assert saved.summary['title'] == 'held out' and saved.summary['N'] == 24 and len(saved.scatter) == 24
    # without detection the reference draws at its fixed 0.5
    threshold.detect(base.copy(), slide_uq=None, plot=tmp_path / 'fixed')
    assert calibration.Calibration.load(tmp_path / 'fixed', 'slide').summary['threshold'] == 0.5


def test_plot_true_still_raises():
    base = tile_table()
    predictions.rename_cols(base, 'cohort')
    with pytest.raises(NotImplementedError):
        threshold.detect(base.copy(), plot=True)
    with pytest.raises(NotImplementedError):
        threshold.apply(base.copy(), 0.05, 0.05, plot=True)


def test_save_round_trips(tmp_path):
    cal = calibration.uncertainty_calibration(processed(), 'tile', 0.06, title='t')
    paths = cal.save(tmp_path, prefix='fig')
    assert sorted(os.path.basename(p) for p in paths.values()) == ['fig_tile_kde.csv', 'fig_tile_loess.csv', 'fig_tile_scatter.csv',
                                                                   'fig_tile_summary.json']
    assert_same(cal, calibration.Calibration.load(tmp_path, 'tile', prefix='fig'))


def test_uq_calibration_follows_the_experiment(tmp_path):
    tables = [tile_table(seed=s) for s in (1, 2, 3)]
    tile, slide = calibration.uq_calibration(tables, 'cohort', 0.05, 0.04, 0.5)
    assert tile.summary['N'] == 3 * 24 * 60 and tile.summary['kind'] == 'tile' and len(tile.scatter) == 1000
    df = pd.concat(tables, ignore_index=True)
    predictions.rename_cols(df, 'cohort')
    df, _ = threshold.process_tile_predictions(df)
    s_df, _ = threshold.process_group_predictions(df[df['uncertainty'] < 0.05], 0.5, 'slide')
    assert_same(slide, calibration.uncertainty_calibration(s_df, 'slide', 0.04))


def test_command_line_on_a_written_table(tmp_path, capsys):
    path = predictions.write_tile_table(tile_table(), str(tmp_path), outcome='cohort')
    out = tmp_path / 'out'
    assert calibration.main([path, '--outcome', 'cohort', '--tile-uq', '0.05', '--slide-uq', '0.04', '--out', str(out), '--host']) == 0
    printed = capsys.readouterr().out.split()
    assert len(printed) == 8 and all(os.path.exists(p) for p in printed)
    tile = calibration.Calibration.load(out, 'tile')
    assert tile.summary['N'] == 24 * 60 and tile.summary['path'] == 'host' and math.isfinite(tile.summary['s'])
    assert calibration.Calibration.load(out, 'slide').summary['threshold'] == 0.04
