"""``biscuit_amd/metrics.py`` on the host (DESIGN.md section 7 "Prediction metrics"): ``delong_host`` and the public functions
against tests/golden/metrics_reference.json.gz -- what the reference's ``biscuit/delong.py`` and ``biscuit/utils.py`` compute from
the seeded cases of tests/_delong_ref.py -- and against that module's O(m n0) restatement.

Held: the AUROC and, where the golden stores it, V bit for bit; V equal to the pairwise means at every size; the covariance
within ``TOL`` = 1e-12 of its scale 0.25 (1 / m + 1 / n0) of the golden, of ``numpy.cov`` and of exact rational arithmetic;
NaN exactly where the golden has it.

``log10 p`` within 1e-9 absolute where the golden is finite and z <= 8.  Derivation: p = 2 sf(z), so d log10 p / dz =
-phi(z) / (sf(z) ln 10), and phi / sf <= z + 1 / z (Mills' ratio), roughly z / ln 10 for the z that matter; z = |d auc| / sqrt(v) with
v = S00 + S11 - 2 S01, the AUROCs bit-exact, so dz = z dv / (2 v) and |d log10 p| <= z (z + 1 / z) |dv| / (2 v ln 10).  With
|dv| <= 4 TOL x scale: for z <= 8 that is at most 65 x 4e-12 x scale / (2 v ln 10) = 5.7e-11 x scale / v.  v is not bounded below
in general -- it is what the test measures -- but in the committed cases scale / v <= 4 (printed and asserted), which leaves 2.3e-10; the cases
whose v is zero have z = 0 / 0 or infinite and are held by the NaN / infinity clause instead."""
import gzip
import json
import logging
import os

import numpy as np
import pandas as pd
import pytest

from biscuit_amd import metrics, threshold
from tests import _delong_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics_reference.json.gz')
NAMES = tuple(R.CASES)


@pytest.fixture(scope='module')
def golden():
    with gzip.open(GOLDEN, 'rt') as f:
        g = json.load(f)
    assert set(g['cases']) == set(NAMES) and g['meta']['threshold'] == R.THRESHOLD
    for name, entry in g['cases'].items():               # the rebuilt inputs are the generator's
        y, P = R.case(name)
        assert (entry['n'], entry['k']) == (len(y), len(P)) and entry['checksum'] == R.checksum(y, P), f'case {name} was rebuilt differently'
        assert ('V' in entry) == (len(y) <= R.STORES_V)
    return g['cases']


def test_the_cases_cover_what_they_claim():
    sizes = {name: R.case(name)[1].shape for name in NAMES}
    assert {k for k, _ in sizes.values()} >= {1, 2, 3, 8}
    assert {n for _, n in sizes.values()} >= {2, 3, 7, 64, 257, 1000, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 3 * R.CHUNK + 1}
    y, P = R.case('n3')
    assert (int(y.sum()), int((1 - y).sum())) == (2, 1)
    y, P = R.case('zeros')
    assert np.signbit(P[P == 0]).any() and not np.signbit(P[P == 0]).all()
    assert np.isposinf(R.case('inf')[1]).any() and np.isneginf(R.case('inf')[1]).any()
    assert (np.diff(R.case('descending')[1][0]) <= 0).all()
    assert len(np.unique(R.case('tied257')[1][0])) < 30


@pytest.mark.parametrize('name', NAMES)
def test_delong_host_against_the_reference_and_the_restatement(golden, name):
    y, P = R.case(name)
    got = metrics.delong_host(y, P, components=True)
    dev = R.check(name, got, golden[name])
    spread = R.cov_deviation(R.restated(name)['cov_numpy'], R.restated(name)['cov_exact'], got['n_pos'], got['n_neg'])
    gold_spread = R.cov_deviation(R.unjson(golden[name]['cov']), R.restated(name)['cov_exact'], got['n_pos'], got['n_neg'])
    print(f'{name}: covariance off by ' + ', '.join(f'{k} {v:.2e}' for k, v in dev.items())
          + f' of the scale; numpy.cov against exact {spread:.2e}, the reference against exact {gold_spread:.2e}')
    assert max(spread, gold_spread) <= R.TOL / 100          # the bound stands at least 100 times above the statements' own spread


def test_exact_values_of_the_degenerate_cases():
    for name, auc, v in (('equal', 0.5, 0.5), ('separated', 1.0, 1.0)):
        got = metrics.delong_host(*R.case(name), components=True)
        assert (got['auc'] == auc).all() and (got['V'] == v).all() and (got['cov'] == 0.0).all(), name
    got = metrics.delong_host(*R.case('n2'))
    assert np.isnan(got['cov']).all() and (got['auc'] == [1.0, 0.0]).all()
    got = metrics.delong_host(*R.case('monotone'), components=True)
    assert R.same_bits(got['V'][0], got['V'][1]) and len(set(got['cov'].reshape(-1).tolist())) == 1 and got['auc'][0] == got['auc'][1]
    y, P = R.case('zeros')                                   # -0.0 + 0.0 = +0.0: the sign of a zero changes nothing
    assert not np.signbit(P + 0.0)[P == 0].any()
    assert R.same_bits(metrics.delong_host(y, P + 0.0, components=True)['V'], metrics.delong_host(y, P, components=True)['V'])


def _z_and_v(res):
    v = res['cov'][0, 0] + res['cov'][1, 1] - 2 * res['cov'][0, 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        return abs(res['auc'][0] - res['auc'][1]) / np.sqrt(v), v


def check_log10_p(name, got, gold, res):
    """``got`` of ``delong_roc_test`` against the golden's value; ``res``: the first two classifiers' covariance result."""
    want = R.unjson(gold['log10_p'])
    assert got.shape == want.shape == (1, 1)
    assert np.isnan(got[0, 0]) == np.isnan(want[0, 0]), f'{name}: NaN where the reference has none, or the reverse'
    if np.isnan(want[0, 0]):
        return
    if not np.isfinite(want[0, 0]):
        assert got[0, 0] == want[0, 0]
        return
    z, v = _z_and_v(res)
    print(f'{name}: z {z:.3f}, scale / v {R.scale(res["n_pos"], res["n_neg"]) / v:.2f}, log10 p off by {abs(got[0, 0] - want[0, 0]):.2e}')
    if z <= 8:
        assert R.scale(res['n_pos'], res['n_neg']) / v <= 4
        assert abs(got[0, 0] - want[0, 0]) <= R.LOG10P_ATOL


@pytest.mark.parametrize('name', [n for n in NAMES if R.case(n)[1].shape[0] >= 2])
def test_delong_roc_test(golden, name):
    y, P = R.case(name)
    check_log10_p(name, metrics.delong_roc_test(y, P[0], P[1]), golden[name], metrics.delong_host(y, P[:2]))


def check_prediction_metrics(name, got, gold):
    want = gold['prediction_metrics']
    assert list(got) == ['auc_low', 'auc_high', 'acc', 'sens', 'spec', 'youden', 'youden_low', 'youden_high']
    for key in ('acc', 'sens', 'spec', 'youden', 'youden_low', 'youden_high'):
        assert R.same_bits(got[key], R.unjson(want[key])), f'{name}: {key} {got[key]!r} is not the reference\'s {want[key]!r}'
    for key in ('auc_low', 'auc_high'):
        g, w = np.float64(got[key]), R.unjson(want[key])
        assert np.isnan(g) == np.isnan(w) and (np.isnan(w) or abs(g - w) <= 1e-12), f'{name}: {key} {g!r} against {w!r}'


@pytest.mark.parametrize('name', NAMES)
def test_prediction_metrics_under_both_seedings(golden, name):
    y, P = R.case(name)
    seed = golden[name]['seed']
    assert seed == R.SEEDS[name]
    np.random.seed(seed)
    check_prediction_metrics(name, metrics.prediction_metrics(y, P[0], R.THRESHOLD), golden[name])
    np.random.seed(12345)
    state = np.random.get_state()
    check_prediction_metrics(name, metrics.prediction_metrics(y, P[0], R.THRESHOLD, seed=seed), golden[name])
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]       # the global generator untouched


def test_prediction_metrics_without_binary_labels(caplog):
    y, P = R.case('n64')
    with caplog.at_level(logging.WARNING, logger='biscuit_amd'):
        got = metrics.prediction_metrics(np.where(y == 1, 2, 0), P[0], R.THRESHOLD, seed=1)
    assert got['auc_low'] is None and got['auc_high'] is None and 'Unable to calculate CI' in caplog.text
    assert np.isfinite(got['youden_low'])


def test_variance_is_the_matrix_entry(golden):
    y, P = R.case('n64')
    auc, var = metrics.delong_roc_variance(y, P[1])
    res = metrics.delong_covariance(y, P)
    assert res['path'] == 'host' and R.same_bits(auc, res['auc'][1])
    assert abs(var - res['cov'][1, 1]) <= R.TOL * R.scale(res['n_pos'], res['n_neg'])
    assert R.same_bits(auc, R.unjson(golden['n64']['auc'])[1])


def test_refusals():
    y, P = R.case('n64')
    bad = P.copy()
    bad[1, 5] = np.nan
    for call in (lambda: metrics.delong_host(y, bad), lambda: metrics.delong_host(np.ones_like(y), P), lambda: metrics.delong_host(np.zeros_like(y), P),
                 lambda: metrics.delong_host(y, np.vstack([P] * 3)), lambda: metrics.delong_host(y[:-1], P), lambda: metrics.delong_host(y * 2, P),
                 lambda: metrics.delong_roc_variance(y, bad[1]), lambda: metrics.delong_roc_test(y, P[0], P[1][:-1])):
        with pytest.raises(ValueError):
            call()
    assert metrics.delong_host(y, np.vstack([P, P, P[:2]]))['cov'].shape == (8, 8)


def test_auc_and_threshold_on_tied_data():
    y, P = R.case('tied257')
    auc, t = metrics.auc_and_threshold(y, P[0])
    fpr, tpr, thresh = threshold._roc(y, P[0])
    assert t == threshold._youden(fpr, tpr, thresh) == thresh[int(np.argmax(tpr - fpr))]
    assert abs(auc - metrics.delong_host(y, P[0])['auc'][0]) <= 1e-12
    # the reference's own statement of the choice: the first (tpr, fpr) pair that attains the maximum
    pairs = list(zip(tpr, fpr))
    assert t == thresh[pairs.index(max(pairs, key=lambda x: x[0] - x[1]))]


# ---------------------------------------------------------------------------------------------------------------- files
def _have_parquet():
    try:
        import pyarrow  # noqa: F401
        return True
    except ImportError:
        try:
            import fastparquet  # noqa: F401
            return True
        except ImportError:
            return False


LAYOUTS = {
    'sf12': ({'slide': ['a', 'b', 'c'], 'cohort-y_true': [0, 1, 1], 'cohort-y_pred0': [0.7, 0.4, 0.2], 'cohort-y_pred1': [0.3, 0.6, 0.8]}, [0, 1, 1], [0.3, 0.6, 0.8]),
    'sf11': ({'slide': ['a', 'b', 'c'], 'y_true0': [1, 0, 0], 'y_true1': [0, 1, 1], 'percent_tiles_positive0': [0.9, 0.5, 0.1],
              'percent_tiles_positive1': [0.1, 0.5, 0.9], 'y_pred0': [0.7, 0.4, 0.2], 'y_pred1': [0.3, 0.6, 0.8]}, [0, 1, 1], [0.1, 0.5, 0.9]),
    'mixed': ({'y_true1': [1, 0, 1], 'a_y_pred0': [0.5, 0.5, 0.5], 'a_y_pred1': [0.25, 0.5, 0.75]}, [1, 0, 1], [0.25, 0.5, 0.75]),
}


@pytest.mark.parametrize('ext', ['csv', 'parquet', 'parquet.gzip'])
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_read_group_predictions_layouts(tmp_path, layout, ext):
    cols, y_true, y_pred = LAYOUTS[layout]
    path = str(tmp_path / f'preds.{ext}')
    if ext == 'csv':
        pd.DataFrame(cols).to_csv(path, index=False)
    else:
        assert _have_parquet(), 'a parquet engine is part of the environment the consumer is tested in'
        pd.DataFrame(cols).to_parquet(path)
    yt, yp = metrics.read_group_predictions(path)
    assert np.array_equal(yt, y_true) and np.array_equal(yp, y_pred)


def test_read_group_predictions_errors(tmp_path):
    with pytest.raises(OSError, match='Could not find predictions file'):
        metrics.read_group_predictions(str(tmp_path / 'missing.csv'))
    p = tmp_path / 'preds.txt'
    p.write_text('y_true1,y_pred0,y_pred1\n0,1,0\n')
    with pytest.raises(ValueError, match='Unrecognized extension'):
        metrics.read_group_predictions(str(p))
    for cols, match in (({'a-y_true': [0], 'b-y_true': [1], 'y_pred0': [0.1], 'y_pred1': [0.9]}, 'Could not find y_true'),
                        ({'y_pred0': [0.1], 'y_pred1': [0.9]}, 'Could not find y_true'),
                        ({'y_true1': [0], 'y_pred1': [0.9]}, 'Expected exactly 2 y_pred columns .*; got 1'),
                        ({'y_true1': [0], 'y_pred0': [0.1], 'y_pred1': [0.9], 'y_pred2': [0.0]}, 'got 3')):
        path = str(tmp_path / 'bad.csv')
        pd.DataFrame(cols).to_csv(path, index=False)
        with pytest.raises(ValueError, match=match):
            metrics.read_group_predictions(path)


# ---------------------------------------------------------------------------------------------------------------- command line
def _tile_table(path, seed, drop_last=False):
    """3 slides, 40 tiles, with positions, under Slideflow's headers."""
    from biscuit_amd import predictions
    rng = np.random.default_rng(seed)
    slides = np.repeat(['s0', 's1', 's2'], [14, 13, 13])
    y = np.repeat([0, 1, 1], [14, 13, 13])
    loc = np.stack([np.arange(40) % 7 * 100, np.arange(40) // 7 * 100], 1)
    p1 = np.clip(0.35 + 0.3 * y + 0.2 * rng.normal(size=40), 0.01, 0.99)
    mean2, std2 = np.stack([1 - p1, p1], 1), np.full((40, 2), 0.02)
    df = predictions.tile_frame('cohort', slides, y, mean2, std2, loc)
    o = np.random.default_rng(9).permutation(40) if seed % 2 else np.arange(40)          # the second table in another row order
    df = df.iloc[o[:-1] if drop_last else o]
    df.to_csv(path, index=False)
    return df


def test_cli_one_table_and_a_comparison(tmp_path):
    a, b, out = str(tmp_path / 'a.csv'), str(tmp_path / 'b.csv'), str(tmp_path / 'sub' / 'm.json')
    da, db = _tile_table(a, 2), _tile_table(b, 3)
    assert metrics.main([a, '--threshold', '0.5', '--outcome', 'cohort', '--level', 'tile', '--seed', '7', '--host', '--out', out]) == 0
    with open(out) as f:
        one = json.load(f)
    y, p = da['cohort-y_true0'].to_numpy(), da['cohort-y_pred1'].to_numpy()
    want = metrics.prediction_metrics(y, p, 0.5, seed=7)
    auc, var = metrics.delong_roc_variance(y, p)
    assert one['rows'] == 40 and one['compare'] == [] and one['path'] == 'host' and (one['n_pos'], one['n_neg']) == (26, 14)
    assert one['auc'] == auc and one['auc_var'] == var and all(one[k] == float(v) for k, v in want.items())
    assert metrics.main([a, '--compare', b, '--threshold', '0.5', '--outcome', 'cohort', '--level', 'tile', '--seed', '7', '--host', '--out', out]) == 0
    with open(out) as f:
        two = json.load(f)
    assert {k: v for k, v in two.items() if k != 'compare'} == {k: v for k, v in one.items() if k != 'compare'}
    q = db.sort_index()['cohort-y_pred1'].to_numpy()                                     # matched on slide and position
    (cmp,) = two['compare']
    assert cmp['table'] == b and cmp['auc'] == metrics.delong_roc_variance(y, q)[0]
    assert cmp['log10_p'] == float(metrics.delong_roc_test(y, p, q)[0, 0]) and cmp['log10_p'] < 0
    # slide level: three rows, the tile rows reduced
    assert metrics.main([a, '--threshold', '0.5', '--outcome', 'cohort', '--level', 'slide', '--seed', '7', '--host', '--out', out]) == 0
    with open(out) as f:
        assert json.load(f)['rows'] == 3


def test_cli_refuses_mismatched_row_sets(tmp_path):
    a, b, out = str(tmp_path / 'a.csv'), str(tmp_path / 'b.csv'), str(tmp_path / 'm.json')
    _tile_table(a, 2)
    db = _tile_table(b, 3, drop_last=True)
    missing = set(range(40)) - set(db.index)
    (row,) = missing
    with pytest.raises(ValueError, match=rf"row \('s\d', {row % 7 * 100}, {row // 7 * 100}\) of the first table is missing"):
        metrics.main([a, '--compare', b, '--threshold', '0.5', '--outcome', 'cohort', '--level', 'tile', '--host', '--out', out])
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match='is not in the first table'):
        metrics.main([b, '--compare', a, '--threshold', '0.5', '--outcome', 'cohort', '--level', 'tile', '--host', '--out', out])


def test_cli_takes_a_group_predictions_file(tmp_path):
    y, P = R.case('n64')
    path, out = str(tmp_path / 'slide_predictions.csv'), str(tmp_path / 'm.json')
    pd.DataFrame({'slide': [f's{i}' for i in range(64)], 'cohort-y_true': y, 'cohort-y_pred0': 1 - P[0], 'cohort-y_pred1': P[0]}).to_csv(path, index=False)
    assert metrics.main([path, '--threshold', '0.5', '--seed', '3', '--host', '--out', out]) == 0
    with open(out) as f:
        got = json.load(f)
    assert got['rows'] == 64 and got['auc'] == metrics.delong_host(y, P[0])['auc'][0]
