"""The metrics behind the reference's result tables (``biscuit/utils.py:364-504``: ``read_group_predictions``,
``prediction_metrics``, ``auc_and_threshold``; ``biscuit/delong.py``: DeLong's covariance of correlated AUROCs, the variance the
AUROC's 95 % interval is built on, and ``delong_roc_test``) under the reference's names, for a table of any size: DeLong's covariance
of k classifiers over n rows is one sort and a few scans per classifier on the GPU (``Engine.delong``, ``csrc/kernels_delong.hip``)
or, for small tables, the same definitions in vectorised numpy (``delong_host``).  Definitions: DESIGN.md section 7 "Prediction
metrics".  The Youden bootstrap (75 000 draws) stays on the host, seeded on request.

    python -m biscuit_amd.metrics TABLE [--compare TABLE2 ...] --threshold T [--outcome NAME] [--level tile|slide|patient]
                                  [--labels CSV] [--seed S] [--host] --out FILE.json
"""
import argparse
import json
import logging
import os
import statistics
import warnings

import numpy as np
import pandas as pd

log = logging.getLogger('biscuit_amd')

MAX_K, MAX_ROWS = 8, 1 << 25                # bq_delong's limits: the midrank sums stay exact integers below 2^53
# Rows from which a table goes to the device when ``threshold.use_device`` is in force (profiles/metrics.txt: the smallest measured n
# at which the whole device call, upload and read-back included, is faster than ``delong_host`` at k = 1 -- 0.78 ms against 19.6 ms
# at 200 000 rows, 5.2 ms against 196 ms at 1.6 M; at 1 000 rows the host's 0.10 ms beats the device call's 0.14 ms).  None would
# route on an explicit engine only.
DEFAULT_MIN_ROWS = 200_000


# ---------------------------------------------------------------------------------------------------------------- DeLong
def _inputs(y_true, scores):
    """``(label bool [n], P float64 [k, n])``; ValueError for what the definitions refuse."""
    y = np.asarray(y_true).reshape(-1)
    P = np.ascontiguousarray(scores, dtype=np.float64)
    if P.ndim == 1:
        P = P.reshape(1, -1)
    if P.ndim != 2 or not 1 <= P.shape[0] <= MAX_K:
        raise ValueError(f'delong: scores are [k, n] with 1 <= k <= {MAX_K}, not {P.shape}')
    n = P.shape[1]
    if n == 0 or len(y) != n or n > MAX_ROWS:
        raise ValueError(f'delong: empty input, length mismatch or more than 2^25 rows ({n} scores, {len(y)} labels)')
    if np.isnan(P).any():
        raise ValueError('delong: a score is NaN')
    if y.dtype != bool and not np.isin(y, (0, 1)).all():
        raise ValueError('delong: labels must be 0/1')
    y = y != 0
    if y.all() or not y.any():
        raise ValueError('delong: only one class present')
    return y, P


def _unbiased_cov(X):
    """``numpy.cov`` of the rows of ``X`` as a 2-D matrix; NaN, silently, for a single column."""
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', category=RuntimeWarning)
        return np.atleast_2d(np.cov(X))


def delong_host(y_true, scores, components=False):
    """``Engine.delong`` in numpy float64: the same definitions and the same result layout.  One argsort per classifier and the
    tie runs' bounds from it; no Python loop over rows."""
    y, P = _inputs(y_true, scores)
    k, n = P.shape
    m = int(y.sum())
    n0 = n - m
    V = np.empty((k, n))
    auc = np.empty(k)
    for r in range(k):
        order = np.argsort(P[r], kind='stable')
        key, lab = P[r][order], y[order]
        start = np.empty(n, bool)
        start[0] = True
        np.not_equal(key[1:], key[:-1], out=start[1:])          # -0.0 == +0.0: one run
        first = np.flatnonzero(start)
        run = np.cumsum(start) - 1
        s, e = first[run], np.append(first[1:], n)[run]         # the row's tie run [s, e) in ascending order
        cum = np.concatenate([[0], np.cumsum(lab)])             # cum[j]: positives among the first j sorted rows
        below_pos, tied_pos = cum[s], cum[e] - cum[s]
        below_neg, tied_neg = s - below_pos, (e - s) - tied_pos
        v = np.where(lab, (0.5 * (2 * below_neg + tied_neg)) / float(n0), 1.0 - (0.5 * (2 * below_pos + tied_pos)) / float(m))
        V[r, order] = v
        tz2 = int((s + e + 1)[lab].sum())                       # sum of 2 tz over the positives, an exact integer
        auc[r] = (0.5 * tz2) / float(m) / float(n0) - ((m + 1.0) / 2.0) / float(n0)
    cov = _unbiased_cov(V[:, y]) / m + _unbiased_cov(V[:, ~y]) / n0
    res = {'auc': auc, 'cov': cov, 'n_pos': m, 'n_neg': n0}
    if components:
        res['V'] = V
    return res


def _route(engine, n):
    """The engine a table of ``n`` rows goes to, or None for the host: an engine given by the caller always; the one of
    ``threshold.use_device`` from ``DEFAULT_MIN_ROWS`` rows on, once that bound is set -- ``calibration._route``'s rule."""
    if engine is not None:
        return engine
    from . import threshold
    eng = threshold._DEVICE['engine']
    if eng is not None and DEFAULT_MIN_ROWS is not None and n >= DEFAULT_MIN_ROWS:
        return eng
    return None


def delong_covariance(y_true, scores, *, engine=None, components=False):
    """AUROC and DeLong's covariance of k classifiers (``scores`` [k, n], or [n] for one) scored on the same rows: the
    generalisation of ``delong_roc_variance`` (k = 1) and of the 2 x 2 matrix behind ``delong_roc_test``.  -> ``{'auc' [k], 'cov'
    [k, k], 'n_pos', 'n_neg', 'path'}`` and, with ``components``, ``'V' [k, n]``.  ``engine``: run it there; without one, on the
    host unless ``threshold.use_device`` routes the table to its engine."""
    n = int(np.shape(scores)[-1]) if np.ndim(scores) else 0
    eng = _route(engine, n)
    if eng is not None:
        res = eng.delong(y_true, scores, components=components)
        res['path'] = 'device'
    else:
        res = delong_host(y_true, scores, components=components)
        res['path'] = 'host'
    return res


def delong_roc_variance(y_true, y_pred, *, engine=None):
    """``(auc, var)`` of one classifier (``delong.py:96-107``): the AUROC and DeLong's variance of it."""
    res = delong_covariance(y_true, np.asarray(y_pred).reshape(1, -1), engine=engine)
    return res['auc'][0], res['cov'][0, 0]


def _log10_p(auc, cov):
    """``delong.py:76-86`` on the host from the 2 x 2 matrix: shape (1, 1); 0 / 0 gives NaN as there."""
    from scipy import stats
    c = np.array([[1, -1]])
    with np.errstate(divide='ignore', invalid='ignore'):
        z = np.abs(np.diff(auc)) / np.sqrt(np.dot(np.dot(c, cov), c.T))
        return np.log10(2) + stats.norm.logsf(z, loc=0, scale=1) / np.log(10)


def delong_roc_test(y_true, p1, p2, *, engine=None):
    """log10 of the p-value of the hypothesis that two AUROCs on the same rows differ (``delong.py:110-123``), shape (1, 1)."""
    res = delong_covariance(y_true, np.vstack((np.asarray(p1).reshape(-1), np.asarray(p2).reshape(-1))), engine=engine)
    return _log10_p(res['auc'], res['cov'])


# ---------------------------------------------------------------------------------------------------------------- the tables' metrics
def prediction_metrics(y_true, y_pred, threshold, seed=None, *, engine=None):
    """``biscuit/utils.py:400-464``, quirks kept: ``y_pred > threshold``; the AUROC's interval ``norm.ppf([0.025, 0.975], auc,
    sqrt(var))`` clipped above 1 only; ``[None, None]`` with a warning when the labels are not exactly {0, 1}; Youden's interval
    from 500 resamples of 150 row indices with the z^2-adjusted rates.  The resamples are the reference's calls, one
    ``choice(np.arange(N), size=(150,))`` each: from NumPy's global legacy generator with ``seed=None`` (``np.random.seed(s)``
    before the call gives the reference's numbers), from ``np.random.RandomState(seed)`` otherwise -- the same stream, the global
    state untouched."""
    from scipy import stats
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    yt = y_true.astype(bool)
    yp = y_pred > threshold
    alpha = 0.05
    z = stats.norm.ppf((1 - alpha / 2))
    tp = np.logical_and(yt, yp).sum()
    fp = np.logical_and(np.logical_not(yt), yp).sum()
    tn = np.logical_and(np.logical_not(yt), np.logical_not(yp)).sum()
    fn = np.logical_and(yt, np.logical_not(yp)).sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        acc = (tp + tn) / (tp + tn + fp + fn)
        sensitivity = tp / (tp + fn)
        specificity = tn / (tn + fp)

    choice = np.random.choice if seed is None else np.random.RandomState(seed).choice
    rows = np.arange(yt.shape[0])
    all_jac = []
    for _ in range(500):
        i = choice(rows, size=(150,))
        _yt, _yp = yt[i], yp[i]
        _tp = np.logical_and(_yt, _yp).sum()
        _fp = np.logical_and(np.logical_not(_yt), _yp).sum()
        _tn = np.logical_and(np.logical_not(_yt), np.logical_not(_yp)).sum()
        _fn = np.logical_and(_yt, np.logical_not(_yp)).sum()
        all_jac.append(((_tn + 0.5 * z**2) / (_tn + _fp + z**2)) - ((_fn + 0.5 * z**2) / (_fn + _tp + z**2)))
    jac = statistics.mean(all_jac)
    jac_var = statistics.variance(all_jac)
    jac_low = jac - z * np.sqrt(jac_var)
    jac_high = jac + z * np.sqrt(jac_var)

    if not np.array_equal(np.unique(y_true), [0, 1]):
        log.warning('Unable to calculate CI; NaNs exist')
        ci = [None, None]
    else:
        auc, var = delong_roc_variance(y_true, y_pred, engine=engine)
        q = np.abs(np.array([0, 1]) - alpha / 2)
        with np.errstate(invalid='ignore'):
            ci = stats.norm.ppf(q, loc=auc, scale=np.sqrt(var))
        ci[ci > 1] = 1
    return {'auc_low': ci[0], 'auc_high': ci[1], 'acc': acc, 'sens': sensitivity, 'spec': specificity,
            'youden': sensitivity + specificity - 1, 'youden_low': jac_low, 'youden_high': jac_high}


def auc_and_threshold(y_true, y_pred):
    """``(AUROC, threshold at the first maximum of tpr - fpr)`` over scikit-learn's ROC curve (``biscuit/utils.py:467-484``)."""
    from sklearn import metrics
    from . import threshold
    fpr, tpr, thresh = threshold._roc(y_true, y_pred)
    return metrics.auc(fpr, tpr), threshold._youden(fpr, tpr, thresh)


def read_group_predictions(path):
    """``(y_true, y_pred)`` of a patient- or slide-level predictions file, CSV or parquet (``biscuit/utils.py:364-397``): the
    labels are ``y_true1`` or else the single column ending in ``y_true``; the predictions ``percent_tiles_positive1`` or else
    the second of exactly two columns with ``y_pred`` in their name.  OSError for a missing file, ValueError otherwise."""
    if not os.path.exists(path):
        raise OSError(f'Could not find predictions file at {path}')
    ext = os.path.splitext(path)[1][1:].lower()
    if ext == 'csv':
        df = pd.read_csv(path)
    elif ext in ('parquet', 'gzip'):
        df = pd.read_parquet(path)
    else:
        raise ValueError(f'Unrecognized extension for prediction file {path}')
    if 'y_true1' in df.columns:
        y_true = df['y_true1'].to_numpy()
    else:
        cols = [c for c in df.columns if c.endswith('y_true')]
        if len(cols) != 1:
            raise ValueError(f'Could not find y_true column at {path}')
        y_true = df[cols[0]].to_numpy()
    if 'percent_tiles_positive1' in df.columns:
        y_pred = df['percent_tiles_positive1'].to_numpy()
    else:
        cols = [c for c in df.columns if 'y_pred' in c]
        if len(cols) != 2:
            raise ValueError(f'Expected exactly 2 y_pred columns at {path}; got {len(cols)}')
        y_pred = df[cols[1]].to_numpy()
    return y_true, y_pred


# ---------------------------------------------------------------------------------------------------------------- command line
def _is_tile_table(path, outcome):
    if os.path.isdir(path):
        return True
    cols = pd.read_parquet(path).columns if path.endswith(('.parquet', '.gzip')) else pd.read_csv(path, nrows=0).columns
    return outcome is not None and 'slide' in cols and any(c in cols for c in (f'{outcome}-y_pred1', f'{outcome}_y_pred1'))


def load_rows(path, level, outcome=None, patients=None):
    """One table as ``(keys, y_true, y_pred)``: a tile table (``predictions.load_tile_predictions``; ``outcome`` names its
    columns) at ``level`` 'tile' -- the key of a row is (slide, loc_x, loc_y) where the table has positions, else (slide, its
    number within the slide) -- or reduced to 'slide' / 'patient' rows by ``threshold.process_group_predictions``, the key the
    group; a group-predictions file (``read_group_predictions``) as it is, the key its ``slide`` / ``patient`` column or the
    row number."""
    from . import predictions, threshold
    path = os.fspath(path)
    if not _is_tile_table(path, outcome):
        if level == 'tile':
            raise ValueError(f'{path}: not a tile table of outcome {outcome!r}; --level tile needs one')
        y_true, y_pred = read_group_predictions(path)
        df = pd.read_csv(path) if path.lower().endswith('csv') else pd.read_parquet(path)
        keys = [str(v) for v in df[level]] if level in df.columns else [str(i) for i in range(len(df))]
        return keys, y_true, y_pred
    df = predictions.load_tile_predictions(path, outcome)
    if level == 'tile':
        if 'loc_x' in df.columns:
            keys = list(zip(df['slide'], df['loc_x'].astype(int), df['loc_y'].astype(int)))
        else:
            keys = list(zip(df['slide'], df.groupby('slide', sort=False).cumcount()))
        return keys, df['y_true'].to_numpy(), df['y_pred'].to_numpy()
    if level == 'patient':
        if patients is None:
            raise ValueError('--level patient needs --labels (slide, patient)')
        df['patient'] = df['slide'].map(patients)
    g, _ = threshold.process_group_predictions(df, pred_thresh=0.5, level=level)
    return [str(v) for v in g[level]], g['y_true'].to_numpy(), g['y_pred'].to_numpy()


def _align(first, other, name):
    """The rows of ``other`` in the order of ``first``; ValueError naming the first difference of the two row sets."""
    keys, y, _ = first
    okeys, oy, op = other
    at = {}
    for i, key in enumerate(okeys):
        if key in at:
            raise ValueError(f'{name}: row {key!r} appears twice')
        at[key] = i
    for key in keys:
        if key not in at:
            raise ValueError(f'{name}: row {key!r} of the first table is missing')
    have = set(keys)
    for key in okeys:
        if key not in have:
            raise ValueError(f'{name}: row {key!r} is not in the first table')
    take = np.array([at[key] for key in keys], dtype=np.int64)
    if not np.array_equal(np.asarray(oy)[take] != 0, np.asarray(y) != 0):
        bad = int(np.flatnonzero((np.asarray(oy)[take] != 0) != (np.asarray(y) != 0))[0])
        raise ValueError(f'{name}: the label of row {keys[bad]!r} differs from the first table')
    return np.asarray(op)[take]


def _jsonable(v):
    if v is None:
        return None
    v = float(v)
    return v if np.isfinite(v) else None


def table_metrics(y_true, y_pred, threshold, seed=None, engine=None):
    """``prediction_metrics`` plus ``auc``, ``auc_var``, ``n_pos`` and ``n_neg`` as plain numbers (NaN and the missing interval:
    None); the AUROC's entries are None where the labels are not exactly {0, 1}."""
    out = {k: _jsonable(v) for k, v in prediction_metrics(y_true, y_pred, threshold, seed=seed, engine=engine).items()}
    if np.array_equal(np.unique(y_true), [0, 1]):
        res = delong_covariance(y_true, y_pred, engine=engine)
        out.update(auc=_jsonable(res['auc'][0]), auc_var=_jsonable(res['cov'][0, 0]), n_pos=res['n_pos'], n_neg=res['n_neg'])
    else:
        out.update(auc=None, auc_var=None, n_pos=int((np.asarray(y_true) != 0).sum()), n_neg=int((np.asarray(y_true) == 0).sum()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.metrics', description=__doc__.split('\n\n')[0])
    ap.add_argument('table', help='a tile-prediction table (CSV, parquet or a run directory) or a group-predictions file')
    ap.add_argument('--compare', nargs='+', default=[], metavar='TABLE', help='tables of the same rows: their metrics and the DeLong test against TABLE')
    ap.add_argument('--threshold', type=float, required=True)
    ap.add_argument('--outcome', help='the outcome that names a tile table\'s columns')
    ap.add_argument('--level', choices=('tile', 'slide', 'patient'), default='slide')
    ap.add_argument('--labels', help='CSV with columns slide, patient')
    ap.add_argument('--seed', type=int, help='seed of the Youden bootstrap; without one, NumPy\'s global generator')
    ap.add_argument('--host', action='store_true', help='numpy on the host; otherwise DeLong\'s covariance runs on the GPU')
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    patients = None
    if a.labels:
        lab = pd.read_csv(a.labels, dtype=str)
        patients = dict(zip(lab['slide'], lab['patient']))
    first = load_rows(a.table, a.level, a.outcome, patients)
    others = [(t, _align(first, load_rows(t, a.level, a.outcome, patients), t)) for t in a.compare]
    engine = None
    if not a.host:
        from .engine import Engine
        from .weights import synthetic_weights
        engine = Engine(synthetic_weights(1), max_batch=1, max_mc=1)     # the tool needs a context, not a trained network
    try:
        _, y, p = first
        result = {'table': os.fspath(a.table), 'level': a.level, 'threshold': a.threshold, 'seed': a.seed, 'rows': len(y),
                  'path': 'host' if a.host else 'device', **table_metrics(y, p, a.threshold, a.seed, engine), 'compare': []}
        for name, q in others:
            entry = {'table': os.fspath(name), **table_metrics(y, q, a.threshold, a.seed, engine)}
            if np.array_equal(np.unique(y), [0, 1]):
                entry['log10_p'] = _jsonable(delong_roc_test(y, p, q, engine=engine)[0, 0])
            else:
                entry['log10_p'] = None
            result['compare'].append(entry)
    finally:
        if engine is not None:
            engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(a.out)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
