"""The data behind the reference's UQ calibration figure (``biscuit/threshold.py:15-122``, ``plot_uncertainty``;
``Experiment.plot_uq_calibration``, ``experiment.py:437-486``) over EVERY row of a table, deterministically: the density of the
uncertainty split by correct / incorrect, the prediction-versus-uncertainty scatter split at the threshold, and the LOESS curve of
P(correct | uncertainty) with its confidence band.  The reference draws the figure from ``df.sample(n=1000)``, unseeded, because
its estimators are an N x N operator and a direct sum; here both are dense sums on the GPU (``Engine.uq_kde`` / ``Engine.uq_loess``,
``csrc/kernels_calib.hip``) or, for small tables, the same definitions in numpy.  Definitions: DESIGN.md section 7 "UQ calibration".
Drawing is left to the reader: ``Calibration.save`` writes the curves as CSV.

    python -m biscuit_amd.calibration TABLE.csv [TABLE.csv ...] --outcome cohort --tile-uq X --slide-uq Y [--slide-pred P]
                                      [--labels CSV] --out DIR [--seed N] [--host]
"""
import argparse
import json
import os
from dataclasses import dataclass, field

import numpy as np
import pandas as pd

GROUPS = ('incorrect', 'correct')           # index = the value of ``correct``
# Rows from which a table goes to the device when ``threshold.use_device`` is in force and names no smaller bound
# (profiles/calibration.txt: the device path, upload and read-back included, is faster at every size measured -- 0.2 ms against
# 18.7 ms at 1 000 rows, 4.7 ms against 32.5 s at 1.6 M -- so the bound is the smallest size measured; below it a host call
# costs under 20 ms).
DEFAULT_MIN_ROWS = 1_000


# ---------------------------------------------------------------------------------------------------------------- host path
def _inputs(x, correct):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(np.asarray(correct) != 0).reshape(-1)
    if len(x) == 0 or len(c) != len(x):
        raise ValueError('calibration: empty input or length mismatch')
    if not np.isfinite(x).all():
        raise ValueError('calibration: uncertainty must be finite')
    return x, c


def kde_host(x, correct, grid=200, cut=3.0):
    """``Engine.uq_kde`` in numpy float64: the same definitions and the same result layout."""
    x, c = _inputs(x, correct)
    grid = int(grid)
    out = {'support': np.full((2, grid), np.nan), 'density': np.full((2, grid), np.nan), 'n': np.zeros(2, np.int64),
           'min': np.zeros(2), 'max': np.zeros(2), 'mean': np.zeros(2), 'std': np.zeros(2), 'bw': np.zeros(2),
           'valid': np.zeros(2, bool)}
    for g in (0, 1):
        xg = x[c == bool(g)]
        n = len(xg)
        out['n'][g] = n
        out['min'][g], out['max'][g] = (xg.min(), xg.max()) if n else (np.inf, -np.inf)
        out['mean'][g] = xg.mean() if n else 0.0
        sd = float(np.std(xg, ddof=1)) if n >= 2 else 0.0
        out['std'][g] = sd
        if n < 2 or not sd > 0.0:
            continue
        bw = sd * n ** (-0.2)
        sup = np.linspace(xg.min() - cut * bw, xg.max() + cut * bw, grid)
        dens = np.empty(grid)
        step = max(1, (1 << 22) // n)                # support points per block: at most 4 M terms at a time
        for a in range(0, grid, step):
            z = (xg[None, :] - sup[a:a + step, None]) / bw
            dens[a:a + step] = np.exp(-0.5 * z * z).sum(axis=1)
        out['bw'][g], out['valid'][g] = bw, True
        out['support'][g], out['density'][g] = sup, dens / (n * bw * np.sqrt(2.0 * np.pi))
    return out


def loess_host(x, correct, grid=200, span=0.75):
    """``Engine.uq_loess`` in numpy float64: the same definitions and the same result layout."""
    x, c = _inputs(x, correct)
    grid, n = int(grid), len(x)
    q = int(np.floor(span * n + 1e-5)) if span > 0 else 0
    if not 1 <= q <= n:
        raise ValueError(f'calibration: the window of span {span!r} over {n} rows holds {q} rows; it must hold 1 .. {n}')
    order = np.argsort(x, kind='stable')
    xs, ys = x[order], c[order].astype(np.float64)
    v = np.linspace(xs[0], xs[-1], grid)
    h = np.empty(grid)
    mom = np.zeros((grid, 13))
    for k, x0 in enumerate(v):
        # the q-th smallest |x - x0|: the q nearest rows are consecutive in sorted order
        h[k] = np.minimum.reduce(np.maximum(x0 - xs[:n - q + 1], xs[q - 1:] - x0))
        if not h[k] > 0.0:
            continue
        a, b = np.searchsorted(xs, x0 - h[k], 'left'), np.searchsorted(xs, x0 + h[k], 'right')
        u = (xs[a:b] - x0) / h[k]
        au = np.abs(u)
        w = np.where(au < 1.0, (1.0 - au ** 3) ** 3, 0.0)
        wy, w2 = w * ys[a:b], w * w
        p = np.stack([np.ones_like(u), u, u * u, u ** 3, u ** 4])
        mom[k, 0:5], mom[k, 5:8], mom[k, 8:13] = p @ w, p[:3] @ wy, p @ w2
    m, t, r = mom[:, 0:5], mom[:, 5:8], mom[:, 8:13]
    c0, c1, c2 = m[:, 2] * m[:, 4] - m[:, 3] ** 2, m[:, 1] * m[:, 4] - m[:, 2] * m[:, 3], m[:, 1] * m[:, 3] - m[:, 2] ** 2
    det = m[:, 0] * c0 - m[:, 1] * c1 + m[:, 2] * c2
    bad = ~(h > 0.0) | ~(m[:, 0] > 0.0) | (np.abs(det) < 1e-12 * m[:, 0] ** 3)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.stack([c0 / det, -c1 / det, c2 / det], 1)
    a[bad] = np.nan
    fit = (a * t).sum(1)
    l2 = sum(a[:, i] * a[:, j] * r[:, i + j] for i in range(3) for j in range(3))
    lam = a[:, 0].copy()
    zi, li = interpolate(v, fit, xs), interpolate(v, lam, xs)
    return {'vertex': v, 'fit': fit, 'l2': l2, 'lam': lam, 'h': h, 'nu': float(li.sum()), 'rss': float(((ys - zi) ** 2).sum()),
            'degenerate': int(bad.sum()), 'q': q, 'n': n}


def interpolate(v, f, x):
    """The piecewise-linear interpolant of ``f`` over the vertices ``v`` at ``x``: the segment of a row is the last one whose left
    vertex is <= x (0 .. G - 2); a segment that touches a degenerate vertex gives NaN."""
    j = np.clip(np.searchsorted(v, x, 'right') - 1, 0, len(v) - 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = (x - v[j]) / (v[j + 1] - v[j])
        return f[j] + w * (f[j + 1] - f[j])


def band(raw, level=0.975):
    """What the curve's band needs beyond the fit, from the result of ``uq_loess`` / ``loess_host``: ``(s, dof, t, se, lower,
    upper)`` with dof = N - nu, s^2 = rss / dof, t = t_{level, dof} (``scipy.stats.t.ppf``), se = s sqrt(l2)."""
    from scipy import stats
    dof = raw['n'] - raw['nu']
    with np.errstate(invalid='ignore', divide='ignore'):
        s = float(np.sqrt(raw['rss'] / dof)) if dof > 0 else float('nan')
        tq = float(stats.t.ppf(level, dof)) if dof > 0 else float('nan')
        se = s * np.sqrt(raw['l2'])
    return s, float(dof), tq, se, raw['fit'] - tq * se, raw['fit'] + tq * se


# ---------------------------------------------------------------------------------------------------------------- the result
@dataclass
class Calibration:
    """``kde``: {group: {'support', 'density' (scaled by n_g / N, seaborn's common normalisation), 'density_unit' (integrating to 1),
    'bandwidth'}} for the groups that have a curve; ``loess``: {'vertex', 'fit', 'se', 'lower', 'upper', 'h'}; ``scatter``: a frame
    of y_pred, uncertainty, correct, above; ``summary``: N, the groups' counts, q, s, nu, the t quantile, degenerate vertices, the
    threshold, the kind, the title and which path ran."""
    kind: str
    kde: dict = field(default_factory=dict)
    loess: dict = field(default_factory=dict)
    scatter: pd.DataFrame = None
    summary: dict = field(default_factory=dict)

    def frames(self):
        kde = pd.concat([pd.DataFrame({'group': g, 'support': d['support'], 'density': d['density'], 'density_unit': d['density_unit'],
                                       'bandwidth': d['bandwidth']}) for g, d in self.kde.items()] or
                        [pd.DataFrame({'group': pd.Series([], dtype=str), 'support': [], 'density': [], 'density_unit': [], 'bandwidth': []})],
                        ignore_index=True)
        return kde, pd.DataFrame(self.loess), self.scatter

    @staticmethod
    def paths(directory, kind, prefix='uq_calibration'):
        stem = os.path.join(os.fspath(directory), f'{prefix}_{kind}')
        return {k: f'{stem}_{k}.csv' for k in ('kde', 'loess', 'scatter')} | {'summary': f'{stem}_summary.json'}

    def save(self, directory, prefix='uq_calibration'):
        """Writes ``{prefix}_{kind}_kde.csv``, ``_loess.csv``, ``_scatter.csv`` and ``_summary.json`` -> their paths."""
        os.makedirs(directory, exist_ok=True)
        paths = self.paths(directory, self.kind, prefix)
        for key, frame in zip(('kde', 'loess', 'scatter'), self.frames()):
            frame.to_csv(paths[key], index=False)
        with open(paths['summary'], 'w') as f:
            json.dump(self.summary, f, indent=1, allow_nan=True)
        return paths

    @classmethod
    def load(cls, directory, kind, prefix='uq_calibration'):
        """What ``save`` wrote, value for value."""
        paths = cls.paths(directory, kind, prefix)
        k = pd.read_csv(paths['kde'], float_precision='round_trip', dtype={'group': str})
        kde = {g: {'support': d['support'].to_numpy(), 'density': d['density'].to_numpy(), 'density_unit': d['density_unit'].to_numpy(),
                   'bandwidth': float(d['bandwidth'].iloc[0])} for g, d in k.groupby('group', sort=False)}
        lo = pd.read_csv(paths['loess'], float_precision='round_trip')
        sc = pd.read_csv(paths['scatter'], float_precision='round_trip')
        with open(paths['summary']) as f:
            summary = json.load(f)
        return cls(kind, kde, {c: lo[c].to_numpy(dtype=np.float64) for c in lo.columns}, sc, summary)


def _route(engine, n):
    """The engine a table of ``n`` rows goes to, or None for the host: an engine given by the caller always; the one of
    ``threshold.use_device`` from its bound for this tool on -- ``_youden_threshold``'s rule."""
    if engine is not None:
        return engine
    from . import threshold
    eng = threshold._DEVICE['engine']
    if eng is not None and n >= threshold._DEVICE.get('calibration_min_rows', DEFAULT_MIN_ROWS):
        return eng
    return None


def uncertainty_calibration(df, kind, threshold=None, *, engine=None, grid=200, span=0.75, sample=1000, seed=0, title=None):
    """The calibration data of a processed frame (columns ``uncertainty``, ``correct``, ``y_pred``; ``process_tile_predictions`` /
    ``process_group_predictions`` make one) over all of its rows.  ``kind``: 'tile' draws the scatter panel's rows as a seeded
    sample of ``min(sample, N)`` (``numpy.random.default_rng(seed).choice``, without replacement); any other kind keeps them all.
    ``engine``: run the sums there; without one, on the host unless ``threshold.use_device`` routes the table to its engine."""
    x, c = _inputs(df['uncertainty'].to_numpy(), df['correct'].to_numpy())
    n = len(x)
    eng = _route(engine, n)
    if eng is not None:
        kraw, lraw, path = eng.uq_kde(x, c, grid=grid), eng.uq_loess(x, c, grid=grid, span=span), 'device'
    else:
        kraw, lraw, path = kde_host(x, c, grid=grid), loess_host(x, c, grid=grid, span=span), 'host'
    kde, missing = {}, []
    for g, name in enumerate(GROUPS):
        if kraw['valid'][g]:
            kde[name] = {'support': kraw['support'][g], 'density': kraw['density'][g] * (int(kraw['n'][g]) / n),
                         'density_unit': kraw['density'][g], 'bandwidth': float(kraw['bw'][g])}
        else:
            missing.append(name)
    s, dof, tq, se, lower, upper = band(lraw)
    loess = {'vertex': lraw['vertex'], 'fit': lraw['fit'], 'se': se, 'lower': lower, 'upper': upper, 'h': lraw['h']}
    if kind == 'tile':
        rows = np.sort(np.random.default_rng(seed).choice(n, size=min(int(sample), n), replace=False))
        sub = df.iloc[rows]
    else:
        sub = df
    unc = sub['uncertainty'].to_numpy(dtype=np.float64)
    scatter = pd.DataFrame({'y_pred': sub['y_pred'].to_numpy(dtype=np.float64), 'uncertainty': unc,
                            'correct': sub['correct'].to_numpy().astype(bool),
                            'above': unc >= threshold if threshold is not None else np.zeros(len(unc), bool)})
    summary = {'kind': str(kind), 'title': title, 'threshold': None if threshold is None else float(threshold), 'N': n,
               'n_correct': int(kraw['n'][1]), 'n_incorrect': int(kraw['n'][0]), 'no_density': missing, 'grid': int(grid),
               'span': float(span), 'q': int(lraw['q']), 's': s, 'nu': float(lraw['nu']), 'dof': dof, 't': tq,
               'degenerate_vertices': int(lraw['degenerate']), 'scatter_rows': len(scatter), 'seed': int(seed), 'path': path}
    return Calibration(str(kind), kde, loess, scatter, summary)


def uq_calibration(tables, outcome, tile_uq, slide_uq, slide_pred, patients=None, *, engine=None, grid=200, span=0.75, sample=1000,
                   seed=0, title=None):
    """``Experiment.plot_uq_calibration`` (``experiment.py:437-486``) without the project locator: ``tables`` -- the cross-validation
    tile tables, paths or frames -- are read, renamed and concatenated, ``process_tile_predictions`` marks the tiles, the tile-level
    calibration is computed at ``tile_uq``, the strict ``< tile_uq`` filter applied, ``process_group_predictions`` reduces to slides
    and the slide-level calibration is computed at ``slide_uq``.  -> ``(tile Calibration, slide Calibration)``."""
    from . import predictions, threshold
    frames = []
    for t in tables:
        if isinstance(t, pd.DataFrame):
            t = t.copy()
            predictions.rename_cols(t, outcome)
        else:
            t = predictions.load_tile_predictions(os.fspath(t), outcome)
        frames.append(t)
    df = pd.concat(frames, axis=0, join='outer', ignore_index=True)
    df, _ = threshold.process_tile_predictions(df, patients=patients)
    kw = dict(engine=engine, grid=grid, span=span, sample=sample, seed=seed, title=title)
    tile = uncertainty_calibration(df, 'tile', tile_uq, **kw)
    df = df[df['uncertainty'] < tile_uq]
    s_df, _ = threshold.process_group_predictions(df, pred_thresh=slide_pred, level='slide')
    return tile, uncertainty_calibration(s_df, 'slide', slide_uq, **kw)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.calibration', description=__doc__.split('\n\n')[0])
    ap.add_argument('tables', nargs='+', help='tile-prediction tables (CSV or parquet), e.g. the three cross-validation folds')
    ap.add_argument('--outcome', required=True)
    ap.add_argument('--tile-uq', type=float, required=True)
    ap.add_argument('--slide-uq', type=float, required=True)
    ap.add_argument('--slide-pred', type=float, default=0.5)
    ap.add_argument('--labels', help='CSV with columns slide, patient')
    ap.add_argument('--out', required=True)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--grid', type=int, default=200)
    ap.add_argument('--host', action='store_true', help='numpy on the host; otherwise the sums run on the GPU')
    a = ap.parse_args(argv)
    patients = None
    if a.labels:
        lab = pd.read_csv(a.labels, dtype=str)
        patients = dict(zip(lab['slide'], lab['patient']))
    engine = None
    if not a.host:
        from .engine import Engine
        from .weights import synthetic_weights
        engine = Engine(synthetic_weights(1), max_batch=1, max_mc=1)     # the tools need a context, not a trained network
    try:
        both = uq_calibration(a.tables, a.outcome, a.tile_uq, a.slide_uq, a.slide_pred, patients, engine=engine, grid=a.grid, seed=a.seed)
    finally:
        if engine is not None:
            engine.close()
    for cal in both:
        for p in cal.save(a.out).values():
            print(p)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
