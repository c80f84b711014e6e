"""A plain float64 restatement of DESIGN.md section 7 "UQ calibration" (the density and the calibration curve behind the reference's
``plot_uncertainty``), one grid point at a time over whole arrays: the reference of tests/test_calibration.py (the numpy path of
``biscuit_amd/calibration.py``) and tests/test_gpu_calibration.py (``Engine.uq_kde`` / ``Engine.uq_loess``).  Written from the
definitions, not from either implementation: the window's half-width by sorting the distances, the 3 x 3 system by
``numpy.linalg.solve``, the interpolant segment by segment.  Also the seeded cases both test files share."""
import math

import numpy as np
from scipy import stats

FIT_ATOL = 1e-10          # |fit - reference|
REL = 1e-10               # l2, se and the band, relative
KDE_REL = 1e-12           # the density, relative to the curve's maximum


def case(n, seed=0):
    """x = |normal(0.05, 0.03)| through float32 (what the table holds), c ~ Bernoulli(logistic((0.07 - x) / 0.02))."""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.normal(0.05, 0.03, n)).astype(np.float32).astype(np.float64)
    c = rng.random(n) < 1.0 / (1.0 + np.exp(-(0.07 - x) / 0.02))
    return x, c


def tied_case():
    """257 rows, 60 of them tied at one value."""
    x, c = case(257, seed=1)
    x[100:160] = x[100]
    return x, c


def degenerate_case():
    """400 rows, 320 (80 %) of them at the smallest value: the first vertex has h = 0."""
    x, c = case(400, seed=2)
    x[:320] = x.min()
    return x, c


def one_group_case():
    x, _ = case(300, seed=3)
    return x, np.ones(300, bool)


def kde_ref(x, c, grid=200, cut=3.0):
    """{group index: (support, unit density, bw)} for the groups with n >= 2 and a non-zero standard deviation."""
    out = {}
    for g in (0, 1):
        xg = np.asarray(x, np.float64)[np.asarray(c) == bool(g)]
        n = len(xg)
        if n < 2:
            continue
        sd = math.sqrt(sum((v - xg.mean()) ** 2 for v in xg) / (n - 1))
        if not sd > 0:
            continue
        bw = sd * n ** (-1 / 5)
        sup = np.linspace(xg.min() - cut * bw, xg.max() + cut * bw, grid)
        dens = np.array([np.exp(-0.5 * ((xg - s) / bw) ** 2).sum() for s in sup]) / (n * bw * math.sqrt(2 * math.pi))
        out[g] = (sup, dens, bw)
    return out


def interp_ref(v, f, x):
    """Segment j of a row: the last of 0 .. G - 2 whose left vertex is <= x."""
    out = np.empty(len(x))
    for i, xi in enumerate(x):
        j = 0
        for k in range(1, len(v) - 1):
            if v[k] <= xi:
                j = k
        w = (xi - v[j]) / (v[j + 1] - v[j]) if v[j + 1] != v[j] else float('nan')
        out[i] = f[j] + w * (f[j + 1] - f[j])
    return out


def loess_ref(x, c, grid=200, span=0.75):
    """vertex, fit, l2, lam, h [grid]; nu, rss, s, dof, t, se, lower, upper; degenerate (count), q."""
    x = np.asarray(x, np.float64)
    y = np.asarray(c).astype(np.float64)
    n = len(x)
    q = int(math.floor(span * n + 1e-5))
    v = np.linspace(x.min(), x.max(), grid)
    fit, l2, lam, h = (np.full(grid, np.nan) for _ in range(4))
    for k, x0 in enumerate(v):
        d = np.abs(x - x0)
        h[k] = np.sort(d)[q - 1]
        if h[k] == 0:
            continue
        u = (x - x0) / h[k]
        w = np.where(np.abs(u) < 1, (1 - np.abs(u) ** 3) ** 3, 0.0)
        m = [float((w * u ** p).sum()) for p in range(5)]
        t = np.array([float((w * y * u ** p).sum()) for p in range(3)])
        r = [float((w * w * u ** p).sum()) for p in range(5)]
        A = np.array([[m[i + j] for j in range(3)] for i in range(3)])
        B = np.array([[r[i + j] for j in range(3)] for i in range(3)])
        det = (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
               + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))
        if not m[0] > 0 or abs(det) < 1e-12 * m[0] ** 3:
            continue
        a = np.linalg.solve(A, np.array([1.0, 0.0, 0.0]))
        fit[k], l2[k], lam[k] = a @ t, a @ B @ a, a[0]
    # the interpolant over all rows: vectorised by segment, the definition of interp_ref (tests/test_calibration.py compares the two)
    j = np.clip(np.searchsorted(v, x, 'right') - 1, 0, grid - 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = (x - v[j]) / (v[j + 1] - v[j])
        z, li = fit[j] + w * (fit[j + 1] - fit[j]), lam[j] + w * (lam[j + 1] - lam[j])
    nu = math.fsum(li) if np.isfinite(li).all() else float('nan')
    rss = math.fsum((y - z) ** 2) if np.isfinite(z).all() else float('nan')
    dof = n - nu
    s = math.sqrt(rss / dof) if dof > 0 else float('nan')
    tq = float(stats.t.ppf(0.975, dof)) if dof > 0 else float('nan')
    se = s * np.sqrt(l2)
    return {'vertex': v, 'fit': fit, 'l2': l2, 'lam': lam, 'h': h, 'nu': nu, 'rss': rss, 's': s, 'dof': dof, 't': tq, 'se': se,
            'lower': fit - tq * se, 'upper': fit + tq * se, 'degenerate': int(np.isnan(fit).sum()), 'q': q}


def check_kde(got, x, c, grid=200, cut=3.0):
    """``got``: the result of ``Engine.uq_kde`` / ``calibration.kde_host`` against ``kde_ref`` and scipy.  -> the largest deviation
    relative to the curve's maximum."""
    ref = kde_ref(x, c, grid, cut)
    worst = 0.0
    for g in (0, 1):
        assert bool(got['valid'][g]) == (g in ref), g
        assert int(got['n'][g]) == int((np.asarray(c) == bool(g)).sum())
        if g not in ref:
            assert np.isnan(got['density'][g]).all() and np.isnan(got['support'][g]).all()
            continue
        sup, dens, bw = ref[g]
        xg = np.asarray(x, np.float64)[np.asarray(c) == bool(g)]
        sci = stats.gaussian_kde(xg)(got['support'][g])
        top = dens.max()
        np.testing.assert_allclose(got['support'][g], sup, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(got['bw'][g], bw, rtol=1e-13)
        for other in (dens, sci):
            dev = float(np.abs(got['density'][g] - other).max() / top)
            worst = max(worst, dev)
            assert dev <= KDE_REL, (g, dev)
    return worst


def check_loess(got, x, c, grid=200, span=0.75, ref=None, constant_y=False):
    """``got``: the result of ``Engine.uq_loess`` / ``calibration.loess_host`` (through ``calibration.band``) against ``loess_ref``.
    -> (largest |fit deviation|, {quantity: largest relative deviation} for l2, se and the band's two sides)."""
    from biscuit_amd import calibration
    ref = loess_ref(x, c, grid, span) if ref is None else ref
    s, dof, tq, se, lower, upper = calibration.band(got)
    assert np.array_equal(got['vertex'], ref['vertex'])
    assert np.array_equal(got['h'], ref['h'])
    assert got['q'] == ref['q'] and got['degenerate'] == ref['degenerate']
    assert np.array_equal(np.isnan(got['fit']), np.isnan(ref['fit']))
    ok = ~np.isnan(ref['fit'])
    dfit = float(np.abs(got['fit'][ok] - ref['fit'][ok]).max()) if ok.any() else 0.0
    assert dfit <= FIT_ATOL, dfit
    worst = {}
    if constant_y:
        # y is constant, the fit reproduces it and every residual is a rounding error of the fit: s has no digits to compare, so
        # the band is held to the fit's own bound instead (se = s sqrt(l2), both sides ~1e-16)
        np.testing.assert_allclose(got['l2'][ok], ref['l2'][ok], rtol=REL)
        assert np.abs(se[ok]).max() <= FIT_ATOL and np.abs(ref['se'][ok]).max() <= FIT_ATOL
        assert np.abs(lower[ok] - ref['lower'][ok]).max() <= FIT_ATOL and np.abs(upper[ok] - ref['upper'][ok]).max() <= FIT_ATOL
        return dfit, worst
    for name, a, b in (('l2', got['l2'], ref['l2']), ('se', se, ref['se']), ('lower', lower, ref['lower']), ('upper', upper, ref['upper'])):
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        fin = ~np.isnan(b)
        if fin.any():
            dev = float((np.abs(a[fin] - b[fin]) / np.abs(b[fin])).max())
            worst[name] = dev
            assert dev <= REL, (name, dev)
    if math.isnan(ref['nu']):
        assert math.isnan(got['nu']) and math.isnan(s)
    else:
        assert abs(got['nu'] - ref['nu']) <= REL * abs(ref['nu']) and abs(s - ref['s']) <= REL * ref['s']
    return dfit, worst
