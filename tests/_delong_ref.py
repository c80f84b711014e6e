"""DeLong's covariance restated from its definition, O(m n0), for tests/test_metrics.py and tests/test_gpu_metrics.py -- not the
fast algorithm of ``biscuit_amd/metrics.py`` and ``csrc/kernels_delong.hip`` (DESIGN.md section 7 "Prediction metrics").

For the positives' scores X [m] and the negatives' Y [n0] of one classifier, ``psi = (X > Y) + 0.5 (X == Y)`` over all pairs.  The
structural component of a positive row is the mean of its row of psi, of a negative row the mean of its column.  Stated so that
the arithmetic is fixed: the sum of a row of psi is a half-integer, exact; a positive's V is that sum divided by n0 -- ONE rounded
division; a negative's column mean is 1 - (sum of the column of 1 - psi) / m, the column sum of ``(X < Y) + 0.5 (X == Y)`` again an
exact half-integer -- one rounded division and one rounded subtraction, which is how the reference's ``1.0 - (tz - ty) / m``
evaluates it.  The AUROC is the mean of psi; S = cov(V | positive) / m + cov(V | negative) / n0 with ``numpy.cov``, and once more
in exact rational arithmetic (``fractions``) from the same float64 V: the basis of the tolerance.

The seeded cases of both test files are built here; tests/golden/metrics_reference.json.gz (tools/make_metrics_golden.py) holds a
checksum of each and what the reference computes from it."""
import hashlib
import warnings
from fractions import Fraction

import numpy as np

CHUNK = 2048                 # bq_delong_chunk_rows(n) for every n used here (tests/test_gpu_metrics.py asserts it)
TOL = 1e-12                  # of the scale below: DESIGN.md section 7 "Prediction metrics" states the basis
LOG10P_ATOL = 1e-9
THRESHOLD = 0.5              # of the prediction_metrics cases


def scale(m, n0):
    """The largest value an entry of S can take: V lies in [0, 1], so a class's variance is at most 0.25 (1 + 1 / (count - 1));
    the bound's scale is 0.25 (1 / m + 1 / n0), never zero."""
    return 0.25 * (1.0 / m + 1.0 / n0)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _labels(rng, n, frac=0.4):
    y = rng.random(n) < frac
    y[0], y[1] = True, False
    return y.astype(np.int64)


def _scores(rng, y, k, decimals=None):
    """Scores that lean on the label, through float32; ``decimals``: rounded first, which makes ties."""
    P = 0.4 + 0.2 * y[None, :] + 0.25 * rng.normal(size=(k, len(y)))
    if decimals is not None:
        P = np.round(P, decimals)
    return P.astype(np.float32).astype(np.float64)


def _random(seed, n, k, decimals=None):
    rng = np.random.default_rng(seed)
    y = _labels(rng, n)
    return y, _scores(rng, y, k, decimals)


def _n2():
    return np.array([1, 0], np.int64), np.array([[0.75, 0.25], [0.25, 0.75]])


def _n3():
    return np.array([1, 1, 0], np.int64), np.array([[0.75, 0.25, 0.5], [0.5, 0.5, 0.25]])


def _equal():
    y, _ = _random(21, 50, 2)
    return y, np.full((2, 50), np.float64(np.float32(0.3)))


def _separated():
    y, P = _random(22, 40, 2, 2)
    return y, np.where(y[None, :] == 1, 2.0 + np.abs(P), -2.0 - np.abs(P)).astype(np.float32).astype(np.float64)


def _zeros():
    rng = np.random.default_rng(23)
    y = _labels(rng, 33, 0.5)
    return y, rng.choice(np.array([-0.0, 0.0, -0.5, 0.5]), size=(2, 33))


def _inf():
    y, P = _random(24, 41, 2, 2)
    P[0, [3, 17, 30]] = np.inf
    P[0, [5, 6]] = -np.inf
    P[1, [0, 1]] = np.inf
    P[1, [2, 40]] = -np.inf
    return y, P


def _descending():
    y, P = _random(25, 100, 2, 2)
    o = np.argsort(-P[0], kind='stable')
    return y[o], P[:, o]


def _identical():
    y, P = _random(26, 60, 1, 2)
    return y, np.vstack([P[0], P[0]])


def _monotone():
    y, P = _random(27, 60, 1, 2)
    return y, np.vstack([P[0], 2.0 * P[0] + 1.0])           # exact in float64: strictly increasing, ties kept


CASES = {
    'n2': _n2, 'n3': _n3,
    'n7': lambda: _random(1, 7, 2, 2), 'n64': lambda: _random(2, 64, 3, 2), 'tied257': lambda: _random(3, 257, 3, 1),
    'n1000': lambda: _random(4, 1000, 2, 2),
    'chunk-1': lambda: _random(5, CHUNK - 1, 2, 2), 'chunk+0': lambda: _random(6, CHUNK, 2, 2), 'chunk+1': lambda: _random(7, CHUNK + 1, 2, 2),
    'equal': _equal, 'separated': _separated, 'zeros': _zeros, 'inf': _inf, 'descending': _descending,
    'k1': lambda: _random(8, 129, 1, 2), 'k3': lambda: _random(9, 129, 3), 'k8': lambda: _random(10, 129, 8, 2),
    'identical': _identical, 'monotone': _monotone,
    'big': lambda: _random(11, 3 * CHUNK + 1, 3, 2),        # three chunks and one row: the largest
}
SEEDS = {name: 100 + i for i, name in enumerate(CASES)}      # np.random.seed of the case's prediction_metrics
STORES_V = 257                                               # the golden stores V up to this many rows

_built, _restated = {}, {}


def case(name):
    """``(y int64 [n], P float64 [k, n])`` of a case, built once and read-only."""
    if name not in _built:
        y, P = CASES[name]()
        y, P = np.ascontiguousarray(y), np.ascontiguousarray(P, dtype=np.float64)
        y.setflags(write=False)
        P.setflags(write=False)
        _built[name] = (y, P)
    return _built[name]


def checksum(y, P):
    return hashlib.sha256(np.asarray(y, np.uint8).tobytes() + np.ascontiguousarray(P, np.float64).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def components(y, P):
    """V [k, n] in row order and auc [k] from psi over all pairs, with the arithmetic the module's docstring fixes."""
    y = np.asarray(y) != 0
    P = np.atleast_2d(np.asarray(P, np.float64))
    m, n0 = int(y.sum()), int((~y).sum())
    V, auc = np.empty(P.shape), np.empty(len(P))
    for r, p in enumerate(P):
        X, Y = p[y][:, None], p[~y][None, :]
        gt, eq, lt = X > Y, X == Y, X < Y
        row2 = 2 * gt.sum(1, dtype=np.int64) + eq.sum(1, dtype=np.int64)            # twice the row sums of psi
        col2 = 2 * lt.sum(0, dtype=np.int64) + eq.sum(0, dtype=np.int64)            # twice the column sums of 1 - psi
        V[r, y] = (0.5 * row2) / float(n0)
        V[r, ~y] = 1.0 - (0.5 * col2) / float(m)
        auc[r] = float(Fraction(int(row2.sum()), 2 * m * n0))                       # the mean of psi, rounded once
    return V, auc


def cov_numpy(y, V):
    y = np.asarray(y) != 0
    m, n0 = int(y.sum()), int((~y).sum())
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', category=RuntimeWarning)
        return np.atleast_2d(np.cov(V[:, y])) / m + np.atleast_2d(np.cov(V[:, ~y])) / n0


def cov_exact(y, V):
    """S from the float64 V in exact rational arithmetic, rounded once at the end; NaN where a class has one row."""
    y = np.asarray(y) != 0
    k = len(V)
    S = [[Fraction(0)] * k for _ in range(k)]
    for sel in (y, ~y):
        cnt = int(sel.sum())
        if cnt < 2:
            return np.full((k, k), np.nan)
        rows = [[Fraction(float(v)) for v in V[r, sel]] for r in range(k)]
        dev = []
        for row in rows:
            mean = sum(row) / cnt
            dev.append([v - mean for v in row])
        for a in range(k):
            for b in range(a, k):
                c = sum(u * v for u, v in zip(dev[a], dev[b])) / (cnt - 1) / cnt
                S[a][b] += c
                if a != b:
                    S[b][a] += c
    return np.array([[float(v) for v in row] for row in S])


def restated(name):
    """``{'V', 'auc', 'cov_numpy', 'cov_exact', 'm', 'n0'}`` of a case, computed once and shared."""
    if name not in _restated:
        y, P = case(name)
        V, auc = components(y, P)
        res = {'V': V, 'auc': auc, 'cov_numpy': cov_numpy(y, V), 'cov_exact': cov_exact(y, V), 'm': int(y.sum()), 'n0': int(len(y) - y.sum())}
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _restated[name] = res
    return _restated[name]


# ---------------------------------------------------------------------------------------------------------------- the holds
def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def cov_deviation(S, ref, m, n0):
    """max |S - ref| in units of the scale; NaN must stand exactly where ``ref`` has it."""
    S, ref = np.asarray(S, np.float64), np.asarray(ref, np.float64)
    assert S.shape == ref.shape, (S.shape, ref.shape)
    assert np.array_equal(np.isnan(S), np.isnan(ref)), 'NaN in other places than the reference'
    ok = ~np.isnan(ref)
    return float(np.abs(S[ok] - ref[ok]).max() / scale(m, n0)) if ok.any() else 0.0


def check(name, got, gold):
    """What both paths are held to for a case: ``got`` of ``delong_host`` / ``Engine.delong`` with components, ``gold`` the
    golden's entry.  -> the covariance's largest deviation, in units of the scale, from the golden, numpy and exact statements."""
    y, P = case(name)
    ref = restated(name)
    m, n0 = ref['m'], ref['n0']
    assert (got['n_pos'], got['n_neg']) == (m, n0)
    assert same_bits(got['auc'], unjson(gold['auc'])), f'{name}: auc {got["auc"]} is not the reference\'s {gold["auc"]} bit for bit'
    assert np.abs(got['auc'] - ref['auc']).max() <= 4 * np.finfo(np.float64).eps        # the reference rounds three times, the mean of psi once
    if 'V' in gold:
        assert same_bits(got['V'], unjson(gold['V'])), f'{name}: V differs from the reference\'s v01 / v10'
    assert same_bits(got['V'], ref['V']), f'{name}: V differs from the pairwise means'
    dev = {key: cov_deviation(got['cov'], S, m, n0) for key, S in (('golden', unjson(gold['cov'])), ('numpy', ref['cov_numpy']), ('exact', ref['cov_exact']))}
    assert max(dev.values()) <= TOL, f'{name}: covariance off by {dev} of the scale'
    return dev


def unjson(x):
    """A golden value as float64: lists become arrays, None is NaN."""
    if x is None:
        return np.float64('nan')
    if isinstance(x, list):
        return np.array([unjson(v) for v in x], dtype=np.float64)
    return np.float64(x)
