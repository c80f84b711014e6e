"""Generate tests/golden/metrics_reference.json.gz: what the reference's own ``biscuit/delong.py`` and ``biscuit/utils.py``
compute from the seeded cases of tests/_delong_ref.py (DESIGN.md section 7 "Prediction metrics").

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference exists; its output is committed data, no program text: per
case the checksum of the rebuilt input, ``fastDeLong``'s aucs and covariance, for cases of up to 257 rows ``v01`` / ``v10`` brought
into row order, for cases of two or more classifiers ``delong_roc_test`` of the first two, and ``prediction_metrics`` of the first
classifier under ``np.random.seed(s)``.  The reference's modules are loaded by the unchanged
``oracle.make_consumer_golden.import_reference``; ``np.float``, which they still use, is set in this process first.

usage: python tools/make_metrics_golden.py --ref REFERENCE_CHECKOUT
"""
import argparse
import gzip
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from oracle.make_consumer_golden import import_reference, jsonable        # noqa: E402
from tests import _delong_ref as R                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (the directory that holds biscuit/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'metrics_reference.json.gz'))
    args = ap.parse_args()
    np.float = float                                          # removed from NumPy 1.24; delong.py:16,24,60-62
    mods = import_reference(args.ref)
    delong, utils = mods['delong'], mods['utils']
    # fastDeLong returns only aucs and the covariance: v01 / v10 are caught where it hands them to np.cov
    seen = []
    real_cov = np.cov

    def spy(x, *a, **kw):
        seen.append(np.array(x, dtype=np.float64, copy=True))
        return real_cov(x, *a, **kw)

    cases = {}
    warnings.simplefilter('ignore')
    for name in R.CASES:
        y, P = R.case(name)
        y, P = y.copy(), P.copy()
        order, m = delong.compute_ground_truth_statistics(y)
        del seen[:]
        delong.np.cov = spy
        try:
            with np.errstate(all='ignore'):
                aucs, cov = delong.fastDeLong(P[:, order], m)
        finally:
            delong.np.cov = real_cov
        entry = {'n': int(len(y)), 'k': int(len(P)), 'checksum': R.checksum(y, P), 'seed': R.SEEDS[name], 'auc': jsonable(aucs),
                 'cov': jsonable(np.atleast_2d(cov))}
        if len(y) <= R.STORES_V:
            v01, v10 = (np.atleast_2d(v) for v in seen)
            V = np.empty(P.shape)
            V[:, order[:m]], V[:, order[m:]] = v01, v10
            entry['V'] = jsonable(V)
        with np.errstate(all='ignore'):
            if len(P) >= 2:
                entry['log10_p'] = jsonable(delong.delong_roc_test(y, P[0], P[1]))
            np.random.seed(R.SEEDS[name])
            entry['prediction_metrics'] = jsonable(utils.prediction_metrics(y, P[0], R.THRESHOLD))
        cases[name] = entry
    meta = {'generator': 'tools/make_metrics_golden.py', 'reference': 'jamesdolezal/biscuit @ 2024_10_08', 'numpy': np.__version__,
            'threshold': R.THRESHOLD}
    with gzip.GzipFile(args.out, 'wb', mtime=0) as f:
        f.write(json.dumps({'meta': meta, 'cases': cases}).encode())
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
