"""Golden vectors for ``tests/test_consumer_live.py``: the reference's own ``biscuit/threshold.py`` (``detect``, ``apply``)
on the twelve seeded random frames of that test, and its ``biscuit/utils.py`` ``rename_cols`` on the same 300 random column
sets, imported under the stubs of ``make_consumer_golden.import_reference``.  TEST INFRASTRUCTURE ONLY.  The fixture holds
the parameters the test derives from its seeds and the reference's outputs -- data, no reference source; the test rebuilds
the input frames from the seeds (``make_consumer_golden.make_frame``) and checks they are the ones recorded.

usage: python oracle/make_consumer_live_golden.py --ref <reference checkout>   (writes tests/golden/consumer_live.json.gz)
"""
import argparse
import gzip
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle.make_consumer_golden import import_reference, make_frame        # noqa: E402

SEEDS = range(12)
RENAME_CASES = 300
LEVEL_INT_COLS = ('y_true', 'correct', 'incorrect', 'y_pred_bin')
LEVEL_FLOAT_COLS = ('y_pred', 'uncertainty', 'error')


def num(x):
    """A scalar result as JSON: None stays None, every number a float (NaN is written as NaN)."""
    return None if x is None else float(x)


def frame_case(seed):
    """The frame and the thresholds of case ``seed``, drawn exactly as the test draws them."""
    rng = np.random.default_rng(1000 + seed)
    spec = dict(seed=500 + seed, n_slides=int(rng.integers(6, 40)), tiles_per_slide=int(rng.integers(4, 50)),
                flip_frac=float(rng.uniform(0.1, 0.45)), ragged=bool(seed % 2))
    return rng, spec, make_frame(**spec)


def rename_cases():
    """The 300 random column sets of the rename test, in its order."""
    rng = np.random.default_rng(7)
    names = ['y_true0', 'y_true', 'y_pred0', 'y_pred1', 'uncertainty0', 'uncertainty1']
    out = []
    for _ in range(RENAME_CASES):
        outcome = str(rng.choice(['cohort', 'x-y', 'a_b', '7']))
        cols = ['slide'] + [f'{outcome}{sep}{n}' for n in names for sep in '-_' if rng.random() < 0.45]
        cols += [c for c in ('y_true', 'y_pred', 'label') if rng.random() < 0.15]
        kw = {}
        if rng.random() < 0.2:
            kw['y_pred'] = str(rng.choice(cols))
        out.append((cols, outcome, kw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference (the directory holding biscuit/)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden',
                                                  'consumer_live.json.gz'))
    args = ap.parse_args()
    mods = import_reference(args.ref)
    th, utils = mods['threshold'], mods['utils']
    frames = []
    for seed in SEEDS:
        rng, spec, df = frame_case(seed)
        patients = dict(zip(df['slide'], df['patient']))
        case = {'seed': seed, 'spec': spec, 'rows': len(df), 'y_pred_sum': float(df['y_pred'].sum())}
        try:
            thr, auc = th.detect(df.copy(), patients=patients)
        except Exception as e:  # noqa: BLE001 -- record whatever the reference raises
            case['detect_error'] = type(e).__name__
            frames.append(case)
            continue
        case['detect'] = {'thresholds': {k: num(v) for k, v in thr.items()}, 'auc': num(auc)}
        tile_uq = float(np.quantile(df['uncertainty'], rng.uniform(0.3, 0.9)))
        case['tile_uq'] = tile_uq
        for level in ('slide', 'patient'):
            slide_uq = float(rng.uniform(0.005, 0.04))
            res, s_df = th.apply(df.copy(), tile_uq=tile_uq, slide_uq=slide_uq, tile_pred=0.5, slide_pred=0.45,
                                 patients=patients, level=level)
            ent = {'slide_uq': slide_uq, 'results': {k: num(v) for k, v in res.items()}, 'frame': None}
            if s_df is not None:
                ent['frame'] = {'levels': [str(x) for x in s_df[level]]}
                ent['frame'].update({c: [float(x) for x in s_df[c]] for c in LEVEL_FLOAT_COLS})
                ent['frame'].update({c: [int(x) for x in s_df[c]] for c in LEVEL_INT_COLS})
            case[f'apply_{level}'] = ent
        frames.append(case)
    renames = []
    for cols, outcome, kw in rename_cases():
        a = pd.DataFrame({c: [0] for c in cols})
        utils.rename_cols(a, outcome, **kw)
        renames.append({'columns': cols, 'outcome': outcome, 'kwargs': kw, 'result': list(a.columns)})
    meta = {'generator': 'oracle/make_consumer_live_golden.py', 'reference': 'jamesdolezal/biscuit @ 2024_10_08',
            'versions': {'numpy': np.__version__, 'pandas': pd.__version__}}
    with gzip.open(args.out, 'wt') as f:
        json.dump({'meta': meta, 'frames': frames, 'rename_cols': renames}, f)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
