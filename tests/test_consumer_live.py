"""Differential test of biscuit_amd.threshold against the reference's own biscuit/threshold.py and
biscuit/utils.py on random inputs: twelve seeded frames through ``detect`` / ``apply`` and 300 random column
sets through ``rename_cols``.  The reference's outputs on exactly these inputs are committed data,
``tests/golden/consumer_live.json.gz`` (``oracle/make_consumer_live_golden.py``); the inputs are rebuilt here from
their seeds and checked against what the fixture recorded before anything is compared."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle.make_consumer_live_golden import LEVEL_FLOAT_COLS, LEVEL_INT_COLS, frame_case, rename_cases   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'consumer_live.json.gz')


@pytest.fixture(scope='module')
def ref():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)


def _same(a, b):
    if a is None or b is None:
        assert a is None and b is None
    else:
        assert float(a) == float(b) or (np.isnan(float(a)) and np.isnan(float(b)))


@pytest.mark.parametrize('seed', range(12))
def test_random_frames_match_reference(ref, seed):
    from biscuit_amd import threshold as th
    want = ref['frames'][seed]
    rng, spec, df = frame_case(seed)
    # the inputs are the ones the reference saw
    assert want['seed'] == seed and want['spec'] == spec
    assert len(df) == want['rows'] and float(df['y_pred'].sum()) == want['y_pred_sum']
    patients = dict(zip(df['slide'], df['patient']))
    # detect
    if 'detect_error' in want:
        with pytest.raises(Exception) as ei:
            th.detect(df.copy(), patients=patients)
        assert type(ei.value).__name__ == want['detect_error']
        return
    want_thr, want_auc = want['detect']['thresholds'], want['detect']['auc']
    got_thr, got_auc = th.detect(df.copy(), patients=patients)
    for k in want_thr:
        _same(got_thr[k], want_thr[k])
    _same(got_auc, want_auc)
    # apply at both levels with data-derived thresholds
    tile_uq = float(np.quantile(df['uncertainty'], rng.uniform(0.3, 0.9)))
    assert tile_uq == want['tile_uq']
    for level in ('slide', 'patient'):
        w = want[f'apply_{level}']
        slide_uq = float(rng.uniform(0.005, 0.04))
        assert slide_uq == w['slide_uq']
        g_res, g_df = th.apply(df.copy(), tile_uq=tile_uq, slide_uq=slide_uq, tile_pred=0.5, slide_pred=0.45,
                               patients=patients, level=level)
        for k in w['results']:
            _same(g_res[k], w['results'][k])
        w_df = w['frame']
        if w_df is None:
            assert g_df is None
        else:
            assert [str(x) for x in g_df[level]] == w_df['levels']
            for c in LEVEL_FLOAT_COLS:
                np.testing.assert_allclose(g_df[c].to_numpy(), np.asarray(w_df[c], dtype=np.float64), atol=1e-12)
            for c in LEVEL_INT_COLS:
                assert [int(x) for x in g_df[c]] == w_df[c]


def test_rename_cols_matches_reference_live(ref):
    """Random column sets through ``rename_cols`` against the reference's (utils.py:31-53) on the same sets."""
    import pandas as pd
    from biscuit_amd.predictions import rename_cols
    want = ref['rename_cols']
    cases = rename_cases()
    assert len(cases) == len(want) == 300
    for (cols, outcome, kw), w in zip(cases, want):
        assert (cols, outcome, kw) == (w['columns'], w['outcome'], w['kwargs'])
        b = pd.DataFrame({c: [0] for c in cols})
        rename_cols(b, outcome, **kw)
        assert list(b.columns) == w['result'], (cols, outcome, kw)
