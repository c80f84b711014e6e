"""``Engine.uq_kde`` / ``Engine.uq_loess`` (``csrc/kernels_calib.hip``; DESIGN.md section 7 "UQ calibration") against the per-point
restatement of tests/_calibration_ref.py with the tolerances of tests/test_calibration.py -- the density 1e-12 of the curve's
maximum, the fit 1e-10 absolute, l2, se and the band 1e-10 relative -- at the sizes where the kernels take another path: less than
one chunk, the chunk length and its neighbours, several chunks and a tail, a grid that cuts a vertex tile short.  Then what every
device tool owes: the same bits on a repeat call, with the caller's scratch and on poisoned memory, its profiling classes, its
scratch let go by ``close()``, and the routing of ``calibration.uncertainty_calibration``.  ``-m gpu``."""
import numpy as np
import pandas as pd
import pytest
import torch

from biscuit_amd import calibration, threshold
from tests import _calibration_ref as R
from tests import _poison as P
from tests.test_gpu_abi_homes import _device_tensors, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = _engine()
    yield e
    e.close()


def _cases(chunk):
    out = {'n64': R.case(64), 'n4099': R.case(4099), 'tied257': R.tied_case()}
    for n in (chunk - 1, chunk, chunk + 1):
        out[f'chunk{n - chunk:+d}'] = R.case(n)
    return out


@pytest.fixture(scope='module')
def cases(eng):
    chunk = eng.uq_chunk_rows(4099)
    assert chunk == eng.uq_chunk_rows(64) and 2 * chunk < 4099 and 4099 % chunk      # several chunks and a tail
    return _cases(chunk)


NAMES = ('n64', 'chunk-1', 'chunk+0', 'chunk+1', 'n4099', 'tied257')


@pytest.mark.parametrize('name', NAMES)
def test_against_the_restatement(eng, cases, name):
    x, c = cases[name]
    kdev = R.check_kde(eng.uq_kde(x, c), x, c)
    got = eng.uq_loess(x, c)
    assert got['degenerate'] == 0 and got['n'] == len(x)
    dfit, drel = R.check_loess(got, x, c)
    print(f'{name}: density {kdev:.2e} of the maximum, fit {dfit:.2e}, relative ' + ', '.join(f'{k} {v:.2e}' for k, v in drel.items()))


def test_degenerate_vertices_in_the_same_places(eng):
    x, c = R.degenerate_case()
    got = eng.uq_loess(x, c)
    assert got['h'][0] == 0.0 and got['degenerate'] > 0
    R.check_loess(got, x, c)
    R.check_kde(eng.uq_kde(x, c), x, c)


def test_one_group_only(eng):
    x, c = R.one_group_case()
    kde = eng.uq_kde(x, c)
    assert not kde['valid'][0] and kde['valid'][1]
    R.check_kde(kde, x, c)
    R.check_loess(eng.uq_loess(x, c), x, c, constant_y=True)


def test_grid_of_seven_and_descending_input(eng):
    x, c = R.case(257)
    R.check_kde(eng.uq_kde(x, c, grid=7), x, c, grid=7)
    R.check_loess(eng.uq_loess(x, c, grid=7), x, c, grid=7)
    x, c = R.case(1000)
    o = np.argsort(-x, kind='stable')
    R.check_kde(eng.uq_kde(x[o], c[o]), x, c)
    R.check_loess(eng.uq_loess(x[o], c[o]), x, c)


def test_tensors_and_refusals(eng):
    x, c = R.case(300)
    a = eng.uq_loess(x, c)
    b = eng.uq_loess(torch.from_numpy(x).to(eng.device), torch.from_numpy(c).to(eng.device))
    assert same_bits(a, b)
    bad = x.copy()
    bad[7] = np.inf
    for call in (lambda: eng.uq_kde(bad, c), lambda: eng.uq_loess(bad, c), lambda: eng.uq_kde(x, c, grid=1), lambda: eng.uq_loess(x, c, grid=2000),
                 lambda: eng.uq_loess(x, c, span=1.5), lambda: eng.uq_kde(x, c[:-1])):
        with pytest.raises(ValueError):
            call()


def same_bits(a, b):
    for k in a:
        u, v = np.asarray(a[k]), np.asarray(b[k])
        if u.dtype != v.dtype or u.shape != v.shape or u.tobytes() != v.tobytes():
            return False
    return True


def both(eng, x, c, own_scratch=False, between=None):
    kde = eng.uq_kde(x, c, scratch=eng.uq_kde_scratch(len(x)) if own_scratch else None)
    if between:
        between()
    return kde, eng.uq_loess(x, c, scratch=eng.uq_loess_scratch(len(x)) if own_scratch else None)


def test_same_bits_again_and_with_the_callers_scratch(eng, cases):
    x, c = cases['n4099']
    first, again, own = both(eng, x, c), both(eng, x, c), both(eng, x, c, own_scratch=True)
    for a, b in zip(first, again):
        assert same_bits(a, b)
    for a, b in zip(first, own):
        assert same_bits(a, b)
    assert eng.uq_kde_scratch(4099).numel() == eng._lib.bq_uq_kde_workspace_bytes(4099, 200)
    assert eng.uq_loess_scratch(4099).numel() == eng._lib.bq_uq_loess_workspace_bytes(4099, 200)


@pytest.mark.parametrize('own_scratch', [False, True])
def test_results_do_not_depend_on_stale_bytes(eng, cases, own_scratch):
    import biscuit_amd.engine as engine_mod
    x, c = cases['n4099']
    clean = both(eng, x, c, own_scratch)
    for fill in P.BYTE_FILLS:
        torch.cuda.synchronize(eng.device)
        eng.drop_scratch()
        proxy = P.poisoned_torch(fill)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, 'torch', proxy)
            out = both(eng, x, c, own_scratch, between=eng.drop_scratch)    # the second entry's scratch is poisoned afresh
        torch.cuda.synchronize(eng.device)
        assert proxy.served >= 4                                            # two outputs, two scratch buffers
        proxy.check()
        for a, b in zip(clean, out):
            assert same_bits(a, b), f'a result under 0x{fill:02X} differs from a clean run'


def test_exactly_the_two_new_classes(cases):
    eng = _engine()
    try:
        eng.profile_enable(True)
        both(eng, *cases['n4099'])
        prof = eng.profile_read()
        assert {p.name: p.launches for p in prof} == {'uq_kde': 1, 'uq_loess': 1}
    finally:
        eng.close()


def test_close_lets_go_of_the_scratch(cases):
    eng = _engine()
    both(eng, *cases['n64'])
    assert 'uq' in {k for k, v in eng._tool_ws.items() if _device_tensors(v)}, eng._tool_ws.keys()
    eng.close()
    assert {k: v for k, v in vars(eng).items() if _device_tensors(v)} == {}


def test_calibration_routes_to_the_device(eng):
    x, c = R.case(1000)
    df = pd.DataFrame({'uncertainty': x, 'correct': c, 'y_pred': np.random.default_rng(0).random(1000)})
    host = calibration.uncertainty_calibration(df, 'tile', 0.06)
    threshold.use_device(eng, min_rows=1)
    try:
        dev = calibration.uncertainty_calibration(df, 'tile', 0.06)
        assert threshold.plot_uncertainty(df, 'tile', 0.06).summary['path'] == 'device'
    finally:
        threshold.use_device(None)
    assert host.summary['path'] == 'host' and dev.summary['path'] == 'device'
    assert list(host.kde) == list(dev.kde) == ['incorrect', 'correct']
    for g in host.kde:
        assert np.abs(host.kde[g]['density'] - dev.kde[g]['density']).max() <= R.KDE_REL * host.kde[g]['density'].max()
    assert np.abs(host.loess['fit'] - dev.loess['fit']).max() <= R.FIT_ATOL
    for k in ('se', 'lower', 'upper'):
        np.testing.assert_allclose(dev.loess[k], host.loess[k], rtol=R.REL, atol=0)
    pd.testing.assert_frame_equal(host.scatter, dev.scatter)
    # below the bound the table stays on the host
    threshold.use_device(eng, min_rows=5000, calibration_min_rows=5000)
    try:
        assert calibration.uncertainty_calibration(df, 'tile', 0.06).summary['path'] == 'host'
    finally:
        threshold.use_device(None)
