"""``Engine.delong`` (``csrc/kernels_delong.hip``; DESIGN.md section 7 "Prediction metrics") against the committed golden of the
reference and the O(m n0) restatement of tests/_delong_ref.py, with the holds of tests/test_metrics.py: the AUROC and V bit for
bit, the covariance within 1e-12 of its scale, ``log10 p`` within 1e-9, NaN where the golden has it.  The cases are that file's:
from two rows to three chunks and one row, the chunk length and its neighbours, ties, both zeros, infinities, k = 1, 2, 3, 8.
Then what every device tool owes: the same bits on a repeat call, with the caller's scratch and on poisoned memory, its one
profiling class, its scratch let go by ``close()``, and the routing of ``metrics.delong_roc_variance``.  ``-m gpu``."""
import numpy as np
import pytest
import torch

from biscuit_amd import metrics
from tests import _delong_ref as R
from tests import _poison as P
from tests.test_gpu_abi_homes import _device_tensors, _engine
from tests.test_metrics import NAMES, check_log10_p, check_prediction_metrics, golden  # noqa: F401  (golden: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = _engine()
    yield e
    e.close()


def test_the_chunk_length_is_the_cases(eng):
    for name in NAMES:
        assert eng.delong_chunk_rows(R.case(name)[1].shape[1]) == R.CHUNK


@pytest.mark.parametrize('name', NAMES)
def test_against_the_reference_and_the_restatement(eng, golden, name):  # noqa: F811
    y, S = R.case(name)
    got = eng.delong(y, S, components=True)
    dev = R.check(name, got, golden[name])
    print(f'{name}: covariance off by ' + ', '.join(f'{k} {v:.2e}' for k, v in dev.items()) + ' of the scale')
    host = metrics.delong_host(y, S, components=True)
    assert R.same_bits(got['auc'], host['auc']) and R.same_bits(got['V'], host['V'])


def test_exact_values_of_the_degenerate_cases(eng):
    for name, auc, v in (('equal', 0.5, 0.5), ('separated', 1.0, 1.0)):
        got = eng.delong(*R.case(name), components=True)
        assert (got['auc'] == auc).all() and (got['V'] == v).all() and (got['cov'] == 0.0).all(), name
    assert np.isnan(eng.delong(*R.case('n2'))['cov']).all()
    got = eng.delong(*R.case('monotone'), components=True)
    assert R.same_bits(got['V'][0], got['V'][1]) and len(set(got['cov'].reshape(-1).tolist())) == 1 and got['auc'][0] == got['auc'][1]
    y, S = R.case('zeros')
    assert R.same_bits(eng.delong(y, S + 0.0, components=True)['V'], eng.delong(y, S, components=True)['V'])


@pytest.mark.parametrize('name', [n for n in NAMES if R.case(n)[1].shape[0] >= 2])
def test_delong_roc_test_on_the_device(eng, golden, name):  # noqa: F811
    y, S = R.case(name)
    check_log10_p(name, metrics.delong_roc_test(y, S[0], S[1], engine=eng), golden[name], eng.delong(y, S[:2]))


@pytest.mark.parametrize('name', ['n64', 'tied257', 'chunk+1', 'n3'])
def test_prediction_metrics_on_the_device(eng, golden, name):  # noqa: F811
    y, S = R.case(name)
    check_prediction_metrics(name, metrics.prediction_metrics(y, S[0], R.THRESHOLD, seed=R.SEEDS[name], engine=eng), golden[name])


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_same_bits_again_and_with_the_callers_scratch(eng):
    y, S = R.case('big')
    k, n = S.shape
    first, again = eng.delong(y, S, components=True), eng.delong(y, S, components=True)
    own = eng.delong(y, S, components=True, scratch=eng.delong_scratch(k, n))
    assert same_bits(first, again) and same_bits(first, own)
    assert eng.delong_scratch(k, n).numel() == eng._lib.bq_delong_workspace_bytes(k, n) > 0
    without = eng.delong(y, S)
    assert 'V' not in without and same_bits(without, {key: v for key, v in first.items() if key != 'V'})


@pytest.mark.parametrize('own_scratch', [False, True])
def test_results_do_not_depend_on_stale_bytes(eng, own_scratch):
    import biscuit_amd.engine as engine_mod
    y, S = R.case('big')
    k, n = S.shape

    def run(components):
        return eng.delong(y, S, components=components, scratch=eng.delong_scratch(k, n) if own_scratch else None)
    clean = run(True), run(False)
    for fill in P.BYTE_FILLS:
        torch.cuda.synchronize(eng.device)
        eng.drop_scratch()
        assert 'delong' not in eng._tool_ws
        proxy = P.poisoned_torch(fill)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, 'torch', proxy)
            out = run(True)
            eng.drop_scratch()                                             # the second call's scratch is poisoned afresh
            out = out, run(False)
        torch.cuda.synchronize(eng.device)
        assert proxy.served >= 5                                           # two outputs, V, two scratch buffers
        proxy.check()
        for a, b in zip(clean, out):
            assert same_bits(a, b), f'a result under 0x{fill:02X} differs from a clean run'


def test_exactly_the_one_new_class():
    eng = _engine()
    try:
        eng.profile_enable(True)
        eng.delong(*R.case('n64'))
        eng.delong(*R.case('big'), components=True)
        assert {p.name: p.launches for p in eng.profile_read()} == {'delong': 2}
    finally:
        eng.close()


def test_close_lets_go_of_the_scratch():
    eng = _engine()
    eng.delong(*R.case('n64'))
    assert 'delong' in {k for k, v in eng._tool_ws.items() if _device_tensors(v)}, eng._tool_ws.keys()
    eng.close()
    assert {k: v for k, v in vars(eng).items() if _device_tensors(v)} == {}


def test_variance_routes_to_the_device(eng):
    y, S = R.case('n1000')
    auc_h, var_h = metrics.delong_roc_variance(y, S[0])
    auc_d, var_d = metrics.delong_roc_variance(y, S[0], engine=eng)
    assert metrics.delong_covariance(y, S, engine=eng)['path'] == 'device' and metrics.delong_covariance(y, S)['path'] == 'host'
    assert R.same_bits(auc_h, auc_d)
    assert abs(var_h - var_d) <= R.TOL * R.scale(int(y.sum()), int(len(y) - y.sum()))
    # threshold.use_device: from metrics.DEFAULT_MIN_ROWS rows on, and not below
    from biscuit_amd import threshold
    threshold.use_device(eng)
    try:
        assert len(y) < metrics.DEFAULT_MIN_ROWS and metrics.delong_covariance(y, S)['path'] == 'host'
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(metrics, 'DEFAULT_MIN_ROWS', len(y))
            assert metrics.delong_covariance(y, S)['path'] == 'device'
    finally:
        threshold.use_device(None)
    assert metrics.delong_covariance(y, S)['path'] == 'host'


def test_tensors_and_refusals(eng):
    y, S = R.case('k3')
    a = eng.delong(y, S, components=True)
    b = eng.delong(torch.from_numpy(y).to(eng.device), torch.from_numpy(S).to(eng.device), components=True)
    assert same_bits(a, b)
    one = eng.delong(torch.from_numpy(y != 0), torch.from_numpy(S[0]))                   # host tensors, bool labels, 1-D scores
    assert R.same_bits(one['auc'], a['auc'][:1]) and one['cov'].shape == (1, 1)
    bad = S.copy()
    bad[2, 7] = np.nan
    eng.profile_enable(True)
    try:
        for call in (lambda: eng.delong(y, bad), lambda: eng.delong(np.ones_like(y), S), lambda: eng.delong(np.zeros_like(y), S),
                     lambda: eng.delong(y, np.vstack([S] * 3)), lambda: eng.delong(y[:-1], S), lambda: eng.delong(y * 2, S),
                     lambda: eng.delong(torch.zeros((1 << 25) + 1, dtype=torch.uint8, device=eng.device),
                                        torch.zeros((1 << 25) + 1, dtype=torch.float64, device=eng.device))):
            with pytest.raises(ValueError):
                call()
        assert eng.profile_read() == []                                                  # refused without a launch
    finally:
        eng.profile_enable(False)
    assert eng._lib.bq_delong_workspace_bytes(9, 100) == 0 and eng._lib.bq_delong_workspace_bytes(1, (1 << 25) + 1) == 0
    assert eng._lib.bq_delong_workspace_bytes(8, 1 << 25) > 0
