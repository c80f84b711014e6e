"""The Macenko normaliser's kernel (bq_stain_macenko / bq_stain_macenko_stats) against tests/_macenko_ref.py at the edges of its
order statistics: the cases of tests/_macenko_cases.py (test_macenko_cases.py shows on the CPU that each is what it claims and
that the reference is well defined on it).

Statistics are compared with the float64 reference within max(2e-6, 4 s(case)), s(case) being the reference's own float64 /
float32 difference -- never a number the kernel produced.  The expected bytes are the float64 transform fed the kernel's OWN reported
statistics (both entry points run the same code up to the transform), so a statistic's rounding is measured once and cannot
excuse a byte.  Every case runs alone (n = 1) and once in one batch of all of them.
"""
import numpy as np
import pytest

import _macenko_cases as mc
import _macenko_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(mc.cases())
TWO = [n for n in NAMES if n.startswith('two_pixels')]
FITS = list(mc.fits())


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(seed=1), dtype='bf16', max_batch=8, max_mc=4)
    yield e
    e.close()


def _run(eng, d):
    """One call of each entry point on the device tiles d: dict(stats [n,8] f32, st [n,2] i32, fit: (bytes, status [n]))."""
    import torch
    stats, st = eng.macenko_stats(d)
    out = {'stats': stats.cpu().numpy(), 'st': st.cpu().numpy()}
    for fit, (he, maxc) in mc.fits().items():
        status = torch.full((d.shape[0],), -1, dtype=torch.int32, device=d.device)
        out[fit] = (eng.macenko(d, he, maxc, status=status).cpu().numpy(), status.cpu().numpy())
    return out


@pytest.fixture(scope='module')
def dev():
    import torch
    return torch.from_numpy(np.stack([np.asarray(mc.cases()[n]) for n in NAMES])).cuda()


@pytest.fixture(scope='module')
def alone(eng, dev):
    """{name: _run of the tile alone, n = 1}."""
    return {n: _run(eng, dev[i:i + 1]) for i, n in enumerate(NAMES)}


def _same(a, b):
    """Two _run results (of one tile each, or of the same tiles) agree bit for bit."""
    ok = np.array_equal(a['stats'].view(np.uint32), b['stats'].view(np.uint32)) and np.array_equal(a['st'], b['st'])
    return ok and all(np.array_equal(a[f][0], b[f][0]) and np.array_equal(a[f][1], b[f][1]) for f in FITS)


def _pick(run, i):
    return {'stats': run['stats'][i:i + 1], 'st': run['st'][i:i + 1], **{f: (run[f][0][i:i + 1], run[f][1][i:i + 1]) for f in FITS}}


def test_status_and_tissue_count_are_the_references(alone):
    for name in mc.compared():
        ref, got = mc.reference(name), alone[name]
        assert (int(got['st'][0, 0]), int(got['st'][0, 1])) == (ref['status'], ref['n_tissue']), name
        for f in FITS:                                                           # bq_stain_macenko reports the same status
            assert int(got[f][1][0]) == ref['status'], (name, f)


def test_statistics_against_the_float64_reference(alone):
    """HE (absolute) and maxC (relative) wherever the reference has them -- the NONFINITE sparse_glass tiles included, where both
    sides still report HE and the non-positive maxC."""
    failed = []
    print()
    for name in mc.compared():
        ref, got = mc.reference(name), alone[name]['stats'][0].astype(np.float64)
        assert np.isfinite(got).all(), (name, got)
        d_he = float(np.abs(got[:6].reshape(3, 2) - ref['HE']).max())
        d_c = float(np.abs(got[6:] / ref['maxC'] - 1).max())
        (s_he, s_c), (b_he, b_c) = mc.sensitivity(name), mc.bounds(name)
        print(f'{name:24s} s_HE {s_he:.2e} s_maxC {s_c:.2e}  bound {b_he:.2e} {b_c:.2e}  kernel dHE {d_he:.2e} dmaxC {d_c:.2e}')
        if not (d_he <= b_he and d_c <= b_c):
            failed.append((name, d_he, b_he, d_c, b_c))
    assert not failed, failed


@pytest.mark.parametrize('fit', FITS)
def test_bytes_against_the_transform_of_the_reported_statistics(alone, fit):
    """No byte off by more than 1, at most 1e-3 of a tile's bytes differing (the bounds test_stain_macenko.py holds)."""
    he_ref, maxc_ref = mc.fits()[fit]
    failed = []
    print()
    for name in mc.compared():
        got = alone[name]
        if got['st'][0, 0] != R.OK:
            continue
        x = np.asarray(mc.cases()[name])
        want = R.transform(x, got['stats'][0, :6].reshape(3, 2), got['stats'][0, 6:], he_ref, maxc_ref)
        d = np.abs(got[fit][0][0].astype(np.int16) - want.astype(np.int16))
        print(f'{name:24s} {fit}: max diff {int(d.max())}, differing {int((d > 0).sum())} of {d.size}')
        if not (d.max() <= 1 and (d > 0).mean() <= 1e-3):
            failed.append((name, int(d.max()), float((d > 0).mean())))
    assert not failed, failed


def test_degenerate_tiles_pass_through(eng, dev, alone):
    """Every case with a non-zero status: byte for byte into a fresh buffer, in place, and into a slice of a larger buffer whose
    neighbours stay untouched, with its status delivered through status=."""
    import torch
    he, maxc = mc.fits()['preset']
    degenerate = [n for n in NAMES if alone[n]['st'][0, 0] != R.OK]
    assert set(degenerate) >= {n for n in mc.compared() if mc.reference(n)['status'] != R.OK} and len(degenerate) >= 8
    for name in degenerate:
        i = NAMES.index(name)
        x, want_status = np.asarray(mc.cases()[name]), int(alone[name]['st'][0, 0])
        for f in FITS:
            assert np.array_equal(alone[name][f][0][0], x) and int(alone[name][f][1][0]) == want_status, (name, f)
        inplace = dev[i:i + 1].clone()
        status = torch.full((1,), -1, dtype=torch.int32, device='cuda')
        r = eng.macenko(inplace, he, maxc, out=inplace, status=status)
        assert r.data_ptr() == inplace.data_ptr() and torch.equal(inplace, dev[i:i + 1]) and int(status[0]) == want_status, name
        big = torch.full((3,) + tuple(dev.shape[1:]), 7, dtype=torch.uint8, device='cuda')
        status.fill_(-1)
        eng.macenko(dev[i:i + 1], he, maxc, out=big[1:2], status=status)
        assert torch.equal(big[1], dev[i]) and bool((big[0] == 7).all()) and bool((big[2] == 7).all()), name
        assert int(status[0]) == want_status
    # a normalised tile leaves its neighbours alone too
    i = NAMES.index('full_tissue')
    big = torch.full((3,) + tuple(dev.shape[1:]), 7, dtype=torch.uint8, device='cuda')
    eng.macenko(dev[i:i + 1], he, maxc, out=big[1:2])
    assert np.array_equal(big[1].cpu().numpy(), alone['full_tissue']['preset'][0][0])
    assert bool((big[0] == 7).all()) and bool((big[2] == 7).all())


@pytest.mark.parametrize('name', TWO)
def test_two_pixels(eng, dev, alone, name):
    """The middle eigenvector of two points is arbitrary: only the status rules are asserted."""
    got = alone[name]
    status = int(got['st'][0, 0])
    print(f'\n{name}: status {status} (reference {mc.reference(name)["status"]})')
    assert int(got['st'][0, 1]) == 2 and status in (R.OK, R.SINGULAR, R.NONFINITE)
    for f in FITS:
        assert int(got[f][1][0]) == status
        if status != R.OK:
            assert np.array_equal(got[f][0][0], np.asarray(mc.cases()[name]))
    i = NAMES.index(name)
    assert _same(got, _run(eng, dev[i:i + 1]))                                   # the same outputs in two runs


def test_batch_equals_the_single_runs_in_both_orders(eng, dev, alone):
    import torch
    batch = _run(eng, dev)
    flipped = _run(eng, torch.flip(dev, (0,)).contiguous())
    n = len(NAMES)
    for i, name in enumerate(NAMES):
        assert _same(_pick(batch, i), alone[name]), name
        assert _same(_pick(flipped, n - 1 - i), alone[name]), name
