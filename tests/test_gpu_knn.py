"""``Engine.knn`` (bq_knn, csrc/kernels_knn.hip) against the float64 oracle of tests/_umap_ref.py and the CPU build, on the cases of
tests/_umap_cases.py: ``-m gpu``.  The device is the CPU build on EVERY row, bit for bit.  The near-duplicate rows are where a
kernel that returned its GEMM-form distances would fail; the tight groups are where one that trusted its pruning pass did -- the
kernel before the certificate differed from the CPU build on 200 of the low-rank group's 200 rows at k = 15 and at k = 50 (a
returned neighbour at up to 6.8 x and 2.1 x the true k-th squared distance), on 96 of the full-rank group's 96 (1.018 x), on 200 of
the small group's 200 (1.29 x) and on 149 of the wide control's 200 (1.78 x), which numpy's summation order does not lose."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import umap
from tests import _umap_cases as cases
from tests import _poison as P
from tests import _umap_ref as ref
from tests.test_gpu_abi_homes import _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = _engine()
    yield e
    e.close()


def run(eng, x, k):
    idx, dist = eng.knn(torch.tensor(x).to(eng.device), k)
    return idx.cpu().numpy(), dist.cpu().numpy()


def exhaustive(eng, n):
    """How many of the last call's rows the certificate did not cover."""
    return int(eng.knn_exhaustive_rows(n).sum())


def is_the_cpu_build(eng, x, k, idx, dist):
    """Every row, bit for bit, and the same from a second run."""
    h_idx, h_dist = umap.knn_host(x, k)
    differ = (idx != h_idx).any(1)
    assert not differ.any(), f'{int(differ.sum())} of {len(x)} rows differ from the CPU build (first: row {int(differ.argmax())})'
    assert np.array_equal(dist.view(np.uint32), h_dist.view(np.uint32))       # the direct form's bits are the CPU build's
    idx2, dist2 = run(eng, x, k)
    assert np.array_equal(idx, idx2) and np.array_equal(dist.view(np.uint32), dist2.view(np.uint32))


def test_integer_case_is_the_oracle_exactly(eng):
    x, d2 = cases.integer(), ref.case_sqdist('integer')
    for k in (15, 50):
        idx, dist = run(eng, x, k)
        want = ref.knn(d2, k)
        assert np.array_equal(idx, want)
        assert np.array_equal(dist, np.sqrt(np.take_along_axis(d2, want, 1)).astype(np.float32))
    assert idx[3, :3].tolist() == [3, 7, 200] and idx[200, :3].tolist() == [3, 7, 200]


@pytest.mark.parametrize('name,seed', [('cluster', s) for s in cases.CLUSTER_SEEDS] + [('near_duplicate', 0)])
def test_cluster_cases(eng, name, seed):
    x, d2 = cases.get(name, seed), ref.case_sqdist(name, seed)
    idx, dist = run(eng, x, 15)
    redone = exhaustive(eng, len(x))
    rel = ref.check_table(d2, idx, dist, cases.D)
    print(f'{name} {seed}: relative error {rel:.3e}; {redone} of {len(x)} rows ranked again over all rows')
    is_the_cpu_build(eng, x, 15, idx, dist)


@pytest.mark.parametrize('name,k', [(name, k) for name, (ks, _, _) in {**cases.TIGHT, **cases.CONTROL}.items() for k in ks])
def test_tight_groups(eng, name, k):
    """Groups of more rows than the candidate lists hold, closer together than the GEMM form's rounding error: the pruning pass
    cannot prove these rows, so they are ranked again over all rows -- at least one of them, or the certificate did not run."""
    _, d, rows = {**cases.TIGHT, **cases.CONTROL}[name]
    x, d2 = cases.get(name), ref.case_sqdist(name)
    idx, dist = run(eng, x, k)
    redone = eng.knn_exhaustive_rows(len(x)).cpu().numpy()
    rel = ref.check_table(d2, idx, dist, d)
    print(f'{name} k = {k}: relative error {rel:.3e}; {int(redone.sum())} of {len(x)} rows ranked again over all rows, '
          f'{int(redone[rows].sum())} of the group\'s {len(redone[rows])}')
    is_the_cpu_build(eng, x, k, idx, dist)
    if name in cases.TIGHT:
        assert redone[rows].any()


@pytest.mark.parametrize('n,d,k', cases.SMALL)
def test_small_shapes(eng, n, d, k):
    x = cases.small(n, d)
    idx, dist = run(eng, x, k)
    print(f'{n} x {d}, k = {k}: {exhaustive(eng, n)} rows ranked again over all rows')
    ref.check_table(ref.sqdist(x), idx, dist, d)
    is_the_cpu_build(eng, x, k, idx, dist)
    assert (idx[:, 0] == np.arange(n)).all() and not dist[:, 0].any()


def test_values_that_are_not_finite_are_refused(eng):
    for bad in (float('nan'), float('inf')):
        x = torch.tensor(cases.small(33, 48)).to(eng.device)
        x[5, 7] = bad
        with pytest.raises(ValueError, match='finite'):
            eng.knn(x, 5)


@pytest.mark.parametrize('fill', P.BYTE_FILLS)
def test_the_raw_call_writes_every_place_of_a_row_it_cannot_fill(eng, fill):
    """bq_knn itself, its precondition broken: row 20 holds a NaN, so it is nobody's candidate and has none.  Under poisoned,
    guarded outputs and scratch the finite rows are the CPU build's table of the other 32 rows, and row 20 is -1 / NaN throughout."""
    n, d, k, nan_row = 33, 48, 5, 20
    x = cases.small(n, d).copy()
    x[nan_row, 7] = np.nan
    others = np.delete(np.arange(n), nan_row)
    w_idx, w_dist = umap.knn_host(x[others], k)
    need = eng._lib.bq_knn_workspace_bytes(n, d, k)
    (out_i, chk_i), (out_d, chk_d), (ws, chk_w) = (P.guarded(b, fill, eng.device) for b in (n * k * 4, n * k * 4, need))
    dx = torch.tensor(x).to(eng.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert eng._lib.bq_knn(eng._ctx, ptr(dx), n, d, k, ptr(out_i), ptr(out_d), ptr(ws), need, eng._stream()) == 0
    torch.cuda.synchronize(eng.device)
    for chk in (chk_i, chk_d, chk_w):
        chk()
    idx, dist = out_i.view(torch.int32).view(n, k).cpu().numpy(), out_d.view(torch.float32).view(n, k).cpu().numpy()
    assert np.array_equal(idx[others], others[w_idx]) and np.array_equal(dist[others].view(np.uint32), w_dist.view(np.uint32))
    assert (idx[nan_row] == -1).all() and np.isnan(dist[nan_row]).all()
    assert eng.knn_exhaustive_rows(n, ws).all()                    # (a NaN certifies nothing)


def test_refusals(eng):
    x = torch.zeros((5, 48), dtype=torch.float32, device=eng.device)
    out_i = torch.zeros((5, 6), dtype=torch.int32, device=eng.device)
    out_d = torch.zeros((5, 6), dtype=torch.float32, device=eng.device)
    ws = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for n, d, k in ((5, 48, 6), (5, 48, 0), (5, 48, 65), (5, 40, 2)):
        assert eng._lib.bq_knn_workspace_bytes(n, d, k) == 0
        rc = eng._lib.bq_knn(eng._ctx, ptr(x), n, d, k, ptr(out_i), ptr(out_d), ptr(ws), ws.numel(), eng._stream())
        assert rc < 0 and b'bq_knn' in eng._lib.bq_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.knn(x[:, :d].contiguous(), k)
    need = eng._lib.bq_knn_workspace_bytes(5, 48, 2)
    assert need == 2 * 256 + 5 * 2 * 18 * 4 + 5 * 2 * 4            # flags, norms, candidate lists, the halves' floors
    rc = eng._lib.bq_knn(eng._ctx, ptr(x), 5, 48, 2, ptr(out_i), ptr(out_d), ptr(ws), need - 1, eng._stream())
    assert rc == -4 and b'workspace' in eng._lib.bq_last_error(eng._ctx)
    torch.cuda.synchronize(eng.device)
    assert not out_i.any()                                          # nothing was enqueued
