"""``Engine.knn`` (bq_knn, csrc/kernels_knn.hip) against the float64 oracle of tests/_umap_ref.py and the CPU build, on the cases of
tests/_umap_cases.py: ``-m gpu``.  The near-duplicate rows are where a kernel that returned its GEMM-form distances would fail."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import umap
from tests import _umap_cases as cases
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
    rel = ref.check_table(d2, idx, dist, cases.D)
    h_idx, h_dist = umap.knn_host(x, 15)
    decided = ref.decided(d2, 15, cases.D)
    same = (idx == h_idx).all(1)
    print(f'{name} {seed}: relative error {rel:.3e}; {int(same.sum())} of {len(x)} rows equal the CPU build, {int(decided.sum())} decided')
    assert np.array_equal(idx[decided], h_idx[decided])
    assert np.array_equal(dist[same].view(np.uint32), h_dist[same].view(np.uint32))       # the direct form's bits are the CPU build's
    idx2, dist2 = run(eng, x, 15)
    assert np.array_equal(idx, idx2) and np.array_equal(dist.view(np.uint32), dist2.view(np.uint32))


@pytest.mark.parametrize('n,d,k', cases.SMALL)
def test_small_shapes(eng, n, d, k):
    x = cases.small(n, d)
    idx, dist = run(eng, x, k)
    d2 = ref.sqdist(x)
    ref.check_table(d2, idx, dist, d)
    h_idx, h_dist = umap.knn_host(x, k)
    decided = ref.decided(d2, k, d)
    assert np.array_equal(idx[decided], h_idx[decided])
    assert (idx[:, 0] == np.arange(n)).all() and not dist[:, 0].any()


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
    assert need == 256 + 5 * 2 * 18 * 4
    rc = eng._lib.bq_knn(eng._ctx, ptr(x), 5, 48, 2, ptr(out_i), ptr(out_d), ptr(ws), need - 1, eng._stream())
    assert rc == -4 and b'workspace' in eng._lib.bq_last_error(eng._ctx)
    torch.cuda.synchronize(eng.device)
    assert not out_i.any()                                          # nothing was enqueued
