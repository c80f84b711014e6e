"""The feature map's three entries on memory whose contents are unspecified (DESIGN.md "Buffer contract"): every output and every
scratch buffer ``Engine`` allocates is poisoned and guarded (tests/_poison.py) with each of the bytes 0x00, 0xFF and 0xA5, and
``knn``, ``umap_smooth`` and ``umap_epoch`` give the bits of a clean run with every guard intact.  Then the profiling classes they
open and ``close()`` letting go of their scratch.  ``-m gpu``."""
import numpy as np
import pytest
import torch

from biscuit_amd import umap
from tests import _poison as P
from tests import _umap_cases as cases
from tests.test_gpu_abi_homes import _device_tensors, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = _engine()
    yield e
    e.close()


def up(eng, a):
    return torch.tensor(np.asarray(a)).to(eng.device)


def all_three(eng, own_scratch=False):
    """257 rows of 48 columns (nine query tiles, the last one cut; candidates in both halves of a tile) through ``knn`` at k = 15,
    the table through ``umap_smooth``, its graph through two epochs.  -> host arrays."""
    x = up(eng, cases.small(257, 48))
    idx, dist = eng.knn(x, 15, scratch=eng.knn_scratch(257, 48, 15) if own_scratch else None)
    rho, sigma, w = eng.umap_smooth(idx, dist, scratch=eng._bytes(eng._lib.bq_umap_smooth_scratch_bytes(257)) if own_scratch else None)
    indptr, nbr, eps = umap.fuzzy_graph(idx.cpu().numpy(), w.cpu().numpy(), 50)
    graph = umap.graph_to_device(eng, 257, indptr, nbr, eps)
    y = up(eng, umap.pca_init(cases.small(257, 48)))
    for ep in (1, 2):
        y = eng.umap_epoch(y, graph, ep, 1.0 - (ep - 1) / 50.0, 1.5769, 0.8951, 3)
    return [t.cpu().numpy() for t in (idx, dist, rho, sigma, w, y, graph[3])]


@pytest.mark.parametrize('own_scratch', [False, True])
def test_results_do_not_depend_on_stale_bytes(eng, own_scratch):
    import biscuit_amd.engine as engine_mod
    clean = all_three(eng, own_scratch)
    assert np.isfinite(clean[5]).all() and (clean[0][:, 0] == np.arange(257)).all()
    for fill in P.BYTE_FILLS:
        torch.cuda.synchronize(eng.device)
        eng.drop_scratch()
        proxy = P.poisoned_torch(fill)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, 'torch', proxy)
            out = all_three(eng, own_scratch)
        torch.cuda.synchronize(eng.device)
        assert proxy.served >= 9                                    # idx, dist, two scratch buffers, rho, sigma, w, two positions
        proxy.check()
        for k, (a, b) in enumerate(zip(clean, out)):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f'result {k} under 0x{fill:02X} differs from a clean run'


@pytest.mark.parametrize('own_scratch', [False, True])
def test_rows_ranked_again_do_not_depend_on_stale_bytes(eng, own_scratch):
    """``knn`` alone on the small tight group (257 x 48, k = 15), where most rows are ranked again over all rows: the flags, the
    halves' floors and the second pass's output under poison."""
    import biscuit_amd.engine as engine_mod
    x = up(eng, cases.tight_small())

    def knn(mod):
        scratch = eng.knn_scratch(257, 48, 15) if own_scratch else None
        idx, dist = eng.knn(x, 15, scratch=scratch)
        redone = eng.knn_exhaustive_rows(257, scratch)
        return [t.cpu().numpy() for t in (idx, dist, redone)]
    clean = knn(torch)
    assert clean[2].sum() >= 100 and (clean[0] >= 0).all()
    for fill in P.BYTE_FILLS:
        torch.cuda.synchronize(eng.device)
        eng.drop_scratch()
        proxy = P.poisoned_torch(fill)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, 'torch', proxy)
            out = knn(proxy)
        torch.cuda.synchronize(eng.device)
        assert proxy.served >= 3                                    # idx, dist, the scratch
        proxy.check()
        for k, (a, b) in enumerate(zip(clean, out)):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f'result {k} under 0x{fill:02X} differs from a clean run'


def test_exactly_the_three_new_classes():
    eng = _engine()
    try:
        eng.profile_enable(True)
        all_three(eng)
        prof = eng.profile_read()
        assert {p.name for p in prof} == {'knn', 'umap_smooth', 'umap_epoch'}
        assert {p.name: p.launches for p in prof} == {'knn': 1, 'umap_smooth': 1, 'umap_epoch': 2}
    finally:
        eng.close()


def test_close_lets_go_of_the_scratch():
    eng = _engine()
    all_three(eng)
    assert {'knn', 'umap'} <= {k for k, v in eng._tool_ws.items() if _device_tensors(v)}, eng._tool_ws.keys()
    eng.close()
    assert {k: v for k, v in vars(eng).items() if _device_tensors(v)} == {}
