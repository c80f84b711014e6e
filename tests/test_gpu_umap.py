"""The fuzzy graph's rows, the layout's epochs and the whole map on the GPU (``Engine.umap_smooth``, ``Engine.umap_epoch``,
``umap.embed``; csrc/kernels_umap.hip) against the float64 restatement of tests/_umap_ref.py: ``-m gpu``."""
import numpy as np
import pytest
import torch

from biscuit_amd import umap
from tests import _umap_cases as cases
from tests import _umap_ref as ref
from tests.test_gpu_abi_homes import _engine
from tests.test_umap import EPOCH_HOST_ERR, EPOCH_SEED, epoch_case, epochs_f64

pytestmark = pytest.mark.gpu

# The float64 restatement's whole layout (cluster case, 15 neighbours, 200 epochs, PCA start) under the negative-sampling seeds
# 0 .. 3, measured on the CPU: sklearn's trustworthiness at 15 neighbours, per data seed.  Two hundred epochs amplify any rounding
# difference, so a device run is one more draw from the distribution these four are drawn from, not a copy of the draw with its
# seed: it is held to their mean minus the restatement's own spread (highest - lowest of the four), the largest over the data
# seeds: 0.0009.
REF_TRUST = {0: (0.9871, 0.9876, 0.9877, 0.9876), 1: (0.9889, 0.9882, 0.9886, 0.9880), 2: (0.9880, 0.9879, 0.9881, 0.9879),
             3: (0.9889, 0.9885, 0.9887, 0.9882)}
REF_SPREAD = max(max(v) - min(v) for v in REF_TRUST.values())
assert abs(REF_SPREAD - 0.0009) < 1e-12
PCA_TRUST = {0: 0.9600, 1: 0.9331, 2: 0.9722, 3: 0.9755}           # sklearn's 2-D PCA of the same data (recomputed in the test)


@pytest.fixture(scope='module')
def eng():
    e = _engine()
    yield e
    e.close()


def up(eng, a):
    return torch.tensor(np.asarray(a)).to(eng.device)


def test_smoothing(eng):
    idx, dist = cases.smoothing_table(15)
    rho, sigma, w = (t.cpu().numpy() for t in eng.umap_smooth(up(eng, idx), up(eng, dist)))
    r_rho, r_sigma, r_w, floored = ref.smooth(idx, dist)
    assert floored[-3:].all() and not floored[:-3].any()
    k = idx.shape[1]
    worst = max(abs(ref.smooth_sum(dist[i], float(rho[i]), float(sigma[i])) - np.log2(k)) for i in np.nonzero(~floored)[0])
    print(f'largest |sum - log2 k| = {worst:.3e} (bound {1e-5 + k * 2.0 ** -20:.3e})')
    assert worst <= 1e-5 + k * 2.0 ** -20
    assert np.array_equal(rho, r_rho.astype(np.float32))
    np.testing.assert_allclose(sigma[floored], r_sigma[floored], rtol=1e-5)
    np.testing.assert_allclose(w, r_w, rtol=1e-5, atol=1e-30)
    assert not w[np.arange(len(idx)), 0].any()
    h_rho, h_sigma, h_w = umap.smooth_host(idx, dist)
    np.testing.assert_allclose(sigma, h_sigma, rtol=1e-5)
    with pytest.raises(ValueError):
        eng.umap_smooth(up(eng, idx), up(eng, dist[:, :-1]))


def device_epochs(eng, indptr, nbr, eps, init, a, b, block=0, n=3):
    graph = umap.graph_to_device(eng, len(init), indptr, nbr, eps)
    cur = up(eng, init)
    for ep in range(1, n + 1):
        cur = eng.umap_epoch(cur, graph, ep, 1.0 - (ep - 1) / 200.0, a, b, EPOCH_SEED, block=block)
    return cur.cpu().numpy(), graph[3].cpu().numpy()


def test_three_epochs_against_float64(eng):
    indptr, nbr, eps, init, a, b = epoch_case()
    want, want_next = epochs_f64(indptr, nbr, eps, init, a, b)
    got, nxt = device_epochs(eng, indptr, nbr, eps, init, a, b)
    err = float(np.abs(got - want).max())
    print(f'device against float64 after three epochs: {err:.3e} (bound 4 x {EPOCH_HOST_ERR:.3e})')
    assert np.isfinite(got).all() and err <= 4 * EPOCH_HOST_ERR
    np.testing.assert_allclose(nxt, want_next, rtol=1e-6)
    again, nxt2 = device_epochs(eng, indptr, nbr, eps, init, a, b)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(nxt2, nxt)
    other, _ = device_epochs(eng, indptr, nbr, eps, init, a, b, block=256)      # another launch geometry: the same bits
    assert np.array_equal(other.view(np.uint32), got.view(np.uint32))
    graph = umap.graph_to_device(eng, len(init), indptr, nbr, eps)
    from biscuit_amd.engine import BiscuitHipError
    with pytest.raises(BiscuitHipError, match='block'):
        eng.umap_epoch(up(eng, init), graph, 1, 1.0, a, b, 0, block=100)
    with pytest.raises(BiscuitHipError, match='d_out == d_prev'):
        cur = up(eng, init)
        eng.umap_epoch(cur, graph, 1, 1.0, a, b, 0, out=cur)


def purity(y, lab):
    d = ((y[:, None].astype(np.float64) - y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((lab[d.argmin(1)] == lab).mean())


@pytest.mark.parametrize('seed', cases.CLUSTER_SEEDS)
def test_whole_layout(eng, seed):
    from sklearn.decomposition import PCA
    from sklearn.manifold import trustworthiness
    x, lab = cases.cluster(seed), cases.labels()
    y = umap.embed(eng, x, n_neighbors=15, min_dist=0.1, seed=0, n_epochs=200)
    assert y.shape == (600, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    trust = trustworthiness(x, y, n_neighbors=15)
    pca = trustworthiness(x, PCA(2).fit_transform(x), n_neighbors=15)
    d2 = ref.case_sqdist('cluster', seed).copy()
    np.fill_diagonal(d2, np.inf)
    original = float((lab[d2.argmin(1)] == lab).mean())
    mapped = purity(y, lab)
    print(f'seed {seed}: trustworthiness {trust:.4f} (PCA {pca:.4f}, float64 {REF_TRUST[seed]}), purity {mapped:.4f} (original space {original:.4f})')
    assert abs(pca - PCA_TRUST[seed]) < 5e-4
    assert trust > pca
    assert trust >= float(np.mean(REF_TRUST[seed])) - REF_SPREAD
    assert mapped >= original - 0.01
