"""The inputs of the feature-map tests (tests/test_umap.py, tests/test_gpu_knn.py, tests/test_gpu_umap.py)."""
import functools

import numpy as np

D = 2048
N_CLUSTER, N_LABELS = 600, 12
CLUSTER_SEEDS = (0, 1, 2, 3)
SMALL = ((1, 48, 1), (63, 48, 1), (63, 48, 15), (63, 48, 50), (257, 48, 15), (257, 48, 64), (64, 16, 64))      # (n, D, k)


def labels():
    return np.arange(N_CLUSTER) % N_LABELS


@functools.lru_cache(maxsize=None)
def cluster(seed=0):
    """600 points of 12 clusters (by i % 12): 8 latent dimensions, centres N(0, 4^2), noise N(0, 1), mapped by a Gaussian 8 x 2048
    matrix scaled by 1 / sqrt(8), then ReLU: what pooled activations look like."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (N_LABELS, 8))
    latent = centres[labels()] + rng.normal(0.0, 1.0, (N_CLUSTER, 8))
    m = rng.normal(0.0, 1.0, (8, D)) / np.sqrt(8.0)
    x = np.maximum(latent @ m, 0.0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def integer():
    """300 rows of integers 0 .. 15, rows 7 and 200 copies of row 3: every product and sum stays below 2^24 (2048 x 15^2 x 2 <
    2^20), so fp32 is exact in the GEMM form and in the direct form, and equal distances are decided by the index."""
    x = np.random.default_rng(100).integers(0, 16, (300, D)).astype(np.float32)
    x[7] = x[3]
    x[200] = x[3]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def near_duplicate():
    """The cluster case with 32 rows replaced by another row + 1e-3 N(0, 1): distances 10^-7 of the squared norms, where the GEMM
    form has no digit left."""
    x = cluster(0).copy()
    rng = np.random.default_rng(1000)
    rows = rng.choice(N_CLUSTER, 64, replace=False)
    dst, src = rows[:32], rows[32:]
    x[dst] = x[src] + (1e-3 * rng.normal(0.0, 1.0, (32, D))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def small(n, d, seed=0):
    x = np.random.default_rng(7000 + n + seed).normal(0.0, 1.0, (n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def get(name, seed=0):
    return {'cluster': lambda: cluster(seed), 'integer': integer, 'near_duplicate': near_duplicate}[name]()


def smoothing_table(k=15):
    """A neighbour table for the smoothing: 64 of the cluster case's own rows, then three rows that end on the floor -- one whose
    distances are all equal (2.5), one with zero-distance duplicates in front of equal distances (rho = 1, the smallest NON-zero
    one), and one of zeros only (rho = 0: its floor is the global mean's).  -> (idx, dist) host arrays sorted as ``knn`` sorts them;
    built from float64 distances, so it needs no kernel."""
    from tests import _umap_ref as ref
    d2 = ref.case_sqdist('cluster', 0)
    idx = ref.knn(d2, k)[:64].astype(np.int32)
    dist = np.sqrt(np.take_along_axis(d2[:64], idx.astype(np.int64), 1)).astype(np.float32)
    extra_d = np.zeros((3, k), np.float32)
    extra_d[0, 1:] = 2.5
    extra_d[1, 3:] = 1.0
    extra_i = np.tile(np.arange(100, 100 + k, dtype=np.int32), (3, 1))
    extra_i[:, 0] = (64, 65, 66)
    return np.concatenate([idx, extra_i]), np.concatenate([dist, extra_d])
