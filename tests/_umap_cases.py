"""The inputs of the feature-map tests (tests/test_umap.py, tests/test_gpu_knn.py, tests/test_gpu_umap.py)."""
import functools

import numpy as np

D = 2048
N_CLUSTER, N_LABELS = 600, 12
CLUSTER_SEEDS = (0, 1, 2, 3)
# (n, D, k); D = 80 is the smallest D at which the direct form's 64-element step is taken a second time, and cut
SMALL = ((1, 48, 1), (63, 48, 1), (63, 48, 15), (63, 48, 50), (257, 48, 15), (257, 48, 64), (64, 16, 64), (33, 80, 5))


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


# ---- tight groups: more rows than a query's candidate lists hold, closer together than the GEMM form's rounding error -------
# name -> (k's the case is used at, D, the group's rows); the group is where the pruning pass's order is rounding noise
TIGHT_SCALE = {'tight_lowrank': 1e-3, 'tight_fullrank': 1e-3, 'tight_small': 1e-4}
TIGHT = {'tight_lowrank': ((15, 50), D, slice(100, 300)), 'tight_fullrank': ((15,), D, slice(100, 196)),
         'tight_small': ((15,), 48, slice(57, 257))}
CONTROL = {'wide_control': ((15,), D, slice(100, 300))}


def _low_rank_group(rank, scale):
    """The cluster case with rows 100 .. 299 replaced by ReLU(row 17 + scale N(0, 1)[200, rank] @ M), M standard normal."""
    x = cluster(0).copy()
    rng = np.random.default_rng(5)
    m = rng.normal(0.0, 1.0, (rank, D))
    x[100:300] = np.maximum(x[17] + scale * rng.normal(0.0, 1.0, (200, rank)) @ m, 0.0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tight_lowrank():
    """200 rows on a 2-dimensional patch around row 17, squared distances of 10^-2 against squared norms of 1.8 10^4: the
    neighbours inside the patch are well separated (few directions), and the GEMM form cannot tell them apart."""
    return _low_rank_group(2, TIGHT_SCALE['tight_lowrank'])


@functools.lru_cache(maxsize=None)
def wide_control():
    """The same on 3 dimensions with three times the spread: wide enough for the GEMM form to keep every true neighbour."""
    return _low_rank_group(3, 3e-3)


@functools.lru_cache(maxsize=None)
def tight_fullrank():
    """The cluster case with rows 100 .. 195 replaced by row 17 + 1e-3 N(0, 1) in all 2048 columns: the distances concentrate, so
    a lost neighbour is only a little further than the k-th."""
    x = cluster(0).copy()
    rng = np.random.default_rng(6)
    x[100:196] = x[17] + (TIGHT_SCALE['tight_fullrank'] * rng.normal(0.0, 1.0, (96, D))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tight_small():
    """257 x 48 (nine query tiles, the last one cut), rows N(0, 1) + 20, the last 200 of them row 3 + 1e-4 N(0, 1)."""
    rng = np.random.default_rng(8)
    x = (rng.normal(0.0, 1.0, (257, 48)) + 20.0).astype(np.float32)
    x[57:] = x[3] + (TIGHT_SCALE['tight_small'] * rng.normal(0.0, 1.0, (200, 48))).astype(np.float32)
    x.setflags(write=False)
    return x


def get(name, seed=0):
    return {'cluster': lambda: cluster(seed), 'integer': integer, 'near_duplicate': near_duplicate, 'tight_lowrank': tight_lowrank,
            'tight_fullrank': tight_fullrank, 'tight_small': tight_small, 'wide_control': wide_control}[name]()


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
