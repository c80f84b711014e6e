"""UMAP's stages restated in float64 numpy (DESIGN.md "Feature map (Figure 6)"): what tests/test_umap.py holds the CPU build to
and tests/test_gpu_knn.py / tests/test_gpu_umap.py the kernels.  Written from the same description as csrc/umap_device.h, not
from its code: brute-force neighbours in (distance, index) order, the smoothing bisection, the dense symmetrisation, one epoch
of the gather form (vectorised over the vertices, slot by slot, which is the order a vertex walks its row in) and the
constants' known values."""
import functools

import numpy as np

from oracle.philox import philox4x32_10

NEG_RATE = 5

# (min_dist -> (a, b)) of scipy.optimize.curve_fit on the curve 1 / (1 + a x^(2b)), spread 1, 300 points on [0, 3]
AB = {0.1: (1.57694346, 0.89506088), 0.5: (0.58303002, 1.33416699), 0.0: (1.9328084, 0.79049497)}


def eps_for(d):
    """2 (D + 2) 2^-24: the worst-case relative error of an fp32 sum of D squared differences."""
    return 2.0 * (d + 2) * 2.0 ** -24


def sqdist(x):
    """Every pair's squared distance, the direct form in float64: [n, n]."""
    x = np.asarray(x, np.float64)
    out = np.empty((len(x), len(x)))
    for i in range(len(x)):
        out[i] = ((x - x[i]) ** 2).sum(1)
    return out


def knn(d2, k):
    """``d2`` [n, n] -> ``idx`` [n, k] by (squared distance, index) ascending."""
    n = len(d2)
    idx = np.empty((n, k), np.int64)
    for i in range(n):
        idx[i] = np.lexsort((np.arange(n), d2[i]))[:k]
    return idx


def smooth(idx, dist):
    """-> ``(rho, sigma, w, floored)``: the row's smallest non-zero distance, the bisection's sigma after the floor, the weights and
    whether the floor replaced the search's value."""
    idx, dist = np.asarray(idx), np.asarray(dist, np.float64)
    n, k = dist.shape
    target, mean_all = np.log2(k), dist.mean()
    rho, sigma, w, floored = np.zeros(n), np.zeros(n), np.zeros((n, k)), np.zeros(n, bool)
    for i in range(n):
        d = dist[i]
        nz = d[d > 0]
        rho[i] = nz[0] if len(nz) else 0.0
        t = np.maximum(d[1:] - rho[i], 0.0)
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            psum = np.exp(-t / mid).sum()
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2
        floor = 1e-3 * (d.mean() if rho[i] > 0 else mean_all)
        floored[i] = mid < floor
        sigma[i] = max(mid, floor)
        w[i] = np.where(d - rho[i] <= 0, 1.0, np.exp(-np.maximum(d - rho[i], 0.0) / sigma[i]))
        w[i][idx[i] == i] = 0.0
    return rho, sigma, w, floored


def smooth_sum(dist_row, rho, sigma):
    """sum_{j >= 1} exp(-max(0, d_j - rho) / sigma) in float64."""
    return float(np.exp(-np.maximum(np.asarray(dist_row[1:], np.float64) - rho, 0.0) / sigma).sum())


def graph(idx, w, n_epochs):
    """Dense symmetrisation, pruning and the CSR: ``(indptr, nbr, eps)`` with eps in float64."""
    n = len(idx)
    m = np.zeros((n, n))
    m[np.repeat(np.arange(n), idx.shape[1]), np.asarray(idx).ravel()] = np.asarray(w, np.float64).ravel()
    s = m + m.T - m * m.T
    s[s < s.max() / n_epochs] = 0.0
    indptr, nbr, eps = [0], [], []
    for i in range(n):
        j = np.nonzero(s[i])[0]
        nbr.append(j)
        eps.append(s.max() / s[i, j])
        indptr.append(indptr[-1] + len(j))
    return np.array(indptr, np.int64), np.concatenate(nbr).astype(np.int32), np.concatenate(eps)


def epoch(prev, indptr, nbr, eps, nxt, epoch, alpha, a, b, seed):
    """One epoch of the gather form in float64; ``nxt`` (float64) is advanced in place.  -> the new positions [n, 2]."""
    prev = np.asarray(prev, np.float64)
    n = len(prev)
    cur = prev.copy()
    lens = np.diff(indptr)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    with np.errstate(divide='ignore', invalid='ignore'):
        for s in range(int(lens.max()) if n else 0):
            rows = np.nonzero(lens > s)[0]
            e = indptr[rows] + s
            due = nxt[e] <= epoch
            rows, e = rows[due], e[due]
            if not len(rows):
                continue
            d = cur[rows] - prev[nbr[e]]
            d2 = (d * d).sum(1)
            g = np.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0), 0.0)
            cur[rows] += np.clip(g[:, None] * d, -4.0, 4.0) * alpha
            nxt[e] += eps[e]
            for p in range(NEG_RATE):
                j = (philox4x32_10(epoch, rows, s, p, k0, k1)[0].astype(np.int64) % n)
                d = cur[rows] - prev[j]
                d2 = (d * d).sum(1)
                g = 2.0 * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                step = np.where((d2 > 0)[:, None], np.clip(g[:, None] * d, -4.0, 4.0), 4.0)
                step[j == rows] = 0.0
                cur[rows] += step * alpha
    return cur


def layout(init, indptr, nbr, eps, n_epochs, a, b, seed):
    cur, nxt = np.asarray(init, np.float64), np.asarray(eps, np.float64).copy()
    for ep in range(1, n_epochs + 1):
        cur = epoch(cur, indptr, nbr, eps, nxt, ep, 1.0 - (ep - 1) / n_epochs, a, b, seed)
    return cur


@functools.lru_cache(maxsize=None)
def case_sqdist(name, seed=0):
    """The float64 distances of a case of tests/_umap_cases.py, computed once per process."""
    from tests import _umap_cases as cases
    return sqdist(cases.get(name, seed))


def check_table(d2, idx, dist, d):
    """What any correct fp32 table satisfies against the float64 distances ``d2`` [n, n], with eps = ``eps_for(d)``: rows without
    repeats, sorted by (distance, index); every returned neighbour's float64 squared distance <= (1 + eps) x the oracle's k-th;
    every returned distance squared within relative eps of the float64 value for its index."""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.float64)
    n, k = idx.shape
    eps = eps_for(d)
    assert idx.min() >= 0 and idx.max() < n
    assert all(len(set(row)) == k for row in idx.tolist()), 'a neighbour twice in a row'
    step, same = np.diff(dist, axis=1), np.diff(dist, axis=1) == 0
    assert (step >= 0).all() and (np.diff(idx, axis=1)[same] > 0).all(), 'a row is not sorted by (distance, index)'
    true = np.take_along_axis(d2, idx, 1)
    kth = np.sort(d2, axis=1)[:, k - 1]
    worst = float((true / np.maximum(kth[:, None], 1e-300)).max()) if kth.min() > 0 else None
    assert (true <= (1.0 + eps) * kth[:, None]).all(), f'a neighbour beyond (1 + eps) x the k-th distance (worst ratio {worst})'
    err = np.abs(dist * dist - true)
    rel = float((err / np.maximum(true, 1e-300))[true > 0].max()) if (true > 0).any() else 0.0
    assert (err <= eps * true).all(), f'a distance off by relative {rel:.3e} > eps = {eps:.3e}'
    return rel


K_SLACK = 16


def gemm_form(x, chunk=64):
    """|q|^2 + |c|^2 - 2 q.c of every pair in fp32 throughout, the products accumulated over the columns in chunks of ``chunk``:
    the pruning pass's form, in numpy's summation order rather than the kernel's.  -> fp32 [n, n]."""
    x = np.asarray(x, np.float32)
    sq = (x * x).sum(1, dtype=np.float32)
    dot = np.zeros((len(x), len(x)), np.float32)
    for e in range(0, x.shape[1], chunk):
        dot += x[:, e:e + chunk] @ x[:, e:e + chunk].T
    return (sq[:, None] + sq[None, :]) - np.float32(2) * dot


def pruned_candidates(x, k, chunk=64):
    """An emulation of the pruning pass as the Neighbours paragraph describes it: candidate c belongs to half (c // 4) % 2; of
    each half a query keeps the k + K_SLACK smallest by (GEMM-form value, index).  -> bool [n, n], True where the row is looked
    at again.  It is not the kernel: the matrix instruction sums in another order."""
    g = gemm_form(x, chunk)
    n = len(g)
    keep = np.zeros((n, n), bool)
    for h in (0, 1):
        cols = np.nonzero((np.arange(n) // 4) % 2 == h)[0]
        for q in range(n):
            keep[q, cols[np.lexsort((cols, g[q, cols]))[:k + K_SLACK]]] = True
    return keep


def lost_rows(d2, keep, k, d):
    """Rows of which a true neighbour is not kept, and what the best table over the kept rows then holds lies beyond
    (1 + eps_for(d)) x the k-th float64 squared distance.  -> (bool [n], the worst ratio to the k-th)."""
    kth = np.sort(d2, axis=1)[:, k - 1]
    got = np.sort(np.where(keep, d2, np.inf), axis=1)[:, k - 1]
    lost = got > (1.0 + eps_for(d)) * kth
    ratio = got / np.maximum(kth, 1e-300)
    return lost, float(ratio[lost].max()) if lost.any() else 1.0


def decided(d2, k, d):
    """Rows whose k-th and (k + 1)-th float64 squared distances lie further apart than eps x the distance: there the neighbour SET
    is the same for every correct fp32 table (all rows when k = n)."""
    n = len(d2)
    if k >= n:
        return np.ones(n, bool)
    s = np.sort(d2, axis=1)
    return s[:, k] - s[:, k - 1] > eps_for(d) * s[:, k]
