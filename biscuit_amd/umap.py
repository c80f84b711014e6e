"""UMAP's host stages and the CPU builds of its device stages (DESIGN.md "Feature map (Figure 6)").

UMAP is restated here from memory -- ``umap-learn`` is no dependency --, so the parity with it is *unpinned*; what is pinned is
tests/_umap_ref.py, a float64 numpy restatement.  On the device: the nearest neighbours (``Engine.knn``), the fuzzy graph's rows
(``Engine.umap_smooth``) and the layout's epochs (``Engine.umap_epoch``).  On the host, in numpy, once per map and O(n k): the
curve's constants (``fit_ab``), the symmetric graph as a CSR (``fuzzy_graph``) and the initial positions (``pca_init``, the one
stage that is O(n D^2); tools/bench_umap.py times it).  ``*_host`` are libbiscuit_io's CPU builds of the three device entries.
"""
import numpy as np

NEG_RATE = 5


def n_epochs_for(n):
    """500 epochs up to 10 000 points, 200 above."""
    return 500 if int(n) <= 10000 else 200


def fit_ab(min_dist=0.1, spread=1.0):
    """``(a, b)`` of the layout's curve 1 / (1 + a x^(2b)): the least-squares fit to 1 for x < min_dist, exp(-(x - min_dist) /
    spread) beyond, at 300 points on [0, 3 spread], by Levenberg-Marquardt from (1, 1)."""
    x = np.linspace(0.0, 3.0 * float(spread), 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - float(min_dist)) / float(spread)))
    lx = np.log(np.maximum(x, 1e-300))

    def model(p):
        xb = np.where(x > 0, np.exp(2.0 * p[1] * lx), 0.0)
        f = 1.0 / (1.0 + p[0] * xb)
        return f, np.stack([-xb * f * f, -p[0] * xb * 2.0 * lx * f * f * (x > 0)], 1)
    p, lam = np.array([1.0, 1.0]), 1e-3
    f, jac = model(p)
    cost = float(((f - y) ** 2).sum())
    for _ in range(200):
        g, h = jac.T @ (f - y), jac.T @ jac
        step = np.linalg.solve(h + lam * np.diag(np.diag(h)), -g)
        f2, jac2 = model(p + step)
        cost2 = float(((f2 - y) ** 2).sum())
        if cost2 < cost:
            done = np.abs(step).max() < 1e-12
            p, f, jac, cost, lam = p + step, f2, jac2, cost2, lam * 0.3
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


def fuzzy_graph(idx, w, n_epochs):
    """The symmetric graph of the layout from the membership weights of ``Engine.umap_smooth`` (host arrays: ``idx`` int [n, k],
    ``w`` float [n, k]): w_ij + w_ji - w_ij w_ji, edges below max(w) / n_epochs pruned, every vertex's incident edges -- both
    directions stored -- as a CSR with rows sorted by neighbour.  -> ``(indptr int64 [n + 1], nbr int32 [nnz], eps float32
    [nnz])``, eps = max(w) / w the epochs per sample."""
    idx, w = np.asarray(idx, np.int64), np.asarray(w, np.float64)
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    keep = w.ravel() > 0
    i, j, v = rows[keep], idx.ravel()[keep], w.ravel()[keep]
    fwd, back = i * n + j, j * n + i
    order = np.argsort(fwd, kind='stable')
    fwd_sorted, v_sorted = fwd[order], v[order]
    keys = np.union1d(fwd, back)

    def lookup(q):
        at = np.minimum(np.searchsorted(fwd_sorted, q), max(len(fwd_sorted) - 1, 0))
        return np.where(fwd_sorted[at] == q, v_sorted[at], 0.0) if len(fwd_sorted) else np.zeros(len(q))
    a, b = lookup(keys), lookup(keys % n * n + keys // n)
    s = a + b - a * b
    top = s.max() if len(s) else 1.0
    kept = s >= top / float(n_epochs)
    keys, s = keys[kept], s[kept]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(keys // n, minlength=n), out=indptr[1:])
    return indptr, (keys % n).astype(np.int32), (top / s).astype(np.float32)


def pca_init(x):
    """The initial positions: the two leading principal components of ``x`` [n, D] (float64, through the D x D covariance), each
    component's sign fixed by making its largest-magnitude entry positive, scaled so that the largest magnitude is 10.
    -> float32 [n, 2]."""
    x = np.asarray(x, np.float64)
    xc = x - x.mean(0, keepdims=True)
    if x.shape[0] >= x.shape[1]:
        _, vec = np.linalg.eigh(xc.T @ xc)
        y = xc @ vec[:, ::-1][:, :2]
    else:
        val, vec = np.linalg.eigh(xc @ xc.T)
        y = vec[:, ::-1][:, :2] * np.sqrt(np.maximum(val[::-1][:2], 0.0))
    if y.shape[1] < 2:
        y = np.concatenate([y, np.zeros((len(y), 2 - y.shape[1]))], 1)
    for c in range(2):
        if y[np.abs(y[:, c]).argmax(), c] < 0:
            y[:, c] = -y[:, c]
    top = np.abs(y).max()
    return (y * (10.0 / top if top > 0 else 1.0)).astype(np.float32)


def check_graph(n, indptr, nbr, eps):
    """ValueError unless ``(indptr, nbr, eps)`` is a CSR over ``n`` vertices as ``Engine.umap_epoch`` reads it."""
    indptr, nbr, eps = np.asarray(indptr), np.asarray(nbr), np.asarray(eps)
    if indptr.shape != (n + 1,) or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != len(nbr) or len(eps) != len(nbr):
        raise ValueError('indptr must run from 0 to nnz in n non-decreasing steps')
    if len(nbr) and (nbr.min() < 0 or nbr.max() >= n):
        raise ValueError('a neighbour outside 0 .. n - 1')
    if not (np.isfinite(eps).all() and (eps > 0).all()):
        raise ValueError('epochs per sample must be finite and positive')


def graph_to_device(engine, n, indptr, nbr, eps):
    """The checked CSR on the engine's device with its sample clocks at their start (next = eps): ``Engine.umap_epoch``'s ``graph``."""
    import torch
    check_graph(n, indptr, nbr, eps)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(engine.device)
    return up(indptr, np.int64), up(nbr, np.int32), up(eps, np.float32), up(eps, np.float32).clone()


def layout(engine, graph, init, n_epochs, a, b, seed=0, block=0):
    """``n_epochs`` launches of ``Engine.umap_epoch`` from ``init`` float32 [n, 2] (host), alpha = 1 - (epoch - 1) / n_epochs,
    two position buffers in turn.  -> float32 [n, 2] on the host."""
    import torch
    cur = torch.from_numpy(np.ascontiguousarray(init, np.float32)).to(engine.device)
    other = torch.empty_like(cur)
    for epoch in range(1, int(n_epochs) + 1):
        engine.umap_epoch(cur, graph, epoch, 1.0 - (epoch - 1) / float(n_epochs), a, b, seed, out=other, block=block)
        cur, other = other, cur
    return cur.cpu().numpy()


def embed(engine, features, n_neighbors=50, min_dist=0.1, seed=0, n_epochs=None):
    """``features`` fp32 [N, D] (host or device) -> the map float32 [N, 2] on the host: neighbours and membership weights on the
    device, graph and PCA start on the host, then the epochs on the device.  ``n_neighbors`` is clipped to N."""
    import torch
    x = features if torch.is_tensor(features) else torch.tensor(np.asarray(features, np.float32))
    x = x.to(engine.device).contiguous()
    n = int(x.shape[0])
    k = min(int(n_neighbors), n)
    n_epochs = n_epochs_for(n) if n_epochs is None else int(n_epochs)
    idx, dist = engine.knn(x, k)
    _, _, w = engine.umap_smooth(idx, dist)
    indptr, nbr, eps = fuzzy_graph(idx.cpu().numpy(), w.cpu().numpy(), n_epochs)
    a, b = fit_ab(min_dist)
    return layout(engine, graph_to_device(engine, n, indptr, nbr, eps), pca_init(x.cpu().numpy()), n_epochs, a, b, seed)


# ---- the CPU builds (libbiscuit_io: csrc/umap_host.cpp over csrc/umap_device.h), for tests -------------------------------------------
def knn_host(x, k):
    """``Engine.knn``'s table on the host (bqio_knn: all n rows by the direct form).  ValueError for what the device refuses, an
    ``x`` that is not finite included."""
    from . import tfrecord_native
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    if not np.isfinite(x).all():
        raise ValueError('knn_host takes finite values only: x holds a NaN or an infinity')
    idx, dist = np.empty((n, max(int(k), 0)), np.int32), np.empty((n, max(int(k), 0)), np.float32)
    e = tfrecord_native.lib().bqio_knn(x.ctypes.data, n, d, int(k), idx.ctypes.data, dist.ctypes.data)
    if e != 0:
        raise ValueError(f'bqio_knn(n = {n}, D = {d}, k = {k}): error {e}')
    return idx, dist


def gemm_bound(nq, nc, d):
    """E(nq, nc, D) of csrc/umap_device.h, elementwise over fp32 arrays that broadcast: the worst-case error of the pruning
    pass's GEMM form (bqio_knn_gemm_bound)."""
    from . import tfrecord_native
    nq, nc = np.broadcast_arrays(np.asarray(nq, np.float32), np.asarray(nc, np.float32))
    nq, nc = np.ascontiguousarray(nq), np.ascontiguousarray(nc)
    out = np.empty(nq.shape, np.float32)
    e = tfrecord_native.lib().bqio_knn_gemm_bound(nq.ctypes.data, nc.ctypes.data, nq.size, int(d), out.ctypes.data)
    if e != 0:
        raise ValueError(f'bqio_knn_gemm_bound(D = {d}): error {e}')
    return out


def smooth_host(idx, dist):
    from . import tfrecord_native
    idx, dist = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(dist, np.float32)
    n, k = idx.shape
    rho, sigma, w = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, k), np.float32)
    e = tfrecord_native.lib().bqio_umap_smooth(idx.ctypes.data, dist.ctypes.data, n, k, rho.ctypes.data, sigma.ctypes.data, w.ctypes.data)
    if e != 0:
        raise ValueError(f'bqio_umap_smooth(n = {n}, k = {k}): error {e}')
    return rho, sigma, w


def epoch_host(prev, indptr, nbr, eps, nxt, epoch, alpha, a, b, seed):
    """One epoch on the host; ``nxt`` (float32, contiguous) is advanced in place.  -> float32 [n, 2]."""
    from . import tfrecord_native
    prev = np.ascontiguousarray(prev, np.float32)
    indptr, nbr, eps = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(nbr, np.int32), np.ascontiguousarray(eps, np.float32)
    assert nxt.dtype == np.float32 and nxt.flags.c_contiguous and len(nxt) == len(nbr) == len(eps) and len(indptr) == len(prev) + 1
    out = np.empty_like(prev)
    e = tfrecord_native.lib().bqio_umap_epoch(prev.ctypes.data, out.ctypes.data, len(prev), indptr.ctypes.data, nbr.ctypes.data, eps.ctypes.data,
                                              nxt.ctypes.data, int(epoch), float(alpha), float(a), float(b), int(seed) & (2 ** 64 - 1))
    if e != 0:
        raise ValueError(f'bqio_umap_epoch: error {e}')
    return out
