"""Numpy restatement of exit-flow fine-tuning with training-mode batch norm (DESIGN.md section 7 "Exit-flow fine-tuning", Two
modes), the reference ``bq_exit_grad_bn``, ``bq_exit_bn_move`` and ``bq_exit_train_steps_bn`` are tested against: block 14 in front
of the head of tests/_train_ref.py with each layer normalised by its batch's own statistics, forward, every gradient and the moving
update, in float64 -- and the same formulas with every array ``numpy.float32`` (the twin; its variance takes two passes too).
Generic in ``(H, W, C0, C1, C2)``; the depthwise convolution, the head and the loss are tests/_exit_train_ref.py's.

For one layer, z [M, C] with M = n H W, every position of every tile of the batch:

    mu = (1/M) sum z              var = (1/M) sum (z - mu)^2          (biased; two passes)
    a = gamma / sqrt(var + eps)   b = beta - a mu                     h = relu(a z + b)
    g = dh [h > 0]                xhat = (z - mu) / sqrt(var + eps)   dbeta = sum g       dgamma = sum g xhat
    dz = a (g - dbeta / M - xhat dgamma / M)
    moving_mean <- (1 - f) moving_mean + f mu      moving_var <- (1 - f) moving_var + f var M / (M - 1)       f = 0.01
"""
import numpy as np

from tests import _exit_train_ref as X
from tests import _train_ref as T

BN_EPS = X.BN_EPS
MOMENTUM_F = 0.01
BATCH_STATS = ('mu1', 'var1', 'mu2', 'var2')            # in the order of d_batch_stats


def batch_stats(z, dtype=np.float64):
    """z [..., C] -> ``(mu, var)`` over all leading axes: the mean, then the mean of the squared distances from it (biased)."""
    zf = z.reshape(-1, z.shape[-1])
    M = dtype(zf.shape[0])
    mu = zf.sum(axis=0, dtype=dtype) / M
    d = zf - mu
    return mu, (d * d).sum(axis=0, dtype=dtype) / M


def forward(x, e, dtype=np.float64, shift=None):
    """x [n, H, W, C0], e: the eight trainable tensors (moving statistics in ``e`` are not read) -> ``(f [n, C2], kept)`` in ``dtype``
    arithmetic.  ``shift``: {layer: [C]} added to that layer's z before its statistics are taken (for the shift-invariance check)."""
    t = {k: np.array(e[k], dtype) for k in X.EXIT}
    h, kept = np.asarray(x, dtype), {'t': t}
    zero = dtype(0)
    with np.errstate(invalid='ignore', over='ignore'):
        for l in ('1', '2'):
            u = X.dw(h, t['D' + l])
            z = u @ t['P' + l]
            if shift is not None and l in shift:
                z = z + np.asarray(shift[l], dtype)
            mu, var = batch_stats(z, dtype)
            sd = np.sqrt(var + dtype(BN_EPS))
            a = t['gamma' + l] / sd
            b = t['beta' + l] - a * mu
            y = a * z + b
            kept.update({'in' + l: h, 'u' + l: u, 'z' + l: z, 'a' + l: a, 'sd' + l: sd, 'mu' + l: mu, 'var' + l: var, 'y' + l: y})
            h = np.where(y < 0, zero, y)
            kept['h' + l] = h
        n, H, W, C = h.shape
        f = h.reshape(n, H * W, C).sum(axis=1, dtype=dtype) / dtype(H * W)
    return f, kept


def backward(kept, df, dtype=np.float64, terms=(True, True)):
    """df [n, C2] -> {tensor: grad} of the eight trainable tensors; kept['dz1'], kept['dz2']: the gradients at z.  ``terms``: whether
    ``- dbeta / M`` and ``- xhat dgamma / M`` are there (both, unless a test shows what a missing one costs)."""
    t, g = kept['t'], {}
    n, H, W, C = kept['h2'].shape
    M = dtype(n * H * W)
    dh = np.broadcast_to((np.asarray(df, dtype) / dtype(H * W))[:, None, None, :], (n, H, W, C))
    zero = dtype(0)
    with np.errstate(invalid='ignore', over='ignore'):
        for l in ('2', '1'):
            gr = np.where(kept['h' + l] > 0, dh, zero)
            xhat = (kept['z' + l] - kept['mu' + l]) / kept['sd' + l]
            g['beta' + l] = gr.sum(axis=(0, 1, 2), dtype=dtype)
            g['gamma' + l] = (gr * xhat).sum(axis=(0, 1, 2), dtype=dtype)
            inner = gr
            if terms[0]:
                inner = inner - g['beta' + l] / M
            if terms[1]:
                inner = inner - xhat * (g['gamma' + l] / M)
            dz = kept['a' + l] * inner
            kept['dz' + l], kept['xhat' + l] = dz, xhat
            u = kept['u' + l]
            g['P' + l] = u.reshape(-1, u.shape[-1]).T @ dz.reshape(-1, dz.shape[-1])
            du = dz @ t['P' + l].T
            g['D' + l] = X.dw_weight_grad(kept['in' + l], du)
            if l == '2':
                dh = X.dw_input_grad(du, t['D' + l])
    return g


def loss_and_grad(x, labels, e, w, keeps, rate, dtype=np.float64, terms=(True, True)):
    """``_exit_train_ref.loss_and_grad`` in training mode -> ``(loss, {tensor: grad}, f, stats, kept)``; stats: {'mu1', 'var1', 'mu2',
    'var2'}, the biased batch statistics."""
    f, kept = forward(x, e, dtype)
    loss, g, df = X.head_loss_grad(f, labels, w, keeps, rate, dtype)
    g = dict(g)
    g.update(backward(kept, df, dtype, terms))
    return loss, g, f, {k: kept[k] for k in BATCH_STATS}, kept


def flatten_stats(stats):
    """{'mu1', 'var1', 'mu2', 'var2'} -> one vector in the order of d_batch_stats."""
    return np.concatenate([np.asarray(stats[k]).reshape(-1) for k in BATCH_STATS])


def moving_update(moving, batch, M, c1, dtype=np.float64):
    """The moving statistics [2 c1 + 2 c2] (mean1 | var1 | mean2 | var2) after a step over M rows whose batch statistics were
    ``batch`` (the same layout, biased): the means follow mu, the variances the unbiased var M / (M - 1)."""
    moving, batch = np.asarray(moving, dtype), np.asarray(batch, dtype)
    c2 = (len(moving) - 2 * c1) // 2
    is_var = np.concatenate([np.zeros(c1, bool), np.ones(c1, bool), np.zeros(c2, bool), np.ones(c2, bool)])
    f = dtype(MOMENTUM_F)
    target = np.where(is_var, batch * dtype(M) / dtype(M - 1), batch)
    return (dtype(1) - f) * moving + f * target


# ---- the cases of the GPU test (tests/test_gpu_exit_bn.py) ------------------------------------------------------------------------
_MEMO = {}
CACHE_ROWS = 12                                         # _exit_train_ref.cache()'s six tiles and six more of the same stream
CANDIDATES = 64


def inputs():
    """``(cache [12, 10, 10, 1024], _exit_train_ref's exit tensors, _train_ref's head)``, made once."""
    if 'inputs' not in _MEMO:
        _, e, w = X.inputs()
        _MEMO['inputs'] = (X.cache(CACHE_ROWS), e, w)
        assert np.array_equal(_MEMO['inputs'][0][:X.CACHE_ROWS], X.inputs()[0])
    return _MEMO['inputs']


def _candidate(n, labels_kind, k):
    """Candidate ``k`` of a case: ``_exit_train_ref._candidate``'s sixteen first, then draws of the same shape over the twelve tiles,
    'one' taking either class in turn.  (A batch of one tile has five candidates there, and in batch mode -- features normalised,
    logits near zero, a loss near ln 2 that hardly feels them -- the float32 loss of all five is the correctly rounded one: no
    float32 neighbour of it is within 8 x its figure.)"""
    if k < X.CANDIDATES:
        return X._candidate(n, labels_kind, k)
    rng = np.random.default_rng([17, n, k])
    rows = rng.permutation(np.array([0] + list(range(2, CACHE_ROWS))))[:n].astype(np.int64)
    if n >= 3:
        rows[1] = 1                                     # the all-zero tile
        rows[2] = rows[0]                               # and one tile twice
    labels = rng.integers(0, 2, n).astype(np.uint8) if labels_kind == 'mixed' else np.full(n, k % 2, np.uint8)
    if labels_kind == 'mixed' and n >= 2:
        labels[0], labels[1] = 0, 1
    return rows, labels


def _betas_off_the_kink(x_rows, e):
    """``e`` with both betas moved so that no unit of THIS batch sits at ReLU's kink: in batch mode the pre-activations depend on the
    batch's statistics, so the betas are placed per case (layer 1 first: layer 2's statistics depend on it).  float64 only."""
    e = dict(e)
    for l in ('1', '2'):
        _, kept = forward(x_rows, e)
        y = kept['y' + l]
        e['beta' + l] = (e['beta' + l].astype(np.float64) + X._off_the_kink(y.reshape(-1, y.shape[-1]))).astype(np.float32)
    _, kept = forward(x_rows, e)
    for l in ('1', '2'):
        assert np.abs(kept['y' + l]).min() > 1e-5, (l, np.abs(kept['y' + l]).min())
    return e


def grad_reference(n, rate, labels_kind, step=3):
    """``(rows, labels, e, loss64, grad64, stats64, twin)``, once per case: ``_exit_train_ref.grad_reference``'s rules -- the first of the
    candidates ``_candidate(n, kind, k)`` whose float32 twin is off float64 by 2^-24 or more in EVERY figure, so that 8 x
    the twin's figure is never 8 x a lucky zero -- with the betas placed for the candidate's own batch.  e: the case's exit tensors.
    twin: {tensor, 'loss', 'mu1' .. 'var2': rel_err of float32 against float64}.  Reads the two numpy computations only."""
    key = (n, rate, labels_kind, step)
    if key not in _MEMO:
        x, e0, w = inputs()
        tried = set()
        for k in range(CANDIDATES):
            rows, labels = _candidate(n, labels_kind, k)
            if (tuple(rows), tuple(labels)) in tried:
                continue
            tried.add((tuple(rows), tuple(labels)))
            e = _betas_off_the_kink(x[rows], e0)
            keeps = X.keep_masks(X.SEED, rows, step, rate)
            l64, g64, _, s64, _ = loss_and_grad(x[rows], labels, e, w, keeps, rate, np.float64)
            l32, g32, _, s32, _ = loss_and_grad(x[rows], labels, e, w, keeps, rate, np.float32)
            twin = {t: T.rel_err(g32[t], g64[t]) for t in g64}
            twin['loss'] = T.rel_err(l32, l64)
            twin.update({s: T.rel_err(s32[s], s64[s]) for s in BATCH_STATS})
            if min(twin.values()) >= X.UNIT:
                break
        else:
            raise AssertionError(f'no candidate of case {key} has a twin off float64 by 2^-24 in every figure')
        _MEMO[key] = (rows, labels, e, l64, g64, s64, twin)
    return _MEMO[key]


# the two-pass case: a channel of z1 with mean 1 and a standard deviation of a few 1e-4
TWO_PASS_N, TWO_PASS_CHANNEL, TWO_PASS_NOISE = 3, 5, 1e-2


def two_pass_case(noise=TWO_PASS_NOISE):
    """``(x float32 [3, 10, 10, 1024], e)``: x = 1 + noise * standard normal, rounded to multiples of 2^-12 (so that the channel's z --
    1024 such values times 2^-10 -- is the same number in float32, in float64 and in whatever order a device adds it: what differs
    between them is the statistics alone); D1 the centre tap alone; column ``TWO_PASS_CHANNEL`` of P1 1/1024 throughout."""
    x0, e0, _ = inputs()
    rng = np.random.default_rng(31)
    x = 1.0 + noise * rng.standard_normal((TWO_PASS_N,) + x0.shape[1:])
    x = (np.round(x * 4096.0) / 4096.0).astype(np.float32)
    e = {k: np.array(v, np.float32) for k, v in e0.items()}
    e['D1'][:] = 0
    e['D1'][1, 1] = 1
    e['P1'][:, TWO_PASS_CHANNEL] = np.float32(1.0 / 1024.0)
    return x, e


def one_pass_var32(z):
    """What the two-pass rule forbids: E[z^2] - mu^2 in float32, over the rows of z [M, C]."""
    z = np.asarray(z, np.float32)
    M = np.float32(z.shape[0])
    mu = z.sum(axis=0, dtype=np.float32) / M
    return (z * z).sum(axis=0, dtype=np.float32) / M - mu * mu
