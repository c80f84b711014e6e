"""Numpy restatement of head training (DESIGN.md section 7 "Head training"), the reference the kernels behind ``bq_head_grad``,
``bq_head_adam`` and ``bq_head_train_steps`` are tested against: forward, mean sparse categorical cross-entropy, gradients, Keras Adam
and the learning-rate schedule, in float64 -- and the same formulas with every array ``numpy.float32`` (``dtype=np.float32``: the twin
whose distance from float64 the device tolerance is derived from).

The keep masks are ``oracle.philox.dropout_keep`` with pass = step and tile = the row's index in the feature cache, the scale
``oracle.philox.dropout_scale`` (the float32 value of the contract, used as it is), like tests/_head_ref.py.  ReLU's derivative is 0
at 0; ReLU keeps NaN.
"""
import numpy as np

from oracle import philox

HEAD = ('hidden_0', 'hidden_1', 'logits')
N_IN = (2048, 1024, 1024)
TENSORS = tuple(f'{name}/{t}' for name in HEAD for t in ('kernel', 'bias'))
B1, B2, EPS = 0.9, 0.999, 1e-7


def tensors(w, dtype=np.float64):
    return {k: np.array(w[k], dtype) for k in TENSORS}


def keep_masks(seed, rows, step, rate):
    """The three keep masks [n, n_in] of the batch ``rows`` at global step ``step``."""
    rows = np.asarray(rows, np.int64)
    return [philox.dropout_keep(seed, rows, int(step), layer, n_in, rate) for layer, n_in in enumerate(N_IN)]


def forward(feat, w, keeps, rate, dtype=np.float64):
    """The forward pass in ``dtype`` arithmetic, the one ``loss_and_grad`` and tests/_validate_ref.py share: feat [n, 2048] ->
    ``(tensors(w, dtype), u, h, scale, zero)``, u the three layers' dropped inputs and h = [x, h0, h1, logits]."""
    t, scale, zero = tensors(w, dtype), dtype(philox.dropout_scale(rate)), dtype(0)
    u, h = [], [np.asarray(feat, dtype)]
    with np.errstate(invalid='ignore', over='ignore'):
        for layer, name in enumerate(HEAD):
            u.append(np.where(keeps[layer], h[-1] * scale, zero))
            z = u[-1] @ t[name + '/kernel'] + t[name + '/bias']
            h.append(np.where(z < 0, zero, z) if layer < 2 else z)
    return t, u, h, scale, zero


def loss_and_grad(feat, labels, w, keeps, rate, dtype=np.float64, want_grad=True):
    """feat [n, 2048] (the gathered rows), labels int [n], w: the six tensors, keeps: ``keep_masks``.  -> ``(loss, {tensor: grad})``
    in ``dtype`` arithmetic."""
    t, u, h, scale, zero = forward(feat, w, keeps, rate, dtype)
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    with np.errstate(invalid='ignore', over='ignore'):
        z = h[-1]
        zs = z - z.max(axis=1, keepdims=True)
        lse = np.log(np.exp(zs).sum(axis=1, keepdims=True))
        logp = zs - lse
        loss = -(logp[np.arange(n), labels]).mean(dtype=dtype)
        if not want_grad:
            return loss, None
        d = np.exp(logp)
        d[np.arange(n), labels] -= dtype(1)
        d = d / dtype(n)
        g = {}
        for layer in (2, 1, 0):
            name = HEAD[layer]
            g[name + '/kernel'] = u[layer].T @ d
            g[name + '/bias'] = d.sum(axis=0, dtype=dtype)
            if layer:
                du = d @ t[name + '/kernel'].T
                d = np.where(keeps[layer] & (h[layer] > 0), du * scale, zero)
    return loss, g


def learning_rate(step, lr=1e-4, decay=0.98, decay_steps=512):
    """Staircase exponential decay: lr * decay ** (step // decay_steps)."""
    return lr * decay ** (step // decay_steps)


def adam(w, m, v, g, step, lr, dtype=np.float64, b1=B1, b2=B2, eps=EPS):
    """One Keras-Adam update of arrays (any shape) -> ``(w', m', v')`` in ``dtype``; t = step + 1."""
    w, m, v, g = (np.asarray(a, dtype) for a in (w, m, v, g))
    t = step + 1
    m2 = dtype(b1) * m + dtype(1 - b1) * g
    v2 = dtype(b2) * v + dtype(1 - b2) * (g * g)
    alpha = dtype(lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t))
    return w - alpha * (m2 / (np.sqrt(v2) + dtype(eps))), m2, v2


def train_steps(feats, rows, labels, w, batch, seed, rate, lr, step0=0, dtype=np.float64):
    """ceil(len(rows) / batch) steps over ``rows`` in order (the last batch short), from zero moments.  ``lr``: one per step.
    -> ``(tensors, losses)`` in ``dtype``."""
    t = tensors(w, dtype)
    m = {k: np.zeros_like(a) for k, a in t.items()}
    v = {k: np.zeros_like(a) for k, a in t.items()}
    rows, labels = np.asarray(rows, np.int64), np.asarray(labels, np.int64)
    losses = []
    for i, a in enumerate(range(0, len(rows), batch)):
        r, y = rows[a:a + batch], labels[a:a + batch]
        loss, g = loss_and_grad(np.asarray(feats)[r], y, t, keep_masks(seed, r, step0 + i, rate), rate, dtype)
        losses.append(loss)
        for k in TENSORS:
            t[k], m[k], v[k] = adam(t[k], m[k], v[k], g[k], step0 + i, lr[i], dtype)
    return t, np.array(losses, dtype)


def rel_err(a, ref):
    """max|a - ref| / max|ref| (0 / 0 = 0)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    top = float(np.abs(a - ref).max()) if a.size else 0.0
    den = float(np.abs(ref).max()) if ref.size else 0.0
    return top / den if den > 0 else (0.0 if top == 0 else np.inf)


# ---- the cases of the GPU test (tests/test_gpu_train.py) and of the float32 twin's error (tests/test_train.py) ------------------------
CACHE_ROWS = 40
GRAD_N = (1, 3, 32, 33, 128)
GRAD_RATES = (0.0, 0.1, 0.5)
GRAD_LABELS = ('mixed', 'one')
SEED = 77


def cache(rows=CACHE_ROWS, seed=5):
    """Half-normal feature rows (post-ReLU-like), float32 [rows, 2048]; row 7 is all zeros."""
    f = np.abs(np.random.default_rng(seed).standard_normal((rows, 2048))).astype(np.float32)
    f[7] = 0
    return f


def head():
    """``synthetic_weights(1)``'s head with the last 8 units of hidden_0 dead: their kernel columns and biases negative."""
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    t = {k: np.array(w[k], np.float32) for k in TENSORS}
    t['hidden_0/kernel'][:, -8:] = -np.abs(t['hidden_0/kernel'][:, -8:]) - np.float32(1e-3)
    t['hidden_0/bias'][-8:] = np.float32(-0.5)
    return t


def grad_case(n, labels_kind, case_seed=0):
    """(rows int64 [n] into the cache, labels uint8 [n]) of one gradient case: the rows repeat once n exceeds the cache."""
    rng = np.random.default_rng([11, n, case_seed])
    rows = (rng.permutation(CACHE_ROWS)[:n] if n <= CACHE_ROWS else rng.integers(0, CACHE_ROWS, n)).astype(np.int64)
    if n >= 3:
        rows[1] = 7                                     # the all-zero row
    labels = rng.integers(0, 2, n).astype(np.uint8) if labels_kind == 'mixed' else np.ones(n, np.uint8)
    if labels_kind == 'mixed' and n >= 2:
        labels[0], labels[1] = 0, 1
    return rows, labels


_MEMO = {}


def grad_reference(n, rate, labels_kind, step=3):
    """``(rows, labels, loss64, grad64, twin: {tensor or 'loss': rel_err of float32 against float64})``, computed once per case."""
    key = (n, rate, labels_kind, step)
    if key not in _MEMO:
        f, w = cache(), head()
        rows, labels = grad_case(n, labels_kind)
        keeps = keep_masks(SEED, rows, step, rate)
        l64, g64 = loss_and_grad(f[rows], labels, w, keeps, rate, np.float64)
        l32, g32 = loss_and_grad(f[rows], labels, w, keeps, rate, np.float32)
        twin = {k: rel_err(g32[k], g64[k]) for k in TENSORS}
        twin['loss'] = rel_err(l32, l64)
        _MEMO[key] = (rows, labels, l64, g64, twin)
    return _MEMO[key]
