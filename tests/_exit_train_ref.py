"""Numpy restatement of exit-flow fine-tuning (DESIGN.md section 7 "Exit-flow fine-tuning"), the reference the kernels behind
``bq_exit_features``, ``bq_exit_grad`` and ``bq_exit_train_steps`` are tested against: block 14 with frozen batch-norm statistics in
front of the head of tests/_train_ref.py, forward and every gradient, in float64 -- and the same formulas with every array
``numpy.float32`` (the twin whose distance from float64 the device tolerance is derived from).  Generic in ``(H, W, C0, C1, C2)``
and in the head's sizes: the shapes are the arrays' own.

    u1 = dw(x, D1)   z1 = u1 P1   h1 = relu(a1 z1 + b1)      a = gamma / sqrt(var + eps), b = beta - a mean
    u2 = dw(h1, D2)  z2 = u2 P2   h2 = relu(a2 z2 + b2)      f = mean over the positions of h2 -> the head

dw: 3 x 3 depthwise, zero padding 1, stride 1, no bias.  ReLU's derivative is 0 at 0.
"""
import numpy as np

from oracle import philox
from tests import _train_ref as T

BN_EPS = 1e-3
LAYERS = ('block14_sepconv1', 'block14_sepconv2')
# the exit vector's tensors in its order, under short names: D [3, 3, C], P [Cin, Cout], gamma, beta [Cout]
EXIT = ('D1', 'P1', 'gamma1', 'beta1', 'D2', 'P2', 'gamma2', 'beta2')
STATS = ('mean1', 'var1', 'mean2', 'var2')
KERAS = {'D1': LAYERS[0] + '/depthwise_kernel', 'P1': LAYERS[0] + '/pointwise_kernel', 'gamma1': LAYERS[0] + '_bn/gamma',
         'beta1': LAYERS[0] + '_bn/beta', 'mean1': LAYERS[0] + '_bn/moving_mean', 'var1': LAYERS[0] + '_bn/moving_variance',
         'D2': LAYERS[1] + '/depthwise_kernel', 'P2': LAYERS[1] + '/pointwise_kernel', 'gamma2': LAYERS[1] + '_bn/gamma',
         'beta2': LAYERS[1] + '_bn/beta', 'mean2': LAYERS[1] + '_bn/moving_mean', 'var2': LAYERS[1] + '_bn/moving_variance'}


def from_keras(w):
    """The twelve block-14 tensors of a weight dict under the short names, D as [3, 3, C] and P as [Cin, Cout]."""
    out = {}
    for k, name in KERAS.items():
        a = np.asarray(w[name])
        out[k] = a.reshape(3, 3, -1) if k[0] == 'D' else a.reshape(a.shape[-2], a.shape[-1]) if k[0] == 'P' else a
    return out


def _pad(x):
    n, H, W, C = x.shape
    xp = np.zeros((n, H + 2, W + 2, C), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return xp


def dw(x, D):
    """out[y][x] = sum over (ky, kx) of in[y + ky - 1][x + kx - 1] D[ky][kx], zeros outside; x [n, H, W, C], D [3, 3, C]."""
    n, H, W, C = x.shape
    xp, out = _pad(x), np.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] * D[ky, kx]
    return out


def dw_input_grad(du, D):
    """The transpose of ``dw`` in x: dx[y][x] = sum over (ky, kx) of du[y - ky + 1][x - kx + 1] D[ky][kx]."""
    n, H, W, C = du.shape
    dp, out = _pad(du), np.zeros_like(du)
    for ky in range(3):
        for kx in range(3):
            out += dp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] * D[ky, kx]
    return out


def dw_weight_grad(x, du):
    """The transpose of ``dw`` in D: dD[ky][kx] = sum over tiles and positions of in[y + ky - 1][x + kx - 1] du[y][x]."""
    n, H, W, C = x.shape
    xp, out = _pad(x), np.zeros((3, 3, C), x.dtype)
    for ky in range(3):
        for kx in range(3):
            out[ky, kx] = (xp[:, ky:ky + H, kx:kx + W] * du).sum(axis=(0, 1, 2), dtype=x.dtype)
    return out


def forward(x, e, dtype=np.float64):
    """x [n, H, W, C0], e: the twelve tensors -> ``(f [n, C2], kept)`` in ``dtype`` arithmetic; kept: what the backward pass reads."""
    t = {k: np.array(e[k], dtype) for k in EXIT + STATS}
    h, kept = np.asarray(x, dtype), {'t': t}
    zero = dtype(0)
    with np.errstate(invalid='ignore', over='ignore'):
        for l in ('1', '2'):
            sd = np.sqrt(t['var' + l] + dtype(BN_EPS))
            a = t['gamma' + l] / sd
            b = t['beta' + l] - a * t['mean' + l]
            u = dw(h, t['D' + l])
            z = u @ t['P' + l]
            y = a * z + b
            kept.update({'in' + l: h, 'u' + l: u, 'z' + l: z, 'a' + l: a, 'sd' + l: sd})
            h = np.where(y < 0, zero, y)
            kept['h' + l] = h
        n, H, W, C = h.shape
        f = h.reshape(n, H * W, C).sum(axis=1, dtype=dtype) / dtype(H * W)
    return f, kept


def backward(kept, df, dtype=np.float64):
    """df [n, C2] -> {tensor: grad} of the eight trainable tensors."""
    t, g = kept['t'], {}
    n, H, W, C = kept['h2'].shape
    dh = np.broadcast_to((np.asarray(df, dtype) / dtype(H * W))[:, None, None, :], (n, H, W, C))
    zero = dtype(0)
    with np.errstate(invalid='ignore', over='ignore'):
        for l in ('2', '1'):
            gr = np.where(kept['h' + l] > 0, dh, zero)
            g['beta' + l] = gr.sum(axis=(0, 1, 2), dtype=dtype)
            g['gamma' + l] = (gr * ((kept['z' + l] - t['mean' + l]) / kept['sd' + l])).sum(axis=(0, 1, 2), dtype=dtype)
            dz = gr * kept['a' + l]
            u = kept['u' + l]
            g['P' + l] = u.reshape(-1, u.shape[-1]).T @ dz.reshape(-1, dz.shape[-1])
            du = dz @ t['P' + l].T
            g['D' + l] = dw_weight_grad(kept['in' + l], du)
            if l == '2':
                dh = dw_input_grad(du, t['D' + l])
    return g


def head_loss_grad(feat, labels, w, keeps, rate, dtype=np.float64):
    """``_train_ref.loss_and_grad`` and, beside it, the gradient with respect to ``feat``: -> ``(loss, {tensor: grad}, dfeat)``.
    The backward chain is ``_train_ref``'s own, walked once more down to the input's dropout."""
    loss, g = T.loss_and_grad(feat, labels, w, keeps, rate, dtype)
    t, u, h, scale, zero = T.forward(feat, w, keeps, rate, dtype)
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    with np.errstate(invalid='ignore', over='ignore'):
        z = h[-1]
        zs = z - z.max(axis=1, keepdims=True)
        logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
        d = np.exp(logp)
        d[np.arange(n), labels] -= dtype(1)
        d = d / dtype(n)
        for layer in (2, 1, 0):
            du = d @ t[T.HEAD[layer] + '/kernel'].T
            d = np.where(keeps[layer] & (h[layer] > 0), du * scale, zero) if layer else np.where(keeps[0], du * scale, zero)
    return loss, g, d


def keep_masks(seed, rows, step, rate, n_in=T.N_IN):
    rows = np.asarray(rows, np.int64)
    return [philox.dropout_keep(seed, rows, int(step), layer, k, rate) for layer, k in enumerate(n_in)]


def loss_and_grad(x, labels, e, w, keeps, rate, dtype=np.float64):
    """x [n, H, W, C0] (the gathered rows), e: block 14's twelve tensors, w: the head's six -> ``(loss, {tensor: grad}, f)``: the
    gradients of the eight exit tensors under their short names and of the head's six under ``_train_ref.TENSORS``."""
    f, kept = forward(x, e, dtype)
    loss, g, df = head_loss_grad(f, labels, w, keeps, rate, dtype)
    g = dict(g)
    g.update(backward(kept, df, dtype))
    return loss, g, f


def train_steps(acts, rows, labels, e, w, batch, seed, rate, lr, step0=0, dtype=np.float64):
    """ceil(len(rows) / batch) steps of one Adam over all fourteen tensors, as ``_train_ref.train_steps`` -> ``(e, w, losses)``."""
    e = {k: np.array(e[k], dtype) for k in EXIT + STATS}
    w = T.tensors(w, dtype)
    names = [(e, k) for k in EXIT] + [(w, k) for k in T.TENSORS]
    m = {k: np.zeros_like(d[k]) for d, k in names}
    v = {k: np.zeros_like(d[k]) for d, k in names}
    rows, labels = np.asarray(rows, np.int64), np.asarray(labels, np.int64)
    losses = []
    for i, a in enumerate(range(0, len(rows), batch)):
        r, y = rows[a:a + batch], labels[a:a + batch]
        loss, g, _ = loss_and_grad(np.asarray(acts)[r], y, e, w, keep_masks(seed, r, step0 + i, rate), rate, dtype)
        losses.append(loss)
        for d, k in names:
            d[k], m[k], v[k] = T.adam(d[k], m[k], v[k], g[k], step0 + i, lr[i], dtype)
    return e, w, np.array(losses, dtype)


def flatten(e, w=None):
    """The exit vector float32 [P_EXIT] (and the head's behind it with ``w``), and the statistics float32 [2 C1 + 2 C2]."""
    parts = [np.asarray(e[k], np.float32).reshape(-1) for k in EXIT]
    if w is not None:
        parts += [np.asarray(w[k], np.float32).reshape(-1) for k in T.TENSORS]
    return np.concatenate(parts), np.concatenate([np.asarray(e[k], np.float32).reshape(-1) for k in STATS])


def split_grad(vec, e, w):
    """A flat gradient [P_ALL] -> {tensor: array} in the shapes of ``e`` and ``w``."""
    out, at = {}, 0
    for d, names in ((e, EXIT), (w, T.TENSORS)):
        for k in names:
            n = int(np.asarray(d[k]).size)
            out[k] = np.asarray(vec[at:at + n]).reshape(np.asarray(d[k]).shape)
            at += n
    assert at == len(vec)
    return out


# ---- the cases of the GPU test (tests/test_gpu_exit_train.py) ---------------------------------------------------------------------
CACHE_ROWS = 6
GRAD_N = (1, 2, 3, 5)
GRAD_RATES = (0.0, 0.1)
GRAD_LABELS = ('mixed', 'one')
SEED = 77


def cache(rows=CACHE_ROWS, seed=5):
    """Half-normal activations (post-ReLU-like), float32 [rows, 10, 10, 1024]; tile 1 is all zeros."""
    x = np.abs(np.random.default_rng(seed).standard_normal((rows, 10, 10, 1024))).astype(np.float32)
    x[1] = 0
    return x


def _off_the_kink(y, span=8):
    """y [positions, C]: a channel's pre-activations -> shift [C] that puts zero in the middle of the widest of the gaps between
    the ``span`` sorted values either side of it (0 for a channel of one sign)."""
    ys = np.sort(y, axis=0)
    R, C = ys.shape
    k = (ys < 0).sum(axis=0)
    shift = np.zeros(C)
    for c in np.flatnonzero((k > 0) & (k < R)):
        seg = ys[max(k[c] - span, 0):min(k[c] + span, R), c]
        j = int(np.argmax(np.diff(seg)))
        shift[c] = -(seg[j] + seg[j + 1]) / 2
    return shift


def exit_tensors(seed=1):
    """``synthetic_weights(seed, hard=True)``'s block 14 -- the parity stress set: variances spread over [0.25, 4], means off zero --
    with the last 8 channels of layer 1 dead (beta far below zero).

    Both betas are then moved, channel by channel and by less than the distance between neighbouring pre-activations, so that over
    the whole of ``cache()`` no unit of block 14 sits at ReLU's kink: among the 2 10^6 pre-activations of a case a few would
    otherwise lie within float32 rounding of zero, where float32 and float64 disagree on the DERIVATIVE (0 or 1) by right, and the
    twin's figure would measure that coin, not arithmetic (one such unit moved D1's figure from 5e-7 to 6e-4)."""
    from biscuit_amd.weights import synthetic_weights
    e = {k: np.array(v, np.float32) for k, v in from_keras(synthetic_weights(seed, hard=True)).items()}
    e['beta1'][-8:] = np.float32(-50.0)
    x = cache()
    for l in ('1', '2'):
        _, kept = forward(x, e)
        y = kept['a' + l] * kept['z' + l] + (e['beta' + l].astype(np.float64) - kept['a' + l] * e['mean' + l].astype(np.float64))
        e['beta' + l] = (e['beta' + l].astype(np.float64) + _off_the_kink(y.reshape(-1, y.shape[-1]))).astype(np.float32)
    _, kept = forward(x, e)
    for l in ('1', '2'):
        y = kept['a' + l] * kept['z' + l] + (e['beta' + l].astype(np.float64) - kept['a' + l] * e['mean' + l].astype(np.float64))
        assert np.abs(y).min() > 1e-4, (l, np.abs(y).min())
    return e


def _candidate(n, labels_kind, k):
    """Candidate ``k`` of a case: ``(rows int64 [n] into the cache, labels uint8 [n])``."""
    rng = np.random.default_rng([13, n, k])
    rows = rng.permutation(np.array([0, 2, 3, 4, 5]))[:n].astype(np.int64)
    if n >= 3:
        rows[1] = 1                                     # the all-zero tile
        rows[2] = rows[0]                               # and one tile twice
    labels = rng.integers(0, 2, n).astype(np.uint8) if labels_kind == 'mixed' else np.ones(n, np.uint8)
    if labels_kind == 'mixed' and n >= 2:
        labels[0], labels[1] = 0, 1
    return rows, labels


_MEMO = {}


def inputs():
    """``(cache(), exit_tensors(), _train_ref.head())``, made once."""
    if 'inputs' not in _MEMO:
        _MEMO['inputs'] = (cache(), exit_tensors(), T.head())
    return _MEMO['inputs']


UNIT = 2.0 ** -24                                       # float32's unit roundoff
CANDIDATES = 16


def grad_reference(n, rate, labels_kind, step=3):
    """``(rows, labels, loss64, grad64, f64, twin)``, computed once per case; twin: {tensor, 'loss' or 'feat': rel_err of float32
    against float64}.

    The device is allowed 8 x the twin's figure with nothing added to it, so a case must not be one where the twin sits on float64 by
    luck.  The loss is one number and ``logits/bias`` two: where the float32 result happens to be the correctly rounded float64 one,
    its figure is below ``UNIT`` -- down to 1e-9 among the candidates -- and no other float32 answer, its neighbour included, is
    within 8 x that.  A case is therefore the first of its candidates (rows and labels drawn from ``[13, n, k]``, k = 0, 1, ...)
    whose twin is off float64 by ``UNIT`` or more in EVERY figure.  The choice reads the two numpy computations only."""
    key = (n, rate, labels_kind, step)
    if key not in _MEMO:
        x, e, w = inputs()
        for k in range(CANDIDATES):
            rows, labels = _candidate(n, labels_kind, k)
            keeps = keep_masks(SEED, rows, step, rate)
            l64, g64, f64 = loss_and_grad(x[rows], labels, e, w, keeps, rate, np.float64)
            l32, g32, f32 = loss_and_grad(x[rows], labels, e, w, keeps, rate, np.float32)
            twin = {t: T.rel_err(g32[t], g64[t]) for t in g64}
            twin['loss'], twin['feat'] = T.rel_err(l32, l64), T.rel_err(f32, f64)
            if min(twin.values()) >= UNIT:
                break
        else:
            raise AssertionError(f'no candidate of case {key} has a twin off float64 by 2^-24 in every figure')
        _MEMO[key] = (rows, labels, l64, g64, f64, twin)
    return _MEMO[key]


def grad_case(n, labels_kind, rate=0.1):
    """``(rows, labels)`` of the gradient case."""
    return grad_reference(n, rate, labels_kind)[:2]
