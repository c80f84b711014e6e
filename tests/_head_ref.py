"""Float64 numpy restatement of the MC-dropout head (DESIGN.md "MC head"), the reference the kernels behind ``bq_mc_head`` are
tested against, and the rescaled heads that compute the same function in real arithmetic.

Per pass and layer the keep mask is ``oracle.philox.dropout_keep`` and the scale ``oracle.philox.dropout_scale`` (the float32
value of the contract, used as it is); every product, sum, ReLU and the softmax are float64.  ReLU keeps NaN, as the kernels do.
"""
import numpy as np

from oracle import philox

HEAD = ('hidden_0', 'hidden_1', 'logits')
N_IN = (2048, 1024, 1024)


def head_tensors(w):
    """The six head tensors of a weight dict, float64."""
    return {f'{name}/{t}': np.asarray(w[f'{name}/{t}'], np.float64) for name in HEAD for t in ('kernel', 'bias')}


def passes(feat, w, rate, seed, tile_index, mc_n, pass0=0):
    """Softmax probabilities [mc_n, n, 2] float64 of passes pass0 .. pass0 + mc_n - 1.  feat [n, 2048]; w: the six head tensors
    (any dict holding them); tile_index: int [n], the Philox tile counters (the oracle keeps their low 32 bits)."""
    feat = np.asarray(feat, np.float64)
    tile_index = np.asarray(tile_index, np.int64)
    assert feat.ndim == 2 and feat.shape[1] == N_IN[0] and tile_index.shape == (feat.shape[0],)
    t = head_tensors(w)
    scale = float(philox.dropout_scale(rate))
    out = np.empty((mc_n, feat.shape[0], 2))
    with np.errstate(invalid='ignore', over='ignore'):
        for p in range(mc_n):
            h = feat
            for layer, (name, n_in) in enumerate(zip(HEAD, N_IN)):
                keep = philox.dropout_keep(seed, tile_index, pass0 + p, layer, n_in, rate)
                h = np.where(keep, h * scale, 0.0) @ t[name + '/kernel'] + t[name + '/bias']
                if layer < 2:
                    h = np.where(h < 0.0, 0.0, h)                      # NaN stays NaN
            z = h - h.max(axis=1, keepdims=True)
            e = np.exp(z)
            out[p] = e / e.sum(axis=1, keepdims=True)
    return out


def mc(feat, w, rate, seed, tile_index, mc_n):
    """(mean [n, 2], population std [n, 2]) float64 over mc_n passes."""
    pr = passes(feat, w, rate, seed, tile_index, mc_n)
    return pr.mean(axis=0), pr.std(axis=0)


def scale_features(w, k):
    """The head that takes features * 2^k: hidden_0/kernel * 2^-k (float32, exact in the range the tests use)."""
    out = dict(w)
    out['hidden_0/kernel'] = np.ldexp(np.asarray(w['hidden_0/kernel'], np.float32), -k).astype(np.float32)
    return out


def scale_hidden(w, k):
    """The same head with hidden_0 * 2^k: (hidden_0 kernel, bias) * 2^k and hidden_1/kernel * 2^-k (ReLU is homogeneous)."""
    out = dict(w)
    for t, e in (('hidden_0/kernel', k), ('hidden_0/bias', k), ('hidden_1/kernel', -k)):
        out[t] = np.ldexp(np.asarray(w[t], np.float32), e).astype(np.float32)
    return out
