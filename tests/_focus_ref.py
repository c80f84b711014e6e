"""An independent numpy restatement of the heatmap's focus mask (DESIGN.md "Heatmap input", Focus mask), for tests/test_focus.py and
tests/test_gpu_focus.py: everything in int64 over edge-padded shifted views, the taps from ``math.exp``, the union by fancy
indexing through maps made with ``fractions.Fraction``.  Nothing here imports ``biscuit_amd.tissue``."""
import math
from fractions import Fraction

import numpy as np

S = 2_550_000                                                                # integer units per unit of the [0, 1] gray image


def taps(sigma=3.0):
    """Python ints [2 r + 1], r = int(4 sigma + 0.5): rint(65536 g_k), the centre made to close the sum to 65536."""
    r = int(4.0 * sigma + 0.5)
    e = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]
    tot = math.fsum(e)
    w = [int(round(65536.0 * v / tot)) for v in e]                           # (no tap of a Gaussian sits on a .5 tie)
    w[r] += 65536 - sum(w)
    return w


def gray(img):
    a = np.asarray(img).astype(np.int64)
    return 2125 * a[:, :, 0] + 7154 * a[:, :, 1] + 721 * a[:, :, 2]


def laplace_abs(g):
    h, w = g.shape
    p = np.pad(g, 1, mode='edge')
    return np.abs(4 * g - p[0:h, 1:w + 1] - p[2:h + 2, 1:w + 1] - p[1:h + 1, 0:w] - p[1:h + 1, 2:w + 2])


def _pass(a, w, axis):
    r = (len(w) - 1) // 2
    n = a.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode='edge')
    acc = np.zeros(a.shape, np.int64)
    for k, wk in enumerate(w):
        acc += wk * (p[k:k + n, :] if axis == 0 else p[:, k:k + n])
    return (acc + 32768) >> 16


def value(img, w=None):
    """uint8 [H, W, 3] -> V int64 [H, W]: horizontal pass, rounding, vertical pass, rounding."""
    w = taps() if w is None else [int(v) for v in w]
    lap = laplace_abs(gray(img))
    assert lap.max(initial=0) <= 4 * S
    return _pass(_pass(lap, w, 1), w, 0)


def units(threshold):
    """floor(threshold * S), the product in float64."""
    return int(math.floor(float(threshold) * float(S)))


def focus(img, thr=51000, w=None):
    """-> (plane uint8 [H, W]: 1 in focus / 0 out of focus, the number of zeros, V)."""
    v = value(img, w)
    plane = (v > thr).astype(np.uint8)
    return plane, int((plane == 0).sum()), v


def nearest_map(n_to, n_from):
    return np.array([math.floor(Fraction((2 * i + 1) * n_from, 2 * n_to)) for i in range(n_to)], np.int64)


def union_counts(otsu_plane, T, focus_plane, col, row):
    """Per cell of the ranges on the Otsu plane: pixels with otsu <= T or the resized focus plane 0."""
    ho, wo = otsu_plane.shape
    hf, wf = focus_plane.shape
    resized = focus_plane[nearest_map(ho, hf)[:, None], nearest_map(wo, wf)[None, :]]
    bad = (otsu_plane <= T) | (resized == 0)
    out = np.zeros((len(row), len(col)), np.int32)
    for gy, (ya, yb) in enumerate(np.asarray(row).tolist()):
        for gx, (xa, xb) in enumerate(np.asarray(col).tolist()):
            out[gy, gx] = int(bad[ya:yb, xa:xb].sum())
    return out


def keep(counts, col, row, qc_fraction=0.6):
    col, row = np.asarray(col, np.int64), np.asarray(row, np.int64)
    area = (row[:, 1] - row[:, 0])[:, None] * (col[:, 1] - col[:, 0])[None, :]
    frac = counts.astype(np.float64) / area.astype(np.float64)
    return ~(frac > qc_fraction), frac
