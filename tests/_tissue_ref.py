"""An independent numpy restatement of the heatmap's tissue mask (DESIGN.md "Heatmap input", Tissue mask), for
tests/test_tissue.py and tests/test_gpu_tissue.py: the saturation from its formula, the 7 x 7 median by sorting the 49 edge-padded
shifted views, Otsu by brute force over ``fractions.Fraction``, cell ranges and counts by plain loops.  Nothing here imports
``biscuit_amd.tissue``."""
import math
from fractions import Fraction

import numpy as np


def saturation(img):
    """uint8 [H, W, 3] -> uint8 [H, W]: S = ((mx - mn) * sdiv[mx] + 2048) >> 12, sdiv[0] = 0, sdiv[v] = rint(255 * 4096 / v)."""
    sdiv = np.array([0] + [int(np.rint(255.0 * 4096.0 / v)) for v in range(1, 256)], np.int64)
    a = np.asarray(img).astype(np.int64)
    mx, mn = a.max(2), a.min(2)
    s = ((mx - mn) * sdiv[mx] + 2048) >> 12
    assert s.min() >= 0 and s.max() <= 255
    return s.astype(np.uint8)


def median7(s):
    """uint8 [H, W] -> the 25th smallest of every pixel's 49 neighbours, coordinates clamped to the image."""
    h, w = s.shape
    p = np.pad(s, 3, mode='edge')
    views = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(7) for dx in range(7)])
    return np.sort(views, axis=0)[24]


def blur(img):
    """(plane uint8 [H, W], hist int64 [256]) of a thumbnail."""
    plane = median7(saturation(img))
    return plane, np.bincount(plane.reshape(-1), minlength=256)


def otsu(hist):
    """The smallest t in 0 .. 254 with the largest (s0 n1 - s1 n0)^2 / (n0 n1) over the t whose two classes are both occupied;
    0 when there is none."""
    h = [int(v) for v in hist]
    best, best_score = 0, None
    for t in range(255):
        n0, n1 = sum(h[:t + 1]), sum(h[t + 1:])
        if n0 == 0 or n1 == 0:
            continue
        s0 = sum(i * h[i] for i in range(t + 1))
        s1 = sum(i * h[i] for i in range(t + 1, 256))
        score = Fraction((s0 * n1 - s1 * n0) ** 2, n0 * n1)
        if best_score is None or score > best_score:
            best, best_score = t, score
    return best


def cell_ranges(gw, gh, W, H, slide_w0, slide_h0, stride, extract_px):
    def axis(n_cells, n_px, extent0):
        out = []
        for g in range(n_cells):
            lo = math.floor(Fraction(g * stride * n_px, extent0))
            hi = min(n_px, max(lo + 1, math.ceil(Fraction((g * stride + extract_px) * n_px, extent0))))
            out.append((lo, hi))
        return np.array(out, np.int32).reshape(n_cells, 2)
    return axis(gw, W, slide_w0), axis(gh, H, slide_h0)


def cell_counts(plane, T, col, row):
    out = np.zeros((len(row), len(col)), np.int32)
    for gy, (ya, yb) in enumerate(np.asarray(row).tolist()):
        for gx, (xa, xb) in enumerate(np.asarray(col).tolist()):
            out[gy, gx] = int((plane[ya:yb, xa:xb] <= T).sum())
    return out


def cell_fractions(counts, col, row):
    out = np.zeros(counts.shape, np.float64)
    for gy, (ya, yb) in enumerate(np.asarray(row).tolist()):
        for gx, (xa, xb) in enumerate(np.asarray(col).tolist()):
            out[gy, gx] = float(counts[gy, gx]) / float((yb - ya) * (xb - xa))
    return out


def mask(thumb, gw, gh, slide_w0, slide_h0, stride, extract_px, qc_fraction=0.6):
    """The whole definition: -> (keep bool [gh, gw], T, every cell's background fraction)."""
    plane, hist = blur(thumb)
    T = otsu(hist)
    col, row = cell_ranges(gw, gh, thumb.shape[1], thumb.shape[0], slide_w0, slide_h0, stride, extract_px)
    frac = cell_fractions(cell_counts(plane, T, col, row), col, row)
    return ~(frac > qc_fraction), T, frac
