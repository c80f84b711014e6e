"""Host side of the heatmap's tissue mask (DESIGN.md "Heatmap input", Tissue mask): Otsu QC on the slide's thumbnail -- the
saturation channel, a 7 x 7 median, one inverse Otsu threshold, and every grid cell that is mostly background dropped before
anything of it is read at full resolution.  It restates Slideflow's ``qc='otsu'`` FROM MEMORY (neither Slideflow nor OpenCV is
here to pin it against) in integer arithmetic throughout, so the device and a numpy restatement agree bit for bit.  Here: the
saturation table the kernel receives (``sdiv_table``), the exact Otsu threshold of the 256 histogram counts (``otsu_threshold``),
the grid cells' ranges in thumbnail pixels (``cell_ranges``), the keep decision (``keep_from_counts``) and the argument checks.
The device side is ``Engine.tissue_blur`` / ``Engine.tissue_cells`` (csrc/kernels_tissue.hip); ``Heatmap.from_slide(qc='otsu')``
puts the two together.

The focus mask (DESIGN.md "Heatmap input", Focus mask) is the other half of Slideflow's ``qc='both'``: its Gaussian blur filter,
also restated from memory in integers -- gray, |Laplacian|, a separable Gaussian and one threshold on a 4 um / pixel thumbnail.
Here: the Gaussian's integer taps (``focus_taps``), the threshold in integer units (``focus_units``), the thumbnail's width
(``focus_width``), the nearest-neighbour map that lays the focus plane over the Otsu plane (``plane_map``) and the argument checks
(``check_focus``).  The device side is ``Engine.tissue_focus`` / ``Engine.tissue_cells_union`` (csrc/kernels_focus.hip);
``Heatmap.from_slide(focus_threshold=...)`` puts them together.  ``QC_METHODS`` stays ``('otsu',)``: Slideflow's ``'blur'`` is
spelled ``focus_threshold=0.02`` and its ``'both'`` ``qc='otsu', focus_threshold=0.02``."""
import math

import numpy as np

QC_METHODS = ('otsu',)
QC_WIDTH = 2048                          # default thumbnail width
QC_FRACTION = 0.6                        # a cell is dropped when more than this share of its thumbnail pixels is background
MEDIAN_K = 7                             # the median's window, MEDIAN_K x MEDIAN_K with a replicated border
SAT_SHIFT = 12                           # S = ((mx - mn) * sdiv[mx] + 2^11) >> 12
MAX_GRID = 1 << 15                       # cells a side ``bq_tissue_cells`` takes
FOCUS_SCALE = 2_550_000                  # integer units per unit of the [0, 1] gray image: G = 2125 r + 7154 g + 721 b
FOCUS_MPP = 4.0                          # microns per pixel of the focus thumbnail
FOCUS_SIGMA = 3.0                        # the Gaussian's sigma, in thumbnail pixels
FOCUS_THRESHOLD = 0.02                   # a pixel is out of focus iff its blurred |Laplacian| is <= this (Slideflow's default)
FOCUS_TAP_SHIFT = 16                     # the taps sum to 2^16
FOCUS_MAX_RADIUS = 16                    # the largest radius ``bq_tissue_focus`` takes


def sdiv_table():
    """int32 [256]: ``sdiv[0] = 0``, ``sdiv[v] = rint(255 * 4096 / v)`` -- the table behind the 8-bit saturation ``S = ((mx -
    mn) * sdiv[mx] + 2048) >> 12`` (OpenCV's 8-bit RGB -> HSV, restated)."""
    t = np.zeros(256, np.int32)
    t[1:] = np.rint(255.0 * (1 << SAT_SHIFT) / np.arange(1, 256, dtype=np.float64)).astype(np.int32)
    return t


def check_hist(hist):
    """The histogram as a list of 256 Python ints; ValueError for another shape, a non-integer type or a negative count."""
    h = np.asarray(hist)
    if h.shape != (256,) or h.dtype.kind not in 'iu':
        raise ValueError(f'a histogram is 256 integers, not {h.dtype} {list(h.shape)}')
    h = [int(v) for v in h]
    if min(h) < 0:
        raise ValueError('negative histogram count')
    return h


def otsu_threshold(hist):
    """Otsu's threshold of a 256-bin histogram in exact integer arithmetic: for t in 0 .. 254 with both classes occupied (n0 =
    sum_{i <= t} h[i], n1 = N - n0, s0 = sum_{i <= t} i h[i], s1 likewise above t) the score is (s0 n1 - s1 n0)^2 / (n0 n1);
    scores are compared as fractions by cross-multiplication, so ties are exact.  -> the smallest t with the largest score, 0
    when no t qualifies (at most one occupied bin).  A pixel is background iff its value is <= the threshold."""
    h = check_hist(hist)
    n, s = sum(h), sum(i * v for i, v in enumerate(h))
    best, best_num, best_den = 0, -1, 1
    n0 = s0 = 0
    for t in range(255):
        n0 += h[t]
        s0 += t * h[t]
        n1 = n - n0
        if n0 == 0 or n1 == 0:
            continue
        d = s0 * n1 - (s - s0) * n0
        num, den = d * d, n0 * n1
        if num * best_den > best_num * den:                              # strictly larger: the first of equals stays
            best, best_num, best_den = t, num, den
    return best


def _axis_ranges(n_cells, n_px, extent0, stride, extract_px):
    out = np.empty((n_cells, 2), np.int32)
    for g in range(n_cells):
        a0 = g * stride
        lo = (a0 * n_px) // extent0
        if lo >= n_px:
            raise ValueError(f'grid cell {g} starts at level-0 pixel {a0}, outside the slide ({extent0})')
        hi = min(n_px, max(lo + 1, -((-(a0 + extract_px) * n_px) // extent0)))
        out[g] = (lo, hi)
    return out


def cell_ranges(gw, gh, W, H, slide_w0, slide_h0, stride, extract_px):
    """The grid's cells in pixels of a ``W`` x ``H`` thumbnail of the ``slide_w0`` x ``slide_h0`` slide, in integer arithmetic:
    cell gx covers level-0 pixels [gx * stride, gx * stride + extract_px), columns ``x_a = floor(x0 * W / slide_w0)`` to ``x_b =
    min(W, max(x_a + 1, ceil((x0 + extract_px) * W / slide_w0)))``, rows likewise.  -> (col int32 [gw, 2], row int32 [gh, 2]),
    every range non-empty and inside the thumbnail."""
    vals = (gw, gh, W, H, slide_w0, slide_h0, stride, extract_px)
    if any(int(v) != v for v in vals):
        raise ValueError('cell_ranges takes integers')
    gw, gh, W, H, slide_w0, slide_h0, stride, extract_px = (int(v) for v in vals)
    if not (1 <= gw <= MAX_GRID and 1 <= gh <= MAX_GRID):
        raise ValueError(f'a grid is 1 .. {MAX_GRID} cells a side, not {gh} x {gw}')
    if W < 1 or H < 1 or W * H >= 1 << 31:
        raise ValueError(f'a thumbnail has 1 <= W, H and W * H < 2^31, not {W} x {H}')
    if slide_w0 < 1 or slide_h0 < 1 or stride < 1 or extract_px < 1:
        raise ValueError('slide_w0, slide_h0, stride and extract_px must be positive')
    return _axis_ranges(gw, W, slide_w0, stride, extract_px), _axis_ranges(gh, H, slide_h0, stride, extract_px)


def check_fraction(qc_fraction):
    f = float(qc_fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f'qc_fraction must lie in [0, 1], not {qc_fraction!r}')
    return f


def keep_from_counts(counts, col, row, qc_fraction=QC_FRACTION):
    """bool [gh, gw]: a cell is dropped iff ``count / area > qc_fraction`` in float64, ``area`` the pixels of its range."""
    f = check_fraction(qc_fraction)
    counts, col, row = np.asarray(counts), np.asarray(col, np.int64), np.asarray(row, np.int64)
    if col.ndim != 2 or col.shape[1] != 2 or row.ndim != 2 or row.shape[1] != 2 or counts.shape != (len(row), len(col)):
        raise ValueError(f'counts {list(counts.shape)} do not belong to ranges {list(row.shape)} x {list(col.shape)}')
    area = (row[:, 1] - row[:, 0])[:, None] * (col[:, 1] - col[:, 0])[None, :]
    if (area <= 0).any() or (counts < 0).any() or (counts > area).any():
        raise ValueError('an empty range, or a count outside [0, area]')
    return ~(counts.astype(np.float64) / area.astype(np.float64) > f)


def check_mask(mask, gh, gw, name='cell_mask'):
    """A caller's keep mask as a bool [gh, gw] array; ValueError for another shape or type."""
    m = np.asarray(mask)
    if m.dtype != np.bool_ or m.shape != (gh, gw):
        raise ValueError(f'{name} must be bool [{gh}, {gw}] (the slide\'s grid), not {m.dtype} {list(m.shape)}')
    return m


def focus_taps(sigma=FOCUS_SIGMA):
    """int32 [2 r + 1], ``r = int(4 sigma + 0.5)`` (scipy's ``truncate=4``): ``w[k] = rint(65536 g_k)`` of the normalised Gaussian
    ``g_k ~ exp(-(k - r)^2 / (2 sigma^2))``, the centre tap corrected so that the sum is exactly 65536.  ValueError for a sigma
    that is not finite, or whose radius is outside 1 .. 16 (what ``bq_tissue_focus`` takes)."""
    sigma = float(sigma)
    if not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f'focus_sigma must be a positive finite number, not {sigma!r}')
    r = int(4.0 * sigma + 0.5)
    if not 1 <= r <= FOCUS_MAX_RADIUS:
        raise ValueError(f'focus_sigma {sigma!r} gives a radius of {r}; the kernel takes 1 .. {FOCUS_MAX_RADIUS}')
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * x * x / (sigma * sigma))
    g /= g.sum()
    w = np.rint(g * (1 << FOCUS_TAP_SHIFT)).astype(np.int64)
    w[r] += (1 << FOCUS_TAP_SHIFT) - int(w.sum())
    assert int(w.sum()) == 1 << FOCUS_TAP_SHIFT and int(w.min()) >= 0
    return w.astype(np.int32)


def focus_units(threshold=FOCUS_THRESHOLD):
    """``thr = floor(threshold * FOCUS_SCALE)``: a pixel is out of focus iff ``V <= thr`` (51 000 for 0.02).  ValueError for a
    threshold that is not finite, negative, or beyond int32 in units."""
    t = float(threshold)
    if not math.isfinite(t) or t < 0.0:
        raise ValueError(f'focus_threshold must be a finite number >= 0, not {threshold!r}')
    thr = math.floor(t * FOCUS_SCALE)
    if thr >= 1 << 31:
        raise ValueError(f'focus_threshold {threshold!r} is beyond every value the blurred Laplacian takes (at most 4)')
    return int(thr)


def focus_width(slide_w0, mpp, focus_mpp=FOCUS_MPP):
    """The focus thumbnail's width: ``max(1, min(slide_w0, round(slide_w0 * mpp / focus_mpp)))``."""
    return max(1, min(int(slide_w0), int(round(int(slide_w0) * float(mpp) / float(focus_mpp)))))


def plane_map(n_to, n_from):
    """int32 [n_to]: ``m[i] = ((2 i + 1) n_from) // (2 n_to)`` in Python integers -- the pixel of an ``n_from``-long axis that the
    centre of pixel ``i`` of an ``n_to``-long axis falls into (a nearest-neighbour resize).  Non-decreasing, inside [0, n_from)."""
    if int(n_to) != n_to or int(n_from) != n_from or n_to < 1 or n_from < 1 or n_from >= 1 << 31:
        raise ValueError(f'plane_map takes two positive lengths, not {n_to!r} and {n_from!r}')
    n_to, n_from = int(n_to), int(n_from)
    return np.array([((2 * i + 1) * n_from) // (2 * n_to) for i in range(n_to)], np.int32)


def check_focus(threshold, mpp=FOCUS_MPP, sigma=FOCUS_SIGMA):
    """-> (thr in integer units, focus_mpp, the taps); ValueError as ``focus_units`` / ``focus_taps``, and for a ``focus_mpp`` that
    is not a positive finite number."""
    thr = focus_units(threshold)
    m = float(mpp)
    if not math.isfinite(m) or m <= 0.0:
        raise ValueError(f'focus_mpp must be a positive finite number, not {mpp!r}')
    return thr, m, focus_taps(sigma)
