"""Host side of the heatmap's tissue mask (DESIGN.md "Heatmap input", Tissue mask): Otsu QC on the slide's thumbnail -- the
saturation channel, a 7 x 7 median, one inverse Otsu threshold, and every grid cell that is mostly background dropped before
anything of it is read at full resolution.  It restates Slideflow's ``qc='otsu'`` FROM MEMORY (neither Slideflow nor OpenCV is
here to pin it against) in integer arithmetic throughout, so the device and a numpy restatement agree bit for bit.  Here: the
saturation table the kernel receives (``sdiv_table``), the exact Otsu threshold of the 256 histogram counts (``otsu_threshold``),
the grid cells' ranges in thumbnail pixels (``cell_ranges``), the keep decision (``keep_from_counts``) and the argument checks.
The device side is ``Engine.tissue_blur`` / ``Engine.tissue_cells`` (csrc/kernels_tissue.hip); ``Heatmap.from_slide(qc='otsu')``
puts the two together."""
import numpy as np

QC_METHODS = ('otsu',)
QC_WIDTH = 2048                          # default thumbnail width
QC_FRACTION = 0.6                        # a cell is dropped when more than this share of its thumbnail pixels is background
MEDIAN_K = 7                             # the median's window, MEDIAN_K x MEDIAN_K with a replicated border
SAT_SHIFT = 12                           # S = ((mx - mn) * sdiv[mx] + 2^11) >> 12
MAX_GRID = 1 << 15                       # cells a side ``bq_tissue_cells`` takes


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
