"""An independent numpy / Python-int restatement of the heatmap's region-of-interest mask (DESIGN.md "Heatmap input",
Region-of-interest mask), for tests/test_roi.py and tests/test_gpu_roi.py: the doubled edge table, the two pairs of sample tables, the
plane (a loop over edges, vectorised over the pixels of the rows an edge straddles, in int64, asserting that no |d| reaches 2^62) and
the two keep decisions.  Nothing here imports ``biscuit_amd.roi``."""
import numpy as np

from tests import _tissue_ref as T


def edge_table(polygons):
    """(edges int32 [E, 4] = doubled (ax, ay, bx, by), starts int32 [P + 1]); every polygon closed last vertex to first."""
    rows, starts = [], [0]
    for poly in polygons:
        pts = [(int(x), int(y)) for x, y in np.asarray(poly).tolist()]
        for k, (ax, ay) in enumerate(pts):
            bx, by = pts[(k + 1) % len(pts)]
            rows.append((2 * ax, 2 * ay, 2 * bx, 2 * by))
        starts.append(len(rows))
    return np.array(rows, np.int32).reshape(-1, 4), np.array(starts, np.int32)


def center_tables(gw, gh, stride, extract_px):
    """Doubled cell centres: cell g covers level-0 pixels [g stride, g stride + extract_px), centre g stride + extract_px / 2."""
    return (np.array([2 * g * stride + extract_px for g in range(gw)], np.int32),
            np.array([2 * g * stride + extract_px for g in range(gh)], np.int32))


def raster_size(slide_w0, slide_h0, roi_width):
    wr = min(int(roi_width), int(slide_w0))
    return wr, max(1, int(round(int(slide_h0) * wr / int(slide_w0))))


def raster_tables(slide_w0, slide_h0, roi_width):
    """Doubled pixel centres of the [Hr, Wr] raster, floored: pixel x's centre is (x + 1/2) slide_w0 / Wr."""
    wr, hr = raster_size(slide_w0, slide_h0, roi_width)
    return (np.array([((2 * x + 1) * int(slide_w0)) // wr for x in range(wr)], np.int32),
            np.array([((2 * y + 1) * int(slide_h0)) // hr for y in range(hr)], np.int32))


def plane(xs, ys, polygons):
    """uint8 [H, W]: 1 iff (xs[x], ys[y]) is inside any polygon; inside one polygon iff an odd number of its edges count."""
    X, Y = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64)
    assert X.min() >= 0 and X.max() <= 1 << 29 and Y.min() >= 0 and Y.max() <= 1 << 29
    edges, starts = edge_table(polygons)
    assert np.abs(edges.astype(np.int64)).max() <= 1 << 28
    inside = np.zeros((len(Y), len(X)), bool)
    for p in range(len(starts) - 1):
        odd = np.zeros_like(inside)
        for ax, ay, bx, by in edges[starts[p]:starts[p + 1]].astype(np.int64).tolist():
            rows = np.flatnonzero((ay > Y) != (by > Y))                      # (never a horizontal edge)
            if len(rows) == 0:
                continue
            d = (bx - ax) * (Y[rows, None] - ay) - (X[None, :] - ax) * (by - ay)
            assert int(np.abs(d).max()) < 1 << 62
            odd[rows] ^= (d > 0) if by > ay else (d < 0)
        inside |= odd
    return inside.astype(np.uint8)


def keep_center(pl, method):
    assert method in ('inside', 'outside')
    return (pl == 1) if method == 'inside' else (pl == 0)


def keep_share(pl, gw, gh, slide_w0, slide_h0, stride, extract_px, share, method):
    """A cell's pixels of the raster plane ``pl`` (the ranges of the tissue mask's ``cell_ranges``): 'inside' keeps it iff inside /
    area >= share, 'outside' iff outside / area >= share, in float64."""
    assert method in ('inside', 'outside') and 0.0 < share <= 1.0
    col, row = T.cell_ranges(gw, gh, pl.shape[1], pl.shape[0], slide_w0, slide_h0, stride, extract_px)
    out = np.zeros((gh, gw), bool)
    for gy, (ya, yb) in enumerate(row.tolist()):
        for gx, (xa, xb) in enumerate(col.tolist()):
            cell = pl[ya:yb, xa:xb]
            n = int((cell == 1).sum()) if method == 'inside' else int((cell == 0).sum())
            out[gy, gx] = float(n) / float(cell.size) >= share
    return out
