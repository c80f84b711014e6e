"""Host side of the heatmap's region-of-interest mask (DESIGN.md "Heatmap input", Region-of-interest mask): a pathologist's polygons
-> the grid cells inside them, so that ``Heatmap.from_slide(rois=...)`` runs the model over the annotated region only.  It restates
Slideflow's ROI filter FROM MEMORY (neither Slideflow nor shapely is here to pin it against: ``ROI_Name,X_base,Y_base`` CSV files, one
polygon per name in level-0 pixels, ``roi_method`` inside / outside / auto / ignore, ``roi_filter_method`` 'center' or a share of the
tile) in integer arithmetic throughout, so the device and a numpy restatement agree integer for integer.  Here: the CSV reader
(``read_csv``), the polygon checks (``check_polygons``), the doubled edge table the kernel receives (``edge_table``), the two pairs of
sample tables (``center_tables``: the cells' centres; ``raster_tables``: the pixel centres of a thumbnail-sized raster), the keyword
checks (``check_method``, ``check_filter``) and the two keep decisions (``keep_from_plane``, ``keep_from_share``).  The device side is
``Engine.roi_plane`` (csrc/kernels_roi.hip) and, for the share, ``Engine.tissue_cells``; ``Heatmap.from_slide(rois=...)`` puts them
together."""
import csv
import math

import numpy as np

ROI_METHODS = ('auto', 'inside', 'outside', 'ignore')
ROI_WIDTH = 2048                         # default width of the raster a share is counted on
COORD_MAX = 1 << 27                      # |level-0 vertex coordinate| <= 2^27
SAMPLE_MAX = 1 << 29                     # 0 <= doubled sample coordinate <= 2^29
MAX_EDGES = 1 << 20                      # edges ``bq_roi_plane`` takes
CSV_COLUMNS = ('ROI_Name', 'X_base', 'Y_base')


def read_csv(path):
    """Slideflow's ROI CSV -> a list of int32 [n, 2] (x, y) arrays in level-0 pixels, one per ``ROI_Name`` in order of first
    appearance (rows of one name may be interleaved with another's).  The header must hold ``ROI_Name``, ``X_base`` and ``Y_base``,
    in any column order; other columns are ignored; a coordinate is ``int(float(s))``.  ValueError for a missing column, a
    coordinate that is no finite number, and a polygon of fewer than three points (named)."""
    with open(path, newline='') as f:
        rows = csv.reader(f)
        header = [h.strip() for h in next(rows, [])]
        missing = [c for c in CSV_COLUMNS if c not in header]
        if missing:
            raise ValueError(f'{path}: an ROI file has the columns {", ".join(CSV_COLUMNS)}; missing: {", ".join(missing)}')
        i_name, i_x, i_y = (header.index(c) for c in CSV_COLUMNS)
        points = {}
        for n, r in enumerate(rows, 2):
            if not any(c.strip() for c in r):
                continue
            try:
                x, y = float(r[i_x]), float(r[i_y])
                if not (math.isfinite(x) and math.isfinite(y)):
                    raise ValueError
                points.setdefault(r[i_name], []).append((int(x), int(y)))
            except (ValueError, IndexError):
                raise ValueError(f'{path}, line {n}: not an ROI vertex: {r!r}') from None
    for name, pts in points.items():
        if len(pts) < 3:
            raise ValueError(f'{path}: polygon {name!r} has {len(pts)} points; a polygon needs at least three')
    return check_polygons(list(points.values()))


def check_polygons(polygons):
    """A caller's polygons as a list of contiguous int32 [n, 2] arrays.  ValueError for anything that is not a non-empty sequence of
    integer [n >= 3, 2] arrays with every coordinate in [-2^27, 2^27], or that has more than 2^20 vertices in all.  A polygon is
    closed implicitly (last vertex to first); self-intersection and zero area are legal."""
    if not isinstance(polygons, (list, tuple)) or len(polygons) == 0:
        raise ValueError('rois must be a non-empty list of int [n, 2] arrays of (x, y) vertices')
    out = []
    for i, poly in enumerate(polygons):
        a = np.asarray(poly)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 3 or a.dtype.kind not in 'iu':
            raise ValueError(f'polygon {i} must be an integer [n >= 3, 2] array of (x, y) vertices, not {a.dtype} {list(a.shape)}')
        if int(a.min()) < -COORD_MAX or int(a.max()) > COORD_MAX:
            raise ValueError(f'polygon {i} has a coordinate outside [-2^27, 2^27]')
        out.append(np.ascontiguousarray(a, np.int32))
    if sum(len(a) for a in out) > MAX_EDGES:
        raise ValueError(f'{sum(len(a) for a in out)} vertices; the mask takes at most {MAX_EDGES}')
    return out


def edge_table(polygons):
    """-> (edges int32 [E, 4], starts int32 [P + 1]): polygon i's vertices v_0 .. v_{n-1} become the n rows (2 v_k.x, 2 v_k.y,
    2 v_{k+1 mod n}.x, 2 v_{k+1 mod n}.y) -- doubled, the closing edge last -- at rows [starts[i], starts[i + 1])."""
    polygons = check_polygons(polygons)
    starts = np.zeros(len(polygons) + 1, np.int32)
    starts[1:] = np.cumsum([len(a) for a in polygons])
    edges = np.concatenate([np.concatenate([2 * a, 2 * np.roll(a, -1, axis=0)], axis=1) for a in polygons]).astype(np.int32)
    return np.ascontiguousarray(edges), starts


def _table(values, what):
    if min(values) < 0 or max(values) > SAMPLE_MAX:
        raise ValueError(f'{what}: a doubled sample coordinate leaves [0, 2^29]')
    return np.array(values, np.int32)


def _ints(what, **kw):
    for k, v in kw.items():
        if int(v) != v or int(v) < 1:
            raise ValueError(f'{what}: {k} must be a positive integer, not {v!r}')
    return [int(v) for v in kw.values()]


def center_tables(gw, gh, stride, extract_px):
    """The sample tables of ``roi_filter_method='center'``: (xs int32 [gw], ys int32 [gh]) with ``xs[gx] = 2 gx stride +
    extract_px``, the doubled centre of cell gx (level-0 pixels [gx stride, gx stride + extract_px)), ``ys`` likewise."""
    gw, gh, stride, extract_px = _ints('center_tables', gw=gw, gh=gh, stride=stride, extract_px=extract_px)
    return (_table([2 * g * stride + extract_px for g in range(gw)], 'center_tables'),
            _table([2 * g * stride + extract_px for g in range(gh)], 'center_tables'))


def raster_size(slide_w0, slide_h0, roi_width=ROI_WIDTH):
    """(Wr, Hr) of the raster a share is counted on, the geometry of ``wsi.WSI.thumbnail(roi_width)`` (nothing is read): ``Wr =
    min(roi_width, slide_w0)``, ``Hr = max(1, round(slide_h0 * Wr / slide_w0))`` (float64 division, Python's round)."""
    slide_w0, slide_h0, roi_width = _ints('raster_size', slide_w0=slide_w0, slide_h0=slide_h0, roi_width=roi_width)
    wr = min(roi_width, slide_w0)
    return wr, max(1, int(round(slide_h0 * wr / slide_w0)))


def raster_tables(slide_w0, slide_h0, roi_width=ROI_WIDTH):
    """The sample tables of a share: (xs int32 [Wr], ys int32 [Hr]) over ``raster_size``'s raster with ``xs[x] = ((2 x + 1)
    slide_w0) // Wr``, the doubled level-0 coordinate of pixel x's centre, floored; ``ys[y] = ((2 y + 1) slide_h0) // Hr``."""
    wr, hr = raster_size(slide_w0, slide_h0, roi_width)
    slide_w0, slide_h0 = int(slide_w0), int(slide_h0)
    if wr * hr >= 1 << 31:
        raise ValueError(f'a raster has W * H < 2^31, not {wr} x {hr}')
    return (_table([((2 * x + 1) * slide_w0) // wr for x in range(wr)], 'raster_tables'),
            _table([((2 * y + 1) * slide_h0) // hr for y in range(hr)], 'raster_tables'))


def check_method(roi_method, have_polygons):
    """``roi_method`` resolved to 'inside', 'outside' or 'ignore': 'auto' is 'inside' with polygons and 'ignore' without.
    ValueError for another string, and for 'inside' / 'outside' without polygons."""
    if roi_method not in ROI_METHODS:
        raise ValueError(f'roi_method must be one of {ROI_METHODS}, not {roi_method!r}')
    if roi_method == 'auto':
        return 'inside' if have_polygons else 'ignore'
    if roi_method != 'ignore' and not have_polygons:
        raise ValueError(f'roi_method={roi_method!r} needs rois')
    return roi_method


def check_filter(roi_filter_method):
    """``roi_filter_method`` as 'center' or a float share in (0, 1]; ValueError for anything else."""
    if isinstance(roi_filter_method, str):
        if roi_filter_method == 'center':
            return 'center'
        raise ValueError(f"roi_filter_method must be 'center' or a share in (0, 1], not {roi_filter_method!r}")
    try:
        f = float(roi_filter_method)
    except (TypeError, ValueError):
        raise ValueError(f"roi_filter_method must be 'center' or a share in (0, 1], not {roi_filter_method!r}") from None
    if isinstance(roi_filter_method, bool) or not 0.0 < f <= 1.0:
        raise ValueError(f"roi_filter_method must be 'center' or a share in (0, 1], not {roi_filter_method!r}")
    return f


def check_width(roi_width):
    if int(roi_width) != roi_width or int(roi_width) < 1:
        raise ValueError(f'roi_width must be at least 1, not {roi_width!r}')
    return int(roi_width)


def keep_from_plane(plane, method):
    """'center': the plane of the cells' centres (uint8 [gh, gw] of 0 / 1) -> bool [gh, gw]; 'inside' keeps the ones, 'outside' the
    zeros."""
    p = np.asarray(plane)
    if p.ndim != 2 or p.dtype != np.uint8 or (p > 1).any():
        raise ValueError('plane must be uint8 [gh, gw] of 0 and 1')
    if method not in ('inside', 'outside'):
        raise ValueError(f"method must be 'inside' or 'outside', not {method!r}")
    return p == (1 if method == 'inside' else 0)


def keep_from_share(outside, col, row, share, method):
    """A share: ``outside`` int [gh, gw], every cell's raster pixels outside the region (``Engine.tissue_cells(plane, 0, col,
    row)``), and the cells' ranges (``tissue.cell_ranges``) -> bool [gh, gw].  With ``area`` the pixels of a cell's range and
    ``inside = area - outside``, 'inside' keeps a cell iff ``inside / area >= share`` and 'outside' iff ``outside / area >= share``,
    both in float64."""
    f = check_filter(share)
    if f == 'center' or method not in ('inside', 'outside'):
        raise ValueError(f"keep_from_share takes a share in (0, 1] and 'inside' or 'outside', not {share!r} and {method!r}")
    outside, col, row = np.asarray(outside), np.asarray(col, np.int64), np.asarray(row, np.int64)
    if col.ndim != 2 or col.shape[1] != 2 or row.ndim != 2 or row.shape[1] != 2 or outside.shape != (len(row), len(col)):
        raise ValueError(f'counts {list(outside.shape)} do not belong to ranges {list(row.shape)} x {list(col.shape)}')
    area = (row[:, 1] - row[:, 0])[:, None] * (col[:, 1] - col[:, 0])[None, :]
    if (area <= 0).any() or (outside < 0).any() or (outside > area).any():
        raise ValueError('an empty range, or a count outside [0, area]')
    n = outside.astype(np.int64) if method == 'outside' else area - outside.astype(np.int64)
    return n.astype(np.float64) / area.astype(np.float64) >= f


def plane_host(xs, ys, polygons):
    """The CPU build of ``Engine.roi_plane`` (``bqio_roi_plane``, libbiscuit_io): uint8 [H, W], 1 where the doubled sample point
    (xs[x], ys[y]) lies inside any polygon.  For tests.  ValueError for what the entry refuses."""
    from . import tfrecord_native
    edges, starts = edge_table(polygons)
    xs, ys = np.ascontiguousarray(xs, np.int32), np.ascontiguousarray(ys, np.int32)
    if xs.ndim != 1 or ys.ndim != 1:
        raise ValueError('xs and ys must be int32 [W] and [H]')
    plane = np.empty((len(ys), len(xs)), np.uint8)
    e = tfrecord_native.lib().bqio_roi_plane(edges.ctypes.data, len(edges), starts.ctypes.data, len(starts) - 1, xs.ctypes.data, len(xs),
                                             ys.ctypes.data, len(ys), plane.ctypes.data)
    if e != 0:
        raise ValueError(f'bqio_roi_plane: error {e}')
    return plane
