"""The planes and polygons that tests/test_roi.py (the CPU build) and tests/test_gpu_roi.py (the kernel) both rasterise, with the
restatement's plane of every one computed once (tests/_roi_ref.py)."""
import functools

import numpy as np

from tests import _roi_ref as R

SIZES = [(1, 1), (3, 5), (64, 64), (67, 131), (300, 517)]                   # (H, W): one pixel, ragged rows, several workgroups a row


def geometry(size):
    """A 'slide' of (7 W + 3) x (5 H + 2) level-0 pixels under an [H, W] raster: (w0, h0, xs, ys), the doubled pixel centres floored
    -- odd and even entries both occur."""
    h, w = size
    w0, h0 = 7 * w + 3, 5 * h + 2
    xs = np.array([((2 * x + 1) * w0) // w for x in range(w)], np.int32)
    ys = np.array([((2 * y + 1) * h0) // h for y in range(h)], np.int32)
    return w0, h0, xs, ys


def _a(*pts):
    return np.array(pts, np.int32).reshape(-1, 2)


def _rect(x0, y0, x1, y1):
    return _a((x0, y0), (x1, y0), (x1, y1), (x0, y1))


def ring(cx, cy, r_out, r_in, n=1500):
    """n integer points around (cx, cy), the radius alternating every 25 vertices between r_out and r_in: a cogwheel."""
    k = np.arange(n)
    t = 2.0 * np.pi * k / n
    r = np.where((k // 25) % 2 == 0, float(r_out), float(r_in))
    return np.stack([np.rint(cx + r * np.cos(t)), np.rint(cy + r * np.sin(t))], 1).astype(np.int32)


def polygon_cases(size):
    """name -> list of int32 [n, 2] polygons in the level-0 pixels of ``geometry(size)``."""
    w0, h0, xs, ys = geometry(size)
    rng = np.random.default_rng(1000 * size[0] + size[1])
    squares = [_rect(w0 // 8, h0 // 8, 5 * w0 // 8, 5 * h0 // 8), _rect(3 * w0 // 8, 3 * h0 // 8, 7 * w0 // 8, 7 * h0 // 8)]
    even_x, even_y = [int(v) // 2 for v in xs if v % 2 == 0], [int(v) // 2 for v in ys if v % 2 == 0]
    on = _rect(even_x[0] if even_x else 0, even_y[0] if even_y else 0, even_x[-1] if even_x else w0, even_y[-1] if even_y else h0)
    small = []
    for _ in range(40):
        cx, cy, n = int(rng.integers(0, w0)), int(rng.integers(0, h0)), int(rng.integers(3, 7))
        small.append(np.stack([cx + rng.integers(-w0 // 6 - 2, w0 // 6 + 3, n), cy + rng.integers(-h0 // 6 - 2, h0 // 6 + 3, n)], 1)
                     .astype(np.int32))
    cog = ring(w0 // 2, h0 // 2, 0.47 * min(w0, h0), 0.3 * min(w0, h0))
    return {
        'triangle': [_a((w0 // 8, h0 // 8), (7 * w0 // 8, h0 // 4), (w0 // 3, 7 * h0 // 8))],
        'concave_u': [_a((w0 // 10, h0 // 10), (9 * w0 // 10, h0 // 10), (9 * w0 // 10, 9 * h0 // 10), (7 * w0 // 10, 9 * h0 // 10),
                         (7 * w0 // 10, 3 * h0 // 10), (3 * w0 // 10, 3 * h0 // 10), (3 * w0 // 10, 9 * h0 // 10), (w0 // 10, 9 * h0 // 10))],
        'bowtie': [_a((w0 // 8, h0 // 8), (7 * w0 // 8, 7 * h0 // 8), (7 * w0 // 8, h0 // 8), (w0 // 8, 7 * h0 // 8))],
        'two_squares': squares,
        'outside': [_a((2 * w0, 2 * h0), (3 * w0, 2 * h0), (3 * w0, 3 * h0)), _rect(-3 * w0, -3 * h0, -w0, -h0)],
        'covers': [_rect(-10, -10, w0 + 10, h0 + 10)],
        'negative': [_a((-w0, -h0), (w0, h0 // 2), (w0 // 2, h0))],
        'collinear': [_a((1, 1), (w0 // 2, w0 // 2), (w0, w0), (w0 // 4, w0 // 4))],
        'on_samples': [on],
        # 3 + 1500 + 4 edges: more than any chunk of the kernel, and polygon boundaries at edges 3 and 1503, inside chunks
        'ring': [_a((0, 0), (w0 // 4, 0), (0, h0 // 4)), cog, _rect(w0 // 2, h0 // 2, w0, h0)],
        'forty_small': small,
    }


@functools.lru_cache(maxsize=None)
def expected(size):
    """name -> the restatement's plane (read-only), computed once per size."""
    w0, h0, xs, ys = geometry(size)
    out = {}
    for name, polys in polygon_cases(size).items():
        out[name] = R.plane(xs, ys, polys)
        out[name].setflags(write=False)
    return out


def check_known(size, name, got):
    """What a case must show whatever the restatement says."""
    w0, h0, xs, ys = geometry(size)
    if name in ('outside', 'collinear'):
        assert not got.any(), name
    if name == 'covers':
        assert got.all(), name
    if name == 'two_squares':                                                # union, not XOR: the overlap is inside
        ox = (xs > 2 * (3 * w0 // 8)) & (xs < 2 * (5 * w0 // 8))
        oy = (ys > 2 * (3 * h0 // 8)) & (ys < 2 * (5 * h0 // 8))
        assert (got[np.ix_(oy, ox)] == 1).all() and (size[0] < 64 or (ox.any() and oy.any())), name
    if name == 'bowtie' and size[0] >= 64:                                   # the two lobes (left, right) in; above and below the knot out
        assert got[size[0] // 2, size[1] // 8 + 1] == 1 and got[size[0] // 2, 7 * size[1] // 8 - 2] == 1
        assert got[size[0] // 4, size[1] // 2] == 0 and got[3 * size[0] // 4, size[1] // 2] == 0
    if name in ('ring', 'forty_small', 'triangle', 'concave_u') and size[0] >= 64:
        assert got.any() and not got.all(), name
