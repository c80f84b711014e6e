"""Inputs that cover the Reinhard normaliser's whole pixel domain: pure numpy, deterministic, shared by the CPU test of the cases
themselves (test_stain_cases.py) and the kernel comparison (test_gpu_stain_domain.py).

  switching-point tiles   8 tiles of uniform random bytes, each normalised to its OWN statistics.  The transform is then close to
                          the identity, and the linear value ``c`` that enters the sRGB encode lands exactly on every one of the
                          255 switching points of the encode and a few ulps below each: every entry of the kernel's table is
                          probed from both sides.
  box tiles x regimes     8 tiles drawn from colour boxes under 4 target fits (an H&E-like one, its stds x 5 -- far out of gamut on
                          both sides --, stds = 0 -- one colour -- and stds = 1e-3).
  constant colours        greys, cube corners, a 6^3 lattice and the dark colours whose X/Xn, Y/Yn, Z/Zn lie nearest to the
                          cube-root / linear switch at 0.008856 on either side: a constant tile's mean reads the forward conversion
                          back exactly.
  degenerate tiles        constant tiles (a channel deviation of exactly 0 is NaN, then byte 0) and tiles constant in all but one
                          pixel.
"""
import functools

import numpy as np

from oracle import stain

PX = 299
NPIX = PX * PX
F = np.float32

# ---- switching-point tiles -----------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def switch_tiles():
    """uint8 [8, 299, 299, 3], read-only."""
    t = np.random.default_rng(5).integers(0, 256, (8, PX, PX, 3)).astype(np.uint8)
    t.setflags(write=False)
    return t


# ---- box tiles and their target regimes ------------------------------------------------------------------------------------------------

BOX_NAMES = ('cube', 'dark', 'bright', 'midgrey6', 'he_pink', 'red_face', 'low_contrast', 'ramp')


@functools.lru_cache(maxsize=None)
def box_tiles():
    """uint8 [8, 299, 299, 3] in the order of BOX_NAMES, read-only."""
    rng = np.random.default_rng(17)

    def box(lo, hi):                                   # inclusive per-channel bounds
        lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
        return np.stack([rng.integers(int(lo[c]), int(hi[c]) + 1, (PX, PX)) for c in range(3)], -1).astype(np.uint8)

    cube = box(0, 255)
    dark = box(0, 40)
    bright = box(215, 255)
    grey = box(125, 130)
    pink = box((150, 60, 130), (240, 180, 230))
    face = box((255, 0, 0), (255, 255, 255))
    low = (box(0, 255).astype(F) * F(0.15) + F(100)).astype(np.uint8)
    x = np.broadcast_to(np.linspace(0, 255, PX), (PX, PX))
    ramp = np.stack([x, x * 0.6 + 40, 255 - x], -1).astype(np.uint8)
    t = np.stack([cube, dark, bright, grey, pink, face, low, ramp])
    t.setflags(write=False)
    return t


HE_MEANS = (65.3127, 19.871, -10.442)
HE_STDS = (15.21, 7.93, 6.07)
REGIMES = {                                            # name -> (target_means, target_stds)
    'he': (HE_MEANS, HE_STDS),
    'he_x5': (HE_MEANS, tuple(5 * s for s in HE_STDS)),
    'std0': (HE_MEANS, (0.0, 0.0, 0.0)),
    'std1e-3': (HE_MEANS, (1e-3, 1e-3, 1e-3)),
}

# ---- constant colours --------------------------------------------------------------------------------------------------------------------

DARK_MAX = 40
N_NEAREST = 8


@functools.lru_cache(maxsize=None)
def dark_switch_colours():
    """uint8 [3 * 16, 3]: for each of X, Y, Z the 8 colours with r, g, b <= 40 whose t = X/Xn (...) lies nearest below (or on) 0.008856
    -- the linear segment -- and the 8 nearest above it -- the cube root --, out of all 41^3 dark colours."""
    g = np.arange(DARK_MAX + 1, dtype=np.uint8)
    cols = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    ts = stain.xyz_over_white(cols)
    out = []
    for t in ts:
        order = np.argsort(t, kind='stable')
        k = int(np.searchsorted(t[order], stain.T_SWITCH, side='right'))       # order[:k] has t <= switch
        assert k >= N_NEAREST and len(order) - k >= N_NEAREST
        out += [cols[order[k - N_NEAREST:k]], cols[order[k:k + N_NEAREST]]]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def constant_colours():
    """uint8 [m, 3], duplicates removed, first occurrence kept, read-only."""
    greys = np.repeat(np.arange(256)[:, None], 3, 1)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    lv = np.arange(0, 256, 51)
    lattice = np.stack(np.meshgrid(lv, lv, lv, indexing='ij'), -1).reshape(-1, 3)
    allc = np.concatenate([greys, corners, lattice, dark_switch_colours()]).astype(np.uint8)
    _, first = np.unique(allc, axis=0, return_index=True)
    c = np.ascontiguousarray(allc[np.sort(first)])
    c.setflags(write=False)
    return c


CONST_CHUNK = 64
# the bound of a constant tile's deviation: E[x^2] - mu^2 cancels to within 2^-52 * npix * mu^2 in float64, whatever the order
CONST_SD_REL = float(np.sqrt(2.0 ** -52 * NPIX))


def constant_lab(colours):
    """The oracle's float32 L, a, b of each colour: [m, 3]."""
    L, a, b = stain.rgb_to_lab(np.asarray(colours, np.uint8)[None])
    return np.stack([L[0], a[0], b[0]], 1)


# ---- degenerate tiles --------------------------------------------------------------------------------------------------------------------

DEGENERATE_CONSTANTS = ((0, 0, 0), (255, 255, 255), (9, 9, 9))


def one_pixel_tiles():
    """uint8 [2, 299, 299, 3]: constant 9 with one pixel's green raised by one count; a tile constant in all but its last pixel."""
    a = np.full((PX, PX, 3), 9, np.uint8)
    a[150, 77, 1] = 10
    b = np.empty((PX, PX, 3), np.uint8)
    b[...] = (120, 80, 140)
    b[-1, -1] = (255, 255, 255)
    return np.stack([a, b])


# ---- helpers shared by both tests ----------------------------------------------------------------------------------------------------------

def own_fit(tile):
    """(means[3], stds[3]) float32 of one tile: the target that puts it in the identity regime."""
    return stain.fit(np.asarray(tile))


def linear_values(tile, tm, ts, stats=None):
    """float32 [299, 299, 3]: the linear RGB c of one tile under a fit, as it enters the sRGB encode."""
    return stain.lab_to_linear(*stain.normalised_lab(np.asarray(tile)[None], tm, ts, stats))[0]


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at |want|."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
