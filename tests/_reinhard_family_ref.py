"""TEST INFRASTRUCTURE -- numpy restatement of Slideflow's Reinhard family as DESIGN.md section 7 "Reinhard family" states it
(``reinhard_fast`` = 0, ``reinhard`` = 1, ``reinhard_fast_mask`` = 2, ``reinhard_mask`` = 3: flags BRIGHTNESS = 1, MASK = 2).
Written from that section; the LAB arithmetic is ``oracle/stain.py``'s, nothing is shared with ``biscuit_amd/stain.py``.

``analyse`` is steps B, M and S of one tile, ``normalise`` the whole method.  ``normalise(..., stats=)`` takes the tissue statistics
from outside, as ``oracle.stain.reinhard_fast`` does: two correct reductions in different summation orders may differ in the last
bit of a mean, and a comparison of the transform itself must not inherit that.
"""
import numpy as np

from oracle import stain as O

F = np.float32
BRIGHTNESS, MASK = 1, 2
OK, NO_TISSUE, DARK = 0, 1, 2
PCT = 0.9
MASK_THRESHOLD = 0.93


def mask_level(mask_threshold=MASK_THRESHOLD):
    """mask_L: 100 * mask_threshold in float64, rounded once to float32."""
    return F(100.0 * float(mask_threshold))


def percentile90(L):
    """The 90th percentile of the float32 values ``L`` (any shape): numpy's 'linear' rule at v = 0.9 (N - 1) in float64 over the
    sorted values, numpy's _lerp, rounded once to float32."""
    s = np.sort(np.asarray(L, F).reshape(-1)).astype(np.float64)
    n = s.size
    v = PCT * float(n - 1)
    lo = int(np.floor(v))
    t = v - lo
    a, b = s[lo], s[min(lo + 1, n - 1)]
    d = b - a
    return F(b - d * (1.0 - t) if t >= 0.5 else a + d * t)


def brightness_table(p):
    """uint8 [256]: byte c -> trunc(min(float32(c) * (100.0f / p), 255.0f))."""
    s = F(100.0) / F(p)
    return np.trunc(np.minimum((np.arange(256, dtype=F) * s).astype(F), F(255.0))).astype(np.uint8)


def analyse(tile, flags, mask_L=None):
    """Steps B, M, S of one tile [px, px, 3] uint8 -> dict: status, p (float32), bright (I', uint8; the tile itself when DARK),
    tissue (bool [px, px]; None when DARK), m, frac (float32 m / N), mu and sd (float32 [3]; NaN unless status is OK)."""
    tile = np.asarray(tile, np.uint8)
    assert tile.ndim == 3 and tile.shape[0] == tile.shape[1] and tile.shape[2] == 3 and 0 <= flags <= 3
    mask_L = mask_level() if mask_L is None else F(mask_L)
    npix = tile.shape[0] * tile.shape[1]
    nan3 = np.full(3, np.nan, F)
    out = {'status': OK, 'p': F(100.0), 'bright': tile, 'tissue': None, 'm': 0, 'frac': F(0.0), 'mu': nan3, 'sd': nan3.copy()}
    if flags & BRIGHTNESS:
        p = percentile90(O.rgb_to_lab(tile[None])[0])
        out['p'] = p
        if not np.isfinite(p) or p <= 0:
            out['status'] = DARK
            return out
        out['bright'] = brightness_table(p)[tile]
    L, a, b = (c[0] for c in O.rgb_to_lab(out['bright'][None]))
    tissue = L < mask_L if flags & MASK else np.ones(L.shape, bool)
    m = int(tissue.sum())
    out['tissue'] = tissue
    if m == 0:
        out['status'] = NO_TISSUE
        return out
    out['m'], out['frac'] = m, F(float(m) / float(npix))
    mu, sd = O.lab_stats(L[tissue][None], a[tissue][None], b[tissue][None])
    out['mu'], out['sd'] = mu[0], sd[0]
    return out


def fit(target, flags, mask_L=None):
    """(target_means, target_stds) float32 [3] of one target image; ValueError when it is DARK or has NO_TISSUE."""
    r = analyse(target, flags, mask_L)
    if r['status'] != OK:
        raise ValueError(f"degenerate target (status {r['status']})")
    return r['mu'], r['sd']


def normalise(tile, flags, target_means, target_stds, mask_L=None, stats=None):
    """One tile [px, px, 3] uint8 -> (uint8 [px, px, 3], status).  ``stats`` = (mu [3], sd [3]) float32 replaces the tissue
    statistics of step S (status, percentile and mask stay the restatement's own)."""
    r = analyse(tile, flags, mask_L)
    if r['status'] != OK:
        return r['bright'].copy(), r['status']
    mu, sd = (r['mu'], r['sd']) if stats is None else (np.asarray(stats[0], F).reshape(3), np.asarray(stats[1], F).reshape(3))
    bright = r['bright']
    moved = O.reinhard_fast(bright[None], target_means, target_stds, stats=(mu.reshape(1, 3), sd.reshape(1, 3)))[0]
    return np.where(r['tissue'][..., None], moved, bright), OK
