"""Stain normalisation in front of the staging kernel (hp.py:19 ``normalizer='reinhard_fast'``, the rest of Slideflow's Reinhard
family -- ``'reinhard'``, ``'reinhard_mask'``, ``'reinhard_fast_mask'`` --, or ``'macenko'``).

Mirrors the object the reference calls at results.py:251-252
(``interface.wsi_normalizer.rgb_to_rgb(image)``): a fitted normaliser with ``rgb_to_rgb``, ``fit`` and
``get_fit``; the arithmetic runs in the HIP kernel behind ``bq_stain_reinhard_fast``.  The target
statistics are the ``norm_fit`` block of a Slideflow model's ``params.json`` -- they are read from
there (``from_params``) or fitted to a target image, never hard-coded.  ``Macenko`` is the same object for a model trained
with ``normalizer='macenko'`` (kernel behind ``bq_stain_macenko``; DESIGN.md "Macenko").  ``Reinhard``, ``ReinhardMask`` and
``ReinhardFastMask`` are ``reinhard_fast`` with a brightness standardisation in front and / or a tissue mask (kernel behind
``bq_stain_reinhard``; DESIGN.md "Reinhard family"); their fit has ``reinhard_fast``'s keys.  ``normalise`` is the one dispatch
every driver calls.
"""
import json

import numpy as np
import torch

TILE_PX = 299
METHODS = ('reinhard_fast', 'macenko', 'reinhard', 'reinhard_mask', 'reinhard_fast_mask')

# The Reinhard family (DESIGN.md "Reinhard family"; restated from Slideflow's definitions and UNPINNED like Macenko's constants: a box
# with Slideflow settles them; kernels_reinhard.hip holds the same values).  A method is a pair of flags.
REINHARD_BRIGHTNESS, REINHARD_MASK = 1, 2
REINHARD_FLAGS = {'reinhard_fast': 0, 'reinhard': REINHARD_BRIGHTNESS, 'reinhard_fast_mask': REINHARD_MASK,
                  'reinhard_mask': REINHARD_BRIGHTNESS | REINHARD_MASK}
REINHARD_BRIGHT_PCT = 90.0         # brightness standardisation: this percentile of the tile's L becomes L = 100
REINHARD_MASK_THRESHOLD = 0.93     # a pixel is tissue when its L is below 100 * this (Slideflow's default)
# per-tile status of the family's kernel: NO_TISSUE leaves the brightness stage's bytes, DARK passes the tile through unchanged
REINHARD_OK, REINHARD_NO_TISSUE, REINHARD_DARK = 0, 1, 2
# the methods whose kernel reports a per-tile status (``normalise(..., status=)``): 0 is a normalised tile in all of them
STATUS_METHODS = ('macenko', 'reinhard', 'reinhard_mask', 'reinhard_fast_mask')

# Macenko's constants (Macenko 2009 in the numpy form of HEnorm_python, recalled and UNPINNED: a box with Slideflow settles them;
# kernels_stain.hip holds the same values)
MACENKO_IO = 255.0                 # transmitted light intensity
MACENKO_ALPHA = 1.0                # percentile of the extreme stain angles
MACENKO_BETA = 0.15                # OD below which a pixel is background
MACENKO_CONC_PCT = 99.0            # percentile of the concentrations (maxC)
MACENKO_OVER_TO = 254.0            # HEnorm_python's quirk: Inorm > 255 becomes 254, not 255
MACENKO_DET_MIN = 1e-12            # |det(HE^T HE)| below this: a degenerate tile (status 2)
MACENKO_HE_REF = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))     # default fit: HERef (3x2, columns H, E)
MACENKO_MAXC_REF = (1.9705, 1.0308)                                          # and maxCRef
# the norm_fit keys of a Macenko model's params.json (Slideflow, recalled: parsed in macenko_fit only)
MACENKO_KEY_HE, MACENKO_KEY_MAXC = 'stain_matrix_target', 'target_concentrations'
# per-tile status of the Macenko kernel: a tile whose status is not OK passes through unchanged
STAIN_OK, STAIN_FEW_TISSUE, STAIN_SINGULAR, STAIN_NONFINITE = 0, 1, 2, 3


def macenko_fit(norm_fit):
    """(HE float32 [3,2], maxC float32 [2]) of a Macenko ``norm_fit``; ValueError when a key is missing, a shape is wrong, a value
    is not finite or a concentration is not > 0."""
    if not isinstance(norm_fit, dict) or MACENKO_KEY_HE not in norm_fit or MACENKO_KEY_MAXC not in norm_fit:
        raise ValueError(f"a macenko norm_fit needs {MACENKO_KEY_HE!r} (3x2) and {MACENKO_KEY_MAXC!r} (2)")
    try:
        he = np.asarray(norm_fit[MACENKO_KEY_HE], dtype=np.float64)
        maxc = np.asarray(norm_fit[MACENKO_KEY_MAXC], dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f'macenko norm_fit: {e}') from None
    if he.shape != (3, 2) or maxc.shape != (2,):
        raise ValueError(f'macenko norm_fit: {MACENKO_KEY_HE} must be 3x2 and {MACENKO_KEY_MAXC} 2 values, '
                         f'not {he.shape} and {maxc.shape}')
    if not (np.isfinite(he).all() and np.isfinite(maxc).all()):
        raise ValueError('macenko norm_fit: non-finite value')
    if not (maxc > 0).all():
        raise ValueError(f'macenko norm_fit: {MACENKO_KEY_MAXC} must be > 0')
    return he.astype(np.float32), maxc.astype(np.float32)


def reinhard_fit(norm_fit):
    """(target_means, target_stds), float32 [3] each, of a reinhard_fast ``norm_fit``; ValueError when they are missing, are not three
    numbers each or hold a value that is not finite in float32.  A std of 0 (every pixel becomes the target mean's colour) or below
    is legal: defined arithmetic."""
    if not isinstance(norm_fit, dict) or 'target_means' not in norm_fit or 'target_stds' not in norm_fit:
        raise ValueError("a reinhard_fast norm_fit needs 'target_means' and 'target_stds'")
    try:
        with np.errstate(over='ignore'):
            means = np.asarray(norm_fit['target_means'], dtype=np.float64).astype(np.float32)
            stds = np.asarray(norm_fit['target_stds'], dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f'reinhard_fast norm_fit: {e}') from None
    if means.shape != (3,) or stds.shape != (3,):
        raise ValueError(f'reinhard_fast norm_fit: target_means and target_stds must be 3 values each, not {means.shape} and {stds.shape}')
    if not (np.isfinite(means).all() and np.isfinite(stds).all()):
        raise ValueError('reinhard_fast norm_fit: non-finite value')
    return means, stds


def check(normalizer, norm_fit):
    """Validate a (normalizer, norm_fit) pair as the drivers take it: ``norm_fit=None`` is no normaliser whatever the name;
    an unknown name or a fit of another method raises ValueError."""
    if norm_fit is None:
        return
    if normalizer in REINHARD_FLAGS:
        reinhard_fit(norm_fit)
    elif normalizer == 'macenko':
        macenko_fit(norm_fit)
    else:
        raise ValueError(f'normalizer must be one of {METHODS}, not {normalizer!r}')


def normalise(engine, tiles, normalizer, norm_fit, out=None, status=None):
    """The stain normaliser of a model in front of the staging kernel: uint8 NHWC tiles on the engine's device -> normalised
    tiles (``out`` may be ``tiles``: in place).  ``norm_fit=None``: no normaliser, ``tiles`` is returned as it is.  ``status``
    (int32 [n], the methods of STATUS_METHODS only; optional) receives the per-tile status (STAIN_* for Macenko, REINHARD_* for
    the Reinhard family; 0 is a normalised tile in both)."""
    if norm_fit is None:
        return tiles
    if normalizer == 'reinhard_fast':
        means, stds = reinhard_fit(norm_fit)
        return engine.reinhard_fast(tiles, means, stds, out=out)
    if normalizer in REINHARD_FLAGS:
        means, stds = reinhard_fit(norm_fit)
        return engine.reinhard(tiles, means, stds, REINHARD_FLAGS[normalizer], REINHARD_MASK_THRESHOLD, out=out, status=status)
    if normalizer == 'macenko':
        he, maxc = macenko_fit(norm_fit)
        return engine.macenko(tiles, he, maxc, out=out, status=status)
    raise ValueError(f'normalizer must be one of {METHODS}, not {normalizer!r}')


def make_normalizer(engine, normalizer, norm_fit):
    """The ``wsi_normalizer`` object of a (normalizer, norm_fit) pair, None for no normaliser."""
    check(normalizer, norm_fit)
    if norm_fit is None:
        return None
    if normalizer == 'macenko':
        he, maxc = macenko_fit(norm_fit)
        return Macenko(engine, he, maxc)
    cls = {'reinhard': Reinhard, 'reinhard_mask': ReinhardMask, 'reinhard_fast_mask': ReinhardFastMask}.get(normalizer, ReinhardFast)
    return cls(engine, *reinhard_fit(norm_fit))


class ReinhardFast:
    method = 'reinhard_fast'

    def __init__(self, engine, target_means=None, target_stds=None):
        self.engine = engine
        self.target_means = None if target_means is None else np.asarray(target_means, np.float32).reshape(3)
        self.target_stds = None if target_stds is None else np.asarray(target_stds, np.float32).reshape(3)

    @classmethod
    def from_params(cls, engine, params):
        """``params``: dict or path of a Slideflow params.json holding ``norm_fit``."""
        if not isinstance(params, dict):
            with open(params) as f:
                params = json.load(f)
        fit = params.get('norm_fit')
        if not fit or 'target_means' not in fit or 'target_stds' not in fit:
            raise ValueError("params.json has no norm_fit with target_means / target_stds")
        return cls(engine, *reinhard_fit(fit))

    def _as_batch(self, image):
        t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        if t.dtype != torch.uint8:
            raise TypeError('stain normalisation takes uint8 RGB')
        single = t.dim() == 3
        t = t.unsqueeze(0) if single else t
        if tuple(t.shape[1:]) != (TILE_PX, TILE_PX, 3):
            raise ValueError(f'expected [n,{TILE_PX},{TILE_PX},3] uint8 tiles, got {tuple(t.shape)}')
        return t.to(self.engine.device).contiguous(), single

    def fit(self, target):
        """Fit to one target tile [299,299,3] uint8: stores its CIE-LAB channel means / stds."""
        t, _ = self._as_batch(target)
        st = self.engine.lab_stats(t[:1]).cpu().numpy()[0]
        self.target_means, self.target_stds = st[:3].copy(), st[3:].copy()
        return self

    def get_fit(self):
        return {'target_means': self.target_means.tolist(), 'target_stds': self.target_stds.tolist()}

    def rgb_to_rgb(self, image):
        if self.target_means is None:
            raise RuntimeError('normaliser is not fitted (fit() or from_params())')
        t, single = self._as_batch(image)
        out = self.engine.reinhard_fast(t, self.target_means, self.target_stds)
        return out[0] if single else out


class Reinhard(ReinhardFast):
    """Slideflow's ``normalizer='reinhard'``: ``reinhard_fast`` after a brightness standardisation of the tile (and of the target
    it is fitted to).  The fit has ``reinhard_fast``'s keys.  Tiles of any square size the kernel takes (1..1024 px)."""
    method = 'reinhard'
    mask_threshold = REINHARD_MASK_THRESHOLD

    @property
    def flags(self):
        return REINHARD_FLAGS[self.method]

    def _as_batch(self, image):
        t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        if t.dtype != torch.uint8:
            raise TypeError('stain normalisation takes uint8 RGB')
        single = t.dim() == 3
        t = t.unsqueeze(0) if single else t
        if t.dim() != 4 or t.shape[3] != 3 or t.shape[1] != t.shape[2] or not 1 <= t.shape[1] <= 1024:
            raise ValueError(f'expected [n,px,px,3] uint8 tiles with 1 <= px <= 1024, got {tuple(t.shape)}')
        return t.to(self.engine.device).contiguous(), single

    def fit(self, target):
        """Fit to one square target tile [px,px,3] uint8: stores the CIE-LAB channel means / stds of its tissue pixels after the
        brightness stage, whichever of the two the method has (ValueError for a target that is too dark or has no tissue)."""
        t, _ = self._as_batch(target)
        stats, st = self.engine.reinhard_stats(t[:1], self.flags, self.mask_threshold)
        status = int(st[0])
        if status != REINHARD_OK:
            raise ValueError(f'the target tile is degenerate for {self.method} (status {status}: '
                             f'{"no tissue pixel" if status == REINHARD_NO_TISSUE else "too dark to standardise"})')
        s = stats.cpu().numpy()[0]
        self.target_means, self.target_stds = s[:3].copy(), s[3:6].copy()
        return self

    def rgb_to_rgb(self, image):
        if self.target_means is None:
            raise RuntimeError('normaliser is not fitted (fit() or from_params())')
        t, single = self._as_batch(image)
        out = self.engine.reinhard(t, self.target_means, self.target_stds, self.flags, self.mask_threshold)
        return out[0] if single else out


class ReinhardMask(Reinhard):
    """Slideflow's ``normalizer='reinhard_mask'``: ``reinhard`` with the statistics and the transform over the tissue pixels only
    (L below 100 * mask_threshold after the brightness stage); the others keep the brightness stage's bytes."""
    method = 'reinhard_mask'


class ReinhardFastMask(Reinhard):
    """Slideflow's ``normalizer='reinhard_fast_mask'``: ``reinhard_mask`` without the brightness stage."""
    method = 'reinhard_fast_mask'


class Macenko(ReinhardFast):
    """Slideflow's ``normalizer='macenko'`` (the object ``wsi_normalizer`` is for such a model): the fit is the target's stain
    matrix HE (3x2, columns H and E) and its 99th-percentile concentrations maxC.  The kernel computes every tile's own HE and
    maxC and maps its concentrations onto the fit; a degenerate tile (no tissue, one colour) passes through unchanged."""
    method = 'macenko'

    def __init__(self, engine, stain_matrix=None, concentrations=None):
        self.engine = engine
        self.stain_matrix, self.concentrations = None, None
        if stain_matrix is not None:
            self.stain_matrix, self.concentrations = macenko_fit({MACENKO_KEY_HE: stain_matrix, MACENKO_KEY_MAXC: concentrations})

    @classmethod
    def preset(cls, engine):
        """The default fit (HEnorm_python's HERef / maxCRef)."""
        return cls(engine, MACENKO_HE_REF, MACENKO_MAXC_REF)

    @classmethod
    def from_params(cls, engine, params):
        """``params``: dict or path of a Slideflow params.json holding a Macenko ``norm_fit``."""
        if not isinstance(params, dict):
            with open(params) as f:
                params = json.load(f)
        he, maxc = macenko_fit(params.get('norm_fit'))
        return cls(engine, he, maxc)

    def fit(self, target):
        """Fit to one target tile [299,299,3] uint8: stores its HE and maxC (ValueError for a degenerate target)."""
        t, _ = self._as_batch(target)
        stats, st = self.engine.macenko_stats(t[:1])
        status = int(st[0, 0])
        if status != STAIN_OK:
            raise ValueError(f'the target tile is degenerate for Macenko (status {status})')
        s = stats.cpu().numpy()[0].astype(np.float64)
        self.stain_matrix, self.concentrations = macenko_fit({MACENKO_KEY_HE: s[:6].reshape(3, 2), MACENKO_KEY_MAXC: s[6:]})
        return self

    def get_fit(self):
        return {MACENKO_KEY_HE: self.stain_matrix.tolist(), MACENKO_KEY_MAXC: self.concentrations.tolist()}

    def rgb_to_rgb(self, image):
        if self.stain_matrix is None:
            raise RuntimeError('normaliser is not fitted (fit(), from_params() or preset())')
        t, single = self._as_batch(image)
        out = self.engine.macenko(t, self.stain_matrix, self.concentrations)
        return out[0] if single else out
