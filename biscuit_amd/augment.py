"""Training augmentation: Slideflow's ``augment='xyrjb'`` (``biscuit/hp.py:23``) as a table of per-tile draws and a device call
(DESIGN.md section 7 "Training augmentation").

A tile's augmentation is four bytes ``(k, flips, quality, blur)`` -- ``PARAM_COLUMNS`` -- that ``Engine.augment`` (``bq_augment``,
csrc/kernels_augment.hip) and ``apply_host`` (``bqio_augment``: the same routines, csrc/augment_device.h, on the CPU) turn into
pixels: ``blur(flip_ud(flip_lr(rot90^k(jpeg_quality(tile)))))``.  ``draw`` makes the table for a whole cohort on the host, so that a
tile's draw is a function of ``(seed, view, its row)`` alone, whatever the batching.

Restated from memory, unpinned against Slideflow's ``process_image``: the order j, r, x, y, b; JPEG with probability 0.5 at a
quality uniform in 50..100 (``tf.image.random_jpeg_quality``); blur with probability 0.1 and its choice of sigma; TensorFlow's
libjpeg settings and tfa's rounding.  Pinned: Pillow's pixels for ``j``, numpy for ``r``, ``x``, ``y``, the integer statement and
scipy for ``b`` (tests/test_augment.py).  Out of scope: Slideflow's stain augmentation ``n``."""
import numpy as np

LETTERS = 'xyrjb'
PARAM_COLUMNS = ('k', 'flips', 'quality', 'blur')     # rot90 count 0..3; bit 0 = x[:, ::-1], bit 1 = x[::-1]; 0 / 1..100; 0 / 1..4
JPEG_P, JPEG_QUALITY = 0.5, (50, 100)
BLUR_P = 0.1
BLUR_CDF = (0.5, 0.75, 0.875)             # index 1, 2, 3, 4 (sigma = 0.5 index) with probabilities 1/2, 1/4, 1/8, 1/8
MIN_PX, MAX_PX = 8, 4096


def parse(spec):
    """The letters of ``spec`` in ``LETTERS``' order, each once: any order and repeats are taken, ``''`` / None mean none; ValueError
    for any other character."""
    spec = '' if spec is None else str(spec)
    bad = sorted(set(spec) - set(LETTERS))
    if bad:
        raise ValueError(f'augment {spec!r}: unknown letter(s) {"".join(bad)!r}; the augmenter takes letters out of {LETTERS!r}')
    return ''.join(c for c in LETTERS if c in spec)


def _rng(seed, view, letter, second=False):
    """A letter's stream; its second quantity (j's quality, b's sigma) has a stream of its own, so that row i of either does not
    depend on how many rows are drawn."""
    return np.random.default_rng([int(seed), int(view), ord(letter)] + ([1] if second else []))


def draw(n, spec, seed, view):
    """The parameter table uint8 [n, 4] (``PARAM_COLUMNS``) of ``n`` tiles under ``spec`` for ``(seed, view)``.  Every letter draws
    from its own stream ``numpy.random.default_rng([seed, view, ord(letter)])`` for all rows at once: row i is tile i's draw
    whatever n and the batching, and enabling one letter does not change another's draws."""
    letters, n = parse(spec), int(n)
    out = np.zeros((n, 4), np.uint8)
    if 'r' in letters:
        out[:, 0] = _rng(seed, view, 'r').integers(0, 4, n)
    if 'x' in letters:
        out[:, 1] |= (_rng(seed, view, 'x').random(n) < 0.5).astype(np.uint8)
    if 'y' in letters:
        out[:, 1] |= (_rng(seed, view, 'y').random(n) < 0.5).astype(np.uint8) << 1
    if 'j' in letters:
        on = _rng(seed, view, 'j').random(n) < JPEG_P
        quality = _rng(seed, view, 'j', True).integers(JPEG_QUALITY[0], JPEG_QUALITY[1] + 1, n)
        out[:, 2] = np.where(on, quality, 0)
    if 'b' in letters:
        on = _rng(seed, view, 'b').random(n) < BLUR_P
        index = 1 + np.searchsorted(BLUR_CDF, _rng(seed, view, 'b', True).random(n), side='right')
        out[:, 3] = np.where(on, index, 0)
    return out


def check_params(params, n=None):
    """``params`` as a contiguous uint8 [n, 4] host array; ValueError for another shape or a byte out of range."""
    p = np.asarray(params)
    if p.ndim != 2 or p.shape[1] != 4 or (n is not None and p.shape[0] != n):
        raise ValueError(f'augmentation parameters are uint8 [n, 4] {PARAM_COLUMNS}, not {p.shape}')
    if p.size and (p.min() < 0 or (p.max(axis=0) > (3, 3, 100, 4)).any()):
        raise ValueError('an augmentation parameter outside k 0..3, flips 0..3, quality 0..100, blur 0..4')
    return np.ascontiguousarray(p, np.uint8)


def apply_host(tiles, params, threads=None):
    """uint8 [n, px, px, 3] and the table [n, 4] -> ``(augmented tiles, status int32 [n])`` on the CPU (``bqio_augment``): what
    ``Engine.augment`` computes, byte for byte.  ValueError for what the library refuses (px outside 8..4096, a byte out of range)."""
    from . import tfrecord_native as tn
    tiles = np.ascontiguousarray(tiles, np.uint8)
    if tiles.ndim != 4 or tiles.shape[1] != tiles.shape[2] or tiles.shape[3] != 3:
        raise ValueError(f'tiles are uint8 [n, px, px, 3], not {tiles.shape}')
    n, px = tiles.shape[0], tiles.shape[1]
    params = np.ascontiguousarray(params, np.uint8)
    if params.shape != (n, 4):
        raise ValueError(f'augmentation parameters are uint8 [{n}, 4], not {params.shape}')
    out, status = np.empty_like(tiles), np.zeros(n, np.int32)
    if tn.lib().bqio_augment(tiles.ctypes.data, n, px, params.ctypes.data, out.ctypes.data, status.ctypes.data,
                             int(threads or tn.default_threads())) != 0:
        raise ValueError(tn.lib().bqio_augment_last_error().decode())
    return out, status


def blur_weights(blur):
    """The library's integer weights of blur index 1..4 (sigma = 0.5 index): int64 [2 r + 1], summing to 65536."""
    from . import tfrecord_native as tn
    w = np.zeros(13, np.uint16)
    r = tn.lib().bqio_augment_blur_weights(int(blur), w.ctypes.data)
    if r < 0:
        raise ValueError(tn.lib().bqio_augment_last_error().decode())
    return w[:2 * r + 1].astype(np.int64)
