"""The oracle of tests/test_augment.py and tests/test_gpu_augment.py: the training augmentation (csrc/augment_device.h) restated
with Pillow (``j``), numpy (``r``, ``x``, ``y``) and, for ``b``, the integer statement in numpy beside scipy's float64 filter.  A
parameter row is ``(k, flips, quality, blur)``."""
import io

import numpy as np


def jpeg(tile, quality):
    """Pillow's pixels after a round trip at ``quality`` and 4:2:0; ``quality`` 0: the tile."""
    if quality == 0:
        return np.asarray(tile)
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.asarray(tile)).save(b, 'JPEG', quality=int(quality), subsampling='4:2:0')
    return np.asarray(Image.open(io.BytesIO(b.getvalue())).convert('RGB'))


def dihedral(x, k, flips):
    x = np.rot90(x, int(k))
    if flips & 1:
        x = x[:, ::-1]
    if flips & 2:
        x = x[::-1]
    return x


def weights(blur):
    """int64 [2 r + 1]: floor(65536 g / sum(g) + 0.5) at sigma = 0.5 blur, r = int(3 sigma + 0.5), the centre tap taking what the
    rounding left of 65536."""
    sigma = 0.5 * blur
    r = int(3 * sigma + 0.5)
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * d * d / (sigma * sigma))
    w = np.floor(65536.0 * g / g.sum() + 0.5).astype(np.int64)
    w[r] += 65536 - w.sum()
    return w


def blur_int(img, blur):
    """The integer statement: mirror padding without the edge sample (numpy's 'reflect'), a row pass (sum + 128) >> 8, a column
    pass (sum + 2^23) >> 24."""
    if blur == 0:
        return np.asarray(img)
    w = weights(blur)
    r = len(w) // 2
    px = img.shape[0]
    p = np.pad(np.asarray(img, np.int64), ((0, 0), (r, r), (0, 0)), mode='reflect')
    h = (sum(w[i] * p[:, i:i + px] for i in range(2 * r + 1)) + 128) >> 8
    assert h.max() <= 65280
    p = np.pad(h, ((r, r), (0, 0), (0, 0)), mode='reflect')
    v = (sum(w[i] * p[i:i + px] for i in range(2 * r + 1)) + (1 << 23)) >> 24
    return v.astype(np.uint8)


def blur_scipy(img, blur):
    from scipy.ndimage import gaussian_filter
    s = 0.5 * blur
    return np.rint(gaussian_filter(np.asarray(img, np.float64), (s, s, 0), mode='mirror', truncate=3)).astype(np.uint8)


def compose(tiles, params):
    """blur(flip_ud(flip_lr(rot90^k(jpeg(tile))))) of every tile, uint8 [n, px, px, 3]."""
    return np.stack([blur_int(dihedral(jpeg(t, p[2]), p[0], p[1]), p[3]) for t, p in zip(tiles, np.asarray(params).tolist())])


def composition_table():
    """16 rows in which every letter is active at least once, every quarter turn and both flips occur, row 5 has all active, and
    rows 3 and 8 are all zero."""
    t = np.zeros((16, 4), np.uint8)
    t[:, 0] = [0, 1, 2, 0, 3, 1, 0, 2, 0, 3, 1, 2, 0, 3, 1, 2]
    t[:, 1] = [0, 1, 2, 0, 3, 3, 1, 0, 0, 2, 0, 1, 3, 0, 2, 1]
    t[:, 2] = [50, 0, 75, 0, 100, 60, 0, 1, 0, 95, 0, 83, 0, 50, 0, 0]
    t[:, 3] = [0, 1, 0, 0, 2, 4, 3, 0, 0, 0, 4, 1, 2, 0, 0, 3]
    return t
