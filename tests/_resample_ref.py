"""Pillow's 8-bit LANCZOS resampler restated in numpy, and the case matrix the resampling tests share.

The restatement follows Pillow's ``src/libImaging/Resample.c``: coefficients in float64 with ``math.sin``, rounded to 22
fractional bits away from zero; a pass is ``(2**21 + sum coef * byte) >> 22`` clipped to 0..255; the horizontal pass runs first
and is rounded to uint8, the vertical pass runs over its result."""
import math

import numpy as np

WIDTHS = (150, 299, 300, 302, 303, 450, 598, 604, 1190, 1225)
PX = 299
BITS = 22


def _lanczos(x):
    if not (-3.0 <= x < 3.0):
        return 0.0

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3)


def taps_ref(src, px):
    """(bounds int32 [px, 2], coef int32 [px, ksize])"""
    scale = src / px
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((px, 2), np.int32)
    coef = np.zeros((px, ksize), np.int32)
    for xx in range(px):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), src) - xmin
        k = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            coef[xx, x] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coef


def _pass(img, bounds, coef):
    """Resample axis 1 of img [rows, src, 3] -> [rows, px, 3]."""
    out = np.empty((img.shape[0], bounds.shape[0], 3), np.uint8)
    a = img.astype(np.int64)
    for x, (first, count) in enumerate(bounds):
        acc = (a[:, first:first + count] * coef[x, :count].astype(np.int64)[None, :, None]).sum(1) + (1 << (BITS - 1))
        out[:, x] = np.clip(acc >> BITS, 0, 255)
    return out


def resize_ref(img, px=PX):
    """uint8 [src, src, 3] -> uint8 [px, px, 3]"""
    if img.shape[0] == px:
        return img.copy()
    bounds, coef = taps_ref(img.shape[0], px)
    h = _pass(img, bounds, coef)
    return _pass(h.transpose(1, 0, 2), bounds, coef).transpose(1, 0, 2)


def case(src, seed=None):
    """(canvas uint8 [H, W, 3], origin int32 [n, 2]): a random canvas with a flat 255 and a flat 0 area that holds two
    overlapping windows of ``src`` pixels, and origins inside it, overlapping, partly outside on each side and wholly outside."""
    rng = np.random.default_rng(1000 + src if seed is None else seed)
    H, W = src + 37, src + src // 2 + 21
    canvas = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    canvas[: H // 5, : W // 2] = 255
    canvas[-(H // 6):, W // 3:] = 0
    origin = np.array([[0, 0], [src // 2, 11], [W - src, H - src],          # inside, overlapping
                       [-7, 5], [9, -13], [W - src + 5, 3], [4, H - src + 9], [-(src // 3), -(src // 4)],   # partly outside
                       [W + 3, 2], [-src - 1, -src - 1]], np.int32)          # wholly outside
    return canvas, origin


def pillow_tiles(canvas, origin, src, px=PX):
    """What Pillow gives for every window: cut from a white-padded copy of the canvas, ``resize((px, px), LANCZOS)``."""
    from PIL import Image
    H, W = canvas.shape[:2]
    pad = 2 * src + 8
    big = np.full((H + 2 * pad, W + 2 * pad, 3), 255, np.uint8)
    big[pad:pad + H, pad:pad + W] = canvas
    out = np.empty((len(origin), px, px, 3), np.uint8)
    for i, (x, y) in enumerate(origin):
        win = big[pad + y:pad + y + src, pad + x:pad + x + src]
        assert win.shape == (src, src, 3)
        out[i] = win if src == px else np.asarray(Image.fromarray(win).resize((px, px), Image.LANCZOS))
    return out


def uneven_slide_geometry():
    """A slide read from its 4 x level whose grid does not fall on whole level pixels and whose last window leaves the level
    by a pixel: searched over MPP and width with ``wsi.WSI``'s own arithmetic.  -> (mpp, width, extract_px) or None."""
    for i in range(400):
        mpp = round(0.2400 + i * 0.0001, 4)
        e = int(302 / mpp)
        for w in range(2 * e, 2 * e + 8):
            lw = w // 4
            ds = w / lw
            if ds > (e / PX) * 1.0001:
                continue
            src = max(1, int(round(e / ds)))
            x1 = int(round(e / ds))
            if x1 + src - lw >= 1 and abs(e / ds - round(e / ds)) > 0.2:
                return mpp, w, e
    return None
