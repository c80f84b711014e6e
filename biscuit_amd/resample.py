"""Host side of the heatmap's input stage (DESIGN.md "Heatmap input"): the tap tables of Pillow's LANCZOS resampler
(``bqio_resample_taps``), the CPU restatement of the tile resampler (``bqio_tile_resample``) and the table of the background
filter.  The device side is ``Engine.tile_resample`` / ``Engine.tile_grayspace`` (csrc/kernels_resample.hip)."""
import numpy as np

from . import tfrecord_native

MIN_RATIO, MAX_RATIO = 1 / 8, 8             # px / 8 <= src_px <= 8 px (include/biscuit_io.h)


class ResampleError(ValueError):
    pass


def ksize(src_px, px):
    """Taps per output coordinate for ``src_px`` -> ``px``; ResampleError outside the supported range."""
    k = tfrecord_native.lib().bqio_resample_ksize(int(src_px), int(px))
    if k < 0:
        raise ResampleError(f'resampling {src_px} -> {px} px is outside the supported range (0 < px <= 4096, px / 8 <= src_px <= 8 px)')
    return int(k)


def taps(src_px, px):
    """(bounds int32 [px, 2] = first source coordinate and number of taps, coef int32 [px, ksize] with 22 fractional bits):
    Pillow's coefficient tables for ``Image.resize((px, px), Image.LANCZOS)`` of a ``src_px`` wide image."""
    k = ksize(src_px, px)
    bounds = np.zeros((px, 2), np.int32)
    coef = np.zeros((px, k), np.int32)
    e = tfrecord_native.lib().bqio_resample_taps(int(src_px), int(px), bounds.ctypes.data, coef.ctypes.data, k)
    if e != k:
        raise ResampleError(f'bqio_resample_taps({src_px}, {px}): error {e}')
    return bounds, coef


def tile_resample(canvas, origin, src_px, px=299):
    """The CPU restatement of ``Engine.tile_resample``: canvas uint8 [H, W, 3], origin int32 [n, 2] of (x, y) -> uint8
    [n, px, px, 3], the bytes Pillow's LANCZOS gives for each ``src_px`` window (255 outside the canvas)."""
    canvas = np.ascontiguousarray(canvas, np.uint8)
    origin = np.ascontiguousarray(origin, np.int32).reshape(-1, 2)
    if canvas.ndim != 3 or canvas.shape[2] != 3:
        raise ValueError('canvas must be uint8 [H, W, 3]')
    n = origin.shape[0]
    out = np.empty((n, max(int(px), 0), max(int(px), 0), 3), np.uint8)
    e = tfrecord_native.lib().bqio_tile_resample(canvas.ctypes.data, canvas.shape[0], canvas.shape[1], origin.ctypes.data, n,
                                                 int(src_px), int(px), out.ctypes.data)
    if e != 0:
        raise ResampleError(f'bqio_tile_resample({src_px} -> {px}, n = {n}): error {e}')
    return out


def grayspace_limit(threshold):
    """int32 [256]: ``limit[mx]`` = the smallest ``mx - mn`` that is NOT grey under the float64 definition ``s = 0 if mx == 0 else
    (mx - mn) / mx; grey iff s < threshold`` (``mx + 1`` when every difference is grey), so that a pixel is grey iff
    ``mx - mn < limit[mx]``: the table ``Engine.tile_grayspace`` compares against."""
    t = float(threshold)
    if not np.isfinite(t):
        raise ValueError('grayspace_threshold must be finite')
    limit = np.zeros(256, np.int32)
    limit[0] = 1 if 0.0 < t else 0
    for mx in range(1, 256):
        d = 0
        while d <= mx and d / mx < t:
            d += 1
        limit[mx] = d
    return limit


def grayspace_count(tiles, threshold):
    """Grey pixels per tile by the float64 definition (numpy; the reference of the kernel): tiles uint8 [n, h, w, 3] -> int64 [n]."""
    t = np.asarray(tiles)
    mx = t.max(-1).astype(np.float64)
    mn = t.min(-1).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(mx == 0, 0.0, (mx - mn) / np.where(mx == 0, 1.0, mx))
    return (s < float(threshold)).reshape(t.shape[0], -1).sum(1)
