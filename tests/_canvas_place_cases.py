"""Shared by tests/test_canvas_place.py (CPU) and tests/test_gpu_canvas_place.py: one 16 x 16 segment per codec, the grid of
places and clip rectangles both canvas decoders are held to, the CPU decoders' canvases over that grid (computed once), and the
window rule of csrc/canvas_place.h restated in canvas coordinates with Python's unbounded integers."""
import functools

import numpy as np

from biscuit_amd import tfrecord_native as tn
from tests import _j2k_cases as jc
from tests import _wsi_jpeg_cases as wj

SEG = 16
H, W = 20, 23                                # the pitch 3 W = 69 is odd
BIG = 2 ** 31
# inside; cut on the left, right, top, bottom; wholly outside on each side; the ends of int32, for the 64-bit sums
PLACES = [(3, 2), (-5, 2), (15, 2), (3, -7), (3, 10), (-16, 2), (23, 2), (3, -16), (3, 20), (-BIG, -BIG), (BIG - 1, BIG - 1)]
# the whole canvas; one pixel; empty (x1 == x0, x1 < x0); larger than the canvas; negative corners, and the ends of int32
CLIPS = [(0, 0, W, H), (5, 4, 6, 5), (8, 3, 8, 12), (9, 3, 7, 12), (-10, -10, 100, 100), (-BIG, -BIG, 12, 9), (4, 5, BIG - 1, BIG - 1)]
CODECS = ('jpeg', 'j2k')


def _content():
    """Smooth and mid-range, so that neither codec decodes a sample to 0 or 255 (the tests assert it)."""
    yy, xx = np.mgrid[0:SEG, 0:SEG]
    return np.stack([70 + 6 * xx, 180 - 5 * yy, 90 + 3 * xx + 2 * yy], -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def packed(codec):
    """What the codec's extractor packs for the one segment: the arrays its canvas decoders take first."""
    raw = wj.jpeg(_content(), subsampling=wj.SAMPLINGS['420']) if codec == 'jpeg' else jc.encode(_content(), False, num_resolutions=2, mct=1)
    data = np.frombuffer(raw, np.uint8)
    if codec == 'jpeg':
        return tn.extract_jpeg_segments(data, [0], [len(raw)], SEG, SEG)
    return tn.j2k_extract(data, [0], [len(raw)], SEG, SEG)


def cpu_decode(codec, place, clip, fill, shape=(H, W)):
    """The CPU canvas decoder of ``codec`` over a canvas of ``fill`` -> the canvas; the one segment decodes (status 0)."""
    canvas = np.full(tuple(shape) + (3,), fill, np.uint8)
    status = (tn.jpeg_decode_canvas if codec == 'jpeg' else tn.j2k_decode_canvas)(*packed(codec), SEG, SEG, [place], canvas, clip)
    assert status.tolist() == [0]
    return canvas


@functools.lru_cache(maxsize=None)
def source(codec):
    """The segment's own pixels as the codec decodes them, uint8 [16, 16, 3]."""
    return cpu_decode(codec, (0, 0), (0, 0, SEG, SEG), 0, (SEG, SEG))


@functools.lru_cache(maxsize=None)
def cpu_canvases(codec):
    """(place index, clip index, fill) -> the CPU decoder's canvas, over the whole grid and fills 0 and 255; read-only."""
    out = {}
    for pi, place in enumerate(PLACES):
        for ci, clip in enumerate(CLIPS):
            for fill in (0, 255):
                out[pi, ci, fill] = cpu_decode(codec, place, clip, fill)
                out[pi, ci, fill].flags.writeable = False
    return out


def window(place, clip):
    """bool [H, W]: the canvas pixels the rule says are written -- those inside the canvas, the clip and the segment's square."""
    x0, y0 = max(clip[0], 0, place[0]), max(clip[1], 0, place[1])
    x1, y1 = min(clip[2], W, place[0] + SEG), min(clip[3], H, place[1] + SEG)
    mask = np.zeros((H, W), bool)
    if x1 > x0 and y1 > y0:
        mask[y0:y1, x0:x1] = True
    return mask
