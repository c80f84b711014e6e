"""The rule of csrc/canvas_place.h -- exactly the pixels of a segment inside both the canvas and the clip rectangle are written --
held over both CPU canvas decoders (``tfrecord_native.jpeg_decode_canvas``, ``tfrecord_native.j2k_decode_canvas``) against a
numpy restatement, over the grid of places and rectangles of tests/_canvas_place_cases.py.  A pixel counts as written where the
decode into a canvas of 0 and the decode into a canvas of 255 agree.  The device decoders are held to these canvases byte for
byte in tests/test_gpu_canvas_place.py."""
import numpy as np
import pytest

from biscuit_amd import tfrecord_native as tn
from tests import _canvas_place_cases as cp

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


@pytest.mark.parametrize('codec', cp.CODECS)
def test_the_content_shows_what_is_written(codec):
    """No decoded sample is 0 or 255, so a written pixel differs from both fills and the two decodes can only agree on it."""
    src = cp.source(codec)
    assert src.shape == (cp.SEG, cp.SEG, 3) and src.min() > 0 and src.max() < 255
    assert (cp.W * 3) % 2 == 1


def _written(codec, pi, ci):
    a, b = cp.cpu_canvases(codec)[pi, ci, 0], cp.cpu_canvases(codec)[pi, ci, 255]
    same = a == b
    assert (same.all(-1) == same.any(-1)).all(), 'a pixel written in part'
    assert (a[~same.all(-1)] == 0).all() and (b[~same.all(-1)] == 255).all(), 'an unwritten pixel changed'
    return same.all(-1)


@pytest.mark.parametrize('ci', range(len(cp.CLIPS)), ids=lambda ci: 'clip%d' % ci)
def test_both_decoders_write_exactly_the_window(ci):
    clip = cp.CLIPS[ci]
    for pi, place in enumerate(cp.PLACES):
        want = cp.window(place, clip)
        written = {codec: _written(codec, pi, ci) for codec in cp.CODECS}
        assert np.array_equal(written['jpeg'], written['j2k']), (place, clip)
        assert np.array_equal(written['jpeg'], want), (place, clip)
        ys, xs = np.nonzero(want)                                       # and what is written is the segment's pixel (y - py, x - px)
        for codec in cp.CODECS:
            assert np.array_equal(cp.cpu_canvases(codec)[pi, ci, 255][ys, xs], cp.source(codec)[ys - place[1], xs - place[0]]), (codec, place, clip)


def test_the_grid_reaches_every_kind_of_window():
    """Of the grid: whole segments, windows cut on each side, single pixels and empty windows all occur."""
    counts = {int(cp.window(p, c).sum()) for p in cp.PLACES for c in cp.CLIPS}
    assert {0, 1, cp.SEG * cp.SEG} <= counts and len(counts) > 8
