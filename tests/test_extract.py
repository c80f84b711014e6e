"""The host side of tile extraction (``biscuit_amd/extract.py``) without a device: the append-style TFRecord writer against
``write_slide``, the ``loc`` arithmetic and the row-major ordering of records that arrive band by band."""
import numpy as np
import pytest

from biscuit_amd import extract
from biscuit_amd import tfrecord as tfr
from tests import _jpeg_encode_cases as ec


def _records(n=9, px=17):
    raws = [ec.pillow(px, ec.CONTENTS[i % len(ec.CONTENTS)], 95, '4:2:0') for i in range(n)]
    locs = np.stack([np.arange(n) * 598 + 299, np.arange(n)[::-1] * 598 + 299], 1).astype(np.int64)
    return raws, locs


def test_append_writer_writes_write_slides_bytes(tmp_path):
    raws, locs = _records()
    a, b = str(tmp_path / 'a.tfrecords'), str(tmp_path / 'b.tfrecords')
    tfr.write_slide(a, 'slide-1', raws, locs)
    with tfr.SlideWriter(b, 'slide-1') as w:
        for raw, (lx, ly) in zip(raws, locs):
            w.write(raw, lx, ly)
            assert w.records * 4 <= w.nbytes
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert w.records == len(raws) and w.nbytes == len(open(b, 'rb').read())
    got = list(tfr.read_records(b, verify='crc'))
    assert got == list(tfr.read_records(b, verify='full')) and len(got) == len(raws)      # length CRCs, then the data CRCs too
    for r, raw, (lx, ly) in zip(map(tfr.parse_example, got), raws, locs):
        assert r['image_raw'] == raw and r['slide'] == b'slide-1' and (r['loc_x'], r['loc_y']) == ([lx], [ly])


def test_an_empty_slide_is_an_empty_file(tmp_path):
    p = str(tmp_path / 'e.tfrecords')
    tfr.SlideWriter(p, 'e').close()
    assert open(p, 'rb').read() == b'' and list(tfr.read_records(p, verify='crc')) == []


def test_loc_is_the_tiles_centre_in_level_0_pixels():
    # the 4 x 3 grid of the 2400 x 1800 test slide at 0.5045 um / pixel: extract_px = stride = 598
    loc = extract.tile_loc(np.arange(12), 4, 598, 598)
    assert loc.dtype == np.int64 and loc.shape == (12, 2)
    assert loc[0].tolist() == [299, 299] and loc[3].tolist() == [3 * 598 + 299, 299] and loc[4].tolist() == [299, 598 + 299]
    assert loc[11].tolist() == [3 * 598 + 299, 2 * 598 + 299]
    # stride_div = 2: stride 299, an odd extract_px rounds down
    assert extract.tile_loc([9], 7, 299, 599).tolist() == [[2 * 299 + 299, 1 * 299 + 299]]
    assert extract.tile_loc([], 7, 299, 599).shape == (0, 2)


def test_records_leave_in_row_major_order_whatever_the_banding():
    """A 6 x 4 grid read as two bands of two rows, each split into column ranges 0..3 and 4..5, in batches of 5 that straddle
    the rectangles: the writer sees the cells 0..23 in order, and never holds more than the bands in flight."""
    gw = 6
    rects = [(0, 2, 0, 4), (0, 2, 4, 6), (2, 4, 0, 4), (2, 4, 4, 6)]
    stream = [(gy * gw + gx, r[0]) for r in rects for gy in range(r[0], r[1]) for gx in range(r[2], r[3])]
    assert [c for c, _ in stream] != sorted(c for c, _ in stream)
    seen, held = [], []
    order = extract.RowMajor(lambda cell, image: seen.append((cell, image)))
    for a in range(0, len(stream), 5):
        part = stream[a:a + 5]
        order.add([c for c, _ in part], [b'f%d' % c for c, _ in part], part[-1][1] * gw)
        held.append(len(order.pending))
    order.flush()
    assert seen == [(c, b'f%d' % c) for c in range(24)] and not order.pending
    assert max(held) <= 12 + 5                           # one band's cells (+ a batch), not the slide's 24


def test_quality_and_subsampling_are_checked_before_the_slide_is_opened(tmp_path):
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling='4:2:2'), dict(decode='cpu'), dict(qc='blur')):
        with pytest.raises(ValueError):
            extract.extract_slide(None, str(tmp_path / 'missing.svs'), str(tmp_path), **kw)
    assert not list(tmp_path.iterdir())
