"""The baseline-JPEG encoder's definition (csrc/jpeg_encode_device.h) on the CPU (``bqio_jpeg_encode``) against the bytes Pillow
(libjpeg-turbo) writes: complete files, byte for byte, over tests/_jpeg_encode_cases.py.  The GPU kernels are compiled from the
same header and held to this build in tests/test_gpu_jpeg_encode.py."""
import numpy as np
import pytest

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from tests import _jpeg_encode_cases as ec

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


def encode(names, px, q, s, cap=None):
    tiles = np.stack([ec.tile(px, w) for w in names])
    return tn.jpeg_encode(tiles, q, s, cap=cap)


@pytest.mark.parametrize('px', ec.SIZES)
def test_pillows_files_byte_for_byte(px):
    """Every content x quality x subsampling; the contents of one size stand side by side in one call (299: three at most), so
    this also says that a tile's file does not depend on its neighbours, and that the offsets are exact."""
    for q, s in ec.settings():
        for names in ec.batches(px):
            buf, off, status = encode(names, px, q, s)
            want = [ec.pillow(px, w, q, s) for w in names]
            assert off[0] == 0 and np.array_equal(np.diff(off), [len(w) for w in want]), (px, q, s, names)
            assert len(buf) == off[-1] and not status.any()
            for w, got, ref in zip(names, ec.split(buf, off), want):
                assert got == ref, (px, q, s, w)


def test_single_tile_calls_equal_the_batch():
    for q, s in ((95, '4:2:0'), (100, '4:4:4')):
        buf, off, _ = encode(ec.CONTENTS, 33, q, s)
        for w, got in zip(ec.CONTENTS, ec.split(buf, off)):
            one, off1, _ = encode([w], 33, q, s)
            assert one.tobytes() == got and list(off1) == [0, len(got)]


@pytest.mark.parametrize('px', ec.SIZES)
def test_header(px):
    """SOI through the SOS header depends on (px, q, s) only: Pillow's first bytes for any content."""
    for q, s in ec.settings():
        h = tn.jpeg_encode_header(px, q, s)
        assert len(h) == 623
        assert ec.pillow(px, 'noise', q, s)[:623] == h and ec.pillow(px, 'grey', q, s)[:623] == h, (px, q, s)
    # the layout: marker, segment length
    h = tn.jpeg_encode_header(px)
    p, seen = 2, []
    while p < len(h):
        seen.append((h[p + 1], (h[p + 2] << 8) | h[p + 3]))
        p += 2 + seen[-1][1]
    assert h[:2] == b'\xff\xd8' and p == 623
    assert seen == [(0xE0, 16), (0xDB, 67), (0xDB, 67), (0xC0, 17), (0xC4, 31), (0xC4, 181), (0xC4, 31), (0xC4, 181), (0xDA, 12)]


def test_defaults_are_the_tfrecord_writers():
    """quality 95 at 4:2:0 is what tfrecord.encode_image(tile, 'JPEG') writes today."""
    t = ec.tile(299, 'synthetic')
    buf, off, _ = tn.jpeg_encode(t[None])
    assert buf.tobytes() == tfr.encode_image(t, 'JPEG')


def test_cap_one_byte_short():
    """Status bit 1 for the last tile only; the earlier files intact; the offsets still exact."""
    names = ['noise', 'gradient', 'checker', 'synthetic']
    full, off, status = encode(names, 33, 95, '4:2:0')
    assert not status.any()
    buf, off2, status2 = encode(names, 33, 95, '4:2:0', cap=int(off[-1]) - 1)
    assert np.array_equal(off2, off) and list(status2) == [0, 0, 0, 1]
    assert buf[:off[3]].tobytes() == full[:off[3]].tobytes()
    assert not buf[off[3]:].any()                        # nothing of the file that does not fit
    # sizing call: no buffer at all
    _, off3, status3 = encode(names, 33, 95, '4:2:0', cap=0)
    assert np.array_equal(off3, off) and status3.all()


@pytest.mark.parametrize('px,q,s', [(8, 0, '4:2:0'), (8, 101, '4:2:0'), (8, 95, '4:2:2'), (8, 95, 1), (0, 95, '4:2:0')])
def test_outside_the_subset_is_refused(px, q, s):
    with pytest.raises(ValueError):
        tn.jpeg_encode(np.zeros((1, px, px, 3), np.uint8), q, s)
    with pytest.raises(ValueError):
        tn.jpeg_encode_header(px, q, s)
    if s in tn.SUBSAMPLING:                              # the library's own refusal, with its reason
        off = np.zeros(2, np.int64)
        assert tn.lib().bqio_jpeg_encode(None, 1, px, q, tn.SUBSAMPLING[s], None, 0, off.ctypes.data, None) == -1
        assert b'subset' in tn.lib().bqio_jpeg_encode_last_error()
    assert tn.lib().bqio_jpeg_encode(None, 1, px, q, 1, None, 0, None, None) == -1


def test_px_4096_is_inside_and_4097_outside():
    assert len(tn.jpeg_encode_header(4096)) == 623
    with pytest.raises(ValueError):
        tn.jpeg_encode_header(4097)


@pytest.mark.parametrize('px', ec.SIZES)
def test_the_readers_decoder_reads_every_file_back(px):
    """bqio_decode_jpeg over the encoder's files: the pixels Pillow decodes from them (a stream outside the reader's subset --
    libjpeg replicates chroma two samples wide instead of filtering -- is one the reader refuses for Pillow's files too)."""
    for q, s in ec.settings():
        for names in ec.batches(px):
            buf, off, _ = encode(names, px, q, s)
            for w, raw in zip(names, ec.split(buf, off)):
                try:
                    got = tn.decode_jpeg(raw, px)
                except tn.UnsupportedImage:
                    assert s == '4:2:0' and px <= 4, (px, q, s, w)
                    continue
                assert np.array_equal(got, ec.pillow_pixels(raw)), (px, q, s, w)
