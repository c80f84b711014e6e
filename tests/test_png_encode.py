"""The PNG encoder's definition (csrc/png_encode_device.h) on the CPU (``bqio_png_encode``): the filtered rows against the ones
Pillow writes, byte for byte; the deflate stream -- the project's own -- against any conformant decoder (zlib, Pillow, the project's
reader) and against the three size conditions of DESIGN.md "Tile extraction".  The GPU kernels are compiled from the same header and
held to this build, byte for byte, in tests/test_gpu_png_encode.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from tests import _png_encode_cases as pc

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def encode(tiles, cap=None):
    return tn.png_encode(np.stack(tiles), cap=cap)


def size_cap(px):
    """Condition 1: never much larger than raw."""
    L = pc.stream_bytes(px)
    return L + L // 256 + 128


@pytest.fixture(scope='module')
def files299():
    """name -> file, for the 299-px contents (one encode each, shared by the size tests)."""
    out = {}
    for names in pc.batches(299):
        buf, off, status = encode([pc.tile(299, w) for w in names])
        assert not status.any()
        out.update(zip(names, pc.split(buf, off)))
    return out


@pytest.mark.parametrize('px', pc.SIZES)
def test_every_file_is_a_png_with_pillows_rows(px, tmp_path):
    """Every content of every size: the container, the CRCs, the rows Pillow writes, the pixels back through Pillow and through
    the project's own host reader; the contents of one size stand side by side in one call, so the offsets are exact too."""
    raws, tiles = [], []
    for names in pc.batches(px):
        batch = [pc.tile(px, w) for w in names]
        buf, off, status = encode(batch)
        assert off[0] == 0 and len(buf) == off[-1] and not status.any()
        for w, t, raw in zip(names, batch, pc.split(buf, off)):
            pc.check_container(raw, px)
            got = pc.rows(raw)
            assert got == pc.pillow_rows(px, w), (px, w)
            assert set(got[::1 + 3 * px]) <= pc.FILTERS
            assert np.array_equal(pc.pillow_pixels(raw), t), (px, w)
            assert len(raw) <= size_cap(px), (px, w, len(raw))
            raws.append(raw)
            tiles.append(t)
    path = str(tmp_path / 'p.tfrecords')
    tfr.write_slide(path, 'p', raws)
    with tn.NativeReader(path, 'full') as r:
        dec, _ = r.decode(0, len(raws), px)
        filt, _ = r.decode(0, len(raws), px, rows=True)
    assert np.array_equal(dec, np.stack(tiles))
    assert [f.tobytes() for f in filt] == [pc.rows(raw) for raw in raws]


def test_filter_ties_follow_pillow():
    """Sub / Up / Paeth tie below None: Up.  Sub / Paeth alone tie (above zeros the Paeth predictor is the left byte): Sub."""
    for t, want in ((pc.TIE_UP, [0, 2]), (pc.TIE_PAETH, [1, 0, 1])):
        px = t.shape[0]
        buf, off, _ = encode([t])
        got, ref = pc.rows(buf.tobytes()), pc.rows(tfr.encode_image(t, 'PNG'))
        assert list(ref[::1 + 3 * px]) == want                    # what Pillow does, stated
        assert got == ref


def test_never_much_larger_than_raw():
    """Condition 1 where it binds: noise of every size."""
    for px in pc.SIZES:
        buf, off, _ = encode([pc.tile(px, 'noise')])
        assert off[1] <= size_cap(px), (px, off[1])


def test_matching_works_and_reaches_a_row_back(files299):
    """Condition 2: a Huffman code spends a bit per byte, so no match-less coder gets under L / 8; checker and gradient need
    matches about one row (898 bytes) back."""
    L = pc.stream_bytes(299)
    for w in ('zeros', 'grey', 'white', 'corner', 'checker', 'gradient'):
        assert len(files299[w]) < L // 8, (w, len(files299[w]))


def test_natural_tiles_against_pillows_fastest_setting():
    """Condition 3: over three photo-like tiles the files are, summed, no larger than Pillow's compress_level=1 files (zlib's
    fastest setting in the same container) -- a cap with room only where that setting is well above Pillow's default, which is
    asserted first."""
    seeds = (7, 1, 2)
    tiles = [pc.natural(s) for s in seeds]
    assert np.array_equal(tiles[0], pc.tile(299, 'synthetic'))
    level1 = [len(pc.pillow_file(t, compress_level=1)) for t in tiles]
    default = [len(pc.pillow_file(t)) for t in tiles]
    for a, b in zip(level1, default):
        assert a > 1.05 * b, (level1, default)
    _, off, _ = encode(tiles)
    ours = np.diff(off).tolist()
    print('ours', ours, 'pillow level 1', level1, 'pillow default', default)
    assert sum(ours) <= sum(level1), (ours, level1)


def first_block_type(raw):
    return (pc.zstream(raw)[2] >> 1) & 3


def test_all_three_block_kinds_occur(files299):
    """From the sizes: a 1-px file's deflate stream is 48 bits at most, and a dynamic block cannot be that short (17 + 12 header
    bits, two 8-bit runs of zero lengths to pass the unused literals, six code lengths, five symbols of a five-symbol code: 63
    at least): fixed.  Noise is within condition 1 of raw, which no Huffman code over 256 equally likely bytes reaches:
    stored.  The photo-like tile is below 0.7 L, which neither stored nor the fixed code (8 bits or more per literal) can be:
    dynamic.  The first block's type bits say the same."""
    L = pc.stream_bytes(299)
    buf, off, _ = encode([pc.tile(1, 'noise')])
    one = buf.tobytes()
    assert len(pc.zstream(one)) - 6 <= 6 and first_block_type(one) == 1
    assert L < len(files299['noise']) <= size_cap(299) and first_block_type(files299['noise']) == 0
    assert len(files299['synthetic']) < 0.7 * L and first_block_type(files299['synthetic']) == 2


def test_cap_protocol():
    """Sizing call, a buffer one byte short (status bit 1 for the last tile only, the earlier files intact, the offsets still
    exact), the exact buffer."""
    tiles = [pc.tile(21, w) for w in ('noise', 'gradient', 'checker', 'synthetic')]
    full, off, status = encode(tiles)
    assert not status.any() and len(full) == off[-1]
    _, off0, status0 = encode(tiles, cap=0)
    assert np.array_equal(off0, off) and status0.all()
    buf, off1, status1 = encode(tiles, cap=int(off[-1]) - 1)
    assert np.array_equal(off1, off) and list(status1) == [0, 0, 0, 1]
    assert buf[:off[3]].tobytes() == full[:off[3]].tobytes() and not buf[off[3]:].any()
    exact, off2, status2 = encode(tiles, cap=int(off[-1]))
    assert exact.tobytes() == full.tobytes() and not status2.any()


def test_a_file_does_not_depend_on_the_batch():
    """One call, single-tile calls and a split in two: the same files."""
    tiles = list(pc.mixed(9, px=33)) + [pc.tile(74, 'synthetic')[:33, :33]]
    buf, off, _ = encode(tiles)
    whole = pc.split(buf, off)
    for i, t in enumerate(tiles):
        one, off1, _ = encode([t])
        assert one.tobytes() == whole[i] and list(off1) == [0, len(whole[i])]
    a, offa, _ = encode(tiles[:4])
    b, offb, _ = encode(tiles[4:])
    assert pc.split(a, offa) + pc.split(b, offb) == whole


@pytest.mark.parametrize('px', [0, -1, 4097])
def test_bad_arguments_are_refused(px):
    off = np.zeros(2, np.int64)
    assert tn.lib().bqio_png_encode(None, 1, px, None, 0, off.ctypes.data, None) == -1
    assert b'subset' in tn.lib().bqio_png_encode_last_error()
    if px == 0:
        with pytest.raises(ValueError):
            tn.png_encode(np.zeros((1, 0, 0, 3), np.uint8))
        t = np.zeros((1, 4, 4, 3), np.uint8)
        status = np.zeros(1, np.int32)
        assert tn.lib().bqio_png_encode(t.ctypes.data, 1, 4, None, 0, None, status.ctypes.data) == -1           # no offsets
        assert tn.lib().bqio_png_encode(None, 1, 4, None, 0, off.ctypes.data, status.ctypes.data) == -1         # no tiles
        assert tn.lib().bqio_png_encode(t.ctypes.data, 1, 4, None, 8, off.ctypes.data, status.ctypes.data) == -1   # a size without a buffer
        assert tn.lib().bqio_png_encode(t.ctypes.data, -1, 4, None, 0, off.ctypes.data, status.ctypes.data) == -1
        assert tn.lib().bqio_png_encode(None, 0, 4, None, 0, off.ctypes.data, None) == 0 and off[0] == 0


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_selfcheck_under_the_sanitizers(tmp_path):
    """tests/png_encode_selfcheck.cpp -- the header's routines over flats, noise and a ramp at 1, 5, 74 and 299 px, inflated with
    zlib, and ``round_items`` (csrc/bq_rounds.h) against the expression it replaced -- built with AddressSanitizer and UBSan as a
    program of its own and run."""
    exe = str(tmp_path / 'png_encode_selfcheck')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-I', os.path.join(ROOT, 'biscuit_amd', 'csrc'), os.path.join(ROOT, 'tests', 'png_encode_selfcheck.cpp'),
                            '-o', exe, '-lz'], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert 'ok' in run.stdout
