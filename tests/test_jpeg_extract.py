"""The host half of the device JPEG decoder: ``bqio_extract_jpeg`` (the header walk of csrc/jpeg_baseline.h, the scan bytes
unstuffed and packed, table sets de-duplicated) followed by ``bqio_jpeg_decode_extracted`` -- the routines of csrc/jpeg_device.h,
the ones the GPU kernels are compiled from, run on the CPU -- against Pillow (libjpeg-turbo) byte for byte, on the matrix of
tests/test_jpeg.py; what the host decoder refuses the extractor refuses; damaged streams are accepted with libjpeg's bytes or
carry a status.  Choice of section 1 of the feature: grey tiles and restart intervals are REFUSED (``UnsupportedImage``), such a
slide stays on the host decoder."""
import io

import numpy as np
import pytest

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from tests import _jpeg_cases as jc

Image = pytest.importorskip('PIL.Image')
pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')


@pytest.mark.parametrize('px', jc.SIZES)
def test_extract_then_decode_gives_libjpegs_bytes(px, tmp_path):
    """Every encoding of the matrix, all of one size in ONE call: none refused, every status 0, Pillow's bytes."""
    cases = jc.matrix(px)
    assert len(cases) >= 40
    raws = [r for r, _ in cases]
    path = str(tmp_path / 'm.tfrecords')
    locs = np.arange(2 * len(raws), dtype=np.int64).reshape(-1, 2)
    tfr.write_slide(path, 'm', raws, locs)
    scan, desc, tables = jc.extract(path, 0, len(raws), px)
    with tn.NativeReader(path) as r:
        assert np.array_equal(r.extract_jpeg(0, len(raws), px, None, None, None)[2], locs)
    assert tables.shape[0] >= 8 and len(set(desc[:, 2].tolist())) == 3      # optimised tables differ per file; three samplings
    assert (desc[:, 0] % 16 == 0).all() and int(desc[-1, 0]) + int(desc[-1, 1]) + int(tn.lib().bqio_jpeg_ecs_pad()) <= scan.size
    got, status = tn.jpeg_decode_extracted(scan, desc, tables, px)
    assert not status.any(), status
    for i, (raw, what) in enumerate(cases):
        assert np.array_equal(got[i], jc.pillow(raw)), (px, what)
        assert np.array_equal(got[i], tn.decode_jpeg(raw, px)), (px, what)


def test_saturated_colours_grey_and_restart_intervals(tmp_path):
    raws = jc.saturated()
    for (scan, desc, tables), raw in zip(jc.extract_each(tmp_path, raws, 299, 'sat'), raws):
        got, status = tn.jpeg_decode_extracted(scan, desc, tables)
        assert status[0] == 0 and np.array_equal(got[0], jc.pillow(raw))
    img = jc.photo(299, 2)
    outside = [jc.enc(img[..., 0], quality=90)]                                 # one component
    for kw in (dict(restart_marker_blocks=5), dict(restart_marker_rows=1), dict(restart_marker_blocks=1)):
        for ss in (0, 1, 2):
            outside.append(jc.enc(img, quality=85, subsampling=ss, **kw))
            assert outside[-1].count(b'\xff\xd0') > 0
    for raw, res in zip(outside, jc.extract_each(tmp_path, outside, 299, 'outside')):
        assert isinstance(res, tn.UnsupportedImage)                             # the device subset's two extra refusals ...
        assert np.array_equal(tn.decode_jpeg(raw), jc.pillow(raw))              # ... of files the host decoder takes


def test_what_the_host_decoder_refuses_the_extractor_refuses(tmp_path):
    img = jc.photo(299, 3)
    raw = jc.enc(img, quality=85)
    cmyk = io.BytesIO()
    Image.fromarray(img).convert('CMYK').save(cmyk, format='JPEG', quality=85)
    files = [jc.enc(img, quality=85, progressive=True), raw[: len(raw) // 2], raw[: len(raw) // 2] + b'\xff\xd9',
             raw.replace(b'\xff\xc0', b'\xff\xc9', 1), cmyk.getvalue(), b'\xff\xd8\xff']
    for ss, kw in ((0, {}), (2, {}), (2, {'restart_marker_blocks': 7})):        # the scan cut to nothing before a valid EOI
        r2 = jc.enc(jc.photo(299, 5), quality=90, subsampling=ss, **kw)
        sos = r2.index(b'\xff\xda')
        hdr = sos + 2 + int.from_bytes(r2[sos + 2:sos + 4], 'big')
        for keep in (0, 1, 2, 7, 8, 9, 33, 500):
            files.append(r2[:hdr] + r2[hdr:hdr + keep].replace(b'\xff', b'\x7f') + b'\xff\xd9')
        files.append(r2[:hdr] + b'\x00\x00\xff\xd9')
    n_refused = 0
    for f, res in zip(files, jc.extract_each(tmp_path, files, 299, 'refused')):
        with pytest.raises(tn.UnsupportedImage):
            tn.decode_jpeg(f)
        if isinstance(res, tn.UnsupportedImage):                                # refused by the markers or the scan's structure
            n_refused += 1
            continue
        _, status = tn.jpeg_decode_extracted(*res)                              # or by the entropy decoder: a status, as the host's
        assert status[0] != 0
    assert n_refused >= 6
    res = jc.extract_each(tmp_path, [raw], 298, 'size')[0]
    assert isinstance(res, ValueError) and not isinstance(res, tn.UnsupportedImage)         # a tile of another size
    png = str(tmp_path / 'png.tfrecords')
    tfr.write_slide(png, 'png', jc.photo(64, 1)[None])
    with tn.NativeReader(png) as r, pytest.raises(tn.UnsupportedImage):
        r.extract_jpeg(0, 1, 64, None, None, None)


def test_damaged_streams_agree_or_carry_a_status(tmp_path):
    """The 600 byte-flipped files of tests/test_jpeg.py (same seed, same recipe) through the pair: whatever it accepts equals
    Pillow's bytes, the rest is refused by the extractor or carries a status.  The floor on the number accepted is the host
    decoder's own count on the same files less 5 %: the two subsets differ only by grey and restart files, which a flipped
    byte makes of a colour file only by hitting the component count or planting a DRI marker."""
    files = jc.byte_flipped(600)
    host = 0
    for f in files:
        try:
            tn.decode_jpeg(f)
            host += 1
        except (tn.UnsupportedImage, ValueError):
            pass
    accepted = 0
    for f, res in zip(files, jc.extract_each(tmp_path, files, 299, 'flipped')):
        if isinstance(res, Exception):
            continue
        got, status = tn.jpeg_decode_extracted(*res)
        if status[0] == 0:
            accepted += 1
            assert np.array_equal(got[0], jc.pillow(f))
    print(f'accepted {accepted} of {len(files)}; the host decoder accepts {host}')
    assert host > 100 and accepted >= host - host // 20


def test_one_call_with_different_table_sets_and_samplings(tmp_path):
    """Tiles of three samplings, four qualities and optimised tables in one call, in an order that interleaves them; tiles
    that share tables share a set."""
    img = [jc.photo(64, s) for s in range(4)]
    raws = [jc.enc(img[i % 4], quality=q, subsampling=ss, optimize=opt)
            for i, (q, ss, opt) in enumerate([(75, 0, False), (95, 2, False), (75, 1, True), (75, 2, False), (30, 0, True), (95, 0, False),
                                              (75, 0, False), (95, 1, False)])]
    path = str(tmp_path / 'sets.tfrecords')
    tfr.write_slide(path, 'sets', raws, np.zeros((len(raws), 2), np.int64))
    for threads in (1, 3, 16):
        with tn.NativeReader(path) as r:
            scan, desc = np.zeros(1 << 20, np.uint8), np.zeros((len(raws), 4), np.uint32)
            tables = np.zeros((8, tn.jpeg_table_bytes()), np.uint8)
            used, nt, _ = r.extract_jpeg(0, len(raws), 64, scan, desc, tables, threads=threads)
        assert nt == 4                                   # quality 75 / 95 with the default Huffman tables, two optimised files
        ts = desc[:, 3]
        assert ts[0] == ts[3] == ts[6] and ts[1] == ts[5] == ts[7] and len({int(ts[0]), int(ts[1]), int(ts[2]), int(ts[4])}) == 4
        got, status = tn.jpeg_decode_extracted(scan[:used], desc, tables[:nt], 64)
        assert not status.any()
        for g, raw in zip(got, raws):
            assert np.array_equal(g, jc.pillow(raw))


def test_a_buffer_too_small_says_what_is_needed(tmp_path):
    raws = [jc.enc(jc.photo(64, s), quality=90, optimize=True) for s in range(3)]
    path = str(tmp_path / 'small.tfrecords')
    tfr.write_slide(path, 'small', raws, np.zeros((3, 2), np.int64))
    with tn.NativeReader(path) as r:
        used, nt, _ = r.extract_jpeg(0, 3, 64, None, None, None)
        assert nt == 3 and used >= sum(len(x) for x in raws) // 2
        desc = np.zeros((3, 4), np.uint32)
        with pytest.raises(MemoryError) as e:
            r.extract_jpeg(0, 3, 64, np.zeros(used - 1, np.uint8), desc, np.zeros((3, tn.jpeg_table_bytes()), np.uint8))
        assert e.value.args[1] == used
        with pytest.raises(MemoryError) as e:
            r.extract_jpeg(0, 3, 64, np.zeros(used, np.uint8), desc, np.zeros((2, tn.jpeg_table_bytes()), np.uint8))
        assert e.value.args[2] == 3


def test_a_slide_with_one_progressive_record_stays_on_the_host(tmp_path):
    """``TFRecordSource.jpeg_ok``: decided per slide before its first chunk.  One progressive record among baseline ones -> False,
    and the slide decodes exactly as today (the whole slide through the fallback); a clean JPEG slide -> True, and its chunks
    through ``read_jpeg`` give the tiles ``read`` gives; a PNG slide is no JPEG slide; without gpu_decode nothing changes."""
    from biscuit_amd.inference import TFRecordSource
    imgs = [jc.photo(299, s) for s in range(6)]
    raws = [jc.enc(a, quality=85, subsampling=s % 3) for s, a in enumerate(imgs[:5])] + [jc.enc(imgs[5], quality=85, progressive=True)]
    mixed, good, png = (str(tmp_path / f'{n}.tfrecords') for n in ('mixed', 'good', 'png'))
    tfr.write_slide(mixed, 'mixed', raws, np.zeros((6, 2), np.int64))
    tfr.write_slide(good, 'good', raws[:5], np.zeros((5, 2), np.int64))
    tfr.write_slide(png, 'png', np.stack(imgs[:2]))
    want = np.stack([jc.pillow(x) for x in raws])
    src = TFRecordSource(mixed, 6, z=True)
    assert not src.z_ok() and not src.jpeg_ok()
    out = np.zeros((2, 299, 299, 3), np.uint8)
    src.read(0, 2, out)
    assert src._reader is None and src._fallback is not None and np.array_equal(out, want[:2])
    src.read(4, 2, out)
    assert np.array_equal(out, want[4:6])
    src.close()
    src = TFRecordSource(good, 5, z=True)
    assert not src.z_ok() and src.jpeg_ok()
    scan, desc = np.zeros(1 << 20, np.uint8), np.zeros((5, 4), np.uint32)
    tables = np.zeros((4, tn.jpeg_table_bytes()), np.uint8)
    used, nt = src.read_jpeg(1, 4, scan, desc, tables)
    got, status = tn.jpeg_decode_extracted(scan[:used], desc[:4], tables[:nt])
    src.read(1, 4, full := np.zeros((4, 299, 299, 3), np.uint8))
    assert not status.any() and np.array_equal(got, full) and np.array_equal(got, want[1:5])
    src.close()
    assert not TFRecordSource(good, 5).jpeg_ok()                                 # gpu_decode off: never asked, never true
    src = TFRecordSource(png, 2, z=True)
    assert src.z_ok() and not src.jpeg_ok()
    src.close()
