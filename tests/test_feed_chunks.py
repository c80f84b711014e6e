"""The chunk filler and the two compressed tile formats of biscuit_amd/feed.py on the CPU: a cohort of PNG and JPEG slides is packed
into small slots the way the feeder does it, every finished slot is unpacked through the SAME layout function the device side uses
(on numpy here) and decoded with zlib / the CPU build of the device JPEG routines, and every tile is held against the host decoder."""
import zlib

import numpy as np
import pytest

from biscuit_amd import feed
from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from tests import _jpeg_cases as jc

pytest.importorskip('PIL.Image')
pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')

PX = 64
CAPS = (3, 5, 8)                 # tiles per chunk: a short ramp, then 8 (the last repeats)


def _cohort(tmp_path):
    """[(name, path, tiles)]: two PNG slides, a JPEG slide on the default tables, two with optimised (per-file) tables at 4:2:0 / 4:4:4."""
    img = [jc.photo(PX, s) for s in range(69)]
    slides = [('png0', np.stack(img[:19])), ('png1', np.stack(img[19:26])),
              ('jdef', [jc.enc(a, quality=85, subsampling=1) for a in img[26:31]]),
              ('j420', [jc.enc(a, quality=80, subsampling=2, optimize=True) for a in img[31:50]]),
              ('j444', [jc.enc(a, quality=95, subsampling=0, optimize=True) for a in img[50:69]])]
    out = []
    for name, records in slides:
        path = str(tmp_path / f'{name}.tfrecords')
        tfr.write_slide(path, name, records, np.zeros((len(records), 2), np.int64))
        out.append((name, path, len(records)))
    return out


def _pack(sources):
    """``_Feeder._compressed`` without ring and device: slots are numpy arrays full of stale bytes, a finished chunk is the slice the
    feeder would upload.  -> ([(fmt, state, segs, uploaded bytes)], the slides that met a chunk without room for their tables)."""
    done, turned_away, open_, n_chunks = [], [], None, 0

    def emit():
        nonlocal open_
        if open_ is not None and open_[0].segs:
            c, buf = open_
            done.append((c.fmt, c.state, c.segs, buf[:c.hdr + c.pos].copy()))
        open_ = None
    for si, src in enumerate(sources):
        fmt = next(f for f in feed.FORMATS if f.ok(src))
        first = 0
        while first < src.n_tiles:
            if open_ is not None and open_[0].fmt is not fmt:
                emit()
            if open_ is None:
                buf = np.full(2 << 20, 0xa5, np.uint8)
                open_ = (feed._Filling(fmt, 0, buf, CAPS[min(n_chunks, len(CAPS) - 1)], PX), buf)
                n_chunks += 1
            c = open_[0]
            cnt = c.add(src, si, si, first, src.n_tiles - first)
            if not cnt and first == 0 and c.segs and c.n < c.cap:
                turned_away.append(si)
            first += cnt
            if not cnt or c.n == c.cap:
                emit()
    emit()
    return done, turned_away


@pytest.mark.parametrize('jpeg_sets', [16, 3])
def test_packed_chunks_unpack_to_the_host_decoders_tiles(tmp_path, monkeypatch, jpeg_sets):
    """Every tile of the cohort, through pack -> layout -> CPU decode, equals the host decoder's; the chunks' segments are the
    slides' tiles in dataset order, each once.  The run holds a slide that spans chunks, a chunk that spans slides, a PNG chunk
    followed by a JPEG chunk and -- with three table sets per chunk -- a JPEG slide that finds the open chunk without room for its
    tables and starts the next one; each is asserted, so that a change of encoder defaults cannot empty the test unnoticed."""
    monkeypatch.setattr(feed, 'JPEG_SETS', jpeg_sets)
    cohort = _cohort(tmp_path)
    sources = [feed.TFRecordSource(path, n, PX, z=True) for _, path, n in cohort]
    assert [(s.z_ok(), s.jpeg_ok()) for s in sources] == [(True, False)] * 2 + [(False, True)] * 3
    chunks, turned_away = _pack(sources)

    # the segments: every slide's [0, n_tiles) in dataset order, nothing twice, nothing missing
    at = [0] * len(cohort)
    order = [seg for _, _, segs, _ in chunks for seg in segs]
    assert [si for _, si, _, _ in order] == sorted(si for _, si, _, _ in order)
    for li, si, first, cnt in order:
        assert li == si and first == at[si] and cnt > 0
        at[si] += cnt
    assert at == [n for _, _, n in cohort]

    compared = [0] * len(cohort)
    for fmt, state, segs, data in chunks:
        n = sum(cnt for *_, cnt in segs)
        if fmt is feed.PNG_Z:
            off, ln, z = fmt.layout(data, state)
            got = [zlib.decompress(z[int(off[i]):int(off[i]) + int(ln[i])].tobytes()) for i in range(n)]
            want = []
            for _, si, first, cnt in segs:
                with tn.NativeReader(cohort[si][1]) as r:
                    want += [t.tobytes() for t in r.decode(first, cnt, PX, rows=True)[0]]
            same = [g == w for g, w in zip(got, want)]
        else:
            cap, n_sets = state.cap, len(state.sets)
            desc, tables, scan = fmt.layout(data, cap)
            assert tables.shape == (jpeg_sets, tn.jpeg_table_bytes()) and n_sets <= jpeg_sets and n <= cap
            got, status = tn.jpeg_decode_extracted(scan, desc[:n], tables[:n_sets], PX)
            assert not status.any(), (segs, status)
            want = np.zeros((n, PX, PX, 3), np.uint8)
            k = 0
            for _, si, first, cnt in segs:
                sources[si].read(first, cnt, want[k:k + cnt])
                k += cnt
            same = [np.array_equal(g, w) for g, w in zip(got, want)]
            # 'jdef' tiles share ONE set (the default tables), every optimised file brings its own
            names = [cohort[si][0] for _, si, _, cnt in segs for _ in range(cnt)]
            assert n_sets == ('jdef' in names) + sum(nm != 'jdef' for nm in names), (segs, n_sets)
        assert len(same) == n and all(same), (fmt.name, segs, same)
        for _, si, _, cnt in segs:
            compared[si] += cnt
    assert compared == [n for _, _, n in cohort]
    for s in sources:
        s.close()

    # the four situations
    in_chunks = [sum(any(si == k for _, si, _, _ in segs) for _, _, segs, _ in chunks) for k in range(len(cohort))]
    assert max(in_chunks) > 1                                                    # a slide spans several chunks
    assert any(len({si for _, si, _, _ in segs}) > 1 for _, _, segs, _ in chunks)   # a chunk spans several slides
    kinds = [fmt.name for fmt, *_ in chunks]
    assert ('PNG', 'JPEG') in zip(kinds, kinds[1:])                               # a PNG chunk, then a JPEG chunk
    if jpeg_sets == 3:                  # 'j420' arrives behind 'jdef' (one set, 5 of the chunk's 8 tiles): 1 + 3 sets > 3
        assert 3 in turned_away
        assert [segs[0][1:3] for _, _, segs, _ in chunks].count((3, 0)) == 1     # ... and is the first of the next chunk
    else:
        assert not turned_away
