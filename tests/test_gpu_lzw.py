"""A slide's LZW tiles decoded on the device: ``Engine.lzw_decode_canvas`` against its CPU statement
(``tfrecord_native.lzw_decode_canvas``) and against the reader, byte for byte and status for status, over the streams of
tests/test_lzw.py; many segments of mixed kinds side by side, rounds, a refused segment between decoded ones, clip and out-of-canvas
places, poisoned scratch; then ``Heatmap.from_slide(decode='gpu')`` against ``decode='host'`` bit for bit with the path each band
took counted, ``extract_slide``, and the loud fallback for tiles larger than the decoder takes: ``-m gpu``."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI, TiffSlide
from tests import _lzw_cases as lc
from tests import _poison

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 2, 0xA5              # rows in front of and behind the device canvas

VALID = lc.valid_cases()


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=2)
    yield e
    e.close()


def _pack(raws):
    ln = [len(r) for r in raws]
    return tn.lzw_pack(np.frombuffer(b''.join(raws), np.uint8), np.cumsum([0] + ln[:-1]), ln)


def _device_canvas(eng, packed, seg_w, seg_h, place, shape, clip, predictor=1, scratch=None, fill=255):
    """One ``lzw_decode_canvas`` call into a filled canvas that stands between guard rows.  -> (canvas, status) on the host"""
    data, desc = packed
    dev = eng.device
    h, w = shape
    buf = torch.full(((h + 2 * GUARD) * w * 3,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    canvas = buf[GUARD * w * 3:(GUARD + h) * w * 3].view(h, w, 3)
    canvas.fill_(fill)
    status = eng.lzw_decode_canvas(torch.from_numpy(data).to(dev), torch.from_numpy(desc.view(np.int32)).to(dev), seg_w, seg_h,
                                   torch.from_numpy(np.ascontiguousarray(place, np.int32)).to(dev), canvas, clip, predictor=predictor,
                                   scratch=scratch)
    torch.cuda.synchronize(dev)
    flat = buf.cpu().numpy()
    assert (flat[:GUARD * w * 3] == GUARD_BYTE).all() and (flat[(GUARD + h) * w * 3:] == GUARD_BYTE).all(), 'guard rows touched'
    return flat[GUARD * w * 3:(GUARD + h) * w * 3].reshape(h, w, 3), status.cpu().numpy()


def _both(eng, raws, seg_w, seg_h, place, shape, clip, predictor=1, scratch=None, fill=255):
    packed = _pack(raws)
    cpu = np.full(tuple(shape) + (3,), fill, np.uint8)
    cpu_status = tn.lzw_decode_canvas(*packed, seg_w, seg_h, place, cpu, clip, predictor=predictor)
    got, status = _device_canvas(eng, packed, seg_w, seg_h, place, shape, clip, predictor, scratch, fill)
    return got, status, cpu, cpu_status, packed


@pytest.mark.parametrize('case', VALID, ids=lambda c: c[0])
def test_device_equals_cpu_statement_and_the_picture(eng, case):
    name, raw, w, h, pred, a = case
    # the segment twice: whole, and cut by the canvas and the clip; the canvas starts as 7s, so that white pixels show as written
    got, status, cpu, cpu_status, _ = _both(eng, [raw, raw], w, h, [[1, 2], [w + 2, h // 2]], (h + 9, 2 * w + 2), (0, 1, 2 * w + 1, h + 5), pred,
                                            fill=7)
    assert (status == 0).all() and np.array_equal(status, cpu_status)
    assert np.array_equal(got, cpu)
    assert np.array_equal(got[2:2 + h, 1:1 + w], a)


def test_malformed_streams_get_the_cpu_statements_status(eng):
    """Every malformed stream of tests/test_lzw.py that fits the decoder, one call per geometry: the host's status (which that
    file holds against libtiff) and the host's canvas -- a refused segment's window keeps the fill."""
    by_geom = {}
    for name, raw, w, rows in lc.malformed_cases():
        by_geom.setdefault((w, rows), []).append((name, raw))
    seen = set()
    for (w, rows), items in by_geom.items():
        if max(w, rows) > tn.LZW_MAX_SIDE:
            continue
        raws = [r for _, r in items]
        place = [[k * w, 0] for k in range(len(raws))]
        got, status, cpu, cpu_status, _ = _both(eng, raws, w, rows, place, (rows, w * len(raws)), (0, 0, w * len(raws), rows), fill=9)
        assert status.tolist() == cpu_status.tolist(), [n for n, _ in items]
        assert np.array_equal(got, cpu)
        for k, st in enumerate(status):
            if st:
                assert (got[:, k * w:(k + 1) * w] == 9).all()
        seen |= set(status.tolist())
    assert {0, tn.LZW_HEAD, tn.LZW_CODE, tn.LZW_SHORT, tn.LZW_FULL} <= seen


def _mixed(n, w=96, h=80, predictor=2):
    """n segments of w x h of mixed kinds -- and so of very different code counts and lengths --, and their pixels"""
    kinds = ['noise', 'flat', 'smooth', 'white']
    tiles = [lc.content(kinds[k % 4], w, h, k) for k in range(n)]
    raws = [(lc.libtiff_stream(t, predictor) if k % 3 else lc.encode((lc.difference(t) if predictor == 2 else t).tobytes(), eoi=bool(k & 1)))
            for k, t in enumerate(tiles)]
    return tiles, raws


@pytest.fixture(scope='module')
def seventy():
    return _mixed(70)


def test_seventy_mixed_segments_in_one_call(eng, seventy):
    tiles, raws = seventy
    assert len({len(r) for r in raws}) > 30 and max(map(len, raws)) > 50 * min(map(len, raws))
    place = [(k % 10 * 96, k // 10 * 80) for k in range(70)]
    got, status, cpu, cpu_status, _ = _both(eng, raws, 96, 80, place, (560, 960), (0, 0, 960, 560), predictor=2)
    assert (status == 0).all() and np.array_equal(status, cpu_status) and np.array_equal(got, cpu)
    for k, t in enumerate(tiles):
        assert np.array_equal(got[k // 10 * 80:k // 10 * 80 + 80, k % 10 * 96:k % 10 * 96 + 96], t), k


def test_rounds_and_the_workspace_error(eng, seventy):
    from biscuit_amd.engine import BiscuitHipError
    tiles, raws = seventy[0][:7], seventy[1][:7]
    place = [(k * 96, 0) for k in range(7)]
    per = int(eng._lib.bq_lzw_canvas_scratch_bytes(1, 96, 80))
    assert per == 96 * 80 * 3 and int(eng._lib.bq_lzw_canvas_scratch_bytes(7, 96, 80)) == 7 * per
    assert int(eng._lib.bq_lzw_canvas_scratch_bytes(1, 5, 3)) == 48 and int(eng._lib.bq_lzw_canvas_scratch_bytes(3000, 5, 3)) == 1024 * 48
    scratch = torch.empty(3 * per + 100, dtype=torch.uint8, device=eng.device)     # three rounds: 3 + 3 + 1
    got, status, cpu, cpu_status, packed = _both(eng, raws, 96, 80, place, (80, 672), (0, 0, 672, 80), predictor=2, scratch=scratch)
    assert (status == 0).all() and np.array_equal(got, cpu) and np.array_equal(got, np.concatenate(tiles, 1))
    with pytest.raises(BiscuitHipError, match='scratch smaller than one segment'):
        _device_canvas(eng, packed, 96, 80, place, (80, 672), (0, 0, 672, 80), 2, scratch=torch.empty(per - 1, dtype=torch.uint8, device=eng.device))
    # no segments: nothing is launched, nothing is written
    none = (packed[0][:0], packed[1][:0])
    got, status = _device_canvas(eng, none, 96, 80, np.zeros((0, 2), np.int32), (4, 4), (0, 0, 4, 4), fill=3)
    assert len(status) == 0 and (got == 3).all()


def test_a_refused_segment_between_decoded_ones(eng):
    a, b = lc.content('smooth', 64, 64, 1), lc.content('noise', 64, 64, 2)
    good = lc.encode(lc.difference(a).tobytes())
    for bad, want in [(good[:len(good) // 2], tn.LZW_SHORT), (b'x' * 10, tn.LZW_HEAD),
                      (lc.encode(lc.content('noise', 64, 64, 3).tobytes(), clear_at=None), tn.LZW_FULL)]:
        raws = [good, bad, lc.encode(lc.difference(b).tobytes())]
        place = [[0, 0], [64, 0], [128, 0]]
        got, status, cpu, cpu_status, packed = _both(eng, raws, 64, 64, place, (64, 192), (0, 0, 192, 64), predictor=2)
        assert status.tolist() == [0, want, 0] == cpu_status.tolist()
        assert np.array_equal(got, cpu) and (got[:, 64:128] == 255).all() and np.array_equal(got[:, :64], a) and np.array_equal(got[:, 128:], b)
    # a descriptor the decoder does not take (an offset that is no multiple of 16) is refused before anything is read through it
    data, desc = packed
    desc = desc.copy()
    desc[0, 0] += 4
    cpu = np.full((64, 192, 3), 255, np.uint8)
    cpu_status = tn.lzw_decode_canvas(data, desc, 64, 64, place, cpu, (0, 0, 192, 64), predictor=2)
    got, status = _device_canvas(eng, (data, desc), 64, 64, place, (64, 192), (0, 0, 192, 64), 2)
    assert status.tolist() == [tn.LZW_DESC, tn.LZW_FULL, 0] == cpu_status.tolist() and np.array_equal(got, cpu) and (got[:, :128] == 255).all()


@pytest.mark.parametrize('predictor', [1, 2])
def test_clip_and_places_outside_the_canvas(eng, predictor):
    """Segments left of, above, right of and below a 50 x 71 canvas (its pitch no multiple of 4), one inside, one outside the
    clip altogether, under a clip inside the canvas; every window the host's, the guard rows intact (``_device_canvas``)."""
    sw, sh = 33, 20
    tiles = [lc.content(k, sw, sh, i) for i, k in enumerate(['noise', 'smooth', 'noise', 'smooth', 'noise', 'flat'])]
    raws = [lc.encode((lc.difference(t) if predictor == 2 else t).tobytes()) for t in tiles]
    place = [[-9, -7], [60, 40], [19, 14], [-20, 25], [30, -15], [200, 300]]
    got, status, cpu, cpu_status, _ = _both(eng, raws, sw, sh, place, (50, 71), (3, 2, 69, 47), predictor, fill=7)
    assert (status == 0).all() and np.array_equal(got, cpu)
    assert np.array_equal(got[14:34, 19:52], tiles[2]) and np.array_equal(got[2:13, 3:24], tiles[0][9:, 12:])
    assert (got[:2] == 7).all() and (got[47:] == 7).all() and (got[:, :3] == 7).all() and (got[:, 69:] == 7).all()


@pytest.mark.parametrize('fill', _poison.BYTE_FILLS)
def test_poisoned_scratch_changes_nothing(eng, seventy, fill):
    tiles, raws = seventy[0][:6], seventy[1][:6]
    raws = raws[:3] + [raws[3][:100]] + raws[4:]                          # (one refused: its scratch is never read)
    place = [(k * 96 - 5, -3) for k in range(6)]
    packed = _pack(raws)
    cpu = np.full((80, 560, 3), 255, np.uint8)
    cpu_status = tn.lzw_decode_canvas(*packed, 96, 80, place, cpu, (0, 0, 560, 80), predictor=2)
    for n_scratch in (6, 4):                                              # one round, and two
        scratch, check = _poison.guarded(int(eng._lib.bq_lzw_canvas_scratch_bytes(n_scratch, 96, 80)), fill, eng.device)
        got, status = _device_canvas(eng, packed, 96, 80, place, (80, 560), (0, 0, 560, 80), 2, scratch=scratch)
        check()
        assert status.tolist() == cpu_status.tolist() == [0, 0, 0, tn.LZW_SHORT, 0, 0] and np.array_equal(got, cpu)


def test_device_equals_read_region(eng, tmp_path):
    """A tiled slide's band through ``region_segments`` and the device equals ``read_region``, border tiles and all."""
    path, a, _ = lc.slide_file(tmp_path, 1.0, w=300, h=210, tile=64)
    with TiffSlide(path) as s:
        for (x, y, w, h) in [(0, 0, 300, 210), (-10, -5, 200, 100), (130, 100, 200, 150)]:
            sg = s.region_segments(0, x, y, w, h)
            packed = tn.lzw_pack(sg.data, sg.offsets, sg.lengths)
            got, status = _device_canvas(eng, packed, sg.seg_w, sg.seg_h, sg.place, sg.shape, sg.clip, sg.predictor)
            assert (status == 0).all() and np.array_equal(got, s.read_region(0, x, y, w, h))


def _same(a, b):
    return np.array_equal(a.logits, b.logits) and np.array_equal(a.uncertainty, b.uncertainty) and np.array_equal(a.grid, b.grid)


# 64 um at 1 um a pixel: tiles of 64 level-0 pixels, resampled to 299; canvas_bytes = 1: one grid row per band
KW = dict(mc_n=2, seed=3, batch=16, canvas_bytes=1, tile_um=64)


def test_heatmap_with_device_decode_equals_host_decode(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path, _, _ = lc.slide_file(tmp_path, 1.0, w=600, h=450, tile=64, predictor=2)
    w = WSI(path, 299, 64)
    assert (w.grid_w, w.grid_h, w.level, w.src_px) == (9, 7, 0, 64)
    n_seg = sum(len(b[4]) for b in w.bands(1, segments=True))
    w.close()
    host = Heatmap.from_slide(eng, path, decode='host', **KW)
    gpu = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    assert _same(gpu, host)
    assert host.decode_stats == {'gpu_bands': 0, 'host_bands': 7, 'segments': 0}
    assert gpu.decode_stats == {'gpu_bands': 7, 'host_bands': 0, 'segments': n_seg} and n_seg > 7
    # one tile damaged: that band is the host's, which says so
    from biscuit_amd.wsi import SlideError

    def cut(pages):
        pages[0]['segs'][2 * 10 + 3] = pages[0]['segs'][2 * 10 + 3][:30]
    path2, _, _ = lc.slide_file(tmp_path, 1.0, w=600, h=450, tile=64, predictor=2, mutate=cut, name='cut.tif')
    with pytest.raises(SlideError, match='damaged LZW segment 23'):
        Heatmap.from_slide(eng, path2, decode='gpu', **KW)


def test_extract_slide_then_evaluate_equals_from_slide(eng, tmp_path):
    from biscuit_amd import tfrecord as tfr
    from biscuit_amd.extract import extract_slide
    path, _, _ = lc.slide_file(tmp_path, 1.0, w=280, h=200, tile=64, predictor=2)
    outs = []
    for decode in ('host', 'gpu'):
        out = str(tmp_path / f'{decode}.tfrecords')
        info = extract_slide(eng, path, out, tile_um=64, decode=decode, img_format='png', canvas_bytes=1, batch=16)
        recs = [tfr.parse_example(r) for r in tfr.read_records(out, verify='full')]
        outs.append(([np.asarray(Image.open(io.BytesIO(r['image_raw']))) for r in recs], info))
    (host, hi), (gpu, gi) = outs
    assert len(host) == len(gpu) == 12 and all(np.array_equal(x, y) for x, y in zip(host, gpu))
    assert gi['decode_stats']['gpu_bands'] == 3 and gi['decode_stats']['host_bands'] == 0 and hi['decode_stats']['gpu_bands'] == 0
    # the records are the reader's tiles in grid order, and evaluate() over them is from_slide, per tile, bit for bit
    from biscuit_amd import inference as inf
    from biscuit_amd.heatmap import Heatmap
    tiles, _ = WSI(path, 299, 64).tiles()
    assert np.array_equal(np.stack(gpu), tiles)
    hm = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    res = inf.evaluate(eng, inf.slides_from_tfrecords([str(tmp_path / 'gpu.tfrecords')], {'lzw': 1}), outcome='cohort', mc_n=2, seed=3, batch=16)
    df = res.tile_df
    mean = np.stack([df['cohort-y_pred0'].to_numpy(), df['cohort-y_pred1'].to_numpy()], 1).astype(np.float32)
    std = np.stack([df['cohort-uncertainty0'].to_numpy(), df['cohort-uncertainty1'].to_numpy()], 1).astype(np.float32)
    assert np.array_equal(mean, hm.logits.reshape(12, 2)) and np.array_equal(std, hm.uncertainty.reshape(12, 2))


def test_tiles_larger_than_the_decoder_takes_fall_back_loudly_and_exactly(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    side = tn.LZW_MAX_SIDE + 16
    a = lc._img(side, 64, 3)
    pages = [dict(w=side, h=64, tw=side, th=64, comp=5, predictor=2, segs=[lc.libtiff_stream(a, 2)], desc='Aperio |MPP = 1.0')]
    path = lc.write_slide(tmp_path / 'wide.tif', pages)
    with TiffSlide(path) as s:
        assert s.region_segments(0, 0, 0, side, 64).seg_w == side and np.array_equal(s.read_region(0, 0, 0, side, 64), a)
    host = Heatmap.from_slide(eng, path, decode='host', **KW)
    gpu = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    assert _same(gpu, host)
    assert gpu.decode_stats == {'gpu_bands': 0, 'host_bands': 1, 'segments': 0}
