"""A slide's JPEG 2000 tiles decoded on the device: ``Engine.j2k_decode_canvas`` against its CPU statement
(``tfrecord_native.j2k_decode_canvas``) byte for byte and status for status, rounds, a refused segment between decoded ones,
``Heatmap.from_slide(decode='gpu')`` against ``decode='host'`` bit for bit with the path each band took counted, the fallback, and
``extract_slide(decode='gpu')``: ``-m gpu``.  Damaged streams are the CPU build's under the sanitizers (tests/test_sanitizers_j2k.py);
here only what the extractor refuses before anything is launched, and one status path."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI
from tests import _j2k_cases as jc

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 2, 0xA5              # rows in front of and behind the device canvas


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=2)
    yield e
    e.close()


def _device_canvas(eng, packed, seg_w, seg_h, place, shape, clip, ycc=False, scratch=None, fill=255):
    """One ``j2k_decode_canvas`` call into a white canvas that stands between guard rows.  -> (canvas, status) on the host"""
    desc, blocks, cw = packed
    dev = eng.device
    h, w = shape
    buf = torch.full(((h + 2 * GUARD) * w * 3,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    canvas = buf[GUARD * w * 3:(GUARD + h) * w * 3].view(h, w, 3)
    canvas.fill_(fill)
    status = eng.j2k_decode_canvas(torch.from_numpy(desc).to(dev), torch.from_numpy(blocks).to(dev), torch.from_numpy(cw).to(dev), seg_w, seg_h,
                                   torch.from_numpy(np.ascontiguousarray(place, np.int32)).to(dev), canvas, clip, ycc=ycc, scratch=scratch)
    torch.cuda.synchronize(dev)
    flat = buf.cpu().numpy()
    assert (flat[:GUARD * w * 3] == GUARD_BYTE).all() and (flat[(GUARD + h) * w * 3:] == GUARD_BYTE).all(), 'guard rows touched'
    return flat[GUARD * w * 3:(GUARD + h) * w * 3].reshape(h, w, 3), status.cpu().numpy()


def _both(eng, raws, seg_w, seg_h, place, shape, clip, ycc=False, scratch=None, strict=True, fill=255):
    data = np.frombuffer(b''.join(raws), np.uint8)
    ln = [len(r) for r in raws]
    packed = tn.j2k_extract(data, np.cumsum([0] + ln[:-1]), ln, seg_w, seg_h, strict=strict)
    cpu = np.full(tuple(shape) + (3,), fill, np.uint8)
    cpu_status = tn.j2k_decode_canvas(*packed, seg_w, seg_h, place, cpu, clip, ycc=ycc)
    got, status = _device_canvas(eng, packed, seg_w, seg_h, place, shape, clip, ycc, scratch, fill)
    return got, status, cpu, cpu_status, packed


@pytest.mark.parametrize('case', jc.GPU_CASES, ids=lambda c: '%dx%d_%s_%s%s' % (c[0], c[1], c[2], 'irr' if c[3] else 'rev', '_ycc' if c[4] else ''))
def test_device_equals_cpu_statement(eng, case):
    w, h, kind, irreversible, ycc, kw = case
    a = jc.content(kind, w, h, 7)
    raws = [jc.encode(jc.ycc_of(a) if ycc else a, irreversible, **kw), jc.encode((jc.ycc_of(a) if ycc else a)[::-1].copy(), irreversible, **kw)]
    # two segments, the second cut by the canvas and the clip; the canvas starts as 7s, so that white pixels show as written
    got, status, cpu, cpu_status, packed = _both(eng, raws, w, h, [[1, 2], [w + 2, h // 2]], (h + 9, 2 * w + 2), (0, 1, 2 * w + 1, h + 5), ycc,
                                                 fill=7)
    assert (status == 0).all() and np.array_equal(status, cpu_status)
    assert np.array_equal(got, cpu)
    if not irreversible:                                                 # (and the CPU statement's bytes are the picture's)
        want = np.asarray(Image.fromarray(jc.ycc_of(a), 'YCbCr').convert('RGB')) if ycc else a
        assert np.array_equal(got[2:2 + h, 1:1 + w], want)
    if kw.get('quality_layers') == [40, 20, 8]:                          # the three-layer stream is really truncated
        full = 3 * (packed[1][:, 7] - packed[1][:, 8]) - 2
        assert (packed[1][:, 9] < full).any() and packed[0][0, 28] == 3


def test_more_blocks_than_a_wave_of_mixed_sizes_and_rounds(eng):
    """Eight 96 x 80 segments with 32 x 32 and 16 x 64 code blocks, both transforms, in one call (hundreds of blocks of many
    sizes); then the same call with scratch for three segments only, so that the round loop runs three times."""
    raws, place = [], []
    for k in range(8):
        a = jc.content('photo' if k % 2 else 'noise', 96, 80, k)
        raws.append(jc.encode(a, bool(k & 2), num_resolutions=1 + k % 4, mct=k & 1, codeblock_size=(32, 32) if k < 4 else (16, 64),
                              progression=jc.PROGRESSIONS[k % 5]))
        place.append((k % 4 * 96, k // 4 * 80))
    got, status, cpu, cpu_status, packed = _both(eng, raws, 96, 80, place, (160, 384), (0, 0, 384, 160))
    sizes = {(int(b[5]), int(b[6])) for b in packed[1]}
    assert len(packed[1]) >= 65 and len(sizes) > 4
    assert (status == 0).all() and np.array_equal(status, cpu_status) and np.array_equal(got, cpu)
    per = int(eng._lib.bq_j2k_canvas_scratch_bytes(1, 96, 80))
    assert per == 96 * 80 * 24 and int(eng._lib.bq_j2k_canvas_scratch_bytes(8, 96, 80)) == 8 * per
    scratch = torch.empty(3 * per + 100, dtype=torch.uint8, device=eng.device)
    again, status = _device_canvas(eng, packed, 96, 80, place, (160, 384), (0, 0, 384, 160), scratch=scratch)
    assert (status == 0).all() and np.array_equal(again, cpu)


def test_a_refused_segment_between_decoded_ones(eng):
    good, bad = jc.refusals()
    other = jc.j2k(jc.content('noise', 64, 64, 1), irreversible=True, num_resolutions=2)
    raws = [good, bad['cblk_style'][0], other]
    got, status, cpu, cpu_status, packed = _both(eng, raws, 64, 64, [[0, 0], [64, 0], [128, 0]], (64, 192), (0, 0, 192, 64), strict=False)
    assert status.tolist() == [0, 32, 0] == cpu_status.tolist()
    assert np.array_equal(got, cpu) and (got[:, 64:128] == 255).all() and np.array_equal(got[:, :64], jc.pillow(good))
    # one status path of the device's own: a block row that points outside its plane is caught before anything is indexed by it
    desc, blocks, cw = packed
    blocks = blocks.copy()
    blocks[0, 3] = 60
    cpu = np.full((64, 192, 3), 255, np.uint8)
    cpu_status = tn.j2k_decode_canvas(desc, blocks, cw, 64, 64, [[0, 0], [64, 0], [128, 0]], cpu, (0, 0, 192, 64))
    got, status = _device_canvas(eng, (desc, blocks, cw), 64, 64, [[0, 0], [64, 0], [128, 0]], (64, 192), (0, 0, 192, 64))
    assert status.tolist() == [16, 32, 0] == cpu_status.tolist() and np.array_equal(got, cpu) and (got[:, :128] == 255).all()
    # the same row naming another segment: it lies outside that segment's range of the table, so it is nobody's on either build
    blocks[0, 0] = 2
    cpu = np.full((64, 192, 3), 255, np.uint8)
    cpu_status = tn.j2k_decode_canvas(desc, blocks, cw, 64, 64, [[0, 0], [64, 0], [128, 0]], cpu, (0, 0, 192, 64))
    got, status = _device_canvas(eng, (desc, blocks, cw), 64, 64, [[0, 0], [64, 0], [128, 0]], (64, 192), (0, 0, 192, 64))
    assert status.tolist() == [0, 32, 0] == cpu_status.tolist() and np.array_equal(got, cpu)


def _same(a, b):
    return np.array_equal(a.logits, b.logits) and np.array_equal(a.uncertainty, b.uncertainty) and np.array_equal(a.grid, b.grid)


# 64 um at 1 um a pixel: tiles of 64 level-0 pixels, resampled to 299; canvas_bytes = 1: one grid row per band
KW = dict(mc_n=2, seed=3, batch=16, canvas_bytes=1, tile_um=64)


@pytest.mark.parametrize('comp', [33005, 33003])
def test_heatmap_with_device_decode_equals_host_decode(eng, tmp_path, comp):
    from biscuit_amd.heatmap import Heatmap
    path, _, _ = jc.slide_file(tmp_path, 1.0, w=280, h=200, tile=64, comp=comp, num_resolutions=3)
    w = WSI(path, 299, 64)
    assert (w.grid_w, w.grid_h, w.level, w.src_px) == (4, 3, 0, 64)
    n_seg = sum(len(b[4]) for b in w.bands(1, segments=True))
    w.close()
    host = Heatmap.from_slide(eng, path, decode='host', **KW)
    gpu = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    assert _same(gpu, host)
    assert host.decode_stats == {'gpu_bands': 0, 'host_bands': 3, 'segments': 0}
    assert gpu.decode_stats == {'gpu_bands': 3, 'host_bands': 0, 'segments': n_seg} and n_seg > 3
    # one tile replaced by a stream outside the subset (several tiles): that band is the host's, the result is the same
    a = jc._img(280, 200, 5)

    def swap(pages):
        t = a[64:128, 128:192]
        pages[0]['segs'][1 * 5 + 2] = jc.j2k(jc.ycc_of(t) if comp == 33003 else t, irreversible=False, mct=0 if comp == 33003 else 1,
                                              tile_size=(32, 32))
    path2, _, _ = jc.slide_file(tmp_path, 1.0, w=280, h=200, tile=64, comp=comp, num_resolutions=3, mutate=swap, name='swapped.svs')
    gpu2 = Heatmap.from_slide(eng, path2, decode='gpu', **KW)
    assert _same(gpu2, host) and gpu2.decode_stats['host_bands'] == 1 and gpu2.decode_stats['gpu_bands'] == 2


def test_extract_slide_with_device_decode(eng, tmp_path):
    from biscuit_amd.extract import extract_slide
    from biscuit_amd import tfrecord as tfr
    path, _, _ = jc.slide_file(tmp_path, 1.0, w=280, h=200, tile=64, comp=33005, num_resolutions=3)
    outs = []
    for decode in ('host', 'gpu'):
        out = str(tmp_path / f'{decode}.tfrecords')
        info = extract_slide(eng, path, out, tile_um=64, decode=decode, img_format='png', canvas_bytes=1, batch=16)
        recs = [tfr.parse_example(r) for r in tfr.read_records(out, verify='full')]
        outs.append(([np.asarray(Image.open(io.BytesIO(r['image_raw']))) for r in recs], info))
    (host, hi), (gpu, gi) = outs
    assert len(host) == len(gpu) == 12 and all(np.array_equal(x, y) for x, y in zip(host, gpu))
    assert gi['decode_stats']['gpu_bands'] == 3 and gi['decode_stats']['host_bands'] == 0 and hi['decode_stats']['gpu_bands'] == 0
    assert os.path.getsize(str(tmp_path / 'gpu.tfrecords')) > 0
