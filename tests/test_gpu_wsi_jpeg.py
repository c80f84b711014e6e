"""A slide's own JPEG tiles decoded on the device: ``Engine.jpeg_decode_canvas`` against its CPU statement and against
``TiffSlide.read_region`` (Pillow) byte for byte, ``Heatmap.from_slide(decode='gpu')`` against ``decode='host'`` bit for bit with
the path each band took counted, the fallback, and the ``--gpu-decode`` command line: ``-m gpu``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.wsi import WSI, SlideError, TiffSlide
from tests._wsi_jpeg_cases import SAMPLINGS, SHAPES, jpeg, page, slide_file, write_slide
from tests.test_wsi import _img

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTE = 2, 0xA5              # rows in front of and behind the device canvas


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=4)
    yield e
    e.close()


def _device_canvas(eng, sg, packed, scratch=None):
    """One ``jpeg_decode_canvas`` call into a white canvas that stands between guard rows.  -> (canvas, status) on the host"""
    scan, desc, tables = packed
    dev = eng.device
    h, w = sg.shape
    buf = torch.full(((h + 2 * GUARD) * w * 3,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    canvas = buf[GUARD * w * 3:(GUARD + h) * w * 3].view(h, w, 3)
    canvas.fill_(255)
    status = eng.jpeg_decode_canvas(torch.from_numpy(scan).to(dev), torch.from_numpy(desc.view(np.int32)).to(dev),
                                    torch.from_numpy(tables).to(dev), sg.seg_w, sg.seg_h, torch.from_numpy(sg.place).to(dev), canvas,
                                    sg.clip, scratch=scratch)
    torch.cuda.synchronize(dev)
    flat = buf.cpu().numpy()
    assert (flat[:GUARD * w * 3] == GUARD_BYTE).all() and (flat[(GUARD + h) * w * 3:] == GUARD_BYTE).all(), 'guard rows touched'
    return flat[GUARD * w * 3:(GUARD + h) * w * 3].reshape(h, w, 3), status.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_%dx%d' % s)
@pytest.mark.parametrize('sampling', sorted(SAMPLINGS))
def test_device_canvas_equals_cpu_canvas_equals_read_region(eng, tmp_path, shape, sampling):
    w, h, tw, th = shape
    path = write_slide(tmp_path / 's.tif', [page(_img(w, h, 11), tw, th, SAMPLINGS[sampling])])
    coef = 3 * (2 * -(-tw // 16)) * (2 * -(-th // 16)) * 128           # three planes of whole 16 x 16 units, 128 bytes a block
    assert coef == int(eng._lib.bq_jpeg_canvas_scratch_bytes(1, tw, th))
    with TiffSlide(path) as s:
        # the whole level with a white margin (guard columns: the margin is part of the comparison); then a window of odd width
        # (3 W odd: rows start at every alignment) that cuts segments on all four sides, with scratch for two segments only,
        # so that the round loop runs several times
        for (x, y, ww, hh), rounds in (((-10, -10, w + 20, h + 20), False), ((5, 1, w - 11, h - 3), True)):
            assert not rounds or (3 * ww) % 2 == 1
            sg = s.region_segments(0, x, y, ww, hh)
            assert not rounds or len(sg) > 2
            packed = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)
            scratch = torch.empty(2 * coef + 100, dtype=torch.uint8, device=eng.device) if rounds else None
            got, status = _device_canvas(eng, sg, packed, scratch)
            cpu = np.full((hh, ww, 3), 255, np.uint8)
            cpu_status = tn.jpeg_decode_canvas(*packed, sg.seg_w, sg.seg_h, sg.place, cpu, sg.clip)
            assert (status == 0).all() and np.array_equal(status, cpu_status)
            assert np.array_equal(got, cpu), (x, y)
            assert np.array_equal(got, s.read_region(0, x, y, ww, hh)), (x, y)


def test_clip_and_places_outside_the_canvas_write_nothing_else(eng, tmp_path):
    """Segments placed partly and wholly outside the canvas, a clip rectangle narrower than the canvas and one that reaches
    beyond it: the device writes what the CPU statement writes -- and a refused descriptor writes nothing."""
    a = _img(128, 128, 21)
    path = write_slide(tmp_path / 's.tif', [page(a, 64, 64, 2)])
    with TiffSlide(path) as s:
        sg = s.region_segments(0, 0, 0, 128, 128)
    scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, 64, 64, sg.jpeg_tables)
    sg.shape = (75, 91)
    sg.place = np.array([[-30, -20], [60, -63], [-64, 40], [90, 74]], np.int32)           # the last two: wholly outside
    for clip in ((0, 0, 91, 75), (7, 5, 80, 60), (-1000, -1000, 1 << 30, 1 << 30), (50, 50, 50, 60)):
        sg.clip = clip
        got, status = _device_canvas(eng, sg, (scan, desc, tables))
        cpu = np.full((75, 91, 3), 255, np.uint8)
        assert np.array_equal(tn.jpeg_decode_canvas(scan, desc, tables, 64, 64, sg.place, cpu, clip), status) and (status == 0).all()
        assert np.array_equal(got, cpu), clip
        outside = np.ones((75, 91), bool)
        outside[max(clip[1], 0):max(clip[3], 0), max(clip[0], 0):max(clip[2], 0)] = False
        assert (got[outside] == 255).all()
    assert (got == 255).all()                                                              # (the empty rectangle came last)
    bad = desc.copy()
    bad[0, 2] = 3 | 1 << 8 | 3 << 16                                                      # no sampling of the subset
    sg.clip = (0, 0, 91, 75)
    got, status = _device_canvas(eng, sg, (scan, bad, tables))
    cpu = np.full((75, 91, 3), 255, np.uint8)
    assert np.array_equal(tn.jpeg_decode_canvas(scan, bad, tables, 64, 64, sg.place, cpu, sg.clip), status) and status[0] == 16
    assert np.array_equal(got, cpu) and (got[:44, :34] == 255).all()


def _same(a, b):
    return np.array_equal(a.logits, b.logits) and np.array_equal(a.uncertainty, b.uncertainty) and np.array_equal(a.grid, b.grid)


KW = dict(mc_n=4, seed=3, batch=16, canvas_bytes=1)       # canvas_bytes = 1: one grid row per band


# mpp 1.01: 299 level-0 pixels a tile (copied, 8 x 6 grid); 0.5045: 598 pixels resampled to 299 (4 x 3); 0.2525 with stride_div 4:
# 1196 level-0 pixels = 299 of the 4:4:4 level 1, whose border tiles are cut by the 600 x 450 page (5 x 3)
@pytest.mark.parametrize('mpp,stride_div,level,src_px,bands', [(1.01, 1, 0, 299, 6), (0.5045, 1, 0, 598, 3), (0.2525, 4, 1, 299, 3)])
def test_heatmap_with_device_decode_equals_host_decode(eng, tmp_path, mpp, stride_div, level, src_px, bands):
    from biscuit_amd.heatmap import Heatmap
    path = slide_file(tmp_path, mpp)
    w = WSI(path, stride_div=stride_div)
    assert (w.level, w.src_px, w.grid_h) == (level, src_px, bands)
    n_seg = sum(len(b[4]) for b in w.bands(1, segments=True))
    w.close()
    host = Heatmap.from_slide(eng, path, stride_div=stride_div, decode='host', **KW)
    gpu = Heatmap.from_slide(eng, path, stride_div=stride_div, decode='gpu', **KW)
    assert _same(gpu, host) and (host.logits >= 0).all()
    assert host.decode_stats == {'gpu_bands': 0, 'host_bands': bands, 'segments': 0}
    assert gpu.decode_stats == {'gpu_bands': bands, 'host_bands': 0, 'segments': n_seg} and bands >= 3 and n_seg > bands
    with pytest.raises(ValueError):
        Heatmap.from_slide(eng, path, resample='host', decode='gpu')
    with pytest.raises(ValueError):
        Heatmap.from_slide(eng, path, decode='device')


def test_fallback_is_loud_and_exact(eng, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    from tests.test_wsi import _slide_file
    a = _img(2400, 1800, 5)
    index, rect = 1 * 10 + 2, (512, 256, 768, 512)           # the level-0 tile at (tx 2, ty 1) of 10 across

    def restart(pages):
        pages[0]['segs'][index] = jpeg(a[256:512, 512:768], subsampling=2, streamtype=2, restart_marker_blocks=4)
    path = slide_file(tmp_path, 0.5045, mutate=restart, name='restart.svs')
    w = WSI(path)
    touched = total = 0
    for gy0, gy1, gx0, gx1, sg, origin, src_px in w.bands(1, segments=True):
        (x0, y0, cw, ch), _, _ = w._band_rect(gy0, gy1, gx0, gx1)
        touched += x0 < rect[2] and rect[0] < x0 + cw and y0 < rect[3] and rect[1] < y0 + ch
        total += 1
    w.close()
    assert touched == 1 and total == 3
    host = Heatmap.from_slide(eng, path, decode='host', **KW)
    gpu = Heatmap.from_slide(eng, path, decode='gpu', **KW)
    assert _same(gpu, host)
    assert gpu.decode_stats['host_bands'] == touched and gpu.decode_stats['gpu_bands'] == total - touched
    # a truncated segment: the host's error under both, or -- where Pillow tolerates the truncation -- the host's arrays

    def truncate(pages):
        pages[0]['segs'][index] = pages[0]['segs'][index][:len(pages[0]['segs'][index]) // 2]
    path = slide_file(tmp_path, 0.5045, mutate=truncate, name='truncated.svs')
    try:
        host = Heatmap.from_slide(eng, path, decode='host', **KW)
    except SlideError:
        host = None
    if host is None:
        with pytest.raises(SlideError):
            Heatmap.from_slide(eng, path, decode='gpu', **KW)
    else:
        gpu = Heatmap.from_slide(eng, path, decode='gpu', **KW)
        assert _same(gpu, host) and gpu.decode_stats['host_bands'] == touched
    # a level that is not a tiled JPEG page: every band is the host's, and says so
    deflate, _ = _slide_file(tmp_path)
    gpu = Heatmap.from_slide(eng, deflate, decode='gpu', **KW)
    assert _same(gpu, Heatmap.from_slide(eng, deflate, **KW)) and gpu.decode_stats == {'gpu_bands': 0, 'host_bands': 3, 'segments': 0}


def test_command_line_gpu_decode(tmp_path):
    path = slide_file(tmp_path, 0.5045)
    w = WSI(path)
    n_seg = sum(len(b[4]) for b in w.bands(segments=True))
    w.close()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    outs = []
    for flag in ([], ['--gpu-decode']):
        out = str(tmp_path / ('out' + str(len(flag))))
        p = subprocess.run([sys.executable, '-m', 'biscuit_amd.heatmap', path, '--out', out, '--mc', '4', '--seed', '3', '--batch', '16'] + flag,
                           capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append((np.load(os.path.join(out, 'heatmap.npz')), json.load(open(os.path.join(out, 'summary.json')))))
    (za, sa), (zb, sb) = outs
    assert sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files)
    assert sa['decode_stats'] == {'gpu_bands': 0, 'host_bands': 1, 'segments': 0}
    assert sb['decode_stats'] == {'gpu_bands': 1, 'host_bands': 0, 'segments': n_seg} and sb['tiles_run'] == sa['tiles_run'] == 12
