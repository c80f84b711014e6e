"""What must not move when a tool's entry point moves to the file of its kernel: the profiling class each ``bq_*`` call opens, and
``Engine.close()`` letting go of every device tensor, whichever tool cached it.  One call of every tool at the smallest case its own
test file uses -- the feature map's three have theirs in tests/test_gpu_poison_umap.py: ``-m gpu``."""
import zlib

import numpy as np
import pytest
import torch

from biscuit_amd import stain
from biscuit_amd import tfrecord_native as tn
from biscuit_amd.synthetic import make_tiles
from biscuit_amd.weights import synthetic_weights
from biscuit_amd.wsi import TiffSlide
from tests import _jpeg_cases as jc
from tests import _j2k_cases as j2c
from tests import _jpeg_encode_cases as ec
from tests import _lzw_cases as lc
from tests import _roi_ref as roi_ref
from tests import _wsi_jpeg_cases as wj
from tests.test_wsi import _img

pytestmark = pytest.mark.gpu

# every class a tool's entry point opens; bq_stain_lab_stats, bq_png_unfilter, bq_png_unfilter_strided and bq_slide_finish open none
TOOL_CLASSES = {'stage_u8_standardize', 'stage_f32_to_planar', 'stain_reinhard_fast', 'stain_macenko', 'stain_macenko_stats',
                'range_key', 'range_screen', 'png_inflate', 'jpeg_decode', 'jpeg_decode_canvas', 'jpeg_encode_pixel',
                'jpeg_encode_size', 'jpeg_encode_pack', 'jpeg_encode_stuff', 'png_encode_filter', 'png_encode_match', 'png_encode_code',
                'png_encode_pack', 'j2k_t1', 'j2k_idwt', 'j2k_store', 'lzw_decode', 'lzw_place', 'tile_resample', 'tile_grayspace', 'heatmap_render',
                'tissue_blur', 'tissue_cells', 'tissue_focus', 'tissue_cells_union', 'roi_plane', 'slide_reduce', 'roc_youden'}


def _engine():
    from biscuit_amd.engine import Engine
    return Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)


def _up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# The helpers return what their calls wrote as host arrays -- the documented result regions only: inflated rows up to px (1 + 3 px)
# bytes (the stride's padding is unspecified, include/biscuit_hip.h), encoder bytes up to the last offset, canvases whole (the
# caller fills them first).  ``own_scratch``: every call that takes ``scratch=`` gets one of the size its ``*_scratch`` method
# states (tests/test_gpu_poison_tools.py runs them with allocations that are poisoned and guarded).
def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _png_tools(eng, px=8, own_scratch=False):
    """One zlib stream of px scanlines (filter type 0) through the inflate and both un-filter entries."""
    raw = np.random.default_rng(1).integers(0, 256, (px, 1 + 3 * px), dtype=np.uint8)
    raw[:, 0] = 0
    z = zlib.compress(raw.tobytes(), 6)
    buf = np.frombuffer(z + b'\0' * ((-(len(z) + 32)) % 16 + 32), np.uint8).copy()
    rows, status = eng.png_inflate(_up(eng, buf), _up(eng, np.zeros(1, np.int32)), _up(eng, np.array([len(z)], np.int32)), px,
                                   scratch=eng.inflate_scratch(1) if own_scratch else None)
    tiles = eng.png_unfilter_strided(rows, px)
    assert int(status[0]) == 0 and np.array_equal(tiles.cpu().numpy()[0], raw[:, 1:].reshape(px, px, 3))
    plain = eng.png_unfilter(_up(eng, raw[None]))
    assert torch.equal(plain, tiles)
    assert np.array_equal(rows[0, :raw.size].cpu().numpy(), raw.reshape(-1))
    return _host(rows[:, :px * (1 + 3 * px)], status, tiles, plain)


def _jpeg_tools(eng, tmp_path, own_scratch=False):
    """One 17-px tile decoded, one 16 x 16 segment decoded into a canvas, one 8-px tile encoded."""
    raw = jc.matrix(17)[0][0]
    scan, desc, tables = jc.extract_each(tmp_path, [raw], 17)[0]
    tiles, status = eng.jpeg_decode(_up(eng, scan), _up(eng, desc.view(np.int32)), _up(eng, tables), 17,
                                    scratch=eng.jpeg_scratch(1, 17) if own_scratch else None)
    assert int(status[0]) == 0 and np.array_equal(tiles.cpu().numpy()[0], jc.pillow(raw))
    path = wj.write_slide(tmp_path / 's.tif', [wj.page(_img(16, 16, 11), 16, 16, wj.SAMPLINGS['420'])])
    with TiffSlide(path) as s:
        sg = s.region_segments(0, 0, 0, 16, 16)
        scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)
        canvas = torch.full((16, 16, 3), 255, dtype=torch.uint8, device=eng.device)
        seg_status = eng.jpeg_decode_canvas(_up(eng, scan), _up(eng, desc.view(np.int32)), _up(eng, tables), sg.seg_w, sg.seg_h,
                                            _up(eng, sg.place), canvas, sg.clip,
                                            scratch=eng.jpeg_canvas_scratch(1, sg.seg_w, sg.seg_h) if own_scratch else None)
        assert len(sg) == 1 and int(seg_status[0]) == 0 and np.array_equal(canvas.cpu().numpy(), s.read_region(0, 0, 0, 16, 16))
    buf, off = eng.jpeg_encode(_up(eng, ec.tile(8, 'noise')[None].copy()), 95, '4:2:0',
                               scratch=eng.jpeg_encode_scratch(1, 8, '4:2:0') if own_scratch else None)
    assert ec.split(buf.cpu().numpy(), off) == [ec.pillow(8, 'noise', 95, '4:2:0')]
    return _host(tiles, status, canvas, seg_status, buf[:int(off[-1])], off)


def _png_encode_and_j2k_tools(eng, own_scratch=False):
    """One 8-px tile encoded as PNG, one lossless 16 x 16 JPEG 2000 segment decoded into a canvas."""
    tile = ec.tile(8, 'noise')[None].copy()
    buf, off = eng.png_encode(_up(eng, tile), scratch=eng.png_encode_scratch(1, 8) if own_scratch else None)
    want, want_off, _ = tn.png_encode(tile)
    assert np.array_equal(off.numpy(), want_off) and np.array_equal(buf.cpu().numpy(), want)
    a = _img(16, 16, 11)
    raw = j2c.encode(a, False, num_resolutions=2, mct=1)
    desc, blocks, cw = tn.j2k_extract(np.frombuffer(raw, np.uint8), [0], [len(raw)], 16, 16)
    canvas = torch.full((16, 16, 3), 255, dtype=torch.uint8, device=eng.device)
    status = eng.j2k_decode_canvas(_up(eng, desc), _up(eng, blocks), _up(eng, cw), 16, 16, _up(eng, np.zeros((1, 2), np.int32)), canvas,
                                   (0, 0, 16, 16), scratch=eng.j2k_canvas_scratch(1, 16, 16) if own_scratch else None)
    assert int(status[0]) == 0 and np.array_equal(canvas.cpu().numpy(), a)
    return _host(buf[:int(off[-1])], off, canvas, status)


def _lzw_segments(k):
    """``k`` 16 x 16 noise segments with predictor 2, packed for the decoder -> ``((data, desc), [pixels])``."""
    tiles = [lc.content('noise', 16, 16, seed) for seed in range(k)]
    raws = [lc.encode(lc.difference(t).tobytes()) for t in tiles]
    ln = [len(r) for r in raws]
    return tn.lzw_pack(np.frombuffer(b''.join(raws), np.uint8), np.cumsum([0] + ln[:-1]), ln), tiles


def _lzw_tool(eng, own_scratch=False):
    """One 16 x 16 LZW segment (noise, predictor 2) decoded into a white canvas: the CPU statement's bytes, and the pixels."""
    (data, desc), (a,) = _lzw_segments(1)
    place = np.zeros((1, 2), np.int32)
    want = np.full((16, 16, 3), 255, np.uint8)
    want_status = tn.lzw_decode_canvas(data, desc, 16, 16, place, want, (0, 0, 16, 16), predictor=2)
    canvas = torch.full((16, 16, 3), 255, dtype=torch.uint8, device=eng.device)
    status = eng.lzw_decode_canvas(_up(eng, data), _up(eng, desc.view(np.int32)), 16, 16, _up(eng, place), canvas, (0, 0, 16, 16), predictor=2,
                                   scratch=eng.lzw_canvas_scratch(1, 16, 16) if own_scratch else None)
    assert int(status[0]) == 0 == int(want_status[0]) and np.array_equal(canvas.cpu().numpy(), want) and np.array_equal(want, a)
    return _host(canvas, status)


def _heatmap_tools(eng):
    """A 16-px window resampled to 8 px, its grey pixels counted, and a one-cell heatmap drawn over a 3 x 5 thumbnail."""
    canvas = _up(eng, np.random.default_rng(2).integers(0, 256, (20, 24, 3), dtype=np.uint8))
    tiles = eng.tile_resample(canvas, _up(eng, np.array([[3, 2]], np.int32)), 16, 8)
    gray = eng.tile_grayspace(tiles)
    assert tuple(tiles.shape) == (1, 8, 8, 3) and tuple(gray.shape) == (1,)
    thumb = _up(eng, np.full((3, 5, 3), 100, np.uint8))
    from biscuit_amd.render import PRGN_TRUNC
    out = eng.heatmap_render(_up(eng, np.full((1, 1), 0.5, np.float32)), _up(eng, np.zeros(5, np.int32)), _up(eng, np.zeros(3, np.int32)),
                             _up(eng, PRGN_TRUNC), thumb)
    assert out.shape == thumb.shape
    return _host(tiles, gray, out)


def _mask_tools(eng):
    """A 5 x 7 thumbnail through blur, cells, focus and union with one cell, and one triangle through the ROI plane."""
    thumb = _up(eng, np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8))
    col, row = np.array([[0, 7]], np.int32), np.array([[0, 5]], np.int32)
    plane, hist = eng.tissue_blur(thumb)
    assert int(hist.sum()) == 35
    below = eng.tissue_cells(plane, 255, col, row)
    focus, n_out = eng.tissue_focus(thumb)
    assert int(below[0, 0]) == 35 and int(n_out[0]) == int((focus == 0).sum())
    union = eng.tissue_cells_union(plane, 0, focus, col, row)
    assert int(union[0, 0]) >= int(n_out[0])
    xs, ys, triangle = np.array([2, 6, 14], np.int32), np.array([2, 10], np.int32), [np.array([[0, 0], [8, 0], [0, 8]], np.int32)]
    roi = eng.roi_plane(xs, ys, triangle)
    assert np.array_equal(roi.cpu().numpy(), roi_ref.plane(xs, ys, triangle))
    return _host(plane, hist, below, focus, n_out, union, roi)


def test_every_tool_opens_its_profiling_class_and_no_other(tmp_path):
    from biscuit_amd.engine import RangeScreen
    eng = _engine()
    try:
        eng.profile_enable(True)
        tiles = _up(eng, make_tiles(1, seed=3))
        eng.stage(tiles)
        eng.stage_f32(tiles.float())
        eng.reinhard_fast(tiles, (60.0, 10.0, -5.0), (15.0, 8.0, 6.0))
        eng.lab_stats(tiles)
        eng.macenko(tiles, stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF)
        eng.macenko_stats(tiles)
        eng.range_key(tiles)
        RangeScreen(eng, k=1).update(tiles)
        _png_tools(eng)
        _jpeg_tools(eng, tmp_path)
        _png_encode_and_j2k_tools(eng)
        _lzw_tool(eng)
        _heatmap_tools(eng)
        _mask_tools(eng)
        mean = _up(eng, np.array([[0.25, 0.75]], np.float32))
        mp, mu, count = eng.slide_finish(eng.slide_reduce(mean, mean, _up(eng, np.zeros(1, np.int32)), 1))
        assert int(count[0]) == 1 and float(mp[0]) == 0.75
        assert eng.youden([0, 1], [0.2, 0.9])[1]['j'] == 1.0
        prof = eng.profile_read()
        assert {p.name for p in prof} == TOOL_CLASSES, {p.name for p in prof} ^ TOOL_CLASSES
        assert all(p.launches >= 1 for p in prof)
    finally:
        eng.close()


def _device_tensors(x):
    """Every torch tensor on a GPU reachable from ``x`` through lists, tuples, sets and dicts."""
    if torch.is_tensor(x):
        return [x] if x.is_cuda else []
    if isinstance(x, dict):
        x = list(x.keys()) + list(x.values())
    if isinstance(x, (list, tuple, set)):
        return [t for v in x for t in _device_tensors(v)]
    return []


def test_close_lets_go_of_every_device_tensor(tmp_path):
    """Every cache of the engine touched -- the grown scratch buffers and the per-tool tables --, then ``close()`` twice."""
    eng = _engine()
    _heatmap_tools(eng)             # tables: tile_resample (src_px != px), tile_grayspace
    _mask_tools(eng)                # tables: tissue_blur, tissue_focus; _host_held
    _png_tools(eng)                 # scratch: inflate
    _jpeg_tools(eng, tmp_path)      # scratch: jpeg, jpeg_encode
    _png_encode_and_j2k_tools(eng)  # scratch: png_encode, j2k
    _lzw_tool(eng)                  # scratch: lzw
    tables = {tool for (tool, key), v in eng._tables.items() if _device_tensors(v)}
    scratch = {family for family, v in eng._tool_ws.items() if _device_tensors(v)}
    assert {'tile_resample', 'tile_grayspace', 'tissue_blur', 'tissue_focus'} <= tables, tables
    assert {'inflate', 'jpeg', 'jpeg_encode', 'png_encode', 'j2k', 'lzw'} <= scratch, scratch
    eng.close()
    assert {k: v for k, v in vars(eng).items() if _device_tensors(v)} == {}
    eng.close()
    assert eng._ctx is None and {k: v for k, v in vars(eng).items() if _device_tensors(v)} == {}
