"""The tools on memory whose contents are unspecified (DESIGN.md "Buffer contract"): every output tensor and every scratch buffer
``Engine`` allocates is poisoned and guarded (tests/_poison.py) with each of the bytes 0x00, 0xFF and 0xA5, a caller's own scratch
likewise, and every tool has to give the same bytes under all three -- the bytes its own reference states --, with every guard
intact.  One smallest call of every tool (the helpers of tests/test_gpu_abi_homes.py), then per tool the smallest case of its own
test file that takes more than one round, strip or block: rounds are where scratch is reused inside a call.  ``-m gpu``."""
import numpy as np
import pytest
import torch

from biscuit_amd import stain
from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from biscuit_amd.synthetic import make_tiles
from tests import _focus_ref as focus_ref
from tests import _j2k_cases as j2c
from tests import _jpeg_cases as jc
from tests import _jpeg_encode_cases as ec
from tests import _png_encode_cases as pc
from tests import _poison as P
from tests import _range_ref as range_ref
from tests import _resample_ref as resample_ref
from tests import _tissue_ref as tissue_ref
from tests import test_gpu_abi_homes as homes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = homes._engine()
    yield e
    e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def under_every_fill(eng, fn):
    """``fn()`` -> list of host arrays, once per byte fill with every allocation of the engine poisoned and guarded and its cached
    scratch buffers dropped first (so that they are allocated again, poisoned); the results equal across fills, the guards intact."""
    import biscuit_amd.engine as engine_mod
    results = []
    for fill in P.BYTE_FILLS:
        torch.cuda.synchronize(eng.device)
        eng.drop_scratch()
        proxy = P.poisoned_torch(fill)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, 'torch', proxy)
            out = fn()
        torch.cuda.synchronize(eng.device)
        assert proxy.served >= 1
        proxy.check()
        results.append(out)
    first = results[0]
    for fill, other in zip(P.BYTE_FILLS[1:], results[1:]):
        assert len(other) == len(first)
        for k, (a, b) in enumerate(zip(first, other)):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), f'result {k} under 0x{fill:02X} differs from 0x00'
    return first


# ------------------------------------------------------------------------------------------------ one smallest call of every tool
def test_stage_stain_range_and_slide_tools(eng):
    from biscuit_amd.engine import RangeScreen
    from oracle.xception_ref import standardize
    t = make_tiles(1, seed=3)
    tiles = up(eng, t)

    def calls():
        scr = RangeScreen(eng, k=1)                      # (its slots and workspace are the engine module's allocations too)
        scr.update(tiles, tile_idx0=9)
        mean = up(eng, np.array([[0.25, 0.75]], np.float32))
        mp, mu, count = eng.slide_finish(eng.slide_reduce(mean, mean, up(eng, np.zeros(1, np.int32)), 1))
        thr, info = eng.youden([0, 1, 1, 0, 1], [0.2, 0.9, 0.6, 0.4, 0.3])
        stats, st = eng.macenko_stats(tiles)
        return host(eng.stage(tiles).float(), eng.stage_f32(tiles.float()).float(), eng.reinhard_fast(tiles, (60.0, 10.0, -5.0), (15.0, 8.0, 6.0)),
                    eng.lab_stats(tiles), eng.macenko(tiles, stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF), stats, st, eng.range_key(tiles),
                    *scr.candidates(), scr.tiles, mp, mu, count) + [np.array([thr, info['j'], info['tpr'], info['fpr']])]
    out = under_every_fill(eng, calls)
    assert np.array_equal(out[0], standardize(t).to(torch.float16).float().numpy())
    assert np.array_equal(out[7].view(np.uint32), range_ref.range_key(t).view(np.uint32))
    assert np.array_equal(out[8].view(np.uint32), out[7].view(np.uint32)) and out[9].tolist() == [9] and np.array_equal(out[10], t)
    assert float(out[11][0]) == 0.75 and int(out[13][0]) == 1
    assert out[14][0] == 0.6 and abs(out[14][1] - 2 / 3) < 1e-12            # (J peaks behind the two best scores, both positive)


def test_png_tools(eng):
    under_every_fill(eng, lambda: homes._png_tools(eng, own_scratch=True))
    under_every_fill(eng, lambda: homes._png_tools(eng))


def test_jpeg_tools(eng, tmp_path):
    under_every_fill(eng, lambda: homes._jpeg_tools(eng, tmp_path, own_scratch=True))
    under_every_fill(eng, lambda: homes._jpeg_tools(eng, tmp_path))


def test_png_encode_and_j2k_tools(eng):
    under_every_fill(eng, lambda: homes._png_encode_and_j2k_tools(eng, own_scratch=True))
    under_every_fill(eng, lambda: homes._png_encode_and_j2k_tools(eng))


def test_lzw_tool(eng):
    under_every_fill(eng, lambda: homes._lzw_tool(eng, own_scratch=True))
    under_every_fill(eng, lambda: homes._lzw_tool(eng))


def test_heatmap_tools(eng):
    under_every_fill(eng, lambda: homes._heatmap_tools(eng))


def test_mask_tools(eng):
    under_every_fill(eng, lambda: homes._mask_tools(eng))


# ------------------------------------------------------------------------------------------------ more than one round, strip or block
def test_inflate_more_streams_than_a_wave_holds_tables_for(eng):
    """70 streams of 8-px tiles (two waves of lanes, a slice of the scratch each) through both variants of the inflate."""
    import zlib
    px, n = 8, 70
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 256, (n, px, 1 + 3 * px), dtype=np.uint8)
    raw[:, :, 0] = rng.integers(0, 5, (n, px))
    raw[::3, :, 1:] //= 64                                      # (compressible ones: matches and dynamic blocks)
    parts, off, ln = [], [], []
    at = 0
    for i in range(n):
        z = zlib.compress(raw[i].tobytes(), 6)
        off.append(at); ln.append(len(z))
        parts.append(z + b'\0' * ((-len(z)) % 16))
        at += len(parts[-1])
    buf = np.frombuffer(b''.join(parts) + b'\0' * 32, np.uint8).copy()

    def call():
        rows, status = eng.png_inflate(up(eng, buf), up(eng, np.array(off, np.int32)), up(eng, np.array(ln, np.int32)), px,
                                       scratch=eng.inflate_scratch(n))
        return host(rows[:, :px * (1 + 3 * px)], status, eng.png_unfilter_strided(rows, px))
    try:
        for variant in (5, 0):
            eng.set_option('inflate_variant', variant)
            rows, status, _ = under_every_fill(eng, call)
            assert not status.any() and np.array_equal(rows, raw.reshape(n, -1)), variant
    finally:
        eng.set_option('inflate_variant', 5)


def test_jpeg_decode_of_several_tiles(eng, tmp_path):
    """Five 17-px tiles of different samplings in one call with a scratch of the caller's (``bq_jpeg_decode`` takes rounds only beyond
    2 048 tiles; the canvas entry below is the same kernels in rounds)."""
    raws = [r for r, _ in jc.matrix(17)[:5]]
    path = str(tmp_path / 'r.tfrecords')
    tfr.write_slide(path, 'r', raws, np.zeros((len(raws), 2), np.int64))
    scan, desc, tables = jc.extract(path, 0, len(raws), 17)

    def call():
        return host(*eng.jpeg_decode(up(eng, scan), up(eng, desc.view(np.int32)), up(eng, tables), 17, scratch=eng.jpeg_scratch(5, 17)))
    tiles, status = under_every_fill(eng, call)
    assert not status.any() and all(np.array_equal(tiles[i], jc.pillow(r)) for i, r in enumerate(raws))


def test_jpeg_canvas_in_rounds(eng, tmp_path):
    """A 48 x 32 page of 16 x 16 tiles read through a window that cuts segments on all four sides, with scratch for two segments:
    several rounds; the bytes ``read_region`` gives."""
    from biscuit_amd.wsi import TiffSlide
    from tests import _wsi_jpeg_cases as wj
    from tests.test_wsi import _img
    path = wj.write_slide(tmp_path / 's.tif', [wj.page(_img(48, 32, 11), 16, 16, wj.SAMPLINGS['420'])])
    with TiffSlide(path) as s:
        sg = s.region_segments(0, 5, 1, 37, 29)
        want = s.read_region(0, 5, 1, 37, 29)
    assert len(sg) > 2
    scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)

    def call():
        canvas = torch.full((29, 37, 3), 255, dtype=torch.uint8, device=eng.device)
        status = eng.jpeg_decode_canvas(up(eng, scan), up(eng, desc.view(np.int32)), up(eng, tables), sg.seg_w, sg.seg_h, up(eng, sg.place),
                                        canvas, sg.clip, scratch=eng.jpeg_canvas_scratch(2, sg.seg_w, sg.seg_h))
        return host(canvas, status)
    canvas, status = under_every_fill(eng, call)
    assert not status.any() and np.array_equal(canvas, want)


def test_j2k_decode_in_rounds(eng):
    """Three 32 x 16 segments, both transforms, with scratch for two: two rounds; the CPU statement's bytes."""
    raws = [j2c.encode(j2c.content('photo' if k else 'noise', 32, 16, k), k == 1, num_resolutions=2, mct=1) for k in range(3)]
    ln = [len(r) for r in raws]
    packed = tn.j2k_extract(np.frombuffer(b''.join(raws), np.uint8), np.cumsum([0] + ln[:-1]), ln, 32, 16)
    place = np.array([[0, 0], [33, 3], [-5, 17]], np.int32)             # (cut by the canvas and the clip; no two overlap)
    want = np.full((24, 70, 3), 255, np.uint8)
    want_status = tn.j2k_decode_canvas(*packed, 32, 16, place, want, (1, 0, 69, 23))

    def call():
        canvas = torch.full((24, 70, 3), 255, dtype=torch.uint8, device=eng.device)
        status = eng.j2k_decode_canvas(*(up(eng, a) for a in packed), 32, 16, up(eng, place), canvas, (1, 0, 69, 23),
                                       scratch=eng.j2k_canvas_scratch(2, 32, 16))
        return host(canvas, status)
    canvas, status = under_every_fill(eng, call)
    assert np.array_equal(status, want_status) and not status.any() and np.array_equal(canvas, want)


def test_lzw_decode_in_rounds(eng):
    """Three 16 x 16 segments with scratch for one: three rounds, each over the bytes the round before left; the CPU statement's bytes."""
    (data, desc), tiles = homes._lzw_segments(3)
    place = np.array([[0, 0], [16, 0], [32, 0]], np.int32)
    want = np.full((16, 48, 3), 255, np.uint8)
    want_status = tn.lzw_decode_canvas(data, desc, 16, 16, place, want, (0, 0, 48, 16), predictor=2)
    assert np.array_equal(want, np.concatenate(tiles, 1))

    def call():
        canvas = torch.full((16, 48, 3), 255, dtype=torch.uint8, device=eng.device)
        status = eng.lzw_decode_canvas(up(eng, data), up(eng, desc.view(np.int32)), 16, 16, up(eng, place), canvas, (0, 0, 48, 16), predictor=2,
                                       scratch=eng.lzw_canvas_scratch(1, 16, 16))
        return host(canvas, status)
    canvas, status = under_every_fill(eng, call)
    assert np.array_equal(status, want_status) and not status.any() and np.array_equal(canvas, want)


def test_jpeg_encode_in_rounds(eng):
    """Five mixed 17-px tiles with scratch for two: three rounds; the files of the CPU build, which tests/test_jpeg_encode.py holds
    to Pillow's."""
    tiles = ec.mixed(5, px=17)
    want, want_off, _ = tn.jpeg_encode(tiles, 95, '4:2:0')

    def call():
        buf, off = eng.jpeg_encode(up(eng, tiles), 95, '4:2:0', scratch=eng.jpeg_encode_scratch(2, 17, '4:2:0'))
        return host(buf[:int(off[-1])], off)
    buf, off = under_every_fill(eng, call)
    assert np.array_equal(off, want_off) and np.array_equal(buf, want)


@pytest.mark.parametrize('px', [17, 74])
def test_png_encode_in_rounds_and_blocks(eng, px):
    """Three tiles with scratch for two (two rounds); at 74 px a tile's filtered bytes are two deflate blocks."""
    tiles = np.stack([pc.tile(px, w) for w in ('noise', 'synthetic', 'rows')])
    want, want_off, _ = tn.png_encode(tiles)

    def call():
        buf, off = eng.png_encode(up(eng, tiles), scratch=eng.png_encode_scratch(2, px))
        return host(buf[:int(off[-1])], off)
    buf, off = under_every_fill(eng, call)
    assert np.array_equal(off, want_off) and np.array_equal(buf, want)


@pytest.mark.parametrize('src,px', [(16, 8), (8, 16), (8, 8)])
def test_tile_resample_with_windows_that_leave_the_canvas(eng, src, px):
    canvas, origin = resample_ref.case(src)
    want = resample_ref.pillow_tiles(canvas, origin, src, px)
    got, gray = under_every_fill(eng, lambda: host(*(lambda t: (t, eng.tile_grayspace(t)))(eng.tile_resample(up(eng, canvas), up(eng, origin), src, px))))
    assert np.array_equal(got, want)
    assert gray.shape == (len(origin),)


def test_masks_of_a_37_x_53_thumbnail(eng):
    """Blur, cells, focus and union on a thumbnail of several strips and a grid of 3 x 4 cells, against the numpy restatements."""
    thumb = np.random.default_rng(6).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    thumb[3:35, 4:50] = 200                                     # a flat, bright area: out of focus in its middle, unsaturated
    col = np.array([[0, 14], [13, 27], [27, 40], [40, 53]], np.int32)
    row = np.array([[0, 13], [12, 25], [25, 37]], np.int32)
    plane_ref, hist_ref = tissue_ref.blur(thumb)
    T = tissue_ref.otsu(hist_ref)
    focus_plane_ref, n_out_ref, v_ref = focus_ref.focus(thumb, focus_ref.units(0.02))

    def calls():
        plane, hist = eng.tissue_blur(up(eng, thumb))
        below = eng.tissue_cells(plane, T, col, row)
        focus, n_out, v = eng.tissue_focus(up(eng, thumb), value=True)
        union = eng.tissue_cells_union(plane, T, focus, col, row)
        return host(plane, hist, below, focus, n_out, v, union)
    plane, hist, below, focus, n_out, v, union = under_every_fill(eng, calls)
    assert np.array_equal(plane, plane_ref) and np.array_equal(hist, hist_ref)
    assert np.array_equal(below, tissue_ref.cell_counts(plane_ref, T, col, row))
    assert np.array_equal(focus, focus_plane_ref) and int(n_out[0]) == n_out_ref and np.array_equal(v, v_ref)
    assert np.array_equal(union, focus_ref.union_counts(plane_ref, T, focus_plane_ref, col, row))
    assert 0 < n_out_ref < 37 * 53
