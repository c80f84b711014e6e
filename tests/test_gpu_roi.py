"""The heatmap's region-of-interest mask on the device (DESIGN.md "Heatmap input", Region-of-interest mask): ``Engine.roi_plane``
against the numpy restatement (tests/_roi_ref.py) integer for integer on the planes and polygons of the CPU test, its refusals,
``Heatmap.from_slide(rois=...)`` against the unmasked run bit for bit, and the command line: ``-m gpu``."""
import json
import os

import numpy as np
import pytest

from tests import _roi_cases as C
from tests import _roi_ref as R
from tests.test_gpu_tissue import _deflate_slide, _jpeg_slide

pytestmark = pytest.mark.gpu

KW = dict(mc_n=8, seed=3, batch=16, canvas_bytes=1)
GEOM = dict(gw=4, gh=3, slide_w0=2400, slide_h0=1800, stride=598, extract_px=598)     # the synthetic slide's grid (MPP 0.5045, 302 um)
# an L over the cells (0, 0), (1, 0) and (0, 1) by their centres (299 + 598 g); no cell of grid row 2
ELL = [np.array([[0, 0], [1196, 0], [1196, 598], [598, 598], [598, 1196], [0, 1196]], np.int32)]
# a triangle that cuts cells: shares strictly between 0 and 1
TRIANGLE = [np.array([[100, 50], [2000, 300], [700, 1500]], np.int32)]


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=8)
    yield e
    e.close()


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', C.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plane_equals_reference(eng, size):
    import torch
    w0, h0, xs, ys = C.geometry(size)
    want = C.expected(size)
    for name, polys in C.polygon_cases(size).items():
        d = eng.roi_plane(xs, ys, polys)
        assert torch.is_tensor(d) and d.dtype == torch.uint8 and tuple(d.shape) == size and d.device == eng.device
        got = d.cpu().numpy()
        assert np.array_equal(got, want[name]), (name, size, int((got != want[name]).sum()))
        C.check_known(size, name, got)


def test_rows_on_every_alignment(eng):
    """W = 131 puts the rows of a plane on all four byte alignments; a plane of exactly one dword a row and one of 1 025 pixels (the
    257th pixel group, a second workgroup) on top."""
    polys = [np.array([[3, 2], [5000, 40], [2500, 900], [20, 700]], np.int32), np.array([[0, 0], [9000, 0], [9000, 3]], np.int32)]
    for w, h in ((4, 9), (1025, 5), (1024, 3), (7, 6)):
        xs = np.array([((2 * x + 1) * 9100) // w for x in range(w)], np.int32)
        ys = np.array([((2 * y + 1) * 1000) // h for y in range(h)], np.int32)
        got = eng.roi_plane(xs, ys, polys).cpu().numpy()
        assert np.array_equal(got, R.plane(xs, ys, polys)), (w, h)


def test_bad_arguments(eng):
    """Argument checks only: every refusal is BQ_ERR_ARG (-1) from the C entry before anything is enqueued."""
    import torch
    dev = eng.device
    tri = np.array([[0, 0, 8, 0], [8, 0, 0, 8], [0, 8, 0, 0]], np.int32)
    six = np.concatenate([tri, tri])
    xs, ys = np.array([1, 3, 5], np.int32), np.array([1, 3], np.int32)
    tables = torch.zeros(4 * 6 + 3 + 3 + 2, dtype=torch.int32, device=dev)
    plane = torch.full((2, 3), 7, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(e=tri, s=(0, 3), x=xs, y=ys, tb=tables.data_ptr(), pl=plane.data_ptr(), E=None, P=None, W=None, H=None):
        e, s = np.ascontiguousarray(e, np.int32), np.ascontiguousarray(s, np.int32)
        x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
        r = eng._lib.bq_roi_plane(eng._ctx, e.ctypes.data, len(e) if E is None else E, s.ctypes.data, len(s) - 1 if P is None else P,
                                  x.ctypes.data, len(x) if W is None else W, y.ctypes.data, len(y) if H is None else H, tb, pl, st)
        torch.cuda.synchronize(dev)                                          # (the host tables of a good call are locals)
        return r
    big = np.tile(tri, ((1 << 20) // 3 + 1, 1))
    bad_v, bad_x = tri.copy(), xs.copy()
    bad_v[1, 2] = (1 << 28) + 1
    bad_x[2] = (1 << 29) + 1
    for kw in (dict(tb=None), dict(pl=None), dict(tb=tables.data_ptr() + 4), dict(W=0), dict(H=0), dict(E=2), dict(P=0),
               dict(x=np.ones(1 << 16, np.int32), y=np.ones(1 << 15, np.int32)),                            # H * W = 2^31
               dict(e=six, s=(0, 6, 6)), dict(e=six, s=(0, 2, 6)), dict(e=six, s=(0, 3, 7)), dict(e=six, s=(1, 3, 6)),
               dict(e=big, s=np.arange(0, len(big) + 1, 3)),                                                 # E over the cap
               dict(e=bad_v), dict(x=bad_x), dict(y=np.array([-1, 3], np.int32))):
        assert call(**kw) == -1, list(kw)
    assert b'bq_roi_plane' in eng._lib.bq_last_error(eng._ctx)
    assert (plane.cpu().numpy() == 7).all()                                  # nothing was enqueued
    assert call() == 0 and plane.cpu().numpy().tolist() == [[1, 1, 1], [1, 1, 0]]
    assert call(e=six, s=(0, 3, 6)) == 0 and plane.cpu().numpy().tolist() == [[1, 1, 1], [1, 1, 0]]      # twice the triangle: a union
    good = [np.array([[0, 0], [4, 0], [0, 4]], np.int32)]
    for bad in (dict(xs=bad_x), dict(ys=np.zeros((2, 2), np.int32)), dict(xs=np.zeros(0, np.int32)),
                dict(polygons=[np.array([[0, 0], [1, 1]])]), dict(polygons=[]), dict(polygons=[np.array([[0, 0], [1 << 28, 0], [0, 1]])])):
        with pytest.raises(ValueError):
            eng.roi_plane(**dict(dict(xs=xs, ys=ys, polygons=good), **bad))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _compare(hm, full, keep):
    from biscuit_amd.heatmap import MASKED
    assert np.array_equal(hm.cell_mask, keep) and hm.cell_mask.dtype == np.bool_
    assert np.array_equal(hm.logits[keep], full.logits[keep]) and np.array_equal(hm.uncertainty[keep], full.uncertainty[keep])
    assert (hm.logits[~keep] == MASKED).all() and (hm.uncertainty[~keep] == MASKED).all()
    assert hm.dropped == int((~keep).sum()) == hm.qc['cells_dropped']
    assert sorted(map(tuple, hm.grid.tolist())) == sorted((int(x), int(y)) for y, x in zip(*np.nonzero(keep)))
    assert hm.qc['bands_skipped_rows'] == int((~keep.any(1)).sum()) and hm.qc['bands_read'] == int(keep.any(1).sum())     # canvas_bytes = 1


@pytest.fixture(scope='module')
def slide(eng, tmp_path_factory):
    """The deflate slide, its unmasked heatmap and the restatement's masks, computed once."""
    from biscuit_amd.heatmap import Heatmap
    path = _deflate_slide(tmp_path_factory.mktemp('roi'))
    full = Heatmap.from_slide(eng, path, **KW)
    assert full.roi is None and full.cell_mask is None and full.dropped == 0 and full.logits.shape == (3, 4, 2)
    xs, ys = R.center_tables(GEOM['gw'], GEOM['gh'], GEOM['stride'], GEOM['extract_px'])
    centre = R.keep_center(R.plane(xs, ys, ELL), 'inside')
    assert centre.tolist() == [[True, True, False, False], [True, False, False, False], [False] * 4]
    return path, full, centre


def test_default_is_the_unmasked_run(eng, slide):
    from biscuit_amd.heatmap import Heatmap
    path, full, centre = slide
    for kw in (dict(rois=None, roi_method='auto', roi_filter_method=0.5, roi_width=100), dict(rois=ELL, roi_method='ignore')):
        hm = Heatmap.from_slide(eng, path, **kw, **KW)
        assert hm.roi is None and hm.qc is None and hm.cell_mask is None and hm.dropped == 0
        assert hm.logits.tobytes() == full.logits.tobytes() and hm.uncertainty.tobytes() == full.uncertainty.tobytes()
        assert np.array_equal(hm.grid, full.grid) and hm.decode_stats == full.decode_stats
    for bad in (dict(roi_method='within'), dict(roi_filter_method=0.0), dict(roi_filter_method=1.5), dict(roi_width=0), dict(roi_method='inside'),
                dict(rois=ELL, resample='host'), dict(rois=[np.zeros((2, 2), np.int32)])):                    # its keywords, on or off
        with pytest.raises(ValueError):
            Heatmap.from_slide(eng, path, **bad, **KW)


def test_centre_method_keeps_cells_bit_for_bit(eng, slide):
    from biscuit_amd.heatmap import Heatmap
    path, full, centre = slide
    hm = Heatmap.from_slide(eng, path, rois=ELL, **KW)                       # 'auto' with polygons: inside; 'center'
    _compare(hm, full, centre)
    assert hm.roi == {'method': 'inside', 'filter': 'center', 'polygons': 1, 'vertices': 6, 'cells_dropped': 9}
    assert hm.qc['bands_skipped_rows'] == 1 and hm.qc['bands_read'] == 2 and hm.qc['method'] is None
    assert set(hm.qc) == {'method', 'threshold', 'cells_dropped', 'bands_read', 'bands_skipped_rows'}
    out = Heatmap.from_slide(eng, path, rois=ELL, roi_method='outside', **KW)
    _compare(out, full, ~centre)
    assert out.roi['method'] == 'outside' and out.roi['cells_dropped'] == 3 and out.qc['bands_skipped_rows'] == 0


def test_share_equals_reference(eng, slide, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path, full, centre = slide
    xs, ys = R.raster_tables(2400, 1800, 600)
    pl = R.plane(xs, ys, TRIANGLE)
    want = R.keep_share(pl, share=0.5, method='inside', **GEOM)
    assert 0 < want.sum() < want.size and not np.array_equal(want, R.keep_share(pl, share=0.05, method='inside', **GEOM))
    csv = tmp_path / 'tri.csv'
    csv.write_text('ROI_Name,X_base,Y_base\n' + ''.join(f't,{x},{y}\n' for x, y in TRIANGLE[0].tolist()))
    hm = Heatmap.from_slide(eng, path, rois=str(csv), roi_filter_method=0.5, roi_width=600, **KW)           # (a CSV path, too)
    _compare(hm, full, want)
    assert hm.roi['filter'] == 0.5 and hm.roi['vertices'] == 3
    out_want = R.keep_share(pl, share=0.9, method='outside', **GEOM)
    assert 0 < (out_want & ~centre).sum() < (~centre).sum() and not np.array_equal(out_want, ~want)
    out = Heatmap.from_slide(eng, path, rois=TRIANGLE, roi_method='outside', roi_filter_method=0.9, roi_width=600, cell_mask=~centre, **KW)
    _compare(out, full, out_want & ~centre)
    assert out.roi['cells_dropped'] == int((~out_want).sum())


def test_roi_ands_with_the_other_masks(eng, slide):
    from biscuit_amd.heatmap import Heatmap
    path, full, centre = slide
    otsu = Heatmap.from_slide(eng, path, qc='otsu', qc_width=600, **KW)
    assert otsu.cell_mask.tolist() == [[True, True, False, False], [True, True, False, False], [False] * 4]
    hand = np.ones((3, 4), bool)
    hand[0, 0] = False
    hm = Heatmap.from_slide(eng, path, rois=ELL, qc='otsu', qc_width=600, cell_mask=hand, **KW)
    _compare(hm, full, centre & otsu.cell_mask & hand)
    assert hm.cell_mask.sum() == 2 and hm.qc['method'] == 'otsu' and hm.qc['threshold'] == otsu.qc['threshold'] and hm.roi['cells_dropped'] == 9
    # an ROI that keeps nothing: not an error
    from biscuit_amd.heatmap import MASKED
    none = Heatmap.from_slide(eng, path, rois=[np.array([[5000, 5000], [6000, 5000], [5000, 6000]])], **KW)
    assert (none.logits == MASKED).all() and (none.uncertainty == MASKED).all() and none.grid.shape == (0, 2) and none.dropped == 12
    assert none.qc['bands_read'] == 0 and none.roi['cells_dropped'] == 12 and not none.cell_mask.any()


def test_device_decode_gives_the_same_arrays(eng, slide, tmp_path):
    from biscuit_amd.heatmap import Heatmap
    path, full, centre = slide
    jpeg = _jpeg_slide(tmp_path)
    host = Heatmap.from_slide(eng, jpeg, rois=ELL, **KW)
    dev = Heatmap.from_slide(eng, jpeg, rois=ELL, decode='gpu', **KW)
    assert np.array_equal(dev.cell_mask, centre) and np.array_equal(host.cell_mask, centre)
    assert dev.logits.tobytes() == host.logits.tobytes() and dev.uncertainty.tobytes() == host.uncertainty.tobytes()
    assert np.array_equal(dev.grid, host.grid) and dev.roi == host.roi
    assert dev.decode_stats['gpu_bands'] == 2 and dev.decode_stats['host_bands'] == 0 and host.decode_stats['host_bands'] == 2


def test_command_line(eng, slide, tmp_path, capsys):
    from biscuit_amd import heatmap
    path, full, centre = slide
    csv = tmp_path / 'ell.csv'
    csv.write_text('ROI_Name,X_base,Y_base\n' + ''.join(f'ell,{x},{y}\n' for x, y in ELL[0].tolist()))
    out = str(tmp_path / 'roi')
    heatmap.main([path, '--out', out, '--mc', '8', '--seed', '3', '--batch', '16', '--rois', str(csv), '--roi-method', 'inside',
                  '--roi-filter', 'center', '--roi-width', '600'])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    z = np.load(os.path.join(out, 'heatmap.npz'))
    assert sorted(z.files) == ['cell_mask', 'grid', 'logits', 'uncertainty'] and np.array_equal(z['cell_mask'], centre)
    assert np.array_equal(z['logits'][centre], full.logits[centre]) and (z['logits'][~centre] == -1).all()
    s = json.load(open(os.path.join(out, 'summary.json')))
    assert s == printed and s['roi'] == {'method': 'inside', 'filter': 'center', 'polygons': 1, 'vertices': 6, 'cells_dropped': 9}
    assert 'qc' not in s and s['tiles_run'] == 3 and s['tiles_dropped'] == 9
    plain_keys = {'slide', 'grid_shape', 'tiles_run', 'tiles_dropped', 'seconds', 'tiles_per_s', 'decode_stats'}
    assert set(s) == plain_keys | {'roi'}
    # without the option: exactly today's keys, and the unmasked run's arrays
    plain = str(tmp_path / 'plain')
    heatmap.main([path, '--out', plain, '--mc', '8', '--seed', '3', '--batch', '16'])
    capsys.readouterr()
    z = np.load(os.path.join(plain, 'heatmap.npz'))
    assert sorted(z.files) == ['grid', 'logits', 'uncertainty']
    assert np.array_equal(z['logits'], full.logits) and np.array_equal(z['uncertainty'], full.uncertainty) and np.array_equal(z['grid'], full.grid)
    assert set(json.load(open(os.path.join(plain, 'summary.json')))) == plain_keys
