"""The host side of the heatmap's region-of-interest mask (DESIGN.md "Heatmap input", Region-of-interest mask): ``bqio_roi_plane`` --
the CPU build of the routines the GPU kernel is compiled from -- against the numpy restatement (tests/_roi_ref.py) integer for
integer, the sample tables, the CSV reader and every refusal.  No GPU."""
import numpy as np
import pytest

from biscuit_amd import roi, tfrecord_native
from tests import _roi_cases as C
from tests import _roi_ref as R


@pytest.mark.parametrize('size', C.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plane_equals_reference(size):
    w0, h0, xs, ys = C.geometry(size)
    want = C.expected(size)
    for name, polys in C.polygon_cases(size).items():
        got = roi.plane_host(xs, ys, polys)
        assert got.dtype == np.uint8 and got.shape == size
        assert np.array_equal(got, want[name]), (name, size, int((got != want[name]).sum()))
        C.check_known(size, name, got)


def test_edge_table_equals_reference():
    polys = C.polygon_cases((67, 131))['ring']
    edges, starts = roi.edge_table(polys)
    want_edges, want_starts = R.edge_table(polys)
    assert edges.dtype == np.int32 and starts.dtype == np.int32 and edges.flags.c_contiguous
    assert np.array_equal(edges, want_edges) and np.array_equal(starts, want_starts) and starts.tolist() == [0, 3, 1503, 1507]
    assert edges[2].tolist() == [0, 2 * ((5 * 67 + 2) // 4), 0, 0]            # the first triangle's closing edge: (0, h0 // 4) -> (0, 0)


def test_half_open_by_hand():
    """Samples at the integer level-0 points x = 0 .. 4, y = 0 .. 2 (doubled: even), the rectangle (1, 0) .. (3, 2): its corners and
    its two horizontal edges lie exactly on sample rows and columns.  The left and the y = 0 side are inside, the right and the
    y = 2 side are not; a point on a vertical edge (d == 0) does not count for that edge."""
    xs, ys = np.array([0, 2, 4, 6, 8], np.int32), np.array([0, 2, 4], np.int32)
    rect = [np.array([[1, 0], [3, 0], [3, 2], [1, 2]], np.int32)]
    want = [[0, 1, 1, 0, 0],
            [0, 1, 1, 0, 0],
            [0, 0, 0, 0, 0]]
    assert roi.plane_host(xs, ys, rect).tolist() == want and R.plane(xs, ys, rect).tolist() == want
    assert roi.plane_host(xs, ys, [rect[0][::-1]]).tolist() == want           # the other orientation: the same pixels
    # a triangle with every vertex on a sample: (0, 0), (4, 0), (2, 2) -- the row y = 0 holds x = 0 .. 3 (its left vertex in, its right
    # one out), the row y = 1 holds x = 1 (on the left side: in) and x = 2, not x = 3 (on the right side), the apex row nothing
    tri = [np.array([[0, 0], [4, 0], [2, 2]], np.int32)]
    want = [[1, 1, 1, 1, 0],
            [0, 1, 1, 0, 0],
            [0, 0, 0, 0, 0]]
    assert roi.plane_host(xs, ys, tri).tolist() == want and R.plane(xs, ys, tri).tolist() == want


@pytest.mark.parametrize('geom', [(4, 3, 598, 598), (7, 5, 299, 598), (9, 6, 150, 301), (1, 1, 1, 1), (120, 90, 299, 599)],
                         ids=lambda g: 'x'.join(map(str, g)))
def test_center_tables(geom):
    """(gw, gh, stride, extract_px): stride_div = 1, stride_div = 2 (cells overlap), an odd extract_px (the centre is half a pixel)."""
    xs, ys = roi.center_tables(*geom)
    want_xs, want_ys = R.center_tables(*geom)
    assert xs.dtype == np.int32 and ys.dtype == np.int32 and np.array_equal(xs, want_xs) and np.array_equal(ys, want_ys)
    assert xs[0] == geom[3] and (len(xs), len(ys)) == geom[:2]


@pytest.mark.parametrize('geom', [(2400, 1800, 600), (2400, 1800, 2048), (1000, 700, 2048), (99991, 70001, 2048), (5, 100000, 3),
                                  (7, 3, 1)], ids=lambda g: 'x'.join(map(str, g)))
def test_raster_tables(geom):
    """(slide_w0, slide_h0, roi_width): an exact ratio, a ragged one, a slide narrower than the raster, primes, a sliver."""
    xs, ys = roi.raster_tables(*geom)
    want_xs, want_ys = R.raster_tables(*geom)
    assert xs.dtype == np.int32 and np.array_equal(xs, want_xs) and np.array_equal(ys, want_ys)
    assert (len(xs), len(ys)) == roi.raster_size(*geom) == R.raster_size(*geom) and len(xs) == min(geom[2], geom[0])
    assert (np.diff(xs) >= 0).all() and xs[0] >= 0 and xs[-1] < 2 * geom[0] and ys[-1] < 2 * geom[1]


def test_keep_decisions_equal_reference():
    from biscuit_amd import tissue
    g = dict(gw=7, gh=5, slide_w0=2400, slide_h0=1800, stride=299, extract_px=598)
    polys = [np.array([[200, 100], [2300, 400], [900, 1700]], np.int32)]
    xs, ys = roi.center_tables(g['gw'], g['gh'], g['stride'], g['extract_px'])
    pl = roi.plane_host(xs, ys, polys)
    for method in ('inside', 'outside'):
        assert np.array_equal(roi.keep_from_plane(pl, method), R.keep_center(R.plane(xs, ys, polys), method))
    assert 0 < roi.keep_from_plane(pl, 'inside').sum() < pl.size
    xs, ys = roi.raster_tables(2400, 1800, 600)
    pl = roi.plane_host(xs, ys, polys)
    col, row = tissue.cell_ranges(g['gw'], g['gh'], 600, 450, 2400, 1800, 299, 598)
    outside = np.array([[int((pl[ya:yb, xa:xb] == 0).sum()) for xa, xb in col.tolist()] for ya, yb in row.tolist()], np.int32)
    seen = set()
    for share in (0.05, 0.5, 1.0):
        for method in ('inside', 'outside'):
            got = roi.keep_from_share(outside, col, row, share, method)
            assert got.dtype == np.bool_ and np.array_equal(got, R.keep_share(R.plane(xs, ys, polys), share=share, method=method, **g))
            seen.add(got.tobytes())
    assert len(seen) == 6                                                    # every (share, method) decides differently here


def test_read_csv(tmp_path):
    p = tmp_path / 'slide.csv'
    p.write_text('Y_base,ROI_Name,note,X_base\n'                             # columns in another order, one of them foreign
                 '10.0,a,x,5.9\n'
                 '20,b,x,100\n'                                              # two names interleaved
                 '10.5,a,x,50\n'
                 '20,b,x,200.75\n'
                 '-3e1,a,x,-7.5\n'
                 '90,b,x,150\n'
                 '\n')
    polys = roi.read_csv(str(p))
    assert [a.tolist() for a in polys] == [[[5, 10], [50, 10], [-7, -30]], [[100, 20], [200, 20], [150, 90]]]
    assert all(a.dtype == np.int32 for a in polys)
    q = tmp_path / 'short.csv'
    q.write_text('ROI_Name,X_base,Y_base\nfirst,0,0\nfirst,5,0\nfirst,5,5\nsecond,1,1\nsecond,2,2\n')
    with pytest.raises(ValueError, match='second'):
        roi.read_csv(str(q))
    q.write_text('ROI_Name,X_base\nfirst,0\n')
    with pytest.raises(ValueError, match='Y_base'):
        roi.read_csv(str(q))
    q.write_text('ROI_Name,X_base,Y_base\nfirst,0,zero\n')
    with pytest.raises(ValueError, match='line 2'):
        roi.read_csv(str(q))


# ---- refusals: one test each -----------------------------------------------------------------------------------------------------------
def _call(edges, starts, xs, ys, plane=None, E=None, P=None, W=None, H=None):
    edges, starts = np.ascontiguousarray(edges, np.int32), np.ascontiguousarray(starts, np.int32)
    xs, ys = np.ascontiguousarray(xs, np.int32), np.ascontiguousarray(ys, np.int32)
    if plane is None:
        plane = np.full((len(ys), len(xs)), 7, np.uint8)
    e = tfrecord_native.lib().bqio_roi_plane(edges.ctypes.data, len(edges) if E is None else E, starts.ctypes.data,
                                             len(starts) - 1 if P is None else P, xs.ctypes.data, len(xs) if W is None else W,
                                             ys.ctypes.data, len(ys) if H is None else H, plane.ctypes.data)
    return e, plane


TRI = np.array([[0, 0, 8, 0], [8, 0, 0, 8], [0, 8, 0, 0]], np.int32)
XS, YS = np.array([1, 3, 5], np.int32), np.array([1, 3], np.int32)


def test_the_good_call_is_accepted():
    e, plane = _call(TRI, [0, 3], XS, YS)
    assert e == 0 and plane.tolist() == [[1, 1, 1], [1, 1, 0]]


def test_coordinate_out_of_bounds_refused():
    for i, v in ((0, (1 << 28) + 1), (5, -(1 << 28) - 1)):
        bad = TRI.copy()
        bad.reshape(-1)[i] = v
        e, plane = _call(bad, [0, 3], XS, YS)
        assert e == -1 and (plane == 7).all()
    edge = TRI.copy()
    edge.reshape(-1)[0] = -(1 << 28)                                         # the bound itself is legal
    assert _call(edge, [0, 3], XS, YS)[0] == 0
    for xs, ys in ((np.array([1, -1, 5]), YS), (XS, np.array([1, (1 << 29) + 1])), (np.array([1, 3, (1 << 29) + 1]), YS)):
        e, plane = _call(TRI, [0, 3], xs, ys)
        assert e == -1 and (plane == 7).all()
    assert _call(TRI, [0, 3], np.array([0, 1 << 29, 5]), YS)[0] == 0
    with pytest.raises(ValueError, match='2\\^27'):
        roi.check_polygons([np.array([[0, 0], [(1 << 27) + 1, 0], [0, 5]])])
    with pytest.raises(ValueError, match='2\\^27'):
        roi.check_polygons([np.array([[0, 0], [5, -(1 << 27) - 1], [0, 5]])])
    assert roi.check_polygons([np.array([[0, 0], [1 << 27, -(1 << 27)], [0, 5]])])[0].dtype == np.int32
    with pytest.raises(ValueError):
        roi.center_tables(4, 3, 1 << 28, 598)                                # a cell centre beyond 2^29 doubled


def test_starts_not_increasing_refused():
    six = np.concatenate([TRI, TRI])
    assert _call(six, [0, 3, 6], XS, YS)[0] == 0
    for starts in ([0, 6, 6], [0, 4, 6], [0, 2, 6], [1, 3, 6], [0, 3, 5], [0, 3, 7], [3, 0, 6], [0, -3, 6]):
        e, plane = _call(six, starts, XS, YS)
        assert e == -1 and (plane == 7).all(), starts
    assert _call(TRI[:2], [0, 2], XS, YS)[0] == -1                           # a polygon of two edges
    assert _call(TRI, [0, 3], XS, YS, P=0)[0] == -1
    for bad in ([np.array([[0, 0], [1, 1]])], [np.zeros((3, 3), np.int32)], [np.zeros((3, 2), np.float32)], [], 'abc', None,
                np.array([[0, 0], [4, 0], [0, 4]])):                             # a bare array is not a list of polygons
        with pytest.raises(ValueError):
            roi.check_polygons(bad)


def test_edge_cap_refused():
    cap = 1 << 20
    big = np.tile(TRI, (cap // 3 + 1, 1))                                    # 2^20 + 2 edges
    starts = np.arange(0, len(big) + 1, 3, dtype=np.int32)
    e, plane = _call(big, starts, XS, YS)
    assert len(big) > cap and e == -1 and (plane == 7).all()
    ok = big[:cap - 1]                                                       # 1 048 575 edges = 349 525 triangles: accepted
    e, plane = _call(ok, starts[:len(ok) // 3 + 1], XS, YS)
    assert e == 0 and plane.tolist() == [[1, 1, 1], [1, 1, 0]]               # (an odd number of copies of the triangle, united)
    with pytest.raises(ValueError, match='at most'):
        roi.check_polygons([np.zeros((cap + 1, 2), np.int32)])


def test_plane_of_two_to_the_31_refused():
    xs, ys = np.ones(1 << 16, np.int32), np.ones(1 << 15, np.int32)
    plane = np.full(4, 7, np.uint8)                                          # never written: the call is refused first
    assert _call(TRI, [0, 3], xs, ys, plane=plane)[0] == -1 and (plane == 7).all()
    assert _call(TRI, [0, 3], XS, YS, W=0)[0] == -1 and _call(TRI, [0, 3], XS, YS, H=-1)[0] == -1
    with pytest.raises(ValueError):
        roi.plane_host(xs, ys, [np.array([[0, 0], [4, 0], [0, 4]])])


def test_share_of_zero_or_above_one_refused():
    for bad in (0, 0.0, -0.5, 1.0000001, 2, float('nan'), float('inf'), 'centre', None, True):
        with pytest.raises(ValueError):
            roi.check_filter(bad)
    assert roi.check_filter('center') == 'center' and roi.check_filter(1) == 1.0 and roi.check_filter(0.25) == 0.25
    col, row = np.array([[0, 2]]), np.array([[0, 2]])
    for bad in (0.0, 1.5, 'center'):
        with pytest.raises(ValueError):
            roi.keep_from_share(np.array([[1]]), col, row, bad, 'inside')
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError):
            roi.check_width(bad)


def test_unknown_method_refused():
    for bad in ('within', 'INSIDE', None, 1):
        with pytest.raises(ValueError):
            roi.check_method(bad, True)
    with pytest.raises(ValueError):
        roi.keep_from_plane(np.zeros((2, 2), np.uint8), 'auto')
    assert [roi.check_method(m, True) for m in roi.ROI_METHODS] == ['inside', 'inside', 'outside', 'ignore']


def test_inside_without_polygons_refused():
    for m in ('inside', 'outside'):
        with pytest.raises(ValueError, match='needs rois'):
            roi.check_method(m, False)
    assert roi.check_method('auto', False) == 'ignore' and roi.check_method('ignore', False) == 'ignore'
