"""The heatmap's focus mask on the host (DESIGN.md "Heatmap input", Focus mask; ``biscuit_amd/tissue.py``): the Gaussian's integer
taps, the threshold in integer units, the nearest-neighbour plane map, the numpy restatement (tests/_focus_ref.py) against
``scipy.ndimage`` in float64 within a derived band, and what ``Heatmap.from_slide`` refuses.  The device side is
tests/test_gpu_focus.py."""
import numpy as np
import pytest

from biscuit_amd import tissue
from tests import _focus_ref as F
from tests.test_wsi import _slide_file


def test_taps():
    w = tissue.focus_taps()
    assert w.dtype == np.int32 and w.shape == (25,) and int(w.sum()) == 65536 and (w >= 0).all() and np.array_equal(w, w[::-1])
    assert w.tolist() == F.taps() and int(w.argmax()) == 12
    for sigma in (0.25, 1.0, 2.2, 3.0, 4.1):                                 # r = 1, 4, 9, 12, 16
        w = tissue.focus_taps(sigma)
        r = int(4 * sigma + 0.5)
        assert len(w) == 2 * r + 1 and int(w.sum()) == 65536 and (w >= 0).all() and np.array_equal(w, w[::-1]) and w.tolist() == F.taps(sigma)
    assert len(tissue.focus_taps(4.1)) == 33
    for bad in (4.2, 100.0, 0.1, 0.0, -3.0, float('nan'), float('inf')):     # r = 17, 400, 0; no Gaussian
        with pytest.raises(ValueError):
            tissue.focus_taps(bad)


def test_units_width_and_checks():
    assert tissue.FOCUS_SCALE == F.S == 255 * (2125 + 7154 + 721) and tissue.QC_METHODS == ('otsu',)
    assert tissue.focus_units() == tissue.focus_units(0.02) == F.units(0.02) == 51000
    assert tissue.focus_units(0) == 0 and tissue.focus_units(1.0) == F.S and tissue.focus_units(0.0199999) == 50999
    for bad in (-1, -1e-9, float('nan'), float('inf'), 1e6):
        with pytest.raises(ValueError):
            tissue.focus_units(bad)
    assert tissue.focus_width(100000, 0.25) == 6250 and tissue.focus_width(2400, 0.5045) == 303 and tissue.focus_width(2400, 0.5045, 1.0) == 1211
    assert tissue.focus_width(2400, 8.0) == 2400 and tissue.focus_width(3, 0.25) == 1              # never enlarged, never empty
    thr, mpp, taps = tissue.check_focus(0.02, 4, 3)
    assert (thr, mpp) == (51000, 4.0) and np.array_equal(taps, tissue.focus_taps())
    for bad in (dict(threshold=-1), dict(threshold=float('nan')), dict(mpp=0), dict(mpp=-4.0), dict(mpp=float('nan')), dict(sigma=9.0)):
        with pytest.raises(ValueError):
            tissue.check_focus(**dict(dict(threshold=0.02, mpp=4.0, sigma=3.0), **bad))


@pytest.mark.parametrize('n', [1, 2, 7, 131])
def test_plane_map(n):
    ident = tissue.plane_map(n, n)
    assert ident.dtype == np.int32 and ident.tolist() == list(range(n))                              # equal shapes: the identity
    assert tissue.plane_map(n, 1).tolist() == [0] * n
    triple = tissue.plane_map(n, 3 * n)
    assert triple[0] == 1 and triple[-1] == 3 * n - 2 and triple.tolist() == [3 * i + 1 for i in range(n)]   # the middle of each three
    for n_from in (1, 2, 5, n, 3 * n, 40, 1000):
        m = tissue.plane_map(n, n_from)
        assert np.array_equal(m, F.nearest_map(n, n_from)) and m.min() >= 0 and m.max() < n_from and (np.diff(m) >= 0).all()
        if n_from <= n:
            assert sorted(set(m.tolist())) == list(range(n_from))                                    # shrinking a plane loses no pixel of it
    for bad in ((0, 5), (5, 0), (2.5, 5), (5, 1 << 31)):
        with pytest.raises(ValueError):
            tissue.plane_map(*bad)


def ramped_noise(h, w, seed=0, top=14.0):
    """Noise around mid-grey whose amplitude grows smoothly from 0 on the left to +-``top`` grey levels on the right: the blurred
    |Laplacian| crosses the 0.02 threshold (about +-3 levels of independent noise a channel) inside the image."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    amp = np.linspace(0.0, top, w)[None, :, None] * (0.75 + 0.25 * np.cos(np.linspace(0.0, 3.0, h)))[:, None, None]
    return np.clip(np.rint(128.0 + amp * rng.uniform(-1.0, 1.0, (h, w, 3))), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('shape', [(1, 1), (1, 40), (40, 1), (7, 5), (97, 131), (150, 200)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_reference_value_against_scipy(shape):
    """The integer definition against its float64 statement -- ``gaussian_filter(abs(convolve(gray, K, mode='reflect')), sigma=3,
    mode='nearest', truncate=4)`` on the [0, 1] gray image.  With E = sum |w_k / 65536 - g_k| the two passes differ from the exact
    taps by at most 2 E max(L), each pass rounds by at most half a unit and float64 adds far less than one: bound = (2 E max(L) +
    2) / S.  Measured here (E and the largest figures, printed below): over these shapes and contents the largest |V / S - F| is 62.7 units
    of S (2.5e-5), on the 7 x 5 checkerboard, against that case's bound of 1903 units; on the ramped noise that straddles the
    threshold it is 16.5 units against 352; and no pixel's decision differs from the float statement's."""
    from scipy import ndimage
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    taps = tissue.focus_taps()
    x = np.arange(-12, 13, dtype=np.float64)
    g = np.exp(-0.5 * x * x / 9.0)
    g /= g.sum()
    E = float(np.abs(taps / 65536.0 - g).sum())
    assert E < 4e-4                                                          # (25 roundings of 2^-17, and the centre's correction)
    contents = {'ramp': ramped_noise(h, w), 'ramp_strong': ramped_noise(h, w, 1, 40.0), 'noise': rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
                'checker': (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)[:, :, None].repeat(3, 2)}
    K = np.array([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], np.float64)
    for name, img in contents.items():
        V = F.value(img, taps)
        gray = F.gray(img).astype(np.float64) / F.S
        Fl = ndimage.gaussian_filter(np.abs(ndimage.convolve(gray, K, mode='reflect')), sigma=3, mode='nearest', truncate=4)
        bound = (2.0 * E * float(F.laplace_abs(F.gray(img)).max()) + 2.0) / F.S
        diff = np.abs(V / float(F.S) - Fl)
        disagree = (V <= tissue.focus_units(0.02)) != (Fl <= 0.02)
        print(name, shape, 'E', E, 'max diff (units of S)', float(diff.max()) * F.S, 'bound (units)', bound * F.S, 'disagree', int(disagree.sum()))
        assert (diff <= bound).all(), (name, float(diff.max()), bound)
        assert (np.abs(Fl[disagree] - 0.02) <= bound).all(), name
        assert disagree.mean() <= 0.001, (name, float(disagree.mean()))
        if name == 'ramp' and w >= 100:                                      # the input does straddle the threshold
            share = float((V <= 51000).mean())
            assert 0.1 < share < 0.9, share


def test_from_slide_refusals(tmp_path):
    """None of these reaches the engine; ``qc`` keeps refusing Slideflow's strings for the focus mask."""
    from biscuit_amd.heatmap import Heatmap
    path, _ = _slide_file(tmp_path)
    for kw in (dict(focus_threshold=-1), dict(focus_threshold=float('nan')), dict(focus_mpp=0), dict(focus_threshold=0.02, focus_mpp=0),
               dict(resample='host', focus_threshold=0.02), dict(focus_threshold=0.02, focus_sigma=9.0),
               dict(focus_threshold=0.02, qc_fraction=1.5), dict(qc='blur', focus_threshold=0.02), dict(qc='both', focus_threshold=0.02)):
        with pytest.raises(ValueError):
            Heatmap.from_slide(None, path, **kw)
