"""The Macenko domain cases (tests/_macenko_cases.py) are what they claim to be, and the float64 restatement (tests/_macenko_ref.py)
is well defined on each of them: its own float32 per-pixel variant -- the kernel's stated precision contract -- gives the bound the
kernel is held to in test_gpu_macenko_domain.py.  CPU only."""
import numpy as np
import pytest

import _macenko_cases as mc
import _macenko_ref as R
from biscuit_amd import stain as S

F = np.float32
TIE = 1e-9                      # two float64 reference values closer than this belong to one group (the groups are >= 1e-3 apart)


def _group(values, rank):
    """(position of the element of rank `rank` inside its group of equal values, the group's size, the sorted values)."""
    s = np.sort(values)
    lo, hi = np.searchsorted(s, s[rank] - TIE, 'left'), np.searchsorted(s, s[rank] + TIE, 'right')
    return rank - lo, hi - lo, s


def _angle_ranks(n):
    return mc.rank_and_weight(n, S.MACENKO_ALPHA), mc.rank_and_weight(n, 100 - S.MACENKO_ALPHA)


def _where(variant, pos, size):
    return {'inside': 0 < pos < size - 1, 'last': pos == size - 1, 'first': pos == 0}[variant]


def _colour_mask(name, c):
    return (np.asarray(mc.cases()[name]).reshape(-1, 3) == np.asarray(c, np.uint8)).all(1)


def _tissue_mask(name):
    return ~np.any(R.optical_density(np.asarray(mc.cases()[name])) < S.MACENKO_BETA, axis=1)


# ---------------------------------------------------------------- the set
def test_the_set_is_small_named_and_deterministic():
    cs = mc.cases()
    assert 25 <= len(cs) <= 40                                                       # about 40 tiles at the most
    for name, t in cs.items():
        assert t.shape == (mc.PX, mc.PX, 3) and t.dtype == np.uint8 and not t.flags.writeable, name
    assert len({t.tobytes() for t in cs.values()}) == len(cs)                        # no tile twice
    assert np.array_equal(mc._palette_angle('last'), cs['palette_angle_last'])      # built again: the same bytes
    assert np.array_equal(mc.sparse_tile('tint', 101), cs['sparse_tinted_101'])
    assert np.array_equal(mc._mixed_sign(3, -0.35, 0.5), cs['mixed_sign_a'])
    assert [n for n in cs if n not in mc.compared()] == ['two_pixels_glass', 'two_pixels_tint']
    he2, mc2 = mc.second_fit()
    assert np.isfinite(he2).all() and (mc2 > 0).all()
    assert np.abs(he2 - F(S.MACENKO_HE_REF)).max() > 0.01 and np.abs(mc2 - F(S.MACENKO_MAXC_REF)).max() > 0.1


def test_restated_reference_is_the_same_function():
    """stats() gained a variant and transform() left normalise(): the float64 path computes what it computed."""
    x = np.asarray(mc.cases()['full_tissue'])
    st = R.stats(x)
    C2 = st['C'] / (st['maxC'] / R.MAXC_REF)[:, None]
    Inorm = S.MACENKO_IO * np.exp(-R.HE_REF.dot(C2))
    Inorm[Inorm > 255] = S.MACENKO_OVER_TO
    want = np.reshape(Inorm.T, x.shape).astype(np.uint8)
    assert np.array_equal(R.normalise(x)[0], want)
    assert np.array_equal(R.transform(x, st['HE'], st['maxC']), want)
    det, P = R.pinv2(st['HE'])
    assert abs(det - st['det']) <= 1e-15
    np.testing.assert_allclose(P, np.linalg.pinv(st['HE']), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(R.concentrations(R.optical_density(x), st['HE'], F), st['C'], atol=1e-5)


# ---------------------------------------------------------------- conditions: the reference is well defined on every compared case
@pytest.mark.parametrize('name', mc.compared())
def test_conditions(name):
    st = mc.reference(name)
    assert st['HE'] is not None and st['maxC'] is not None
    l_min, l_mid, l_max = st['evals']
    assert l_mid >= 10 * l_min or l_min == 0, st['evals']
    assert l_min >= -1e-12 * l_max                                                 # (a rounding-size negative l_min is a zero)
    assert l_max >= 2 * l_mid, st['evals']
    assert np.linalg.cond(st['HE']) <= 50
    assert abs(st['det']) >= 1e3 * S.MACENKO_DET_MIN                               # none of the compared cases is SINGULAR
    assert (np.abs(st['maxC']) >= 1e-4).all(), st['maxC']
    assert np.abs(st['phi']).max() <= np.pi - 1e-3
    b_he, b_c = mc.bounds(name)
    assert b_he <= mc.BOUND_MAX and b_c <= mc.BOUND_MAX, (b_he, b_c)


def test_two_pixels_is_the_one_exemption():
    for name in ('two_pixels_glass', 'two_pixels_tint'):
        st = mc.reference(name)
        l_min, l_mid, l_max = st['evals']
        assert st['n_tissue'] == 2 and abs(l_mid) < 1e-12 * l_max                 # rank 1: the middle eigenvector is arbitrary
        assert st['status'] in (R.OK, R.SINGULAR, R.NONFINITE)


# ---------------------------------------------------------------- claims, family by family
@pytest.mark.parametrize('name', ['mixed_sign_a', 'mixed_sign_b'])
def test_mixed_sign_percentile_angles_have_both_signs(name):
    for pp in (np.float64, F):
        st = mc.reference(name, pp)
        assert st['status'] == R.OK
        assert st['minPhi'] < -0.1 and st['maxPhi'] > 0.1, (st['minPhi'], st['maxPhi'])
        assert (st['phi'] < 0).mean() > 0.05 and (st['phi'] > 0).mean() > 0.05
    E = mc.reference(name)['E']
    assert E[:, 1].min() < -0.3 and E[:, 1].max() > 0.3                           # the principal axis has mixed signs


def test_palette_groups_are_separated():
    """The 10 colours' angles and concentrations lie >= 1e-3 apart, so float32 and float64 order the groups alike; colour 0 / 8 are
    the angle order's two ends and hold the largest C[0] / C[1]."""
    for v in mc.VARIANTS:
        for name in (f'palette_angle_{v}', f'palette_conc_{v}'):
            st, st32 = mc.reference(name), mc.reference(name, F)
            tis = _tissue_mask(name)
            phi, c0, c1 = [], [], []
            for c in mc.PALETTE:
                m = _colour_mask(name, c)
                assert m.sum() > 0 and tis[m].all()
                for vals, out in ((st['phi'][m[tis]], phi), (st['C'][0, m], c0), (st['C'][1, m], c1)):
                    assert np.ptp(vals) < TIE
                    out.append(vals[0])
                assert len(np.unique(st32['phi'][m[tis]])) == 1 and len(np.unique(st32['C'][0, m])) == 1
            for vals in (phi, c0, c1):
                assert np.diff(np.sort(vals)).min() >= 1e-3, (name, np.sort(vals))
            assert np.argmin(phi) == 0 and np.argmax(phi) == 8 and np.argmax(c0) == 0 and np.argmax(c1) == 8
            assert st['n_tissue'] == mc.PALETTE_TISSUE and (st['n_tissue'] - 1) % 100 != 0


@pytest.mark.parametrize('variant', mc.VARIANTS)
def test_palette_angle_ranks_sit_where_claimed(variant):
    name = f'palette_angle_{variant}'
    for pp in (np.float64, F):
        st = mc.reference(name, pp)
        (r0, g0), (r1, g1) = _angle_ranks(st['n_tissue'])
        assert 0.1 < g0 < 0.9 and 0.1 < g1 < 0.9                                   # a fractional weight on both
        for r in (r0, r1):
            pos, size, s = _group(st['phi'], r)
            assert _where(variant, pos, size), (variant, r, pos, size)
            assert size >= 500                                                    # a large group, or next to one
            if variant == 'last':
                assert s[r + 1] - s[r] >= 1e-3                                     # the successor is the next colour
            if variant == 'first':
                assert s[r] - s[r - 1] >= 1e-3 and s[r + 1] - s[r] < TIE
    # the three variants give three different fits
    others = [mc.reference(f'palette_angle_{v}')['HE'] for v in mc.VARIANTS if v != variant]
    assert all(np.abs(mc.reference(name)['HE'] - o).max() > 1e-3 for o in others)


@pytest.mark.parametrize('variant', mc.VARIANTS)
def test_palette_concentration_ranks_sit_where_claimed(variant):
    name = f'palette_conc_{variant}'
    assert mc.CONC_RANK == 88506
    for pp in (np.float64, F):
        st = mc.reference(name, pp)
        for t in range(2):
            pos, size, s = _group(st['C'][t], mc.CONC_RANK)
            assert _where(variant, pos, size), (variant, t, pos, size)
            assert size >= 800
            if variant == 'last':
                assert s[mc.CONC_RANK + 1] - s[mc.CONC_RANK] >= 1e-3
            if variant == 'first':
                assert s[mc.CONC_RANK] - s[mc.CONC_RANK - 1] >= 1e-3


def test_sparse_rank_arithmetic():
    """The small counts run floor(0.01 (n-1)) and floor(0.99 (n-1)) where they are 0 and 1, where the successor is the last element
    and where the weight is exactly 0."""
    want = {3: ((0, 0.02), (1, 0.98)), 4: ((0, 0.03), (2, 0.97)), 5: ((0, 0.04), (3, 0.96)), 101: ((1, 0.0), (99, 0.0)),
            102: ((1, 0.01), (99, 0.99)), 500: ((4, 0.99), (494, 0.01))}
    for n, ((r0, g0), (r1, g1)) in want.items():
        (a0, b0), (a1, b1) = _angle_ranks(n)
        assert (a0, a1) == (r0, r1) and abs(b0 - g0) < 1e-9 and abs(b1 - g1) < 1e-9, n
        assert r1 + 1 <= n - 1
    assert _angle_ranks(3)[1][0] + 1 == 2 and _angle_ranks(101)[0][1] == 0.0 and _angle_ranks(101)[1][1] == 0.0


def test_sparse_glass_status_changes_at_the_threshold():
    k0 = mc.glass_threshold()
    assert 895 <= k0 <= 895 + 2 * mc.SPARSE_OUTER
    names = [n for n in mc.cases() if n.startswith('sparse_glass_')]
    assert [int(n.rsplit('_', 1)[1]) for n in names] == list(mc.SPARSE_K) + [k0 - 2, k0 - 1, k0, k0 + 1]
    for name in names:
        k = int(name.rsplit('_', 1)[1])
        for pp in (np.float64, F):
            st = mc.reference(name, pp)
            assert st['n_tissue'] == k
            assert np.isfinite(st['HE']).all() and np.isfinite(st['maxC']).all()
            if k < k0:
                # the 99th percentile of both rows falls inside the background's group of NPIX - k equal negative values
                assert st['status'] == R.NONFINITE and (st['maxC'] <= -1e-3).all(), (name, st['maxC'])
                for t in range(2):
                    pos, size, _ = _group(st['C'][t], mc.CONC_RANK)
                    assert size == mc.NPIX - k and 0 < pos <= size - 1
                    assert (pos == size - 1) == (k == k0 - 1)                     # one count below the change: the group's last element
            else:
                assert st['status'] == R.OK and (st['maxC'] >= 0.05).all(), (name, st['maxC'])


def test_sparse_tinted_is_ok_with_a_saturating_scale():
    for name in [n for n in mc.cases() if n.startswith('sparse_tinted_')]:
        k = int(name.rsplit('_', 1)[1])
        st = mc.reference(name)
        assert st['status'] == R.OK and st['n_tissue'] == k
        assert (R.MAXC_REF / st['maxC']).max() > 10                                # the scale maxCRef / maxC
        if k <= 500:                                                               # maxC is a background pixel's concentration
            tis = _tissue_mask(name)
            for t in range(2):
                order = np.argsort(st['C'][t], kind='stable')
                assert not tis[order[mc.CONC_RANK]] and not tis[order[mc.CONC_RANK + 1]]
        out = R.transform(np.asarray(mc.cases()[name]), st['HE'], st['maxC']).reshape(-1, 3)
        assert (out[_tissue_mask(name)] == 0).mean() > 0.5                        # the transform saturates: most tissue bytes are 0


def test_ink_reaches_the_clamped_bins():
    st = mc.reference('ink_black')
    assert st['status'] == R.OK and st['maxC'][0] > 8
    x = np.asarray(mc.cases()['ink_black']).reshape(-1, 3)
    assert 0.04 < (x.max(1) <= 3).mean() < 0.06
    pos, size, _ = _group(mc.reference('ink_black', F)['C'][0], mc.CONC_RANK)       # ... inside a group of equal keys there
    assert size > 500 and 0 < pos < size - 1
    st = mc.reference('ink_off_wedge')
    assert st['status'] == R.OK and (st['maxC'] < 8).all()
    below = (st['C'] < -8).any(0)
    assert below.sum() == mc.INK_OFF_WEDGE_COUNT and 0.009 < below.mean() < 0.01
    assert (below == _colour_mask('ink_off_wedge', mc.INK_OFF_WEDGE)).all() and not _tissue_mask('ink_off_wedge')[below].any()


def test_full_tissue():
    st = mc.reference('full_tissue')
    assert st['status'] == R.OK and st['n_tissue'] == mc.NPIX


# ---------------------------------------------------------------- the float32 variant: sensitivity and bytes
def test_sensitivity_table():
    """s(case): the float64 reference against its float32 per-pixel variant.  Printed; profiles/macenko_domain.txt holds a copy."""
    print()
    for name in mc.compared():
        a, b = mc.reference(name), mc.reference(name, F)
        assert a['status'] == b['status'] and a['n_tissue'] == b['n_tissue']
        (s_he, s_c), (b_he, b_c) = mc.sensitivity(name), mc.bounds(name)
        print(f'{name:24s} status {a["status"]} n_tissue {a["n_tissue"]:6d}  s_HE {s_he:.2e} s_maxC {s_c:.2e}  '
              f'bound_HE {b_he:.2e} bound_maxC {b_c:.2e}')
        assert s_he < mc.BOUND_MAX / mc.BOUND_FACTOR and s_c < mc.BOUND_MAX / mc.BOUND_FACTOR


@pytest.mark.parametrize('fit', ['preset', 'second'])
def test_float32_variant_bytes_stay_inside_the_byte_bounds(fit):
    """What the GPU test asks of the kernel, asked of the reference's own float32 variant: float64 transform of the float32-reported
    statistics against the float32 transform.  No byte off by more than 1, at most 1e-3 of a tile's bytes differing."""
    he_ref, maxc_ref = mc.fits()[fit]
    print()
    for name in mc.compared():
        st = mc.reference(name, F)
        if st['status'] != R.OK:
            continue
        x = np.asarray(mc.cases()[name])
        want = R.transform(x, st['HE'].astype(F), st['maxC'].astype(F), he_ref, maxc_ref)
        got = R.transform(x, st['HE'], st['maxC'], he_ref, maxc_ref, per_pixel=F)
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        print(f'{name:24s} {fit}: max diff {int(d.max())}, differing {int((d > 0).sum())} of {d.size}')
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3, name
