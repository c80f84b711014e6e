"""Float64 numpy restatement of the Macenko normaliser (DESIGN.md "Macenko"; Macenko 2009 in the numpy form of HEnorm_python),
the reference the kernel behind ``bq_stain_macenko`` is tested against, and a generator of test tiles.

It calls ``np.cov``, ``np.linalg.eigh``, ``np.percentile`` and ``np.linalg.lstsq`` literally; the constants come from
``biscuit_amd.stain`` (the one place they are named).
"""
import numpy as np

from biscuit_amd import stain as S

OK, FEW_TISSUE, SINGULAR, NONFINITE = S.STAIN_OK, S.STAIN_FEW_TISSUE, S.STAIN_SINGULAR, S.STAIN_NONFINITE
HE_REF = np.array(S.MACENKO_HE_REF, np.float64)
MAXC_REF = np.array(S.MACENKO_MAXC_REF, np.float64)


def optical_density(img):
    """[N,3] float64 OD of a [h,w,3] uint8 tile."""
    return -np.log((img.reshape(-1, 3).astype(np.float64) + 1) / S.MACENKO_IO)


def canonical(E):
    """Flip each column so that its entry of largest magnitude is positive."""
    E = E.copy()
    for j in range(E.shape[1]):
        if E[np.argmax(np.abs(E[:, j])), j] < 0:
            E[:, j] = -E[:, j]
    return E


def pinv2(HE):
    """(det(HE^T HE), pinv(HE) [2,3] = (HE^T HE)^-1 HE^T) in float64, the closed form the kernel states."""
    M = HE.T.dot(HE)
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    with np.errstate(all='ignore'):
        P = np.array([[M[1, 1], -M[0, 1]], [-M[1, 0], M[0, 0]]]).dot(HE.T) / det
    return det, P


def _project32(OD, A):
    """[N,k] float32: OD [N,3] and A [3,k] rounded to float32, each product and each sum rounded to float32, left to right."""
    x, a = OD.astype(np.float32), A.astype(np.float32)
    return (x[:, 0:1] * a[0] + x[:, 1:2] * a[1]) + x[:, 2:3] * a[2]


def concentrations(OD, HE, per_pixel=np.float64):
    """[2,N]: lstsq(HE, OD) in float64, or under the kernel's precision contract (per_pixel=np.float32): pinv(HE) in float64,
    rounded to float32, applied in float32."""
    if per_pixel is np.float64:
        return np.linalg.lstsq(HE, OD.T, rcond=None)[0]
    return _project32(OD, pinv2(HE)[1].T).T


def stats(img, canonicalise=True, per_pixel=np.float64):
    """dict(status, n_tissue, HE [3,2] or None, maxC [2] or None, C [2,N] or None, phi [n_tissue], E [3,2], evals [3],
    minPhi, maxPhi) of one tile.  per_pixel=np.float32 follows the kernel's precision contract: the OD table, E and pinv(HE)
    rounded to float32, products, sums and arctan2 in float32, everything else (the tissue statistics, the eigenproblem, the
    percentile interpolation, HE, pinv) in float64."""
    assert per_pixel in (np.float64, np.float32)
    OD = optical_density(img)
    ODhat = OD[~np.any(OD < S.MACENKO_BETA, axis=1)]
    res = {'status': OK, 'n_tissue': int(ODhat.shape[0]), 'HE': None, 'maxC': None, 'C': None}
    if ODhat.shape[0] < 2:
        res['status'] = FEW_TISSUE
        return res
    with np.errstate(all='ignore'):
        evals, V = np.linalg.eigh(np.cov(ODhat.T))
        E = V[:, 1:3]
        if canonicalise:
            E = canonical(E)
        if per_pixel is np.float64:
            That = ODhat.dot(E)
            phi = np.arctan2(That[:, 1], That[:, 0])
        else:
            That = _project32(ODhat, E)
            phi = np.arctan2(That[:, 1], That[:, 0]).astype(np.float64)
        minPhi = np.percentile(phi, S.MACENKO_ALPHA)
        maxPhi = np.percentile(phi, 100 - S.MACENKO_ALPHA)
        res.update(phi=phi, E=E, evals=evals, minPhi=float(minPhi), maxPhi=float(maxPhi))
        vMin = E.dot(np.array([np.cos(minPhi), np.sin(minPhi)]))
        vMax = E.dot(np.array([np.cos(maxPhi), np.sin(maxPhi)]))
        HE = np.array((vMin, vMax)).T if vMin[0] > vMax[0] else np.array((vMax, vMin)).T
        res['HE'] = HE
        M = HE.T.dot(HE)
        det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        res['det'] = float(det)
        if abs(det) < S.MACENKO_DET_MIN:
            res['status'] = SINGULAR
            return res
        C = concentrations(OD, HE, per_pixel).astype(np.float64)
        maxC = np.array([np.percentile(C[0, :], S.MACENKO_CONC_PCT), np.percentile(C[1, :], S.MACENKO_CONC_PCT)])
    res['maxC'], res['C'] = maxC, C
    if not (np.isfinite(HE).all() and np.isfinite(maxC).all() and (maxC > 0).all()):
        res['status'] = NONFINITE
    return res


def transform(img, HE, maxC, he_ref=HE_REF, maxc_ref=MAXC_REF, per_pixel=np.float64):
    """uint8 tile: ``img`` normalised to the fit (he_ref, maxc_ref) given its statistics HE [3,2] and maxC [2].
    per_pixel=np.float32: the kernel's precision contract (he_ref, maxc_ref and the scale maxc_ref / maxC as float32)."""
    OD = optical_density(img)
    HE, maxC = np.asarray(HE, np.float64), np.asarray(maxC, np.float64)
    with np.errstate(over='ignore'):
        if per_pixel is np.float64:
            C2 = concentrations(OD, HE) / (maxC / np.asarray(maxc_ref, np.float64))[:, None]
            Inorm = S.MACENKO_IO * np.exp(-np.asarray(he_ref, np.float64).dot(C2))
        else:
            f = np.float32
            scale = (np.asarray(maxc_ref, f).astype(np.float64) / maxC).astype(f)
            C2 = concentrations(OD, HE, f) * scale[:, None]
            h = np.asarray(he_ref, f)
            Inorm = f(S.MACENKO_IO) * np.exp(-(h[:, 0:1] * C2[0] + h[:, 1:2] * C2[1]))
    Inorm[Inorm > 255] = S.MACENKO_OVER_TO
    return np.reshape(Inorm.T, img.shape).astype(np.uint8)


def normalise(img, he_ref=HE_REF, maxc_ref=MAXC_REF):
    """(uint8 tile, status): the tile normalised to the fit (he_ref, maxc_ref), or unchanged when degenerate."""
    st = stats(img)
    if st['status'] != OK:
        return img.copy(), st['status']
    return transform(img, st['HE'], st['maxC'], he_ref, maxc_ref), OK


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = abs(a.dot(b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(min(1.0, c))))


# ---------------------------------------------------------------- test tiles
HE_TRUE = np.array([[0.60, 0.25], [0.70, 0.85], [0.39, 0.46]], np.float64)       # haematoxylin / eosin OD vectors (columns)
HE_TRUE /= np.linalg.norm(HE_TRUE, axis=0)


def beer_lambert(n, seed, he=HE_TRUE, background=0.3, noise=2.0, px=299):
    """[n,px,px,3] uint8 two-stain mixtures Io exp(-HE c): smooth random concentration fields, a white-background fraction
    and Gaussian sensor noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(px, dtype=np.float64), np.arange(px, dtype=np.float64), indexing='ij')
    out = np.empty((n, px, px, 3), np.uint8)
    for t in range(n):
        c = np.zeros((2, px, px))
        for s in range(2):
            for _ in range(3):
                fx, fy = rng.uniform(0.01, 0.06, 2)
                c[s] += np.cos(fx * xx + fy * yy + rng.uniform(0, 2 * np.pi)) * rng.uniform(0.2, 0.5)
            c[s] = np.clip(c[s] + rng.uniform(0.6, 1.2), 0, None)
        # nuclei and stroma: where one stain dominates the other is faint, so the extreme angles are the pure stains
        fx, fy = rng.uniform(0.02, 0.08, 2)
        h_side = np.cos(fx * xx + fy * yy + rng.uniform(0, 2 * np.pi)) > 0
        c[1, h_side] *= 0.05
        c[0, ~h_side] *= 0.05
        bg = rng.random((px, px)) < background
        c[:, bg] = 0.0
        od = np.einsum('ks,syx->yxk', he, c)
        img = S.MACENKO_IO * np.exp(-od) + rng.normal(0, noise, (px, px, 3))
        out[t] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def degenerate_tiles(px=299):
    """(tiles [4,px,px,3], expected status): white background, one-colour tissue, flat grey, a single tissue pixel."""
    white = np.full((px, px, 3), 250, np.uint8)
    one = np.full((px, px, 3), (150, 60, 140), np.uint8)
    grey = np.full((px, px, 3), 128, np.uint8)
    single = white.copy()
    single[7, 11] = (120, 40, 130)
    return np.stack([white, one, grey, single]), [FEW_TISSUE, SINGULAR, SINGULAR, FEW_TISSUE]


def noise_tile(seed=0, px=299):
    """Isotropic uniform noise: no stain structure at all."""
    return np.random.default_rng(seed).integers(0, 256, (px, px, 3), dtype=np.uint8)


def generator_tiles(n_bl=8, n_photo=4, n_grain=4):
    """The generator tiles of the tests: Beer-Lambert mixtures, stain_case()'s photo-like tiles and make_tiles(grain=4)."""
    from biscuit_amd.synthetic import make_tiles
    from oracle.make_producer_cfg2_golden import stain_case
    bl = beer_lambert(n_bl, seed=11)
    photo = stain_case()[0][:n_photo]
    grain = make_tiles(n_grain, seed=23, slide_bias=[35.0, -40.0, 20.0], grain=4)
    return np.concatenate([bl, photo, grain])
