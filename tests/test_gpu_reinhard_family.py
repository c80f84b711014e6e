"""The Reinhard family's kernel (bq_stain_reinhard / bq_stain_reinhard_stats) against tests/_reinhard_family_ref.py, the numpy
restatement of DESIGN.md "Reinhard family": the pattern of tests/test_gpu_stain_domain.py.

Status, the percentile p and the tissue fraction m / N are compared exactly; means and stds within 1 float32 ulp (two float64
reductions in different orders); the bytes exactly against the restatement fed the kernel's OWN reported statistics, so a
one-ulp difference of a mean cannot excuse a byte.  Tile sizes 1, 2, 7, 33 and 299, batches of 1, 3 and 5, all four flag values.
"""
import ctypes as C

import numpy as np
import pytest

import _reinhard_family_ref as R
import _stain_cases as sc
from oracle import stain as O

pytestmark = pytest.mark.gpu

F = np.float32
TM, TS = F([65.0, 12.0, -8.0]), F([14.0, 7.0, 6.0])
FIT = {'target_means': TM.tolist(), 'target_stds': TS.tolist()}
SIZES, BATCHES, FLAGS = (1, 2, 7, 33, 299), (1, 3, 5), (0, 1, 2, 3)


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(seed=1), dtype='f16', max_batch=8, max_mc=4)
    yield e
    e.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _batch(px):
    """Five tiles of one size: noise; noise with a third of its pixels glass; dark noise with a few bright pixels (the
    brightness table clips at 255); all glass (no tissue under the mask); pale noise around the mask level."""
    rng = np.random.default_rng(100 + px)
    t = np.empty((5, px, px, 3), np.uint8)
    t[0] = rng.integers(0, 256, (px, px, 3))
    t[1] = rng.integers(30, 220, (px, px, 3))
    glass = rng.random((px, px)) < 0.33
    t[1][glass] = rng.integers(245, 256, (int(glass.sum()), 3))
    t[2] = rng.integers(0, 70, (px, px, 3))
    bright = rng.random((px, px)) < 0.05
    t[2][bright] = rng.integers(180, 256, (int(bright.sum()), 3))
    t[3] = rng.integers(250, 256, (px, px, 3))
    t[4] = rng.integers(215, 256, (px, px, 1))                      # greys: L from 86 to 100, on both sides of 93
    return t


_TILES, _ANALYSED, _BYTES = {}, {}, {}


def _tiles(px):
    if px not in _TILES:
        _TILES[px] = _batch(px)
        _TILES[px].setflags(write=False)
    return _TILES[px]


def _analysed(px, i, flags):
    """The restatement's steps B, M, S of tile ``i`` of ``_tiles(px)``, computed once."""
    if (px, i, flags) not in _ANALYSED:
        _ANALYSED[px, i, flags] = R.analyse(_tiles(px)[i], flags)
    return _ANALYSED[px, i, flags]


def _want_bytes(px, i, flags, mu, sd):
    """The restatement's bytes of that tile given the kernel's statistics, computed once per value of the statistics."""
    key = (px, i, flags, mu.tobytes(), sd.tobytes())
    if key not in _BYTES:
        _BYTES[key] = R.normalise(_tiles(px)[i], flags, TM, TS, stats=(mu, sd))
    return _BYTES[key]


def _run(eng, d, flags, **kw):
    """(bytes, status, stats [n, 8], status of the statistics call) on the host."""
    import torch
    st = torch.full((d.shape[0],), -1, dtype=torch.int32, device='cuda')
    out = eng.reinhard(d, TM, TS, flags, status=st, **kw)
    stats, st2 = eng.reinhard_stats(d, flags, **{k: v for k, v in kw.items() if k == 'mask_threshold'})
    return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy(), st2.cpu().numpy()


def _check_tile(tag, tile, r, want_bytes, got, status, stats):
    """One tile's status, statistics and bytes against the restatement's analysis ``r``; ``want_bytes(mu, sd)`` -> (bytes, status)."""
    assert status == r['status'], (tag, status, r['status'])
    mu, sd, p, frac = stats[:3], stats[3:6], stats[6], stats[7]
    assert p.view(np.uint32) == F(r['p']).view(np.uint32), (tag, float(p), float(r['p']))
    assert frac.view(np.uint32) == F(r['frac']).view(np.uint32), (tag, float(frac), float(r['frac']))
    if r['status'] != R.OK:
        assert np.isnan(mu).all() and np.isnan(sd).all(), tag
    else:
        assert not np.isnan(stats).any(), tag
        umu, usd = sc.ulps32(mu, r['mu']), sc.ulps32(sd, r['sd'])
        assert (umu <= 1).all() and (usd <= 1).all(), (tag, umu.tolist(), usd.tolist())
    want, want_status = want_bytes(mu.copy(), sd.copy())
    assert want_status == status
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (tag, len(bad), [(int(y), int(x), int(c), int(got[y, x, c]), int(want[y, x, c])) for y, x, c in bad[:5]])


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('px', SIZES)
def test_status_statistics_and_bytes_match_the_restatement(eng, px, flags):
    tiles = _tiles(px)
    d = _dev(tiles)
    seen = set()
    for n in BATCHES:
        got, st, stats, st2 = _run(eng, d[:n].contiguous(), flags)
        assert np.array_equal(st, st2)
        for i in range(n):
            r = _analysed(px, i, flags)
            _check_tile((px, flags, n, i), tiles[i], r, lambda mu, sd, i=i: _want_bytes(px, i, flags, mu, sd), got[i], int(st[i]), stats[i])
            seen.add(int(st[i]))
    if px >= 7:
        assert R.OK in seen and (R.NO_TISSUE in seen) == bool(flags & R.MASK)
        if flags & R.BRIGHTNESS:                                   # the dark tile clips: some byte below 255 became 255
            bright = _analysed(px, 2, flags)['bright']
            assert ((bright == 255) & (tiles[2] < 255)).any()


def test_flags_0_is_reinhard_fast_byte_for_byte(eng):
    import torch
    d = _dev(_tiles(299))
    assert torch.equal(eng.reinhard(d, TM, TS, 0), eng.reinhard_fast(d, TM, TS))
    stats, st = eng.reinhard_stats(d, 0)
    assert torch.equal(stats[:, :6].contiguous().view(torch.int32), eng.lab_stats(d).view(torch.int32))
    assert not bool(st.any()) and bool((stats[:, 6] == 100).all()) and bool((stats[:, 7] == 1).all())


def _one(eng, tile, flags, mask_threshold=R.MASK_THRESHOLD):
    """One tile through both entries and against the restatement; returns (analysis, bytes, stats [8])."""
    mask_L = R.mask_level(mask_threshold)
    r = R.analyse(tile, flags, mask_L)
    got, st, stats, st2 = _run(eng, _dev(tile[None]), flags, mask_threshold=mask_threshold)
    assert st[0] == st2[0]
    _check_tile(('one', flags), tile, r, lambda mu, sd: R.normalise(tile, flags, TM, TS, mask_L, stats=(mu, sd)), got[0], int(st[0]), stats[0])
    return r, got[0], stats[0]


def test_percentile_edges(eng):
    rng = np.random.default_rng(7)
    # N = 1: v = 0, the successor is the element itself
    t = np.array([[[120, 90, 60]]], np.uint8)
    r, _, stats = _one(eng, t, 1)
    assert stats[6] == O.rgb_to_lab(t[None])[0][0, 0, 0] and r['status'] == R.OK
    # N = 4: v = 2.7, a true interpolation between the third and the fourth value
    t = np.array([[[10, 10, 10], [200, 200, 200]], [[90, 90, 90], [140, 140, 140]]], np.uint8)
    r, _, stats = _one(eng, t, 1)
    L = np.sort(O.rgb_to_lab(t[None])[0].ravel())
    assert L[2] < stats[6] < L[3] and stats[6] == F(np.percentile(L.astype(np.float64), 90))
    # a long run of ties across index lo (N = 1 089, lo = 979): 80 % .. 95 % of the sorted L is one value, then: the run ends
    # exactly at lo, so the successor is another value
    n, lo = 33 * 33, int(np.floor(0.9 * (33 * 33 - 1)))
    for run_end in (int(0.95 * n), lo + 1):
        colours = np.concatenate([rng.integers(0, 100, (int(0.8 * n), 3)), np.tile([[150, 140, 160]], (run_end - int(0.8 * n), 1)),
                                  rng.integers(200, 256, (n - run_end, 3))]).astype(np.uint8)
        t = colours[rng.permutation(n)].reshape(33, 33, 3)
        r, _, stats = _one(eng, t, 3)
        L = np.sort(O.rgb_to_lab(t[None])[0].ravel())
        tie = O.rgb_to_lab(np.array([[[[150, 140, 160]]]], np.uint8))[0][0, 0, 0]
        assert L[lo] == tie and (L[lo + 1] == tie) == (run_end != lo + 1)
        assert stats[6] == F(np.percentile(L.astype(np.float64), 90))
    # bright enough to clip: nine tenths dark, one tenth bright -> s > 2, bytes above 127 become 255
    colours = np.concatenate([rng.integers(20, 90, (1000, 3)), rng.integers(128, 256, (89, 3))]).astype(np.uint8)
    t = colours[rng.permutation(n)].reshape(33, 33, 3)
    r, got, stats = _one(eng, t, 1)
    assert 100.0 / stats[6] > 2 and ((r['bright'] == 255) & (t < 255)).sum() > 50


def test_dark_and_no_tissue(eng):
    import torch
    black = np.zeros((7, 7, 3), np.uint8)
    for flags in (1, 3):
        d = _dev(black[None])
        out = torch.full_like(d, 7)
        st = torch.full((1,), -1, dtype=torch.int32, device='cuda')
        eng.reinhard(d, TM, TS, flags, out=out, status=st)
        assert int(st[0]) == R.DARK and torch.equal(out, d)
        r, got, stats = _one(eng, black, flags)
        assert r['status'] == R.DARK and stats[6] == 0 and np.array_equal(got, black)
    white = np.full((7, 7, 3), 255, np.uint8)
    for flags in (2, 3):
        r, got, stats = _one(eng, white, flags)
        assert r['status'] == R.NO_TISSUE and stats[6] == 100 and stats[7] == 0 and np.array_equal(got, white)
    # NO_TISSUE with I' != I: the brightest tenth white, the rest a grey whose standardised L is not below a raised mask_L
    t = np.full((10, 10, 3), 200, np.uint8)
    t.reshape(100, 3)[np.random.default_rng(3).permutation(100)[:10]] = 255
    thr = 0.95
    r = R.analyse(t, 3, R.mask_level(thr))
    assert r['status'] == R.NO_TISSUE and r['p'] < 100 and (r['bright'] != t).any()               # (on the CPU)
    assert (O.rgb_to_lab(r['bright'][None])[0] >= R.mask_level(thr)).all() and R.mask_level(thr) > R.mask_level()
    r, got, stats = _one(eng, t, 3, mask_threshold=thr)
    assert np.array_equal(got, r['bright']) and (got != t).any() and stats[7] == 0


def test_one_tissue_pixel_falls_under_the_nan_rule(eng):
    t = np.full((7, 7, 3), 255, np.uint8)
    t[3, 4] = (150, 90, 140)
    for flags in (2, 3):
        r, got, stats = _one(eng, t, flags)
        assert r['status'] == R.OK and r['m'] == 1 and stats[7] == F(1 / 49)
        assert (stats[3:6] == 0).all()                                 # sd = 0: target_std / 0 times a zero difference is NaN
        assert (got[3, 4] == 0).all()                                  # and NaN is byte 0
        keep = np.ones((7, 7), bool)
        keep[3, 4] = False
        assert np.array_equal(got[keep], r['bright'][keep])


def test_the_mask_is_a_strict_less_than(eng):
    rng = np.random.default_rng(11)
    levels = np.array([100, 150, 200, 230], np.uint8)
    t = np.repeat(levels[rng.integers(0, 4, (33, 33))][..., None], 3, axis=2)
    L200 = O.rgb_to_lab(np.full((1, 1, 1, 3), 200, np.uint8))[0][0, 0, 0]
    below, at = int((t[..., 0] < 200).sum()), int((t[..., 0] == 200).sum())
    assert below > 0 and at > 0
    for mask_L, m in ((L200, below), (np.nextafter(L200, F(np.inf)), below + at)):
        thr = float(np.float64(mask_L) / 100.0)
        assert R.mask_level(thr).view(np.uint32) == F(mask_L).view(np.uint32)        # the engine hands over exactly this mask_L
        r, got, stats = _one(eng, t, 2, mask_threshold=thr)
        assert r['m'] == m and stats[7] == F(m / (33 * 33))
        assert (got[t[..., 0] == 200] == 200).all() == (m == below)                   # not tissue: its bytes stay


def test_in_place_batch_position_and_repeat(eng):
    import torch
    d = _dev(_tiles(33))
    for flags in FLAGS:
        st5 = torch.empty(5, dtype=torch.int32, device='cuda')
        alone = eng.reinhard(d, TM, TS, flags, status=st5)
        assert torch.equal(eng.reinhard(d, TM, TS, flags), alone)
        inplace = d.clone()
        assert eng.reinhard(inplace, TM, TS, flags, out=inplace) is inplace
        assert torch.equal(inplace, alone)
        stats5, _ = eng.reinhard_stats(d, flags)
        for k in range(5):
            st1 = torch.empty(1, dtype=torch.int32, device='cuda')
            assert torch.equal(eng.reinhard(d[k:k + 1].contiguous(), TM, TS, flags, status=st1)[0], alone[k])
            assert int(st1[0]) == int(st5[k])
            s1, _ = eng.reinhard_stats(d[k:k + 1].contiguous(), flags)
            assert s1.cpu().numpy().tobytes() == stats5[k:k + 1].cpu().numpy().tobytes()
        idx = torch.tensor([4, 2, 0, 3, 1, 2], device='cuda')
        assert torch.equal(eng.reinhard(d[idx].contiguous(), TM, TS, flags), alone[idx])


def test_abi_refuses_bad_arguments(eng):
    import torch
    from biscuit_amd.engine import BiscuitHipError, _ptr
    d = _dev(_tiles(7)[:1])
    out = torch.full_like(d, 7)
    stats = torch.full((1, 8), 7.0, device='cuda')
    f3 = C.c_float * 3
    good = dict(px=7, flags=3, mask_L=93.0, tm=TM.tolist(), ts=TS.tolist())
    nan = float('nan')
    for change, word in (({'px': 0}, 'px'), ({'px': 1025}, 'px'), ({'flags': 4}, 'flags'), ({'flags': -1}, 'flags'),
                         ({'tm': [65.0, nan, -8.0]}, 'non-finite'), ({'ts': [nan, 7.0, 6.0]}, 'non-finite'),
                         ({'ts': [14.0, float('inf'), 6.0]}, 'non-finite'), ({'mask_L': nan}, 'mask_L')):
        a = {**good, **change}
        rc = eng._lib.bq_stain_reinhard(eng._ctx, _ptr(d), 1, a['px'], a['flags'], a['mask_L'], f3(*a['tm']), f3(*a['ts']), _ptr(out), None,
                                        eng._stream())
        assert rc < 0, (change, rc)
        assert word in eng._lib.bq_last_error(eng._ctx).decode(), (change, eng._lib.bq_last_error(eng._ctx).decode())
        if 'tm' not in change and 'ts' not in change:
            rc = eng._lib.bq_stain_reinhard_stats(eng._ctx, _ptr(d), 1, a['px'], a['flags'], a['mask_L'], _ptr(stats), None, eng._stream())
            assert rc < 0 and word in eng._lib.bq_last_error(eng._ctx).decode(), change
    for null in ('tiles', 'out'):
        rc = eng._lib.bq_stain_reinhard(eng._ctx, None if null == 'tiles' else _ptr(d), 1, 7, 3, 93.0, f3(*good['tm']), f3(*good['ts']),
                                        None if null == 'out' else _ptr(out), None, eng._stream())
        assert rc < 0 and 'bad argument' in eng._lib.bq_last_error(eng._ctx).decode()
    with pytest.raises(BiscuitHipError, match='non-finite'):
        eng.reinhard(d, [nan, 0, 0], TS, 3, out=out)
    with pytest.raises(BiscuitHipError, match='mask_L'):
        eng.reinhard(d, TM, TS, 3, mask_threshold=nan, out=out)
    with pytest.raises(BiscuitHipError, match='flags'):
        eng.reinhard_stats(d, 4)
    assert bool((out == 7).all()) and bool((stats == 7).all())                      # a rejected call launches nothing
    r, _, _ = _one(eng, _tiles(7)[1], 3)                                            # and the engine goes on working
    assert r['status'] == R.OK


def test_normalise_and_the_classes(eng):
    import torch
    from biscuit_amd import stain
    tiles = np.array(_tiles(299)[:2])                               # (copies: the classes take the caller's arrays as they are)
    d = _dev(tiles)
    for name, flags in stain.REINHARD_FLAGS.items():
        st = torch.full((2,), -1, dtype=torch.int32, device='cuda')
        got = stain.normalise(eng, d, name, FIT, status=st if name != 'reinhard_fast' else None)
        assert torch.equal(got, eng.reinhard(d, TM, TS, flags))
        assert name == 'reinhard_fast' or st.tolist() == [0, 0]
        norm = stain.make_normalizer(eng, name, FIT)
        assert norm.method == name and torch.equal(norm.rgb_to_rgb(tiles), got) and torch.equal(norm.rgb_to_rgb(tiles[1]), got[1])
    target = np.array(_tiles(33)[1])
    for cls, flags in ((stain.Reinhard, 1), (stain.ReinhardMask, 3), (stain.ReinhardFastMask, 2)):
        norm = cls(eng).fit(target)
        mu, sd = R.fit(target, flags)
        assert (sc.ulps32(norm.target_means, mu) <= 1).all() and (sc.ulps32(norm.target_stds, sd) <= 1).all()
        back = cls.from_params(eng, {'norm_fit': norm.get_fit()})
        assert back.get_fit() == norm.get_fit() and back.method == norm.method
        small = np.array(_tiles(7))
        assert torch.equal(back.rgb_to_rgb(small), eng.reinhard(_dev(small), norm.target_means, norm.target_stds, flags))
    with pytest.raises(ValueError, match='degenerate'):
        stain.Reinhard(eng).fit(np.zeros((7, 7, 3), np.uint8))
    with pytest.raises(ValueError, match='degenerate'):
        stain.ReinhardFastMask(eng).fit(np.full((7, 7, 3), 255, np.uint8))


def test_evaluate_with_reinhard_mask_equals_prenormalised(eng, tmp_path):
    import torch
    from biscuit_amd import stain
    from biscuit_amd.inference import Slide, evaluate
    x = torch.from_numpy(np.stack([_tiles(299)[1], np.full((299, 299, 3), 255, np.uint8)]))      # tissue with glass; glass only
    pre = stain.normalise(eng, x.cuda(), 'reinhard_mask', FIT).cpu()
    assert not torch.equal(pre[0], x[0]) and torch.equal(pre[1], x[1])
    r1 = evaluate(eng, [Slide('a', x, 2, y_true=0)], mc_n=3, seed=5, batch=8, save_dir=str(tmp_path / 'm'), normalizer='reinhard_mask',
                  norm_fit=FIT)
    r2 = evaluate(eng, [Slide('a', pre, 2, y_true=0)], mc_n=3, seed=5, batch=8, save_dir=str(tmp_path / 'p'))
    with open(r1.table_path, 'rb') as f1, open(r2.table_path, 'rb') as f2:
        assert f1.read() == f2.read()
    assert r1.stain_passthrough == 1 and r2.stain_passthrough == 0
