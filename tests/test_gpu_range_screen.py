"""The f16 range screen on the GPU (bq_range_key / bq_range_screen, kernels_screen.hip; evaluate(range_screen=True)): the key bit
for bit against the float64 restatement, the candidate slots against numpy's top k, the silent clamp the sampling monitor misses
caught on every input position, no result changed, nothing launched for bf16 / f32, and the CLI's bytes unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _range_ref as R
from biscuit_amd.synthetic import make_slides, make_tiles
from biscuit_amd.weights import synthetic_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 299 * 299 * 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def key_tiles():
    flat = np.full((1, 299, 299, 3), 128, np.uint8)
    one = flat.copy()
    one[0, 150, 150, 1] = 255
    near = np.full_like(flat, 7)
    near[0, 0, 0, 0] = 8
    spike = flat.copy()
    spike[0, 40:43, 100:103, :] = 255
    return np.concatenate([flat, one, np.zeros_like(flat), np.full_like(flat, 255), near, spike,
                           make_tiles(6, seed=21), make_tiles(4, seed=22, grain=4.0)])


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=64, max_mc=4)
    yield e
    e.close()


def test_range_key_bit_exact_at_every_offset_and_position(eng):
    t = key_tiles()
    ref = R.range_key(t)
    rng = np.random.default_rng(5)
    for off in (0, 1, 2, 3, 5):
        perm = rng.permutation(len(t))
        buf = torch.zeros(len(t) * NB + 16, dtype=torch.uint8, device='cuda')
        view = buf[off:off + len(t) * NB].view(len(t), 299, 299, 3)
        view.copy_(dev(t[perm]))
        got = eng.range_key(view).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref[perm].view(np.uint32)), (off, got, ref[perm])
    big = make_tiles(64, seed=23)
    assert np.array_equal(eng.range_key(dev(big)).cpu().numpy().view(np.uint32), R.range_key(big).view(np.uint32))
    assert eng.range_key(dev(t[:0])).shape == (0,)


def crafted_batches():
    """Tiles with chosen keys and many ties: a few designs, each in several rolled copies -- a permutation of the bytes keeps
    S1, S2, hi and lo, so the key, but not the bytes."""
    designs = []
    for v, size in ((255, 3), (255, 5), (0, 4), (200, 2)):
        d = np.full((299, 299, 3), 128, np.uint8)
        d[60:60 + size, 70:70 + size, :] = v
        designs.append(d)
    designs += list(make_tiles(2, seed=31))
    rng = np.random.default_rng(8)
    tiles = []
    for _ in range(72):
        d = designs[rng.integers(0, len(designs))]
        tiles.append(np.roll(d, (int(rng.integers(0, 299)), int(rng.integers(0, 299))), axis=(0, 1)))
    return np.stack(tiles)


def test_selection_is_numpys_top_k_with_the_right_bytes(eng):
    from biscuit_amd.engine import RangeScreen
    tiles = crafted_batches()
    keys = R.range_key(tiles)
    assert len(np.unique(keys)) < 10                                   # ties everywhere
    gidx = np.arange(1000, 1000 + len(tiles), dtype=np.int64)
    gidx[40:56] = gidx[40:56][::-1] + 500                               # a batch whose indices are not one run (bq_mc_infer's array form)
    for k in (8, 3):
        scr = RangeScreen(eng, k=k, max_batch=32)
        slots, seen = [], []
        for b0, n in ((0, 16), (16, 24), (40, 16), (56, 16)):
            t = dev(tiles[b0:b0 + n])
            if b0 == 40:
                scr.update(t, tile_idx=dev(gidx[b0:b0 + n]))
            else:
                scr.update(t, tile_idx0=int(gidx[b0]))
            batch = [(keys[i], gidx[i], i) for i in range(b0, b0 + n)]
            slots = R.screen_update(slots, batch, k)
            seen += batch
            ck, ci = (x.cpu().numpy() for x in scr.candidates())
            assert scr.filled == len(slots) == min(k, len(seen))
            assert np.array_equal(ci, [s[1] for s in slots]) and np.array_equal(ck.view(np.uint32), np.float32([s[0] for s in slots]).view(np.uint32))
            assert sorted(zip((-ck).tolist(), ci.tolist())) == [(-float(x[0]), int(x[1])) for x in R.top_k(seen, k)]
            got = scr.tiles.cpu().numpy()
            for j, s in enumerate(slots):
                assert np.array_equal(got[j], tiles[s[2]]), (k, b0, j)
        assert scr.screened == len(tiles)
        scr.reset()
        assert scr.filled == 0 and scr.tiles.shape == (0, 299, 299, 3)
        scr.update(dev(tiles[:2]), tile_idx0=7)                        # a new interval starts from empty slots
        assert sorted(scr.candidates()[1].cpu().tolist()) == [7, 8]


# ---------------------------------------------------------------------------------------------------- the gap, closed
def scaled_weights():
    """block1_conv2 stored ~8 x below the f16 limit on ordinary tiles (its BatchNorm scaled up, the two BatchNorms behind it scaled
    back: the same function) -- the construction of the sampling monitor's test, restated."""
    from biscuit_amd.engine import Engine
    w = dict(synthetic_weights(1))
    probe = Engine(w, dtype='f16', max_batch=8, max_mc=4)
    p1 = probe.f16_headroom(dev(make_tiles(8, seed=70)))['max_abs']['block1_conv2']
    probe.close()
    f = 65504.0 / (8.0 * p1)
    for k in ('gamma', 'beta'):
        w['block1_conv2_bn/' + k] = w['block1_conv2_bn/' + k] * np.float32(f)
    for bn in ('block2_sepconv1_bn', 'block2_res_bn'):
        w[bn + '/moving_mean'] = w[bn + '/moving_mean'] * np.float32(f)
        w[bn + '/moving_variance'] = w[bn + '/moving_variance'] * np.float32(f * f)
    return w


def spike_tile():
    t = np.full((299, 299, 3), 128, np.uint8)
    t[40:43, 100:103, :] = 255
    return t


def spiked_slides(at):
    """192 ordinary tiles in two slides (100 + 92) with one spike tile at global index `at`: 6 batches of 32."""
    from biscuit_amd.inference import Slide
    tiles = make_tiles(192, seed=71)
    tiles[at] = spike_tile()
    return [Slide('a', tiles[:100], 100, y_true=0), Slide('b', tiles[100:], 92, y_true=1)]


@pytest.fixture(scope='module')
def scaled():
    from biscuit_amd.engine import Engine, EnginePool
    w = scaled_weights()
    e16 = Engine(w, dtype='f16', max_batch=32, max_mc=4)
    e32 = Engine(w, dtype='f32', max_batch=32, max_mc=4)
    pool = EnginePool(w, n_streams=2, dtype='f16', max_batch=32, max_mc=4)
    yield e16, e32, pool
    pool.close(); e16.close(); e32.close()


def test_screen_catches_the_spike_the_sampling_monitor_misses(scaled, tmp_path):
    from biscuit_amd.engine import F16RangeError
    from biscuit_amd.inference import evaluate
    e16, e32, pool = scaled
    at = 2 * 32 + 20                                                   # position 20 of batch 2
    slides = spiked_slides(at)
    off = evaluate(e16, slides, mc_n=4, seed=5, batch=32, headroom_every=4)
    assert off.f16_checks == 2 and off.f16_headroom >= 2.0 and off.f16_screened == 0     # batches 0 and 4, first 8 tiles: quiet
    truth = evaluate(e32, slides, mc_n=4, seed=5, batch=32)
    d = np.abs(off.tile_df['cohort-y_pred1'].to_numpy() - truth.tile_df['cohort-y_pred1'].to_numpy())
    print(f'spike tile |f16 - f32| = {d[at]:.3e}; other tiles at most {np.delete(d, at).max():.3e}')
    assert d[at] > 1e-3                                                # plausible, finite, wrong: the silent clamp
    assert np.delete(d, at).max() < 1e-3
    with pytest.raises(F16RangeError) as ei:
        evaluate(e16, slides, mc_n=4, seed=5, batch=32, headroom_every=4, range_screen=True, save_dir=str(tmp_path))
    assert f'a tile {at} (global tile {at}, key' in str(ei.value) and 'block1_conv2' in str(ei.value)


def test_screen_catches_the_spike_in_the_final_partial_interval(scaled):
    from biscuit_amd.engine import F16RangeError
    from biscuit_amd.inference import evaluate
    e16, _, _ = scaled
    at = 5 * 32 + 20                                                   # batch 5: the second interval (batches 4, 5) never fills
    slides = spiked_slides(at)
    assert evaluate(e16, slides, mc_n=4, seed=5, batch=32, headroom_every=4).f16_checks == 2
    with pytest.raises(F16RangeError) as ei:
        evaluate(e16, slides, mc_n=4, seed=5, batch=32, headroom_every=4, range_screen=True)
    assert f'b tile {at - 100} (global tile {at}, key' in str(ei.value)
    with pytest.raises(F16RangeError, match=f'global tile {at},'):      # one interval: the whole run, tapped at the end
        evaluate(e16, slides, mc_n=4, seed=5, batch=32, headroom_every=0, range_screen=True)


@pytest.mark.parametrize('at', [2 * 32 + 20, 3 * 32 + 5])
def test_screen_through_a_pool_of_two_streams(scaled, at):
    from biscuit_amd.engine import F16RangeError
    from biscuit_amd.inference import evaluate
    _, _, pool = scaled
    slides = spiked_slides(at)                                         # batch 2 -> engine 0, batch 3 -> engine 1
    assert evaluate(pool, slides, mc_n=4, seed=5, batch=32, headroom_every=2).f16_checks == 3
    with pytest.raises(F16RangeError, match=f'global tile {at},'):
        evaluate(pool, slides, mc_n=4, seed=5, batch=32, headroom_every=2, range_screen=True)


def test_screen_passes_ordinary_tiles_and_reports(scaled):
    from biscuit_amd.inference import Slide, evaluate
    e16, _, pool = scaled
    tiles = make_tiles(192, seed=71)
    slides = [Slide('a', tiles[:100], 100, y_true=0), Slide('b', tiles[100:], 92, y_true=1)]
    for e, every in ((e16, 4), (pool, 2), (e16, 0)):
        r = evaluate(e, slides, mc_n=4, seed=5, batch=32, headroom_every=every, range_screen=True)
        assert r.f16_screened == 192 and r.f16_screen_checks == (2 if every == 4 else 4 if every == 2 else 1)
        assert 2.0 <= r.f16_screen_headroom < 16.0 and r.f16_screen_max_key == R.range_key(tiles).max()


# ---------------------------------------------------------------------------------------------------- no result changes
def test_screen_changes_no_result(tmp_path):
    from biscuit_amd.engine import Engine, EnginePool
    from biscuit_amd.inference import Slide, evaluate
    w = synthetic_weights(1)
    tiles, sidx, y = make_slides(3, 40, seed=4)
    slides = [Slide(f's{i}', tiles[sidx == i], 40, y_true=int(y[i])) for i in range(3)]
    eng = Engine(w, dtype='f16', max_batch=32, max_mc=5)
    pool = EnginePool(w, n_streams=2, dtype='f16', max_batch=32, max_mc=5)
    for e in (eng, pool):
        a = evaluate(e, slides, mc_n=5, seed=9, batch=32, headroom_every=2, save_dir=str(tmp_path / 'off'))
        b = evaluate(e, slides, mc_n=5, seed=9, batch=32, headroom_every=2, save_dir=str(tmp_path / 'on'), range_screen=True)
        assert b.f16_screened == 120 and b.f16_screen_checks > 0 and a.f16_screened == 0
        assert a.tile_df.equals(b.tile_df)
        for f in ('slide_pred', 'slide_unc', 'slide_count'):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert (a.f16_checks, a.f16_headroom) == (b.f16_checks, b.f16_headroom)
        assert open(a.table_path, 'rb').read() == open(b.table_path, 'rb').read()
    pool.close(); eng.close()


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_other_dtypes_launch_nothing(dtype):
    from biscuit_amd.engine import Engine
    from biscuit_amd.inference import Slide, evaluate
    tiles = make_tiles(20, seed=6)
    slides = [Slide('a', tiles, 20, y_true=0)]
    eng = Engine(synthetic_weights(1), dtype=dtype, max_batch=8, max_mc=3)
    eng.profile_enable(True)
    r = evaluate(eng, slides, mc_n=3, seed=1, batch=8, range_screen=True)
    names = [p.name for p in eng.profile_read()]
    eng.profile_enable(False)
    assert r.f16_screened == 0 and r.f16_screen_checks == 0 and not any(n.startswith('range_') for n in names), names
    eng.close()
    f16 = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=3)            # (the positive control)
    f16.profile_enable(True)
    r = evaluate(f16, slides, mc_n=3, seed=1, batch=8, range_screen=True)
    assert r.f16_screened == 20 and 'range_screen' in [p.name for p in f16.profile_read()]
    f16.profile_enable(False)
    f16.close()


def test_cli_bytes_unchanged_by_the_screen(tmp_path):
    outs = {}
    for name, extra in (('on', ['--range-screen']), ('off', []), ('off2', ['--no-range-screen'])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, '-m', 'biscuit_amd', '--synthetic', '3x40', '--batch', '16', '--mc', '3', '--out', str(out)]
                           + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        summary = json.loads(r.stdout.strip().splitlines()[-1])
        summary.pop('tile_table')
        outs[name] = (summary, (out / 'tile_predictions_eval.csv').read_bytes(), (out / 'slide_predictions_cohort_eval.csv').read_bytes())
    assert outs['on'] == outs['off'] == outs['off2'] and outs['on'][0]['tiles'] == 120
