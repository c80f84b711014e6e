"""The Macenko stain normaliser (DESIGN.md "Macenko"): the float64 numpy restatement in tests/_macenko_ref.py on the CPU, the
kernel behind bq_stain_macenko against it on the GPU, and the layers above it -- stain.Macenko, stain.normalise, evaluate,
UncertaintyInterface and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _macenko_ref as R
from biscuit_amd import stain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = {'stain_matrix_target': [list(r) for r in stain.MACENKO_HE_REF], 'target_concentrations': list(stain.MACENKO_MAXC_REF)}


@pytest.fixture(scope='module')
def tiles():
    return R.generator_tiles()


# ---------------------------------------------------------------- CPU
def test_cli_model_hp_accepts_macenko_fit():
    from biscuit_amd.__main__ import model_hp
    hp, fit = model_hp({'hp': {'dropout': 0.2}, 'normalizer': 'macenko', 'norm_fit': FIT, 'path': 'p'})
    assert hp.normalizer == 'macenko' and hp.dropout == 0.2 and fit == FIT
    bad_fits = [None, {}, {'target_means': [1, 2, 3], 'target_stds': [4, 5, 6]},                    # missing / Reinhard's keys
                {'stain_matrix_target': [[1, 2], [3, 4]], 'target_concentrations': [1, 1]},        # 2x2
                {'stain_matrix_target': FIT['stain_matrix_target'], 'target_concentrations': [1, 1, 1]},
                {'stain_matrix_target': [[0.5, float('nan')], [0.7, 0.8], [0.4, 0.5]], 'target_concentrations': [1, 1]},
                {'stain_matrix_target': FIT['stain_matrix_target'], 'target_concentrations': [1.9, 0.0]},
                {'stain_matrix_target': FIT['stain_matrix_target'], 'target_concentrations': [1.9, -1.0]},
                {'stain_matrix_target': FIT['stain_matrix_target'], 'target_concentrations': ['a', 1.0]}]
    for bad in bad_fits:
        with pytest.raises(SystemExit):
            model_hp({'hp': {}, 'normalizer': 'macenko', 'norm_fit': bad, 'path': 'p'})
    for name in ('reinhard', 'vahadane', 'macenko_mask'):
        with pytest.raises(SystemExit):
            model_hp({'hp': {}, 'normalizer': name, 'norm_fit': FIT})


def test_dispatch_refuses_unknown_or_mismatched():
    stain.check('macenko', FIT)
    stain.check('reinhard_fast', {'target_means': [1, 2, 3], 'target_stds': [4, 5, 6]})
    stain.check('anything', None)                                  # no fit: no normaliser
    for name, fit in (('reinhard', FIT), ('macenko', {'target_means': [1, 2, 3], 'target_stds': [4, 5, 6]}),
                      ('reinhard_fast', FIT)):
        with pytest.raises(ValueError):
            stain.check(name, fit)
    with pytest.raises(ValueError):
        stain.normalise(None, None, 'vahadane', FIT)


def test_macenko_from_params_json(tmp_path):
    from biscuit_amd.keras_import import read_params
    he = [[0.6, 0.2], [0.7, 0.8], [0.4, 0.55]]
    with open(tmp_path / 'params.json', 'w') as f:
        json.dump({'hp': {'model': 'xception', 'tile_px': 299, 'normalizer': 'macenko'},
                   'norm_fit': {'stain_matrix_target': he, 'target_concentrations': [1.8, 1.1]}}, f)
    params = read_params(str(tmp_path))
    assert params['normalizer'] == 'macenko'
    m = stain.Macenko.from_params(None, params)
    np.testing.assert_allclose(m.stain_matrix, np.float32(he))
    np.testing.assert_allclose(m.concentrations, np.float32([1.8, 1.1]))
    assert m.get_fit() == {'stain_matrix_target': np.float32(he).tolist(), 'target_concentrations': np.float32([1.8, 1.1]).tolist()}
    m2 = stain.Macenko.from_params(None, str(tmp_path / 'params.json'))
    np.testing.assert_array_equal(m2.stain_matrix, m.stain_matrix)
    np.testing.assert_allclose(stain.Macenko.preset(None).stain_matrix, np.float32(stain.MACENKO_HE_REF))
    with pytest.raises(ValueError):
        stain.Macenko.from_params(None, {'norm_fit': {'target_means': [1, 2, 3], 'target_stds': [4, 5, 6]}})


def test_restatement_recovers_true_stains_h_first():
    for x in R.beer_lambert(8, seed=11):
        st = R.stats(x)
        assert st['status'] == R.OK
        assert R.angle_deg(st['HE'][:, 0], R.HE_TRUE[:, 0]) < 3.0          # measured: at most 1.5 degrees
        assert R.angle_deg(st['HE'][:, 1], R.HE_TRUE[:, 1]) < 3.0


def test_restatement_sign_canonicalisation_changes_nothing(tiles):
    for x in tiles:
        a, b = R.stats(x, canonicalise=True), R.stats(x, canonicalise=False)
        assert a['status'] == b['status'] == R.OK
        np.testing.assert_allclose(a['HE'], b['HE'], atol=1e-12)
        np.testing.assert_allclose(a['maxC'], b['maxC'], rtol=1e-12)


def test_restatement_degenerate_tiles_pass_through():
    deg, want = R.degenerate_tiles()
    for x, w in zip(deg, want):
        out, status = R.normalise(x)
        assert status == w and np.array_equal(out, x)


# ---------------------------------------------------------------- GPU
def _engine(dtype='f32', max_batch=8):
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    return Engine(synthetic_weights(1), dtype=dtype, max_batch=max_batch, max_mc=4)


def _gpu_set(tiles):
    """64 tiles: the generator tiles, repeated with perturbations."""
    rng = np.random.default_rng(5)
    out = [tiles]
    while sum(len(t) for t in out) < 64:
        noise = rng.integers(-3, 4, tiles.shape)
        out.append(np.clip(tiles.astype(np.int16) + noise, 0, 255).astype(np.uint8))
    return np.concatenate(out)[:64]


@pytest.mark.gpu
def test_macenko_stats_match_restatement(tiles):
    import torch
    eng = _engine()
    x = _gpu_set(tiles)
    stats, st = eng.macenko_stats(torch.from_numpy(x).cuda())
    stats, st = stats.cpu().numpy().astype(np.float64), st.cpu().numpy()
    worst_he, worst_c = 0.0, 0.0
    for i in range(len(x)):
        ref = R.stats(x[i])
        assert st[i, 0] == ref['status'] and st[i, 1] == ref['n_tissue'], i
        worst_he = max(worst_he, float(np.abs(stats[i, :6].reshape(3, 2) - ref['HE']).max()))
        worst_c = max(worst_c, float(np.abs(stats[i, 6:] / ref['maxC'] - 1).max()))
    print(f'macenko_stats vs restatement: max |dHE| {worst_he:.3e}, max rel dmaxC {worst_c:.3e}')
    assert worst_he < 2e-6 and worst_c < 2e-6


@pytest.mark.gpu
def test_macenko_bytes_match_restatement(tiles):
    import torch
    eng = _engine()
    x = _gpu_set(tiles)
    out = eng.macenko(torch.from_numpy(x).cuda(), stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF).cpu().numpy()
    ref = np.stack([R.normalise(t)[0] for t in x])
    d = np.abs(out.astype(np.int16) - ref.astype(np.int16))
    print(f'macenko bytes vs restatement: max diff {int(d.max())}, fraction differing {float((d > 0).mean()):.2e}')
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


@pytest.mark.gpu
def test_macenko_degenerate_and_noise_tiles():
    import torch
    eng = _engine()
    deg, want = R.degenerate_tiles()
    x = np.concatenate([deg, R.noise_tile()[None]])
    st = torch.empty(len(x), dtype=torch.int32, device='cuda')
    out = eng.macenko(torch.from_numpy(x).cuda(), stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF, status=st).cpu().numpy()
    st = st.cpu().numpy()
    assert st[:4].tolist() == want
    assert np.array_equal(out[:4], deg)
    assert st[4] == R.normalise(x[4])[1]
    _, st2 = eng.macenko_stats(torch.from_numpy(x).cuda())
    assert st2[:, 0].cpu().numpy().tolist() == st.tolist()


@pytest.mark.gpu
def test_macenko_batch_position_repeatability_in_place(tiles):
    import torch
    eng = _engine()
    he, mc = stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF
    big = _gpu_set(tiles)
    big = np.concatenate([big] * 4)                      # 256 tiles
    d = torch.from_numpy(big).cuda()
    a = eng.macenko(d, he, mc)
    b = eng.macenko(d, he, mc)
    assert torch.equal(a, b)
    one = eng.macenko(d[200:201].contiguous(), he, mc)
    assert torch.equal(one[0], a[200])
    inplace = d.clone()
    r = eng.macenko(inplace, he, mc, out=inplace)
    assert r.data_ptr() == inplace.data_ptr() and torch.equal(inplace, a)


@pytest.mark.gpu
def test_evaluate_with_macenko_equals_prenormalised(tmp_path, tiles):
    import torch
    from biscuit_amd.inference import Slide, evaluate
    eng = _engine('f16', max_batch=16)
    deg, _ = R.degenerate_tiles()
    x = np.concatenate([tiles[:6], deg[:2], tiles[6:12], deg[2:]])        # 16 tiles, 4 degenerate
    pre = eng.macenko(torch.from_numpy(x).cuda(), stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF).cpu()

    def slides(t):
        return [Slide('a', t[:7], 7, y_true=0), Slide('b', t[7:], 9, y_true=1)]
    r1 = evaluate(eng, slides(torch.from_numpy(x)), mc_n=3, seed=5, batch=8, save_dir=str(tmp_path / 'm'),
                  normalizer='macenko', norm_fit=FIT)
    r2 = evaluate(eng, slides(pre), mc_n=3, seed=5, batch=8, save_dir=str(tmp_path / 'p'))
    with open(r1.table_path, 'rb') as f1, open(r2.table_path, 'rb') as f2:
        assert f1.read() == f2.read()
    assert r1.stain_passthrough == 4 and r2.stain_passthrough == 0
    with pytest.raises(ValueError):
        evaluate(eng, slides(torch.from_numpy(x)), mc_n=3, normalizer='macenko', norm_fit={'target_means': [1, 2, 3],
                                                                                       'target_stds': [4, 5, 6]})


@pytest.mark.gpu
def test_f32_predictions_on_kernel_vs_restatement_tiles(tiles):
    import torch
    eng = _engine('f32', max_batch=16)
    x = tiles[:12]
    k = eng.macenko(torch.from_numpy(x).cuda(), stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF)
    ref = torch.from_numpy(np.ascontiguousarray(np.stack([R.normalise(t)[0] for t in x]))).cuda()
    mk, sk = eng.mc_infer(k, 4, 7)
    mr, sr = eng.mc_infer(ref, 4, 7)
    assert float((mk - mr).abs().max()) < 1e-3 and float((sk - sr).abs().max()) < 1e-3


@pytest.mark.gpu
def test_uncertainty_interface_and_fit(tiles):
    import torch
    from biscuit_amd.engine import UncertaintyInterface
    eng = _engine()
    ui = UncertaintyInterface(eng, uq_n=2, norm_fit=FIT, normalizer='macenko')
    assert isinstance(ui.wsi_normalizer, stain.Macenko)
    d = torch.from_numpy(tiles[:3]).cuda()
    assert torch.equal(ui.wsi_normalizer.rgb_to_rgb(d), eng.macenko(d, stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF))
    assert torch.equal(ui.wsi_normalizer.rgb_to_rgb(tiles[1]), eng.macenko(d[1:2], stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF)[0])
    m = stain.Macenko(eng).fit(tiles[0])
    ref = R.stats(tiles[0])
    np.testing.assert_allclose(np.asarray(m.get_fit()['stain_matrix_target']), ref['HE'], atol=2e-6)
    np.testing.assert_allclose(m.get_fit()['target_concentrations'], ref['maxC'], rtol=2e-6)
    with pytest.raises(ValueError):
        stain.Macenko(eng).fit(R.degenerate_tiles()[0][0])
    assert UncertaintyInterface(eng, uq_n=2, norm_fit=None, normalizer='macenko').wsi_normalizer is None


@pytest.mark.gpu
def test_cli_synthetic_with_macenko_params(tmp_path):
    p = tmp_path / 'params.json'
    with open(p, 'w') as f:
        json.dump({'hp': {'normalizer': 'macenko', 'dropout': 0.1}, 'norm_fit': FIT}, f)
    out = tmp_path / 'eval'
    r = subprocess.run([sys.executable, '-m', 'biscuit_amd', '--synthetic', '4x64', '--params', str(p), '--out', str(out),
                        '--mc', '3'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary['tiles'] == 256 and os.path.exists(out / 'tile_predictions_eval.csv')
