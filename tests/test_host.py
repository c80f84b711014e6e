"""CPU tests of the host side: the C-ABI library loads and exports every symbol the
header declares (no compute without a GPU), weight packing matches its definition, the
table contract, partitioning."""
import ctypes
import os
import re
import struct

import numpy as np
import pandas as pd
import pytest

from biscuit_amd import predictions as P
from biscuit_amd import weights as W
from biscuit_amd.distributed import global_tile_offsets, partition_slides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_symbols_exported():
    from biscuit_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'biscuit_hip.h')).read()
    declared = set(re.findall(r'\b(bq_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'bq_ctx', 'bq_config', 'bq_stream_t', 'bq_prof_entry'}
    assert declared == set(_lib.ABI), declared ^ set(_lib.ABI)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    # fails loudly, with a message, when there is no device (never falls back to CPU)
    cfg = _lib.BqConfig(1, 299, 2, 0.1, 8, 30)
    import torch
    if not torch.cuda.is_available():
        assert not _lib.lib.bq_create(0, ctypes.byref(cfg))
        assert b'HIP device' in _lib.lib.bq_last_error(None)
        from biscuit_amd.engine import BiscuitHipError, Engine
        with pytest.raises(BiscuitHipError):
            Engine({}, dtype='bf16')


def test_abi_types_are_the_headers():
    """Every restype and argtype of ``_lib.ABI`` has the width class of the prototype's type at that position: a wrong width in
    one of these lists would corrupt memory on the device, not fail a test."""
    from biscuit_amd import _lib
    from tests._abi_types import assert_abi_matches_header
    assert_abi_matches_header(_lib.ABI, os.path.join(ROOT, 'include', 'biscuit_hip.h'))


def test_the_library_defines_exactly_the_abi():
    """The dynamic symbols of libbiscuit_hip.so that begin with ``bq_`` are the ABI and nothing else, whichever file of csrc/
    defines each: an entry point that a move lost, or a helper that took the prefix, shows here without a GPU."""
    import shutil
    import subprocess
    from biscuit_amd import _lib
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    tools = [shutil.which('nm'), shutil.which('llvm-nm'), os.path.join(rocm, 'llvm', 'bin', 'llvm-nm')]
    nm = next((t for t in tools if t and os.path.exists(t)), None)
    assert nm, 'neither nm nor llvm-nm found: the exported symbols cannot be listed'
    out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split('@')[0] for line in out.splitlines() if line.split()}
    exported = {s for s in defined if s.startswith('bq_')}
    assert exported == set(_lib.ABI), exported ^ set(_lib.ABI)


def test_missing_library_is_an_error(tmp_path):
    from biscuit_amd import _lib
    with pytest.raises(ImportError):
        _lib.load(str(tmp_path / 'nope.so'))


def test_pack_fragments_definition():
    rng = np.random.default_rng(0)
    w = rng.normal(size=(40, 70)).astype(np.float32)
    for vec in (8, 4):
        kpad = 48
        p = W.pack_fragments(w, kpad, vec)
        nfp = p.shape[0]
        assert p.shape == (3, kpad // (2 * vec), 64, vec) and nfp * 32 >= 70
        for nf, kb, lane, v in [(0, 0, 0, 0), (1, 1, 37, 3), (2, kpad // (2 * vec) - 1, 63, vec - 1), (0, 2, 5, 1)]:
            k = kb * 2 * vec + (lane >> 5) * vec + v
            n = nf * 32 + (lane & 31)
            want = w[k, n] if (k < 40 and n < 70) else 0.0
            assert p[nf, kb, lane, v] == want
    assert W.nfrags_padded(728) == 24 and W.nfrags_padded(128) == 4 and W.nfrags_padded(64) == 2
    assert W.pad_channels(728) == 736


def test_bf16_rounding_bits():
    import torch
    x = np.random.default_rng(1).normal(size=1000).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
    assert (W.f32_to_bf16_bits(x) == want).all()


def test_f16_rounding_bits_and_saturation():
    import torch
    x = np.random.default_rng(2).normal(size=1000).astype(np.float32)
    x[:8] = [65504.0, 65519.9, 65520.0, 1e6, -1e6, 6.0e-8, -5.9e-8, 0.0]      # max, just below / at the rounding
    want = torch.from_numpy(np.clip(x, -65504, 65504)).to(torch.float16).view(torch.int16).numpy().astype(np.uint16)
    got = W.f32_to_f16_bits(x)
    assert (got == want).all()
    back = got.view(np.float16).astype(np.float32)
    assert list(back[:5]) == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0] and np.isfinite(back).all()   # saturates, never inf
    assert back[5] == np.float32(2.0 ** -24) and back[6] == -np.float32(2.0 ** -24)                     # subnormals are kept


def test_f16_blob_has_the_layout_of_the_bf16_one():
    """The f16 blob differs from the bf16 one only in the matrix-core weights' bit patterns and the dtype code."""
    w = W.synthetic_weights(3)
    a, b = W.pack_blob(w, 'bf16'), W.pack_blob(w, 'f16')
    assert len(a) == len(b) and struct.unpack_from('<4sIII', b, 0) == (b'BQW1', 1, struct.unpack_from('<4sIII', a, 0)[2], 2)
    n = struct.unpack_from('<4sIII', a, 0)[2]
    for i in range(n):
        ea, eb = (struct.unpack_from('<48sQQ', x, 16 + 64 * i) for x in (a, b))
        assert ea == eb
        nm, off, ln = ea
        nm = nm.rstrip(b'\0').decode()
        half = nm.endswith(('/wp', '/wp16', '/wp32')) and not nm.startswith(('hidden_', 'logits'))
        if not half:
            assert a[off:off + ln] == b[off:off + ln], nm           # fp32 entries: taps, folded BN, head
        elif nm == 'block5_sepconv2/wp':
            fa = (np.frombuffer(a, np.uint16, ln // 2, off).astype(np.uint32) << 16).view(np.float32)
            fb = np.frombuffer(b, np.float16, ln // 2, off).astype(np.float32)
            ref = W.pack_fragments(w['block5_sepconv2/pointwise_kernel'].reshape(728, 728), 736, 8).ravel()
            assert np.abs(fa - ref).max() <= np.abs(ref).max() * 2.0 ** -8
            assert np.abs(fb - ref).max() <= np.abs(ref).max() * 2.0 ** -11      # 8x finer than bf16


def test_fragment_pairs_interleave():
    """kernels_wide.hip's 16x16x32 fragment order: over a pair of fragments a lane (group g of four accumulator rows) owns
    the eight consecutive channels 32q + 8g .. + 7; the map is a bijection on the padded channels."""
    ch = np.array([[W.frag16_channel(nf, r) for r in range(16)] for nf in range(48)])
    assert sorted(ch.ravel()) == list(range(768))
    for q in range(24):
        for g in range(4):
            lane = list(ch[2 * q, 4 * g:4 * g + 4]) + list(ch[2 * q + 1, 4 * g:4 * g + 4])
            assert lane == list(range(32 * q + 8 * g, 32 * q + 8 * g + 8))
    w = np.random.default_rng(0).normal(size=(40, 70)).astype(np.float32)
    p = W.pack_fragments16(w, 64, 96)
    assert p.shape == (2, 6, 64, 8)
    for ks, nf, lane, v in ((0, 0, 0, 0), (1, 3, 37, 5), (0, 5, 63, 7), (1, 4, 20, 2)):
        k, n = ks * 32 + (lane >> 4) * 8 + v, W.frag16_channel(nf, lane & 15)
        assert p[ks, nf, lane, v] == (w[k, n] if (k < 40 and n < 70) else 0.0)


def test_head_weight_split_keeps_fp32_accuracy():
    """kernels_head.hip multiplies fp32 operands as two IEEE halves each: w ~= hi + lo / 2^11.  The pair carries 22
    significand bits, and the three-term product with fp32 accumulation is as close to float64 as a plain fp32 GEMM."""
    rng = np.random.default_rng(5)
    w = rng.uniform(-0.05, 0.05, (2048, 256)).astype(np.float32)
    w[:4, 0] = [0.0, 1e-7, -3e-5, 65000.0]
    hi, lo = (x.view(np.float16).astype(np.float32) for x in W.split_f16(w))
    back = hi + lo / np.float32(W.HEAD_SPLIT_SCALE)
    rel = np.abs(back - w) / np.maximum(np.abs(w), 1e-4)
    assert rel.max() < 2.0 ** -21 and np.isfinite(back).all()
    x = (np.abs(rng.normal(0.8, 0.5, (64, 2048))) * (rng.random((64, 2048)) >= 0.1) / 0.9).astype(np.float32)
    xh, xl = (t.view(np.float16).astype(np.float32) for t in W.split_f16(x))
    ref = x.astype(np.float64) @ w.astype(np.float64)
    three = (xh @ hi) + ((xh @ lo) + (xl @ hi)) / np.float32(W.HEAD_SPLIT_SCALE)
    plain = x @ w
    e3, e1 = np.abs(three - ref), np.abs(plain - ref)
    assert np.sqrt((e3[:, 1:] ** 2).mean()) < 2.0 * np.sqrt((e1[:, 1:] ** 2).mean()) and e3[:, 1:].max() < 1e-5
    blob = W.pack_blob(W.synthetic_weights(3), 'f16')
    n = struct.unpack_from('<4sIII', blob, 0)[2]
    names = {struct.unpack_from('<48sQQ', blob, 16 + 64 * i)[0].rstrip(b'\0').decode(): struct.unpack_from('<48sQQ', blob, 16 + 64 * i)[1:]
             for i in range(n)}
    assert names['hidden_0/wph'][1] == names['hidden_0/wpl'][1] == 32 * 128 * 64 * 8 * 2
    assert names['hidden_1/wph'][1] == 32 * 64 * 64 * 8 * 2 and 'hidden_0/wp' not in names


def test_blob_directory_roundtrip():
    w = W.synthetic_weights(3)
    blob = W.pack_blob(w, 'bf16')
    magic, ver, n, dt = struct.unpack_from('<4sIII', blob, 0)
    assert (magic, ver, dt) == (b'BQW1', 1, 1)
    names = {}
    for i in range(n):
        nm, off, ln = struct.unpack_from('<48sQQ', blob, 16 + 64 * i)
        names[nm.rstrip(b'\0').decode()] = (off, ln)
        assert off % 256 == 0 and off + ln <= len(blob)
    # stem, conv2, res, sepconvs, hidden, logits + the 16x16x32 fragment copy of the 30 wide layers, of the two streaming
    # layers of block 2 and of the block-2 / block-3 shortcuts inside the fused tails (round 4) (16-bit blobs only)
    # ... block 14's two pointwise GEMMs in the same order (kernels_exit.hip)
    # ... and the fused front kernel's two copies: block1_conv1 as f16 hi | lo fragments, block1_conv2 one k-step per tap
    assert len(names) == 3 + 3 + 3 * 4 + 4 * 34 + 3 * 2 + 2 + 30 + 2 + 2 + 2 + 2
    assert {'block2_sepconv1/wp16', 'block2_sepconv2/wp16', 'block2_res/wp16', 'block1_conv1/w16', 'block1_conv2/wp16'} <= set(names)
    assert names['block1_conv1/w16'][1] == 2 * 2 * 64 * 8 * 2 and names['block1_conv2/wp16'][1] == 9 * 4 * 64 * 8 * 2
    # the two halves of the stem weights give the fp32 weights back to 22 bits: hi + lo / 2^11
    off, ln = names['block1_conv1/w16']
    hl = np.frombuffer(blob, np.uint16, ln // 2, off).reshape(2, 2, 64, 8)
    back = hl[0].view(np.float16).astype(np.float64) + hl[1].view(np.float16).astype(np.float64) / 2048.0
    want = W.pack_fragments16(w['block1_conv1/kernel'].reshape(27, 32), 32, 32)[0]
    assert np.abs(back - want).max() <= 2.0 ** -21 * np.abs(want).max()
    assert not any(n.endswith('/wp32') for n in names)
    assert names['block5_sepconv1/wp16'][1] == 23 * 48 * 64 * 8 * 2 and 'block4_sepconv2/wp16' in names
    assert names['block3_sepconv2/wp16'][1] == 8 * 16 * 64 * 8 * 2 and names['block3_sepconv1/wp16'][1] == 4 * 16 * 64 * 8 * 2
    assert names['block2_sepconv2/wp16'][1] == 4 * 8 * 64 * 8 * 2 and names['block2_res/wp16'][1] == 2 * 8 * 64 * 8 * 2
    assert names['block3_res/wp16'][1] == 4 * 16 * 64 * 8 * 2
    assert names['block14_sepconv1/wp16'][1] == 32 * 96 * 64 * 8 * 2 and names['block14_sepconv2/wp16'][1] == 48 * 128 * 64 * 8 * 2
    assert names['block4_sepconv1/wp16'][1] == 8 * 48 * 64 * 8 * 2
    off, ln = names['block5_sepconv2/scale']
    s, b = W.fold_bn(w, 'block5_sepconv2_bn')
    got = np.frombuffer(blob, np.float32, ln // 4, off)
    assert ln == 768 * 4 and np.array_equal(got[:728], s) and not got[728:].any()
    off, ln = names['block5_sepconv2/wp']
    assert ln == 24 * 46 * 64 * 8 * 2
    f32 = W.pack_blob(w, 'f32')
    assert struct.unpack_from('<4sIII', f32, 0)[3] == 0


def test_fold_bn_equals_batchnorm():
    w = W.synthetic_weights(2)
    x = np.random.default_rng(0).normal(size=(5, 128)).astype(np.float32)
    s, b = W.fold_bn(w, 'block2_sepconv1_bn')
    ref = (x - w['block2_sepconv1_bn/moving_mean']) / np.sqrt(w['block2_sepconv1_bn/moving_variance'] + 1e-3) \
        * w['block2_sepconv1_bn/gamma'] + w['block2_sepconv1_bn/beta']
    np.testing.assert_allclose(x * s + b, ref, atol=1e-5)


def test_table_contract(tmp_path):
    mean = np.array([[0.3, 0.7], [0.6, 0.4]], np.float32)
    std = np.array([[0.02, 0.02], [0.05, 0.05]], np.float32)
    df = P.tile_frame('cohort', ['a', 'b'], [1, 0], mean, std)
    assert list(df.columns) == ['slide', 'cohort-y_true0', 'cohort-y_pred0', 'cohort-y_pred1',
                                'cohort-uncertainty0', 'cohort-uncertainty1']
    path = P.save_tile_predictions(df, str(tmp_path))
    assert path.endswith('tile_predictions_eval.csv')
    back = P.load_tile_predictions(path, 'cohort')
    assert {'y_true', 'y_pred', 'uncertainty', 'slide'} <= set(back.columns)
    np.testing.assert_allclose(back['y_pred'], mean[:, 1].astype(np.float64))     # class-1 column
    np.testing.assert_allclose(back['uncertainty'], std[:, 1].astype(np.float64))
    # underscore headers and the '-y_true' fallback (utils.py:31-53)
    d2 = pd.DataFrame({'slide': ['1'], 'o_y_true0': [1], 'o_y_pred1': [0.9], 'o_uncertainty1': [0.1]})
    P.rename_cols(d2, 'o')
    assert {'y_true', 'y_pred', 'uncertainty'} <= set(d2.columns)
    d3 = pd.DataFrame({'slide': ['1'], 'o-y_true': [1], 'o-y_pred1': [0.9], 'o-uncertainty1': [0.1]})
    P.rename_cols(d3, 'o')
    assert 'y_true' in d3.columns
    from biscuit_amd.errors import PredsContainNaNError
    with pytest.raises(PredsContainNaNError):
        P.tile_frame('c', ['a'], [0], np.array([[np.nan, 0.5]], np.float32), std[:1])


def test_partition_and_offsets():
    parts = partition_slides([1000] * 16, 8)
    assert sorted(sum(parts, [])) == list(range(16)) and all(len(p) == 2 for p in parts)
    ragged = [5, 900, 20, 300, 300, 1, 0, 64]
    parts = partition_slides(ragged, 3)
    assert sorted(sum(parts, [])) == list(range(8))
    loads = [sum(ragged[i] for i in p) for p in parts]
    assert max(loads) == 900                     # LPT: the big slide alone
    assert partition_slides(ragged, 3) == parts  # deterministic
    assert partition_slides([], 2) == [[], []]
    assert list(global_tile_offsets([5, 3, 8])) == [0, 5, 8]


def test_hp_mirror():
    from biscuit_amd.hp import nature2022
    hp = nature2022().validate()
    assert (hp.model, hp.tile_px, hp.dropout, hp.hidden_layers, hp.hidden_layer_width, hp.batch_size) == \
        ('xception', 299, 0.1, 2, 1024, 128)
    hp.hidden_layers = 3
    with pytest.raises(ValueError):
        hp.validate()


def test_weight_file_roundtrip_and_validation(tmp_path):
    w = W.synthetic_weights(5)
    assert set(W.expected_shapes()) == set(w)
    path = str(tmp_path / 'model.npz')
    W.save_npz(path, w)
    back = W.load_npz(path)
    assert all(np.array_equal(back[k], w[k]) for k in w)
    bad = dict(w)
    del bad['block7_sepconv2/pointwise_kernel']
    with pytest.raises(ValueError):
        W.validate(bad)
    bad = dict(w); bad['hidden_0/kernel'] = w['hidden_0/kernel'][:, :512]
    with pytest.raises(ValueError):
        W.validate(bad)
    bad = dict(w); bad['logits/bias'] = np.array([np.nan, 0], np.float32)
    with pytest.raises(ValueError):
        W.validate(bad)


def test_cli_model_hp_comes_from_params_json():
    """dropout / uq_n / normalizer of a model's params.json drive the run, never the defaults."""
    from biscuit_amd.__main__ import model_hp
    hp, fit = model_hp(None)
    assert (hp.dropout, hp.uq_n, fit) == (0.1, 30, None)
    nf = {'target_means': [1, 2, 3], 'target_stds': [4, 5, 6]}
    hp, fit = model_hp({'hp': {'dropout': 0.25, 'uq_n': 12}, 'normalizer': 'reinhard_fast', 'norm_fit': nf, 'path': 'p'})
    assert (hp.dropout, hp.uq_n, hp.normalizer) == (0.25, 12, 'reinhard_fast') and fit == nf
    hp, fit = model_hp({'hp': {'dropout': 0.5}, 'normalizer': None, 'norm_fit': None})
    assert hp.dropout == 0.5 and hp.normalizer is None and fit is None
    for bad in ({'hp': {}, 'normalizer': 'macenko', 'norm_fit': nf},          # another normaliser: refuse, do not mis-normalise
                {'hp': {}, 'normalizer': 'reinhard', 'norm_fit': nf},
                {'hp': {}, 'normalizer': None, 'norm_fit': nf},               # a fit but no method named
                {'hp': {}, 'normalizer': 'reinhard_fast', 'norm_fit': None}): # the method but no fit
        with pytest.raises(SystemExit):
            model_hp(bad)
    with pytest.raises(ValueError):
        model_hp({'hp': {'dropout': 1.5}, 'normalizer': None})


def test_heatmap_tile_grid_and_mask_golden():
    """the stride grid of sf.Heatmap(slide, model, stride_div=1) (results.py:217) over a region in
    memory, and the uncertainty mask of results.py:224-225 on a fixed array (golden values written out)."""
    import torch
    from biscuit_amd.heatmap import Heatmap, tile_grid, MASKED
    rng = np.random.default_rng(4)
    region = rng.integers(0, 256, (299 * 2 + 40, 299 * 3 + 7, 3), dtype=np.uint8)
    tiles, grid = tile_grid(region, 299, 1)
    assert tiles.shape == (6, 299, 299, 3) and grid.tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]]
    assert np.array_equal(tiles[4].numpy(), region[299:598, 299:598])          # cell (gx=1, gy=1)
    t2, g2 = tile_grid(torch.from_numpy(region), 299, 13)                       # stride 23: overlapping tiles
    assert t2.shape[0] == ((638 - 299) // 23 + 1) * ((904 - 299) // 23 + 1) and g2[-1].tolist() == [26, 14]
    assert np.array_equal(t2[27 + 2].numpy(), region[23:322, 46:345])           # cell (gx=2, gy=1)
    assert tile_grid(region[:100], 299)[0].shape[0] == 0
    with pytest.raises(ValueError):
        tile_grid(region, 299, 2)                                               # 2 does not divide 299
    # the mask: `uq_mask = hm.uncertainty[:, :, 0] > thresh; hm.logits[uq_mask, :] = [-1, -1]` (strict >)
    hm = Heatmap.__new__(Heatmap)
    hm.uncertainty = np.array([[[0.010, 0.010], [0.030, 0.030], [0.020, 0.020]],
                               [[0.0201, 0.0201], [-1, -1], [0.5, 0.5]]], np.float32)
    hm.logits = np.array([[[0.9, 0.1], [0.2, 0.8], [0.6, 0.4]], [[0.3, 0.7], [-1, -1], [0.5, 0.5]]], np.float32)
    mask = hm.mask_uncertain(0.02)
    assert mask.tolist() == [[False, True, False], [True, False, True]]        # 0.020 is NOT masked (strict), the empty cell neither
    want = np.array([[[0.9, 0.1], [MASKED, MASKED], [0.6, 0.4]], [[MASKED, MASKED], [-1, -1], [MASKED, MASKED]]], np.float32)
    assert np.array_equal(hm.logits, want)


def test_heatmap_region_smaller_than_a_tile():
    """A region that holds no tile: tile_grid returns an empty grid, Heatmap.from_region says so (before it needs a GPU)."""
    from biscuit_amd.heatmap import Heatmap, tile_grid
    small = np.zeros((120, 400, 3), np.uint8)
    tiles, grid = tile_grid(small)
    assert tuple(tiles.shape) == (0, 299, 299, 3) and grid.shape == (0, 2)
    with pytest.raises(ValueError, match='holds no 299 x 299 tile'):
        Heatmap.from_region(None, small)
    tiles, grid = tile_grid(np.zeros((299, 598, 3), np.uint8), stride_div=13)      # one row of cells at stride 23
    assert grid[:, 1].max() == 0 and grid[:, 0].max() == (598 - 299) // 23


def test_tf_fixture_checker_accepts_a_well_formed_file_and_names_what_is_wrong_with_a_bad_one(tmp_path):
    """``tools/make_tf_fixture.py --check`` needs no TensorFlow: the first box that has it must not be able to leave a
    silently unusable fixture (round-3 review, item 8).  A fabricated, well-formed ``io.npz`` passes; every kind of damage
    is named."""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location(
        'make_tf_fixture', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'make_tf_fixture.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(0)
    n = 2
    tiles = rng.integers(0, 256, (n, 299, 299, 3), dtype=np.uint8)
    x = tiles.reshape(n, -1).astype(np.float64)
    std = ((x - x.mean(1, keepdims=True)) / x.std(1, keepdims=True)).reshape(tiles.shape).astype(np.float32)
    io = {'tiles': tiles, 'standardized': std, 'features': rng.random((n, 2048), dtype=np.float32),
          'probs_nodrop': np.array([[0.3, 0.7], [0.6, 0.4]], np.float32)}
    for name in mod.NAMES:
        io[f'tap_{name}'] = rng.random((n,) + mod.TAP_SHAPES[name], dtype=np.float32)
    assert mod.check_io(io) == []
    bad = dict(io); del bad['features']
    assert any('features' in b for b in mod.check_io(bad))
    bad = dict(io); bad['tap_block4_out'] = io['tap_block4_out'][:, :18]
    assert any('tap_block4_out' in b and 'shape' in b for b in mod.check_io(bad))
    bad = dict(io); bad['standardized'] = std.astype(np.float64)
    assert any('dtype' in b for b in mod.check_io(bad))
    bad = dict(io); bad['standardized'] = std[::-1].copy()
    assert any('does not belong' in b for b in mod.check_io(bad))
    bad = dict(io); bad['probs_nodrop'] = np.array([[0.3, 0.9], [0.6, 0.4]], np.float32)
    assert any('probability' in b for b in mod.check_io(bad))
    bad = dict(io); bad['tap_block1_conv2'] = io['tap_block1_conv2'] - 0.5
    assert any('activation' in b for b in mod.check_io(bad))
    # a directory with nothing in it: every file is named
    assert len([b for b in mod.check(str(tmp_path)) if b.startswith('missing file')]) == 4


# ---- activation exponents (weights.py): the host side of the f16 range-by-construction scheme
def test_tensor_plan_covers_every_layer_once_and_shares_exponents_where_tensors_meet():
    from biscuit_amd import weights as W
    plan = W.tensor_plan()
    layers = [l for l, _, _ in plan]
    want = ['block1_conv1', 'block1_conv2'] + [n for n, _, _ in W.sepconv_plan()] + [n for n, _, _ in W.residual_plan()]
    assert sorted(layers) == sorted(want) and len(set(layers)) == len(layers)
    io = {l: (i, o) for l, i, o in plan}
    for b in (2, 3, 4, 13):                                   # both branches of a strided block end on one exponent
        assert io[f'block{b}_sepconv2'][1] == io[f'block{b}_res'][1] == f'block{b}_out'
        assert io[f'block{b}_sepconv1'][0] == io[f'block{b}_res'][0]
    for b in range(5, 13):                                    # the identity shortcuts: one exponent for the whole stream
        assert io[f'block{b}_sepconv1'][0] == io[f'block{b}_sepconv3'][1] == 'block4_out'
    assert io['block13_sepconv1'][0] == io['block13_res'][0] == 'block4_out'
    assert io['block14_sepconv2'][1] == W.FEATURE_TENSOR
    taps = W.tensor_taps()
    assert set(taps) == {o for _, _, o in plan} and 'block12_out' in taps['block4_out'] and 'block4_sepconv2' in taps['block4_out']


def test_activation_exponents_fold_into_the_batchnorm_constants_exactly():
    import struct
    from biscuit_amd import weights as W
    w = W.synthetic_weights(2, hard=True)

    def entries(blob):
        magic, ver, cnt, dt = struct.unpack('<4sIII', blob[:16])
        out = {}
        for i in range(cnt):
            nm, off, ln = struct.unpack('<48sQQ', blob[16 + 64 * i:16 + 64 * (i + 1)])
            out[nm.rstrip(b'\0').decode()] = blob[off:off + ln]
        return out
    a = entries(W.pack_blob(w, 'f16'))
    exp = {'block1_conv2': 3, 'block2_sepconv1': 1, 'block2_out': 4, 'block4_out': 6, 'block7_sepconv2': 2, 'block14_sepconv2': 5}
    b = entries(W.pack_blob(w, 'f16', exp))
    assert set(b) == set(a) | {'act/feat_mul'} and np.frombuffer(b['act/feat_mul'], np.float32)[0] == 32.0
    io = {l: (i, o) for l, i, o in W.tensor_plan()}
    for layer, (tin, tout) in io.items():
        kin, kout = exp.get(tin, 0), exp.get(tout, 0)
        sa, sb = (np.frombuffer(x[layer + '/scale'], np.float32) for x in (a, b))
        ba, bb = (np.frombuffer(x[layer + '/bias'], np.float32) for x in (a, b))
        assert np.array_equal(sb, np.ldexp(sa, kin - kout)) and np.array_equal(bb, np.ldexp(ba, -kout)), layer
    for name in a:                                            # nothing else moves: no weight matrix, no tap, no head tensor
        if not name.endswith(('/scale', '/bias')) or name.startswith(('hidden', 'logits')):
            assert a[name] == b[name], name
    assert W.pack_blob(w, 'bf16') == W.pack_blob(w, 'bf16', {}) and W.pack_blob(w, 'f16', {t: 0 for t in exp}) == W.pack_blob(w, 'f16')
    with pytest.raises(ValueError):
        W.pack_blob(w, 'f16', {'block5_sepconv3': 1})        # not a stored tensor of its own: it only exists as the sum


def test_choose_act_exponents_and_the_equivalent_rescaling():
    from biscuit_amd import weights as W
    from oracle.xception_ref import XceptionOracle
    from biscuit_amd.synthetic import make_tiles
    w = W.synthetic_weights(2, hard=True)
    peaks = {t: 10.0 for _, _, t in W.tensor_plan()}
    assert not any(W.choose_act_exponents(w, peaks).values())                  # fits: nothing to do
    peaks['block4_out'] = 2.0e6
    k = W.choose_act_exponents(w, peaks)
    g = max(W.depthwise_gain(w, f'block{b}_sepconv1') for b in range(5, 14))
    assert k['block4_out'] == int(np.ceil(np.log2(2.0e6 * g / 4096))) and sum(1 for v in k.values() if v) == 1
    assert 2.0e6 * g / 2 ** k['block4_out'] <= 4096 < 2.0e6 * g / 2 ** (k['block4_out'] - 1)
    # the rescaled classifier computes the same function (fp32 oracle, two tiles)
    t = make_tiles(2, seed=9)
    m0, s0 = XceptionOracle(w).mc_predict(t, 4, 11)
    m1, s1 = XceptionOracle(W.equivalent_rescaled(w, 3.0e4)).mc_predict(t, 4, 11)
    assert np.abs(m0 - m1).max() < 2e-5 and np.abs(s0 - s1).max() < 2e-5
