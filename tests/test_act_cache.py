"""The activation cache's stores on the host side (biscuit_amd/train.py; DESIGN.md section 7 "Exit-flow fine-tuning", Sizes): byte
counts, the memory check and its message, the 'auto' ladder, the file format of the 16-bit forms, and the command line.  No device."""
import os

import numpy as np
import pytest
import torch

from biscuit_amd import train as T

ROW32, ROW16 = 409600, 204800


def test_byte_counts_per_store():
    assert T.ACT_STORES == ('f32', 'packed', 'host', 'auto')
    assert T.activation_cache_bytes(1000, 2) == 1000 * ROW32 * 3 == T.activation_cache_bytes(1000, 2, 'f32')
    assert T.activation_cache_bytes(1000, 2, 'packed') == 1000 * ROW16 * 3
    for dtype in ('f16', 'bf16'):
        assert T.activation_cache_bytes(7, 1, 'packed', dtype) == 7 * ROW16 * 2 == T.activation_cache_bytes(7, 1, 'host', dtype)
        assert T.activation_cache_bytes(7, 1, 'f32', dtype) == 7 * ROW32 * 2
    assert T.activation_cache_bytes(7, 0, 'host', 'f32') == 7 * ROW32                # an f32 engine's host cache stays float32
    assert T.act_row_bytes() == ROW32 and T.act_row_bytes('packed') == ROW16
    # tiles per 288 GB card: 600 000 as float32 leave a quarter of the memory free, packed holds twice as many
    assert T.activation_cache_bytes(600000, 0) < 288e9 < T.activation_cache_bytes(1200000, 0)
    assert T.activation_cache_bytes(1200000, 0, 'packed') == T.activation_cache_bytes(600000, 0)
    with pytest.raises(ValueError):
        T.activation_cache_bytes(1, 0, 'auto')
    with pytest.raises(ValueError):
        T.activation_cache_bytes(1, 0, 'host', 'f64')


def test_check_activation_memory_per_store_and_its_message():
    assert T.check_activation_memory(1000, 0, 409600000) == 409600000
    assert T.check_activation_memory(1000, 1, 409600000, 'packed') == 409600000
    assert T.check_activation_memory(1000, 1, 409600000, 'host', 'bf16') == 409600000
    with pytest.raises(ValueError) as err:
        T.check_activation_memory(1000, 1, 500000000)
    text = str(err.value)
    assert '819200000' in text and '500000000' in text and '--act-cache packed' in text and '--act-cache host' in text
    assert 'out of scope' not in text and 'the device has' in text
    with pytest.raises(ValueError) as err:
        T.check_activation_memory(1000, 1, 409599999, 'packed')
    text = str(err.value)
    assert '409600000' in text and '409599999' in text and '204800' in text and '--act-cache host' in text and '--act-cache packed' not in text
    with pytest.raises(ValueError) as err:
        T.check_activation_memory(1000, 0, 1000, 'host', 'f16')
    assert 'the host has 1000 bytes free' in str(err.value) and '204800000' in str(err.value)


def test_the_auto_ladder_on_three_free_memory_figures():
    n, v = 1000, 1
    f32, packed = n * ROW32 * 2, n * ROW16 * 2
    assert T.choose_act_store('auto', 'f16', n, v, f32) == 'f32'                     # fits as it is
    assert T.choose_act_store('auto', 'f16', n, v, f32 - 1) == 'packed'              # one byte short of float32
    assert T.choose_act_store('auto', 'f16', n, v, packed) == 'packed'
    assert T.choose_act_store('auto', 'bf16', n, v, packed - 1) == 'host'            # one byte short of packed
    assert T.choose_act_store('auto', 'f32', n, v, f32 - 1) == 'host'                # an f32 engine has no packed form
    assert T.choose_act_store('auto', 'f32', n, v, f32) == 'f32'
    assert T.choose_act_store('auto', 'f16', n, v, 0, host_free=packed) == 'host'
    with pytest.raises(ValueError, match='the host has'):
        T.choose_act_store('auto', 'f16', n, v, 0, host_free=packed - 1)
    for store in ('f32', 'packed', 'host'):                                          # a named store is itself, or refused
        assert T.choose_act_store(store, 'f16', n, v, f32) == store
    with pytest.raises(ValueError, match='--act-cache packed'):
        T.choose_act_store('f32', 'f16', n, v, f32 - 1)
    with pytest.raises(ValueError):
        T.choose_act_store('disk', 'f16', n, v, f32)


def test_packed_is_refused_for_an_f32_engine_without_a_device():
    with pytest.raises(ValueError) as err:
        T.choose_act_store('packed', 'f32', 10, 0, 1 << 40)
    assert 'lossless' in str(err.value) and 'f32 engine' in str(err.value)
    with pytest.raises(ValueError, match='lossless'):
        T.act_row_bytes('packed', 'f32')
    with pytest.raises(SystemExit, match='--act-cache'):         # the command line refuses before it reads a file or opens a device
        T.main(['x.tfrecords', '--labels', 'l.csv', '--model', 'm', '--out', 'o', '--dtype', 'f32', '--act-cache', 'packed'])


def _cache(acts, mul, views=False):
    n = acts.shape[0]
    feats = np.arange(n * 2048, dtype=np.float32).reshape(n, 2048)
    c = T.ActivationCache(feats, np.arange(n, dtype=np.int64) % 2, np.zeros((n, 2), np.int64), ['a', 'b'], acts=acts, act_mul=mul)
    if views:
        c.views, c.act_views, c.augment, c.augment_seed = np.stack([feats, feats + 1]), torch.stack([acts, acts]), 'xy', 3
    return c


def _raw(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


@pytest.mark.parametrize('dtype', (torch.float16, torch.bfloat16))
def test_save_and_load_keep_the_16_bit_form(tmp_path, dtype):
    rng = np.random.default_rng(4)
    a32 = torch.from_numpy(rng.standard_normal((3, 10, 10, 1024)).astype(np.float32))
    a16 = a32.to(dtype)
    a16[0, 0, 0, :4] = torch.tensor([65504.0 if dtype == torch.float16 else 65280.0, -0.0, 2.0 ** -24, float('inf')]).to(dtype)
    half, full = str(tmp_path / 'half.npz'), str(tmp_path / 'full.npz')
    _cache(a16, 0.125, views=True).save(half)
    _cache(a16.float() * 0.125, 1.0, views=True).save(full)
    back = T.ActivationCache.load(half)
    assert torch.is_tensor(back.acts) and back.acts.dtype == dtype and back.act_views.dtype == dtype and back.act_mul == 0.125
    assert np.array_equal(_raw(back.acts), _raw(a16)) and np.array_equal(_raw(back.act_views[1]), _raw(a16))
    assert (back.augment, back.augment_seed, back.n_views()) == ('xy', 3, 2) and np.array_equal(back.feats, _cache(a16, 1.0).feats)
    ratio = os.path.getsize(half) / os.path.getsize(full)
    print(f'{dtype}: the 16-bit file is {ratio:.3f} of the float32 one')
    assert 0.49 < ratio < 0.52                        # the activations halve; the features, 2 % of the file, do not
    with np.load(half) as z:
        assert str(z['act_type']) == ('f16' if dtype == torch.float16 else 'bf16') and float(z['act_mul']) == 0.125
        assert z['acts'].dtype == (np.float16 if dtype == torch.float16 else np.uint16)
    moved = T.ActivationCache.load(half).to('cpu')                                    # to() keeps the type
    assert moved.acts.dtype == dtype and np.array_equal(_raw(moved.acts), _raw(a16)) and moved.act_views.dtype == dtype
    # the float32 file is the format it always was: no new entry, and it loads as it did
    with np.load(full) as z:
        assert 'act_type' not in z.files and 'act_mul' not in z.files and z['acts'].dtype == np.float32
    old = T.ActivationCache.load(full)
    assert isinstance(old.acts, np.ndarray) and old.acts.dtype == np.float32 and old.act_mul == 1.0
    assert np.array_equal(old.acts.view(np.uint32), (a16.float() * 0.125).numpy().view(np.uint32))


def test_a_file_from_before_the_stores_still_loads(tmp_path):
    a = np.random.default_rng(5).standard_normal((2, 10, 10, 1024)).astype(np.float32)
    path = str(tmp_path / 'old.npz')
    np.savez(path, feats=np.ones((2, 2048), np.float32), acts=a, slide_idx=np.array([0, 1]), loc=np.zeros((2, 2), np.int64),
             slides=np.array(['a', 'b'], dtype=str))
    c = T.ActivationCache.load(path)
    assert isinstance(c.acts, np.ndarray) and np.array_equal(c.acts, a) and c.act_mul == 1.0 and c.act_views is None
    c.to('cpu')
    assert torch.is_tensor(c.acts) and c.acts.dtype == torch.float32


def test_command_line_parses_the_store():
    base = ['x.tfrecords', '--labels', 'l.csv', '--model', 'm', '--out', 'o']
    ap = T.arg_parser()
    assert ap.parse_args(base).act_cache == 'f32'
    for store in T.ACT_STORES:
        assert ap.parse_args(base + ['--trainable', 'exit', '--act-cache', store]).act_cache == store
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--act-cache', 'disk'])
