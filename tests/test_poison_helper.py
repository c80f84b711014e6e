"""tests/_poison.py on CPU tensors: the views it hands out, the guards around them, and the proxy that stands in for ``torch``."""
import types

import numpy as np
import pytest
import torch

from tests import _poison as P

WORDS = {('nan', 'f16'): 0xFFFF, ('nan', 'bf16'): 0xFFFF, ('nan', 'f32'): 0xFFFFFFFF, ('inf', 'f16'): 0x7C00, ('inf', 'bf16'): 0x7F80,
         ('inf', 'f32'): 0x7F800000, ('big', 'f16'): 0x7BFF, ('big', 'bf16'): 0x7F7F, ('big', 'f32'): 0x7F7FFFFF,
         ('zero', 'f16'): 0, ('zero', 'bf16'): 0, ('zero', 'f32'): 0}
DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}


@pytest.mark.parametrize('fill,storage', sorted(WORDS))
def test_network_fills_are_the_words_of_their_storage_type(fill, storage):
    k = 2 if storage != 'f32' else 4
    view, check = P.guarded(10 * k + 1, fill, 'cpu', storage)          # (one byte more than whole words)
    words = view[:10 * k].numpy().view('<u2' if k == 2 else '<u4')
    assert (words == WORDS[fill, storage]).all()
    assert int(view[-1]) == WORDS[fill, storage] & 0xFF                # the partial word: the pattern's first byte
    as_float = view[:10 * k].view(DTYPES[storage]).float()
    if fill == 'nan':
        assert torch.isnan(as_float).all() and (view[:10 * k].view(torch.int16) == -1).all()
    elif fill == 'inf':
        assert (as_float == float('inf')).all()
    elif fill == 'big':
        assert torch.isfinite(as_float).all() and (as_float == torch.finfo(DTYPES[storage]).max).all()
    else:
        assert (as_float == 0).all()
    assert P.holds(view, fill, storage) and P.pattern(fill, DTYPES[storage]) == P.pattern(fill, storage)
    view[3] ^= 1
    assert not P.holds(view, fill, storage)
    check()


def test_fills_of_other_types():
    assert P.BYTE_FILLS == (0x00, 0xFF, 0xA5)
    assert [P.pattern(b) for b in P.BYTE_FILLS] == [b'\x00', b'\xff', b'\xa5']
    assert P.pattern('nan', torch.int32) == b'\xff' and P.pattern('inf', torch.uint8) == b'\x7f'
    inf64 = P.guarded(16, 'inf', 'cpu', torch.float64)[0].view(torch.float64)
    assert (inf64 == float('inf')).all()
    with pytest.raises(ValueError):
        P.pattern('inf', 'f8')
    with pytest.raises(ValueError):
        P.pattern(256)
    with pytest.raises(KeyError):
        P.pattern('stale', 'f16')


@pytest.mark.parametrize('nbytes', [0, 1, 7, 4096, 299 * 299 * 3])
def test_guarded_view_is_exact_aligned_and_guarded(nbytes):
    view, check = P.guarded(nbytes, 0xFF, 'cpu')
    assert view.dtype == torch.uint8 and tuple(view.shape) == (nbytes,) and view.is_contiguous()
    base = P.allocation(view)
    assert base.numel() == nbytes + 2 * P.GUARD and P.GUARD == 4096 and P.GUARD % 512 == 0
    assert view.storage_offset() == P.GUARD                           # the view's address = the allocation's, modulo 512
    if nbytes:
        assert view.data_ptr() - base.data_ptr() == P.GUARD and view.data_ptr() % 512 == base.data_ptr() % 512
    assert (view == 0xFF).all()
    assert (base[:P.GUARD] == P.GUARD_BYTE).all() and (base[P.GUARD + nbytes:] == P.GUARD_BYTE).all() and P.GUARD_BYTE == 0xA5
    check()
    view.fill_(3)                                   # every byte of the view is the caller's
    check()


@pytest.mark.parametrize('where', ['front', 'back', 'far_front', 'far_back'])
def test_a_write_one_byte_outside_the_view_trips_check(where):
    n = 33
    view, check = P.guarded(n, 'nan', 'cpu', 'f16')
    base = P.allocation(view)
    at = {'front': P.GUARD - 1, 'back': P.GUARD + n, 'far_front': 0, 'far_back': n + 2 * P.GUARD - 1}[where]
    check()
    base[at] = 0
    with pytest.raises(AssertionError, match='in front of' if 'front' in where else 'behind'):
        check()
    base[at] = P.GUARD_BYTE
    check()


def test_poison_workspace_sets_exactly_the_bytes_the_library_asks_for():
    asked = []

    def workspace_bytes(ctx, n, mc_n):
        asked.append((ctx, n, mc_n))
        return 4096 + 1000 * n + 10 * mc_n + 2
    eng = types.SimpleNamespace(_lib=types.SimpleNamespace(bq_workspace_bytes=workspace_bytes), _ctx='ctx', device=torch.device('cpu'),
                                dtype='bf16', _ws=torch.zeros(5, dtype=torch.uint8))
    check = P.poison_workspace(eng, 3, 2, 'inf')
    assert asked == [('ctx', 3, 2)] and eng._ws.dtype == torch.uint8 and eng._ws.numel() == 4096 + 3000 + 20 + 2
    assert P.holds(eng._ws, 'inf', 'bf16') and (eng._ws.numpy().view('<u2') == 0x7F80).all()
    check()
    P.allocation(eng._ws)[P.GUARD + eng._ws.numel()] = 1
    with pytest.raises(AssertionError):
        check()


@pytest.mark.parametrize('fill', ['nan', 'inf', 0xA5])
def test_proxy_poisons_empty_and_empty_like_and_nothing_else(fill):
    proxy = P.poisoned_torch(fill)
    cases = [((4, 2), torch.float32), ((3, 5, 7), torch.uint8), ((6,), torch.int32), ((2, 3), torch.float16), ((2, 2), torch.bfloat16),
             ((5,), torch.float64), ((7,), torch.int64), ((0, 3), torch.float32)]
    made = []
    for shape, dtype in cases:
        t = proxy.empty(shape, dtype=dtype, device=torch.device('cpu'))
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == 'cpu' and t.is_contiguous()
        assert t.storage_offset() * t.element_size() == P.GUARD and P.allocation(t).numel() == t.numel() * t.element_size() + 2 * P.GUARD
        raw = t.reshape(-1).view(torch.uint8)
        assert P.holds(raw, fill, dtype)
        if fill == 'nan' and dtype.is_floating_point:
            assert torch.isnan(t).all()
        if fill == 'inf' and dtype.is_floating_point:
            assert (t == float('inf')).all()
        made.append(t)
    assert tuple(proxy.empty(2, 3, dtype=torch.int32, device='cpu').shape) == (2, 3)         # sizes as separate arguments
    assert proxy.empty(4, device='cpu').dtype == torch.get_default_dtype()
    like = proxy.empty_like(made[1])
    assert like.shape == made[1].shape and like.dtype == torch.uint8 and P.holds(like.reshape(-1), fill, torch.uint8)
    assert proxy.served == len(cases) + 3
    proxy.check()
    with pytest.raises(TypeError):
        proxy.empty((2,), dtype=torch.uint8, device='cpu', pin_memory=True)
    # everything else is torch's own
    assert proxy.zeros is torch.zeros and proxy.full is torch.full and proxy.uint8 is torch.uint8 and proxy.cuda is torch.cuda
    assert proxy.is_tensor(made[0]) and proxy.device('cpu') == torch.device('cpu')
    assert (proxy.zeros(3, dtype=torch.float32) == 0).all() and proxy.served == len(cases) + 3
    assert torch.empty is not proxy.empty and np.array_equal(torch.zeros(2).numpy(), [0, 0])   # nothing global was patched
    # a write behind one of the tensors it served: check() finds it
    flat = made[2]
    P.allocation(flat)[P.GUARD + flat.numel() * 4] = 0
    with pytest.raises(AssertionError, match='behind'):
        proxy.check()


def test_only_the_patched_module_sees_the_proxy(monkeypatch):
    import biscuit_amd.engine as engine_mod
    import biscuit_amd.inference as inference_mod
    proxy = P.poisoned_torch('nan')
    monkeypatch.setattr(engine_mod, 'torch', proxy)
    assert engine_mod.torch is proxy and inference_mod.torch is torch
    out = engine_mod.Engine._mean_std(types.SimpleNamespace(device=torch.device('cpu')), 3, None)
    assert proxy.served == 2 and all(torch.isnan(t).all() and tuple(t.shape) == (3, 2) for t in out)
    proxy.check()
    monkeypatch.undo()
    assert engine_mod.torch is torch
