"""Memory whose contents are unspecified on entry, made so on purpose (DESIGN.md "Buffer contract"): poisoned, guarded buffers for
the tests that hold the kernels to "no result depends on stale bytes" -- tests/test_gpu_poison.py (the network and the tools) and
the poisoned parity test of tests/test_gpu_parity.py.  Pure torch, so tests/test_poison_helper.py checks it on CPU tensors.

A buffer is a uint8 view of exactly the bytes asked for inside a larger allocation: ``GUARD`` bytes of ``GUARD_BYTE`` on each side
(a write outside the view trips ``check()``; a read outside it stays inside the allocation), the view itself filled with a poison.
"""
import struct

import numpy as np
import torch

GUARD = 4096            # a multiple of 512: the view keeps the alignment torch.empty gives
GUARD_BYTE = 0xA5

# The network's fills, little-endian words by storage type.  'nan' is every byte 0xFF: a NaN in all three float types and -1 in
# every integer type; 'inf' is +Inf (a max-pool or a ReLU swallows a NaN -- fmaxf(NaN, x) = x -- but not +Inf); 'big' is the
# largest finite value, which wins a max without being Inf.
FILLS = {
    'zero': {'f16': b'\x00\x00', 'bf16': b'\x00\x00', 'f32': b'\x00\x00\x00\x00', 'f64': b'\x00' * 8, 'int': b'\x00'},
    'nan': {'f16': b'\xff\xff', 'bf16': b'\xff\xff', 'f32': b'\xff\xff\xff\xff', 'f64': b'\xff' * 8, 'int': b'\xff'},
    'inf': {'f16': struct.pack('<H', 0x7C00), 'bf16': struct.pack('<H', 0x7F80), 'f32': struct.pack('<I', 0x7F800000),
            'f64': struct.pack('<Q', 0x7FF0000000000000), 'int': b'\x7f'},
    'big': {'f16': struct.pack('<H', 0x7BFF), 'bf16': struct.pack('<H', 0x7F7F), 'f32': struct.pack('<I', 0x7F7FFFFF),
            'f64': struct.pack('<Q', 0x7FEFFFFFFFFFFFFF), 'int': b'\x7f'},
}
# The byte and integer tools' fills: one byte everywhere, whatever the type of the tensor.
BYTE_FILLS = (0x00, 0xFF, 0xA5)

_STORAGE = {torch.float16: 'f16', torch.bfloat16: 'bf16', torch.float32: 'f32', torch.float64: 'f64'}
_WORD = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def pattern(fill, storage=None):
    """The bytes a fill repeats: ``fill`` an int (that byte) or a name of ``FILLS``; ``storage`` 'f16' / 'bf16' / 'f32' or a torch
    dtype (an integer dtype takes the fill's 'int' byte)."""
    if isinstance(fill, int):
        if not 0 <= fill <= 255:
            raise ValueError(f'a byte fill lies in 0 .. 255, not {fill}')
        return bytes([fill])
    by_type = FILLS[fill]
    if isinstance(storage, torch.dtype):
        storage = _STORAGE.get(storage, 'int')
    if storage not in by_type:
        raise ValueError(f'fill {fill!r} needs a storage type of {sorted(by_type)}, not {storage!r}')
    return by_type[storage]


def fill_bytes(view, pat):
    """``view`` (uint8, 1-D, contiguous, its first byte aligned to len(pat)) := ``pat`` repeated; a last partial word gets the
    pattern's first bytes."""
    assert view.dtype == torch.uint8 and view.dim() == 1 and view.is_contiguous()
    k, n = len(pat), view.numel()
    if k == 1 or len(set(pat)) == 1:
        view.fill_(pat[0])
        return
    m = n // k * k
    if m:
        word = int(np.frombuffer(pat, {2: '<i2', 4: '<i4', 8: '<i8'}[k])[0])
        view[:m].view(_WORD[k]).fill_(word)
    if n > m:
        view[m:] = torch.tensor(list(pat[:n - m]), dtype=torch.uint8).to(view.device)


def holds(view, fill, storage=None):
    """Does ``view`` (uint8, 1-D) still hold the fill, byte for byte?"""
    want = torch.empty_like(view)
    fill_bytes(want, pattern(fill, storage))
    return torch.equal(view, want)


def allocation(t):
    """The whole allocation a tensor lives in, guards included, as uint8 (for the tests of this helper)."""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def guarded(nbytes, fill, device, storage=None):
    """``(view, check)``: a uint8 view of exactly ``nbytes`` bytes filled with ``fill`` (``pattern(fill, storage)``) between two
    guards of ``GUARD`` bytes of ``GUARD_BYTE``; ``check()`` asserts that both guards are intact."""
    nbytes = int(nbytes)
    assert nbytes >= 0
    base = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
    base[:GUARD] = GUARD_BYTE
    base[GUARD + nbytes:] = GUARD_BYTE
    view = base[GUARD:GUARD + nbytes]
    fill_bytes(view, pattern(fill, storage))

    def check():
        front, back = base[:GUARD] != GUARD_BYTE, base[GUARD + nbytes:] != GUARD_BYTE
        assert not bool(front.any()), f'{int(front.sum())} bytes written in front of a {nbytes}-byte buffer'
        assert not bool(back.any()), f'{int(back.sum())} bytes written behind a {nbytes}-byte buffer'
    return view, check


def poison_workspace(eng, n, mc_n, fill):
    """``eng._ws`` := a guarded view of exactly ``bq_workspace_bytes(n, mc_n)`` bytes holding ``fill`` in the engine's storage type,
    so that ``Engine._ws_for(n, mc_n)`` hands it to the next call as it is.  Returns its ``check()``."""
    need = int(eng._lib.bq_workspace_bytes(eng._ctx, int(n), int(mc_n)))
    eng._ws = None
    eng._ws, check = guarded(need, fill, eng.device, eng.dtype)
    return check


class PoisonedTorch:
    """Stands where a module says ``torch``: every attribute is torch's own except ``empty`` and ``empty_like``, which return
    poisoned, guarded tensors of the requested shape, dtype and device.  ``served`` counts them, ``check()`` asserts every guard."""

    def __init__(self, fill):
        self.fill = fill
        self.served = 0
        self._checks = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **other):
        if other:
            raise TypeError(f'poisoned torch.empty: unsupported arguments {sorted(other)}')
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        shape = tuple(int(s) for s in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
        view, check = guarded(numel * torch.empty(0, dtype=dtype).element_size(), self.fill, device, dtype)
        self.served += 1
        self._checks.append(check)
        return view.view(dtype).view(shape)

    def empty_like(self, t, **other):
        if other:
            raise TypeError(f'poisoned torch.empty_like: unsupported arguments {sorted(other)}')
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def check(self):
        for c in self._checks:
            c()


def poisoned_torch(fill):
    """The proxy for ``monkeypatch.setattr(biscuit_amd.engine, 'torch', poisoned_torch(fill))``: only that module sees it."""
    return PoisonedTorch(fill)
