"""No result of the network may depend on bytes it did not write (DESIGN.md "Buffer contract").  The workspace, every scratch buffer
and every output tensor are unspecified on entry; here they ARE: filled with NaN, +Inf or the largest finite value of the
context's storage type in front of every call, inside guarded allocations (tests/_poison.py), and every result has to equal the
one computed on zeroed memory bit for bit.  The kernels read -- and mask -- pixels next to the tensors they walk, contract over pad
channels that are zero only because a producer wrote them, and fetch aligned dwords around unaligned tiles: a load moved one row
too far or a pad lane that is no longer written passes every parity test on a fresh (zero) or a reused (finite, same layout)
workspace and fails here.  Run on the MI355X with ``-m gpu``.

Engines: f16, bf16, f32 and the two last-resort 16-bit engines (a blob without the "wp16" / "w16" copies), on the stress weights --
together every route ``choose_route`` can return; the debug taps bring in the routes only a tap selects.  Batches of 1 (both ends of
every activation buffer border a pad) and 3 (image boundaries, an odd count), grids sized for the whole device and for 8 compute
units (a workgroup of the persistent kernels then walks several tiles, and the last one has no next tile)."""
import numpy as np
import pytest
import torch

from biscuit_amd.synthetic import make_tiles
from biscuit_amd.weights import synthetic_weights
from test_gpu_parity import TAPS, _without_16x16_copies
from tests import _poison as P
from tests import _range_ref as R

pytestmark = pytest.mark.gpu

ENGINES = ('f16', 'bf16', 'f32', 'f16-last', 'bf16-last')       # '-last': the last-resort kernels only
POISONS = ('nan', 'inf', 'big')
BATCHES = (1, 3)
GRIDS = (0, 8)
MC = (1, 3)
SEED = 1234
K_ACT_PAD = 4096            # biscuit_hip.hip ws_layout: the workspace's first bytes, which no kernel writes
BLOCK13 = [('block13_res', (10, 10, 1024)), ('block13_sepconv1', (19, 19, 728)), ('block13_sepconv2', (19, 19, 1024))]
NB = 299 * 299 * 3


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope='module')
def engine_of():
    """``engine_of(key)`` -> (engine, has the fused front kernel), built on first use: stress weights, max_batch 4, max_mc 3."""
    import biscuit_amd.engine as engine_mod
    weights = synthetic_weights(1, hard=True)
    made = {}

    def get(key):
        if key not in made:
            dtype, _, last = key.partition('-')
            with pytest.MonkeyPatch.context() as mp:
                if last:
                    real = engine_mod.pack_blob
                    mp.setattr(engine_mod, 'pack_blob', lambda *a, **k: _without_16x16_copies(real(*a, **k)))
                made[key] = engine_mod.Engine(weights, dtype=dtype, max_batch=4, max_mc=3)
        return made[key], key in ('f16', 'bf16')
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope='module')
def tiles():
    return dev(make_tiles(3, seed=57))


def poisoned_call(eng, n, mc_n, fill, fn):
    """``fn()`` on a freshly poisoned, guarded workspace of exactly ``bq_workspace_bytes(n, mc_n)`` bytes, with every tensor the
    engine allocates poisoned and guarded too.  Asserts that the call used that workspace, left its first pad alone, allocated its
    outputs through the proxy and wrote outside none of them."""
    import biscuit_amd.engine as engine_mod
    check_ws = P.poison_workspace(eng, n, mc_n, fill)
    at = eng._ws.data_ptr()
    proxy = P.poisoned_torch(fill)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine_mod, 'torch', proxy)
        out = fn()
    assert eng._ws.data_ptr() == at, 'the engine replaced the poisoned workspace'
    assert P.holds(eng._ws[:K_ACT_PAD], fill, eng.dtype), 'the pad in front of the first activation buffer was written'
    assert proxy.served >= 1
    check_ws()
    proxy.check()
    return out


def network_calls(eng, front, t):
    """(label, mc_n of the workspace, call) of everything the matrix runs on the tiles ``t``."""
    calls = [('backbone_u8', 1, lambda: eng.backbone_u8(t)),
             ('backbone(stage)', 1, lambda: eng.backbone(eng.stage(t)))]
    for mode in ('head', 'full'):
        for mc in MC:
            calls.append((f'mc_infer {mode} {mc}', mc, lambda mode=mode, mc=mc: eng.mc_infer(t, mc, SEED, tile_idx0=7, mc_mode=mode)))
    calls.append(('mc_head 3', 3, lambda: eng.mc_head(eng.backbone_u8(t), 3, SEED, tile_idx0=7)))
    for name, shp in TAPS + BLOCK13:
        if front and name not in ('staged', 'block1_conv1'):
            calls.append((f'tap_u8 {name}', 1, lambda name=name, shp=shp: eng.debug_activation_u8(name, t, shp)))
        else:       # the fused front kernel materialises neither; a context without it has no uint8 tap
            calls.append((f'tap {name}', 1, lambda name=name, shp=shp: eng.debug_activation(name, eng.stage(t), shp)))
    return calls


def run_matrix(eng, front, tiles, fill, grids):
    """{(n, label): [result per grid size]}: every call on a workspace and outputs holding ``fill``."""
    out = {}
    try:
        for n in BATCHES:
            t = tiles[:n].contiguous()
            for cus in grids:
                eng.set_num_cus(cus)
                for label, mc, fn in network_calls(eng, front, t):
                    out.setdefault((n, label), []).append(poisoned_call(eng, n, mc, fill, fn))
    finally:
        eng.set_num_cus(0)
    return out


@pytest.fixture(scope='module')
def on_zeros(engine_of, tiles):
    """``on_zeros(key)``: the matrix of that engine on ZEROED memory with the grid of the whole device, computed once and kept on
    the device -- what every poisoned run has to reproduce."""
    cache = {}

    def get(key):
        if key not in cache:
            eng, front = engine_of(key)
            cache[key] = {k: v[0] for k, v in run_matrix(eng, front, tiles, 'zero', (0,)).items()}
        return cache[key]
    return get


def same(a, b):
    if torch.is_tensor(a):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def finite(a):
    return bool(torch.isfinite(a).all()) if torch.is_tensor(a) else all(finite(x) for x in a)


@pytest.mark.parametrize('fill', POISONS)
@pytest.mark.parametrize('key', ENGINES)
def test_no_result_depends_on_stale_bytes(engine_of, on_zeros, tiles, key, fill):
    """Every network call -- features from uint8 and from staged tiles, ``mc_infer`` in both modes at MC 1 and 3, the head alone,
    every debug tap -- at batch 1 and 3, with the persistent grids sized for the device and for 8 compute units, on a workspace
    and output tensors full of ``fill``: bit for bit the results on zeroed memory (no tolerance: the kernels are deterministic),
    every guard intact, and nothing non-finite in any result."""
    eng, front = engine_of(key)
    want = on_zeros(key)
    got = run_matrix(eng, front, tiles, fill, GRIDS)
    assert set(got) == set(want) and len(want) == len(BATCHES) * (2 + 2 * len(MC) + 1 + len(TAPS) + len(BLOCK13))
    differ = [(n, label, cus) for (n, label), per_grid in got.items() for cus, r in zip(GRIDS, per_grid) if not same(r, want[n, label])]
    assert not differ, f'{key} under {fill}: {len(differ)} results differ from those on zeroed memory, first {differ[:6]}'
    assert all(finite(r) for r in want.values())


# ---------------------------------------------------------------------------------------------- pad channels
# The 728-channel tensors are stored 736 wide and the matrix kernels contract over all 736.  Whatever a walk does, the region a
# 19 x 19 or 37 x 37 tensor occupies was written before by a larger tensor of the same call (block 2's output, the 147 x 147 maps):
# a producer that skips the pad lanes leaves FINITE stale activations there, which zero weights still cancel -- no result moves, on
# any memory.  So the pad lanes are read where they lie: in the workspace, behind the tap that stops the walk at their tensor.
PADDED_TAPS = [('block4_sepconv1', 37), ('block4_sepconv2', 37), ('block4_res', 19), ('block4_out', 19), ('block5_sepconv1', 19),
               ('block5_sepconv2', 19), ('block5_out', 19), ('block8_sepconv2', 19), ('block12_out', 19), ('block13_sepconv1', 19)]


def activation_buffers(n, es):
    """(byte offset, bytes) of the four activation buffers of a workspace for ``n`` tiles of ``es``-byte elements (biscuit_hip.hip
    ws_layout)."""
    buffers, off = [], K_ACT_PAD
    for elems in (147 * 147 * 128,) * 3 + (74 * 74 * 128,):
        buffers.append((off, n * elems * es))
        off += (n * elems * es + K_ACT_PAD + 255) // 256 * 256
    return buffers


@pytest.mark.parametrize('key', ENGINES)
def test_pad_channels_of_the_736_wide_tensors_are_zero(engine_of, tiles, key):
    """Every tensor of 728 channels, where the tap that asks for it leaves it in the workspace (found by its contents: the buffer
    whose first 728 of every 736 channels are the tap's output), has zeros in channels 728 .. 735, on a workspace that held NaN
    or +Inf: each producer -- the wide kernel's epilogue, the tiled GEMM's plain and pooling store passes, the fallback GEMM, the
    pool-and-add kernel -- writes its pad lanes, none inherits them."""
    eng, front = engine_of(key)
    es = 4 if eng.dtype == 'f32' else 2
    for fill in ('nan', 'inf'):
        for n in BATCHES:
            t = tiles[:n].contiguous()
            src = t if front else eng.stage(t)
            for name, hw in PADDED_TAPS:
                tap = eng.debug_activation_u8 if front else eng.debug_activation
                out = poisoned_call(eng, n, 1, fill, lambda: tap(name, src, (hw, hw, 728)))
                rows = n * hw * hw
                found = []
                for off, size in activation_buffers(n, es):
                    if rows * 736 * es > size:
                        continue
                    stored = eng._ws[off:off + rows * 736 * es].view(eng._elt).view(rows, 736)
                    if torch.equal(stored[:, :728].float(), out.view(rows, 728)):
                        found.append(stored[:, 728:])
                assert found, f'{name}: the tapped tensor is in none of the activation buffers (has ws_layout changed?)'
                dirty = [int((p != 0).sum()) for p in found]
                assert not any(dirty), f'{key} {fill} n={n} {name}: {dirty} non-zero pad channel values'


# ---------------------------------------------------------------------------------------------- input neighbours
def tiles_inside_ff(t, off, tail):
    """The tiles ``t`` (numpy uint8 [n,299,299,3]) as a view at byte offset ``off`` of a buffer of 0xFF bytes that goes on for
    ``tail`` bytes behind the last tile (0: the last tile ends the allocation)."""
    n = len(t)
    buf = torch.full((off + n * NB + tail,), 0xFF, dtype=torch.uint8, device='cuda')
    view = buf[off:off + n * NB].view(n, 299, 299, 3)
    view.copy_(dev(t))
    assert view.is_contiguous() and view.data_ptr() % 4 == (buf.data_ptr() + off) % 4
    return view


@pytest.fixture(scope='module')
def dim_tiles():
    """Three tiles whose bytes stay inside 40 .. 167: a neighbour's 0xFF moves a sum, a sum of squares AND the maximum."""
    return (make_tiles(3, seed=58) // 2 + 40).astype(np.uint8)


@pytest.mark.parametrize('at_end', [False, True], ids=['inside', 'at_end'])
@pytest.mark.parametrize('key', ['f16', 'bf16', 'f32'])
def test_input_neighbours_change_nothing(engine_of, dim_tiles, key, at_end):
    """The entry points that take uint8 tiles at any byte offset fetch aligned dwords around them.  Tiles as views at byte offsets
    0 .. 3 inside a buffer of 0xFF -- the byte in front of the first tile and the 1 .. 4 behind the last (the rest of its last
    dword and the next one) are 0xFF, or the last tile ends the allocation --: ``stage`` equals the oracle's standardisation
    exactly, ``range_key`` the float64 statement, and features, ``mc_infer`` and the screen's slots equal those of an aligned
    clone bit for bit."""
    from biscuit_amd.engine import RangeScreen
    from oracle.xception_ref import standardize
    eng, _ = engine_of(key)
    ref = standardize(dim_tiles)
    if key != 'f32':
        ref = ref.to(torch.bfloat16 if key == 'bf16' else torch.float16).float()
    key_ref = R.range_key(dim_tiles)
    ends = set()
    for off in (0, 1, 2, 3):
        view = tiles_inside_ff(dim_tiles, off, 0 if at_end else 1 + (off + 1) % 4)
        ends.add((view.data_ptr() + view.numel()) % 4)
        clone = view.clone()
        assert clone.data_ptr() % 4 == 0 and view.data_ptr() % 4 == off
        assert torch.equal(eng.stage(view).float().cpu(), ref), off
        assert np.array_equal(eng.range_key(view).cpu().numpy().view(np.uint32), key_ref.view(np.uint32)), off
        assert torch.equal(eng.backbone_u8(view), eng.backbone_u8(clone)), off
        assert same(eng.mc_infer(view, 3, SEED), eng.mc_infer(clone, 3, SEED)), off
        a, b = RangeScreen(eng, k=2, max_batch=4), RangeScreen(eng, k=2, max_batch=4)
        a.update(view, tile_idx0=5)
        b.update(clone, tile_idx0=5)
        assert a.filled == b.filled == 2 and same(a.candidates(), b.candidates()) and torch.equal(a.tiles, b.tiles), off
        top = np.argsort(-key_ref.astype(np.float64), kind='stable')[:2]
        assert sorted(a.idx.cpu().tolist()) == sorted(int(5 + i) for i in top)
    assert ends == {0, 1, 2, 3}
