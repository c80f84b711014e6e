"""The network at the batch sizes where its 32-bit byte offsets turn over ("Size limits of the routes").

Every fast route of the 16-bit network forms byte offsets into the activation tensors in 32 bits behind a size predicate; past
it ``choose_route`` hands the layer to a kernel that indexes with 64 bits.  The sizes are the smallest batches that reach each
condition, computed by tests/_batch_limits.py from ``TAPS``' shapes and the predicates' constants:

    dtype      n     what turns there
    f16, bf16  389   block 2's tensors (147 x 147 x 128) pass 2^31 bytes: STREAM x 2 and BLOCK_TAIL run with the sign bit set
    f16, bf16  776   the last batch STREAM / BLOCK_TAIL accept for block 2 (the dropped-store offset lies 2.2 MB behind the end)
    f16, bf16  777   block 2 on FUSED_GEMM + CONV_THEN_POOL; the front kernel's output passes 2^31 (block 3's did at 766)
    f16        1532  block 3 leaves STREAM / WIDE / BLOCK_TAIL; block 4's 37 x 37 x 736 tensors are past 2^31 since 1066
    f16        1553  past the front kernel: the uint8 entry stages the tiles and runs stem + TILE
    f32        195   147 x 147 x 128 x 4 B passes 2^31
    f32        389   ... and 2^32

A batch is six tiles (``make_slides(3, 2, seed=0)``) repeated, tiles 0 and 1 -- the two with oracle taps -- again at its far end,
which is where a wrapped or sign-extended offset lands.  No oracle runs at these sizes; the references are the oracle's n = 2 taps
and the engine's own small runs.  Per size: (1) every image's features equal, bit for bit, those of the first occurrence of its
tile, on both entries; (2) the features of both ends against the oracle; (3) layer by layer, at both ends, every tap whose tensor
or whose layer's input has reached 2^31 bytes or whose walk differs from the n = 2 walk -- against the oracle, and against the
engine's n = 2 tap bit for bit where the walks are the same; (4) ``mc_infer`` against ``mc_head`` in slices; (5) at 776 once more
on a NaN-filled, guarded workspace.  The bounds are those of ``test_every_layer_against_oracle``, imported.

Durations on the MI355X (``--durations=0`` of the whole suite, call phase; the first test of a storage type also runs that type's
oracle on two tiles; the slowest test of tests/test_gpu_parity.py in the same run took 9.09 s):

    f16   389: 0.31 s   776: 0.32 s   777: 0.79 s   1532: 2.55 s   1553: 2.21 s
    bf16  389: 0.22 s   776: 0.29 s   777: 0.71 s
    f32   195: 6.22 s   389: 0.49 s

Peak device memory of the n = 1553 test (``torch.cuda.max_memory_allocated``): 44.1 GiB -- the 29 GB workspace, a 17 GB fp32 tap.
"""
import numpy as np
import pytest
import torch

from tests import _batch_limits as B
from tests import _poison as P
from tests.test_gpu_parity import (FEAT_MAXABS_ULPS, TAPS, ULP, dev, layer_maxabs_ulps, layer_refs, layer_rms_ulps,  # noqa: F401
                                   oracles, tiles, weights)
from tests.test_gpu_schedule import SCHEDULE_16, SCHEDULE_16_N777, SCHEDULE_16_N1532, SCHEDULE_16_N1553, SCHEDULE_32

pytestmark = pytest.mark.gpu

SIZES = B.sizes()
MAX_BATCH = SIZES['16_front_falls']
K_ACT_PAD = 4096                     # csrc/biscuit_hip.hip, ws_layout: the pad in front of the first activation buffer
SHAPES = dict(TAPS)
TAP_INDEX = {name: k for k, (name, _) in enumerate(TAPS)}


@pytest.fixture(scope='module')
def engine_of(weights):
    """``engine_of(dtype)``: one engine per storage type with room for the largest batch, one at a time -- the one before is closed
    and its memory handed back before the next is made."""
    from biscuit_amd.engine import Engine
    held = {}

    def get(dtype):
        if dtype not in held:
            for e in held.values():
                e.close()
            held.clear()
            torch.cuda.empty_cache()
            held[dtype] = Engine(weights, dtype=dtype, max_batch=MAX_BATCH, max_mc=2)
        return held[dtype]
    yield get
    for e in held.values():
        e.close()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def eng(request, engine_of):
    """The engine of the storage type a test names (``parametrize('eng', [...], indirect=True)``): module-scoped, so that pytest runs
    the tests of one type together."""
    return engine_of(request.param)


@pytest.fixture(scope='module')
def d6(tiles):
    return dev(tiles)


def turned(a, b):
    """The steps two schedules differ in: names with another route, or in one walk only."""
    a, b = dict(a), dict(b)
    return {name for name in set(a) | set(b) if a.get(name) != b.get(name)}


def against_oracle(dtype, name, got, ref, where):
    """``got`` (two images of tap ``name``, on the host) within the bounds of ``test_every_layer_against_oracle``."""
    k = TAP_INDEX[name]
    d = np.abs(got - ref)
    assert not np.isnan(got).any(), (name, where)
    if dtype == 'f32':
        print(f'{dtype} {name} {where}: max|d| {d.max():.2e}')
        assert d.max() < 2e-4, (name, where, d.max())
        return
    ulp = ULP[dtype] * np.abs(ref).max()
    rms = np.sqrt((d ** 2).mean()) / np.sqrt((ref ** 2).mean())
    print(f'{dtype} {name} {where}: max|d| {d.max() / ulp:.2f} ulps (bound {layer_maxabs_ulps(k)}), rel. rms {rms / ULP[dtype]:.3f} ulps '
          f'(bound {layer_rms_ulps(k):.2f})')
    assert d.max() < layer_maxabs_ulps(k) * ulp, (name, where, d.max() / ulp, layer_maxabs_ulps(k))
    assert rms < layer_rms_ulps(k) * ULP[dtype], (name, where, rms / ULP[dtype], layer_rms_ulps(k))


def run_size(eng, dtype, n, d6, layer_refs, must_tap=(), poisoned=False):
    """Checks 1-4 (and 5) of the module's docstring on a batch of ``n``; ``must_tap``: taps check 3 has to have found."""
    u8 = dtype != 'f32'                                    # the fp32 context has no uint8 taps: its entry stages the tiles
    idx = torch.tensor(B.batch_index(n), device='cuda')
    batch = d6[idx]
    assert batch.shape[0] == n and batch.is_contiguous()
    ref_taps, feat_ref = layer_refs(dtype)
    fr = feat_ref.numpy()
    feat_tol = 1e-4 if dtype == 'f32' else FEAT_MAXABS_ULPS * ULP[dtype] * np.abs(fr).max()

    # 1, 2: position independence over the whole batch, bit for bit; both ends against the oracle
    staged = eng.stage(batch)
    entries = [('backbone(stage)', eng.backbone(staged))]
    if u8:
        entries.insert(0, ('backbone_u8', eng.backbone_u8(batch)))
    for label, feat in entries:
        first = feat[:6][idx]
        wrong = (feat != first).any(dim=1).nonzero().flatten()
        assert wrong.numel() == 0, (label, n, 'images that differ from the first occurrence of their tile', wrong[:16].tolist(), int(wrong.numel()))
        assert torch.equal(feat, first), (label, n)
        for where, two in (('first two', feat[:2]), ('last two', feat[-2:])):
            dmax = float(np.abs(two.cpu().numpy() - fr).max())
            print(f'{dtype} n={n} {label} features, {where}: max|d| {dmax:.3e} (bound {feat_tol:.3e})')
            assert dmax < feat_tol, (label, where, dmax, feat_tol)
        small = eng.schedule(6, u8=u8 and label == 'backbone_u8')
        if eng.schedule(n, u8=u8 and label == 'backbone_u8') == small:      # the same kernels: the same bits as the six tiles alone
            alone = eng.backbone_u8(d6) if label == 'backbone_u8' else eng.backbone(eng.stage(d6))
            assert torch.equal(feat[:6], alone), (label, n)
    feat = entries[0][1]

    # 3: layer by layer where it matters
    two_u8 = d6[:2].contiguous()
    two_staged = eng.stage(two_u8)
    reaching = set(B.taps_reaching(n, dtype))
    checked = []
    for name, _ in TAPS:
        from_u8 = u8 and name not in ('staged', 'block1_conv1')      # (the uint8 entry materialises neither: the float entry's tap)
        tap_of = (lambda name, src: eng.debug_activation_u8(name, src, SHAPES[name])) if from_u8 else \
                 (lambda name, src: eng.debug_activation(name, src, SHAPES[name]))
        src_n, src_2 = (batch, two_u8) if from_u8 else (staged, two_staged)
        same_walk = eng.schedule(n, u8=from_u8, tap=name) == eng.schedule(2, u8=from_u8, tap=name)
        if name not in reaching and same_walk:
            continue
        got = tap_of(name, src_n)
        four = torch.cat([got[:2], got[-2:]]).cpu()        # (the tap itself is up to 17 GB: it stays on the device)
        del got
        ref = ref_taps[name].permute(0, 2, 3, 1).numpy()
        against_oracle(dtype, name, four[:2].numpy(), ref, f'n={n} first two')
        against_oracle(dtype, name, four[2:].numpy(), ref, f'n={n} last two')
        if same_walk:
            two = tap_of(name, src_2).cpu()
            assert torch.equal(four[:2], two) and torch.equal(four[2:], two), (name, n, 'differs from the n = 2 tap')
        checked.append(name)
    print(f'{dtype} n={n} taps checked: {checked}')
    assert set(must_tap) <= set(checked), (must_tap, checked)

    # 4: the whole entry once, against the head on the features in slices of 256 rows
    mean, std = eng.mc_infer(batch, 2, 1234, tile_idx0=0)
    for k in range(0, n, 256):
        m, s = eng.mc_head(feat[k:k + 256], 2, 1234, tile_idx0=k)
        assert torch.equal(mean[k:k + 256], m) and torch.equal(std[k:k + 256], s), (n, k)

    # 5: once more on memory holding NaN, between guards (tests/test_gpu_poison.py, poisoned_call)
    if poisoned:
        import biscuit_amd.engine as engine_mod
        try:
            check_ws = P.poison_workspace(eng, n, 1, 'nan')
            at = eng._ws.data_ptr()
            proxy = P.poisoned_torch('nan')
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(engine_mod, 'torch', proxy)
                again = eng.backbone_u8(batch)
            assert eng._ws.data_ptr() == at, 'the engine replaced the poisoned workspace'
            assert P.holds(eng._ws[:K_ACT_PAD], 'nan', eng.dtype), 'the pad in front of the first activation buffer was written'
            assert proxy.served >= 1
            check_ws()
            proxy.check()
            assert torch.equal(again, feat), 'the features depend on what the workspace held'
        finally:
            eng._ws = None


BLOCK2 = {'block2_sepconv1', 'block2_sepconv2', 'block2_out'}
BLOCK3 = {'block3_sepconv1', 'block3_sepconv2', 'block3_out'}


@pytest.mark.parametrize('eng', ['f16', 'bf16'], indirect=True)
def test_16_bit_block2_passes_2_to_the_31(eng, d6, layer_refs):
    dtype, n = eng.dtype, SIZES['16_block2_sign']
    assert n == 389
    assert eng.schedule(n) == eng.schedule(n - 1) == SCHEDULE_16          # no route turns: the same kernels with the sign bit set
    run_size(eng, dtype, n, d6, layer_refs, must_tap=BLOCK2)             # (block2_out is the tap that runs the tail)


@pytest.mark.parametrize('eng', ['f16', 'bf16'], indirect=True)
def test_16_bit_last_batch_of_block2_on_the_streaming_kernels(eng, d6, layer_refs):
    dtype, n = eng.dtype, SIZES['16_block2_last']
    assert n == 776
    assert eng.schedule(n) == eng.schedule(n - 1) == SCHEDULE_16
    assert turned(eng.schedule(n), eng.schedule(n + 1)) == BLOCK2
    run_size(eng, dtype, n, d6, layer_refs, must_tap=BLOCK2, poisoned=True)


@pytest.mark.parametrize('eng', ['f16', 'bf16'], indirect=True)
def test_16_bit_block2_on_the_fallback(eng, d6, layer_refs):
    dtype, n = eng.dtype, SIZES['16_block2_falls']
    assert n == 777
    assert eng.schedule(n) == SCHEDULE_16_N777
    assert turned(eng.schedule(n), eng.schedule(n - 1)) == BLOCK2
    run_size(eng, dtype, n, d6, layer_refs, must_tap=BLOCK2 | {'block1_conv2', 'block2_res'} | BLOCK3)


@pytest.mark.parametrize('eng', ['f16'], indirect=True)
def test_f16_block3_on_the_fallback(eng, d6, layer_refs):
    n = SIZES['16_block3_falls']
    assert n == 1532
    assert eng.schedule(n) == SCHEDULE_16_N1532
    assert turned(eng.schedule(n), eng.schedule(n - 1)) == BLOCK3
    # block3_sepconv2 under its tap is WIDE up to the same batch
    assert eng.schedule(n - 1, tap='block3_sepconv2')[-1] == ('block3_sepconv2', 'WIDE')
    assert eng.schedule(n, tap='block3_sepconv2')[-1] == ('block3_sepconv2', 'FUSED_GEMM nsplit=1')
    run_size(eng, 'f16', n, d6, layer_refs, must_tap=BLOCK2 | BLOCK3 | {'block4_sepconv1', 'block4_sepconv2', 'block4_out'})


@pytest.mark.parametrize('eng', ['f16'], indirect=True)
def test_f16_past_the_front_kernel(eng, d6, layer_refs):
    n = SIZES['16_front_falls']
    assert n == 1553 == MAX_BATCH
    assert eng.schedule(n - 1) == SCHEDULE_16_N1532 and eng.schedule(n) == SCHEDULE_16_N1553
    assert turned(eng.schedule(n), eng.schedule(n - 1)) == {'block1_conv2'}
    assert eng.schedule(n) == eng.schedule(n, u8=False)                   # the uint8 entry has become the float entry
    torch.cuda.reset_peak_memory_stats()
    run_size(eng, 'f16', n, d6, layer_refs, must_tap=BLOCK2 | BLOCK3 | {'block1_conv2', 'block4_out'})
    print(f'peak device memory of the n = {n} run: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB')


@pytest.mark.parametrize('eng', ['f32'], indirect=True)
def test_f32_block2_passes_2_to_the_31(eng, d6, layer_refs):
    n = SIZES['32_block2_sign']
    assert n == 195
    assert eng.schedule(n) == eng.schedule(n - 1) == SCHEDULE_32
    run_size(eng, 'f32', n, d6, layer_refs, must_tap=BLOCK2)


@pytest.mark.parametrize('eng', ['f32'], indirect=True)
def test_f32_block2_passes_2_to_the_32(eng, d6, layer_refs):
    n = SIZES['32_block2_wrap']
    assert n == 389
    assert eng.schedule(n) == eng.schedule(n - 1) == SCHEDULE_32
    run_size(eng, 'f32', n, d6, layer_refs, must_tap=BLOCK2 | BLOCK3 | {'block1_conv2', 'block2_res'})
