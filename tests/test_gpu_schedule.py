"""The launch schedule -- which kernel family runs each of Xception's 39 matrix layers -- as ``Engine.schedule`` reports it from
the decision function the launches themselves go through (``choose_route`` in csrc/biscuit_hip.hip).

The expected routes were written from a ``rocprofv3 --kernel-trace`` of the commit BEFORE the dispatcher was split into decision
and launch (batch 256, ``synthetic_weights(1, hard=True)``), kernel names and call counts per dtype, not from this code's output:

* f16 / bf16 from uint8 tiles: front_stream_kernel; sepconv_stream_kernel<64,128> and <128,256,relu> (block2_sepconv1 and
  block3_sepconv1: the streaming kernel, not the wide kernel's 74 x 74 instance); block_tail_stream_kernel and
  block_tail_coop_kernel (blocks 2 and 3); sepconv_wide_kernel 1 + 1 (block 4, 37 x 37), 9 + 8 + 8 (19 x 19: ReLU-in, plain,
  residual) and 2 launches of the 736 -> 512-column instance (block13_sepconv2); gemm_tile_kernel<.., s2, EPI_POOL> twice (blocks
  4 and 13); dw3x3_kernel twice with exit_gemm_kernel<gap = false> and <gap = true> (block 14); no gap_kernel.
* float entry: stem1_kernel and tile_conv_kernel<32, ...> in place of the front kernel, everything else the same.
* taps (uint8 entry): block2_res -> sepconv_stream_kernel<128,128> and gemm_fused_kernel in place of the block-2 tail;
  block3_sepconv2 -> the wide kernel's Geo<74, 2, 256, 256> instance in place of the block-3 tail; block13_res ->
  gemm_tile_kernel<.., s2, no epilogue> in place of the pooled one; block14_sepconv2 -> exit_gemm_kernel<gap = false> twice.
* f32: 40 gemm_fused_kernel launches for the 39 layers (block14_sepconv2, K = 1536, is split in two), four pool_add_kernel, one
  gap_kernel.

A route that needs a batch beyond the 32-bit offset limits (n > 776 at 147 x 147 x 128 in 16 bits) was not observed in that trace
(tests/test_gpu_batch_limits.py runs those batches).  Its DECISION is asserted (``test_16_bit_schedule_beyond_the_32_bit_limits``): the lists are those of the commit that still had the
TILE kinds 1-3, RESPOOL and PIPE routes for n = 777 and n = 1532, read off its ``choose_route`` and the limits of
``stream_supported`` / ``tail_supported`` / ``wide_supported`` (profiles/fallback_removal.txt), with each row that named one of
those routes replaced by FUSED_GEMM -- and block 2's RESPOOL end by CONV_THEN_POOL FUSED_GEMM; every other row as it was.
"""
import pytest
import torch

from biscuit_amd.engine import BiscuitHipError, Engine
from biscuit_amd.weights import synthetic_weights

pytestmark = pytest.mark.gpu

N = 256
FUSED = 'FUSED_GEMM nsplit=1'
MIDDLE = [(f'block{b}_sepconv{i}', 'WIDE') for b in range(5, 13) for i in (1, 2, 3)]
SCHEDULE_16 = ([('block1_conv2', 'FRONT'),
                ('block2_sepconv1', 'STREAM'), ('block2_out', 'BLOCK_TAIL'),
                ('block3_sepconv1', 'STREAM'), ('block3_out', 'BLOCK_TAIL'),
                ('block4_sepconv1', 'WIDE'), ('block4_sepconv2', 'WIDE'), ('block4_out', 'POOL_GEMM')] + MIDDLE +
               [('block13_sepconv1', 'WIDE'), ('block13_sepconv2', 'WIDE'), ('block13_out', 'POOL_GEMM'),
                ('block14_sepconv1', 'DW_THEN_EXIT GAP_EPILOGUE=no'), ('block14_sepconv2', 'DW_THEN_EXIT GAP_EPILOGUE=yes')])
SCHEDULE_32 = ([('block1_conv2', FUSED)] +
               [e for b in (2, 3, 4) for e in ((f'block{b}_sepconv1', FUSED), (f'block{b}_sepconv2', FUSED),
                                               (f'block{b}_out', 'CONV_THEN_POOL ' + FUSED))] +
               [(f'block{b}_sepconv{i}', FUSED) for b in range(5, 13) for i in (1, 2, 3)] +
               [('block13_sepconv1', FUSED), ('block13_sepconv2', FUSED), ('block13_out', 'CONV_THEN_POOL ' + FUSED),
                ('block14_sepconv1', FUSED), ('block14_sepconv2', 'FUSED_GEMM nsplit=2'), ('global_avg_pool', 'GAP_KERNEL')])


@pytest.fixture(scope='module')
def weights():
    return synthetic_weights(1, hard=True)


@pytest.fixture(scope='module', params=['f16', 'bf16'])
def eng16(request, weights):
    eng = Engine(weights, dtype=request.param, max_batch=N, max_mc=1)
    yield eng
    eng.close()


def test_16_bit_schedule_from_uint8_tiles(eng16):
    assert eng16.schedule(N) == SCHEDULE_16


# n = 777: block 2's tensors (147 x 147 x 128) pass the 32-bit offsets of the streaming kernel and of the fused tail
SCHEDULE_16_N777 = ([('block1_conv2', 'FRONT'),
                     ('block2_sepconv1', FUSED), ('block2_sepconv2', FUSED), ('block2_out', 'CONV_THEN_POOL ' + FUSED),
                     ('block3_sepconv1', 'STREAM'), ('block3_out', 'BLOCK_TAIL')] + SCHEDULE_16[5:])
# n = 1532: block 3's (74 x 74 x 256) too; its end falls to the shortcut GEMM with the pooling store pass
SCHEDULE_16_N1532 = (SCHEDULE_16_N777[:4] +
                     [('block3_sepconv1', FUSED), ('block3_sepconv2', FUSED), ('block3_out', 'POOL_GEMM')] + SCHEDULE_16[5:])

# n = 1553: block1_conv2's output (147 x 147 x 64) passes the front kernel's; the uint8 entry stages the tiles and walks the float
# entry's routes (the tile kernel indexes with 64 bits: it has no limit of its own)
SCHEDULE_16_N1553 = [('block1_conv2', 'TILE kind=0')] + SCHEDULE_16_N1532[1:]


def test_16_bit_schedule_beyond_the_32_bit_limits(weights):
    eng = Engine(weights, dtype='f16', max_batch=1532)      # (the workspace grows on demand; a schedule allocates nothing)
    try:
        assert eng.schedule(777) == SCHEDULE_16_N777
        assert eng.schedule(1532) == SCHEDULE_16_N1532
    finally:
        eng.close()


def test_16_bit_schedule_beyond_the_front_kernel(weights):
    eng = Engine(weights, dtype='f16', max_batch=1553)
    try:
        assert eng.schedule(1552) == SCHEDULE_16_N1532
        assert eng.schedule(1553) == SCHEDULE_16_N1553 == eng.schedule(1553, u8=False)
        for tap in ('staged', 'block1_conv1'):               # the uint8 entry refuses them at every batch
            with pytest.raises(BiscuitHipError, match='does not materialise'):
                eng.schedule(1553, tap=tap)
    finally:
        eng.close()


def test_16_bit_float_entry_differs_in_block1_conv2_only(eng16):
    assert eng16.schedule(N, u8=False) == [('block1_conv2', 'TILE kind=0')] + SCHEDULE_16[1:]


@pytest.mark.parametrize('tap, ends', [
    # a tap of a tensor a fusion does not write switches that fusion off, and nothing else; the walk ends behind the tensor
    ('block2_res', [('block2_sepconv2', 'STREAM'), ('block2_out', 'CONV_THEN_POOL FUSED_GEMM nsplit=1')]),
    ('block3_sepconv2', [('block3_sepconv2', 'WIDE')]),
    ('block13_res', [('block13_out', 'CONV_THEN_POOL S2_TILED_GEMM')]),
    ('block14_sepconv2', [('block14_sepconv2', 'DW_THEN_EXIT GAP_EPILOGUE=no')]),
])
def test_16_bit_taps_change_only_the_fusion_they_look_into(eng16, tap, ends):
    block_out = tap.split('_')[0] + '_out' if tap != 'block14_sepconv2' else tap
    k = [name for name, _ in SCHEDULE_16].index(block_out)
    assert eng16.schedule(N, tap=tap) == SCHEDULE_16[:k] + ends


def test_schedule_refuses_what_the_debug_tap_refuses(eng16):
    for tap in ('staged', 'block1_conv1'):
        with pytest.raises(BiscuitHipError, match='does not materialise'):
            eng16.schedule(N, tap=tap)
    with pytest.raises(BiscuitHipError, match='unknown activation: no_such_layer'):
        eng16.schedule(N, tap='no_such_layer')


def test_f32_schedule(weights):
    eng = Engine(weights, dtype='f32', max_batch=N, max_mc=1)
    try:
        assert eng.schedule(N) == SCHEDULE_32                 # mc_infer stages the tiles: the float entry
        assert eng.schedule(N, u8=False) == SCHEDULE_32
        assert not any('GAP_EPILOGUE=yes' in route for _, route in SCHEDULE_32)
        for tap in ('block2_res', 'block3_sepconv2', 'block13_res'):
            k = [name for name, _ in SCHEDULE_32].index(tap.split('_')[0] + '_out' if tap.endswith('_res') else tap)
            assert eng.schedule(N, u8=False, tap=tap) == SCHEDULE_32[:k + 1]
        assert eng.schedule(N, u8=False, tap='block14_sepconv2') == SCHEDULE_32[:-1]
    finally:
        eng.close()


def test_schedule_enqueues_nothing(eng16):
    eng16.profile_enable(True)
    try:
        eng16.schedule(N)
        eng16.schedule(N, u8=False, tap='block13_res')
        torch.cuda.synchronize()
        assert eng16.profile_read() == []
    finally:
        eng16.profile_enable(False)
