"""The batch sizes at which the network's 32-bit byte offsets turn over, computed from the shapes of ``TAPS`` (tests/test_gpu_parity.py)
and the constants of the route predicates in csrc -- not written down: a guard that moves shows up here as a changed size
(tests/test_batch_limits.py holds the numbers, tests/test_gpu_batch_limits.py runs them and ties each to ``Engine.schedule``).

The predicates, as the C++ states them (bq_common.h declares them side by side):

* ``stream_supported`` / ``tail_supported`` (kernels_stream.hip): ``n * H * W * C * 2 <= STREAM_LIMIT`` -- C the channels of the tensor
  the kernel stores through its raw buffer (STREAM) or reads its rows from (BLOCK_TAIL: sepconv1's output);
* ``wide_supported`` (kernels_wide.hip): ``M * Nstore * 2 < WIDE_LIMIT``;
* ``front_supported`` (kernels_front.hip): ``n * 147 * 147 * 64 * 2 <= FRONT_LIMIT``.
"""
from tests.test_gpu_parity import TAPS

STREAM_LIMIT = 0xfffff000       # the offset of the stores the hardware is to drop: the tensor ends at or below it
WIDE_LIMIT = 1 << 32
FRONT_LIMIT = 0xffffff00
SIGN = 1 << 31                  # an (int) cast of a byte offset goes negative from here
WRAP = 1 << 32

SHAPES = dict(TAPS, block13_sepconv2=(19, 19, 1024))      # (the one input below that is not itself a tap of TAPS)
ESIZE = {'f16': 2, 'bf16': 2, 'f32': 4}

# the tensor(s) the layer behind a tap reads: the walk of backbone_impl (csrc/biscuit_hip.hip)
INPUTS = {'staged': (), 'block1_conv1': ('staged',), 'block1_conv2': ('block1_conv1',)}
for _b, _x in ((2, 'block1_conv2'), (3, 'block2_out'), (4, 'block3_out')):
    INPUTS.update({f'block{_b}_res': (_x,), f'block{_b}_sepconv1': (_x,), f'block{_b}_sepconv2': (f'block{_b}_sepconv1',),
                   f'block{_b}_out': (f'block{_b}_sepconv2', _x)})
for _b in range(5, 13):         # (the middle flow's inner tensors have the shape of its block outputs)
    INPUTS[f'block{_b}_out'] = (f'block{_b - 1}_out',)
INPUTS.update({'block13_out': ('block13_sepconv2', 'block12_out'), 'block14_sepconv1': ('block13_out',), 'block14_sepconv2': ('block14_sepconv1',)})


def pad16(c):
    return (c + 15) // 16 * 16


def tile_bytes(name, dtype):
    """Bytes of one tile's part of the stored tensor ``name`` (rows of the channel count padded to 16, as the kernels stride them;
    the staged tile is planar and unpadded)."""
    h, w, c = SHAPES[name]
    return h * w * (c if name == 'staged' else pad16(c)) * ESIZE[dtype]


def first_reaching(per_tile, bound):
    """The smallest batch whose tensor has at least ``bound`` bytes."""
    return -(-bound // per_tile)


def last_within(per_tile, limit, strict=False):
    """The largest batch whose tensor has at most (``strict``: fewer than) ``limit`` bytes."""
    return (limit - 1 if strict else limit) // per_tile


def sizes():
    """{'<element bits>_<what turns>': n} -- the seven rows of the table in tests/test_gpu_batch_limits.py."""
    b2, b3, front = tile_bytes('block2_sepconv1', 'f16'), tile_bytes('block3_sepconv1', 'f16'), tile_bytes('block1_conv2', 'f16')
    assert tile_bytes('block2_sepconv2', 'f16') == b2 and tile_bytes('block3_sepconv2', 'f16') == b3
    last_b2 = last_within(b2, STREAM_LIMIT)                                             # STREAM x 2 and BLOCK_TAIL of block 2
    last_b3 = min(last_within(b3, STREAM_LIMIT), last_within(b3, WIDE_LIMIT, strict=True))   # STREAM, BLOCK_TAIL; WIDE under a tap
    return {'16_block2_sign': first_reaching(b2, SIGN),             # block 2's tensors pass 2^31 bytes
            '16_block2_last': last_b2,                              # the last batch block 2 runs on STREAM / BLOCK_TAIL
            '16_block2_falls': last_b2 + 1,
            '16_block3_falls': last_b3 + 1,
            '16_front_falls': last_within(front, FRONT_LIMIT) + 1,
            '32_block2_sign': first_reaching(tile_bytes('block2_sepconv1', 'f32'), SIGN),
            '32_block2_wrap': first_reaching(tile_bytes('block2_sepconv1', 'f32'), WRAP)}


def taps_reaching(n, dtype, bound=SIGN):
    """The taps of ``TAPS``, in order, whose tensor -- or a tensor the layer behind them reads -- has at least ``bound`` bytes at a
    batch of ``n``."""
    big = lambda name: n * tile_bytes(name, dtype) >= bound
    return [name for name, _ in TAPS if big(name) or any(big(i) for i in INPUTS[name])]


def batch_index(n):
    """Which of six tiles each image of the batch is: ``i % 6``, the last two images tiles 0 and 1 again -- the two tiles with oracle
    taps sit at both ends of every tensor."""
    idx = [i % 6 for i in range(n)]
    idx[-2:] = [0, 1]
    return idx
