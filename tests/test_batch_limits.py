"""tests/_batch_limits.py: the arithmetic that turns the shapes of ``TAPS`` and the constants of the route predicates into the batch
sizes tests/test_gpu_batch_limits.py runs.  The numbers asserted here are worked out by hand from the predicates' text."""
import re
from pathlib import Path

from tests import _batch_limits as B

CSRC = Path(__file__).resolve().parent.parent / 'biscuit_amd' / 'csrc'


def test_bytes_per_tile():
    assert B.tile_bytes('block2_sepconv1', 'f16') == B.tile_bytes('block2_sepconv2', 'bf16') == 147 * 147 * 128 * 2 == 5_531_904
    assert B.tile_bytes('block1_conv2', 'f16') == 2_765_952
    assert B.tile_bytes('block3_sepconv2', 'f16') == 2_803_712
    assert B.tile_bytes('block4_sepconv1', 'f16') == 37 * 37 * 736 * 2            # 728 channels in rows of 736
    assert B.tile_bytes('block2_sepconv1', 'f32') == 11_063_808
    assert B.tile_bytes('staged', 'f32') == 299 * 299 * 3 * 4


def test_the_seven_sizes():
    assert B.sizes() == {'16_block2_sign': 389, '16_block2_last': 776, '16_block2_falls': 777, '16_block3_falls': 1532,
                         '16_front_falls': 1553, '32_block2_sign': 195, '32_block2_wrap': 389}
    b2 = B.tile_bytes('block2_sepconv1', 'f16')
    assert 388 * b2 < 2 ** 31 <= 389 * b2
    assert 776 * b2 == 4_292_757_504 <= 0xfffff000 < 777 * b2
    assert 0xfffff000 - 776 * b2 == 2_205_696                                       # the dropped-store offset, 2.2 MB behind the end
    # what else has turned by then, as the table of tests/test_gpu_batch_limits.py says
    assert B.first_reaching(B.tile_bytes('block1_conv2', 'f16'), B.SIGN) == 777
    assert B.first_reaching(B.tile_bytes('block3_sepconv1', 'f16'), B.SIGN) == 766
    assert B.first_reaching(B.tile_bytes('block4_sepconv1', 'f16'), B.SIGN) == 1066
    assert B.last_within(B.tile_bytes('block4_sepconv1', 'f16'), B.WIDE_LIMIT, strict=True) == 2131   # "n < 2 132 at 37x37"


def test_rounding_at_the_bounds():
    assert B.first_reaching(10, 100) == 10 and B.first_reaching(10, 101) == 11
    assert B.last_within(10, 100) == 10 and B.last_within(10, 100, strict=True) == 9 and B.last_within(10, 109) == 10


def test_taps_reaching_follows_the_tensor_and_its_inputs():
    assert B.taps_reaching(388, 'f16') == [] and B.taps_reaching(194, 'f32') == []
    # 147 x 147 x 128 itself, and the layers that read it: block2_out reads block2_sepconv2
    assert B.taps_reaching(389, 'f16') == ['block2_sepconv1', 'block2_sepconv2', 'block2_out']
    assert B.taps_reaching(195, 'f32') == B.taps_reaching(389, 'f16')
    at_777 = B.taps_reaching(777, 'bf16')
    assert at_777[:2] == ['block1_conv2', 'block2_res'] and 'block3_out' in at_777 and 'block4_sepconv1' not in at_777
    # f32, n = 389: 147 x 147 x 64 x 4 B x 389 is 2 151 910 656 -- just past 2^31
    assert B.taps_reaching(389, 'f32') == ['block1_conv2', 'block2_res', 'block2_sepconv1', 'block2_sepconv2', 'block2_out',
                                           'block3_sepconv1', 'block3_sepconv2', 'block3_out']
    assert set(B.INPUTS) == set(B.SHAPES) - {'block13_sepconv2'}


def test_batch_index():
    idx = B.batch_index(389)
    assert idx[:6] == [0, 1, 2, 3, 4, 5] and idx[-2:] == [0, 1] and len(idx) == 389 and idx[386] == 386 % 6
    assert set(idx) == set(range(6))


def test_the_constants_are_those_of_the_predicates():
    """The limits as csrc spells them: a guard edited there fails here until the helper -- and with it the sizes -- follows."""
    stream = (CSRC / 'kernels_stream.hip').read_text()
    assert len(re.findall(r'\* 2 <= 0xfffff000ll;', stream)) == 2 and B.STREAM_LIMIT == 0xfffff000
    assert 'M * Nstore * 2 < (1ll << 32)' in (CSRC / 'kernels_wide.hip').read_text() and B.WIDE_LIMIT == 1 << 32
    assert 'n * CO * CO * 64 * 2 <= 0xffffff00ll' in (CSRC / 'kernels_front.hip').read_text() and B.FRONT_LIMIT == 0xffffff00
    common = (CSRC / 'bq_common.h').read_text()
    for name in ('stream_supported', 'tail_supported', 'wide_supported', 'exit_supported', 'front_supported'):
        assert f'bool {name}(' in common, name
