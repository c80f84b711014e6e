"""The device PNG encoder (csrc/kernels_png_encode.hip, ``bq_png_encode`` through ``Engine.png_encode``) against the CPU build of
the same routines (``bqio_png_encode``), which tests/test_png_encode.py holds to Pillow's rows, to zlib and to the size
conditions: complete files byte for byte, offset for offset, over tests/_png_encode_cases.py.  ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import tfrecord_native as tn
from biscuit_amd.weights import synthetic_weights
from tests import _png_encode_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    return Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)


def gpu(eng, tiles, **kw):
    buf, off = eng.png_encode(torch.from_numpy(np.ascontiguousarray(tiles)).cuda(), **kw)
    return buf.cpu().numpy(), off.numpy()


@pytest.mark.parametrize('px', pc.SIZES)
def test_same_files_as_the_cpu_build(eng, px):
    """Every content of every size; one call per size below 299, calls of three at 299."""
    for names in pc.batches(px):
        tiles = np.stack([pc.tile(px, w) for w in names])
        want, want_off, _ = tn.png_encode(tiles)
        got, off = gpu(eng, tiles)
        assert np.array_equal(off, want_off), (px, names, off, want_off)
        assert np.array_equal(got, want), (px, names)


def test_filter_tie_tiles(eng):
    for t in (pc.TIE_UP, pc.TIE_PAETH):
        want, want_off, _ = tn.png_encode(t[None])
        got, off = gpu(eng, t[None])
        assert np.array_equal(off, want_off) and np.array_equal(got, want)


def test_scratch_for_one_tile_gives_the_same_bytes(eng):
    """40 mixed tiles of 33 px in one round, in rounds of 7 and in rounds of one; a 74-px batch (two blocks a tile) likewise."""
    for tiles in (pc.mixed(40), np.stack([pc.tile(74, w) for w in pc.CONTENTS])):
        px = tiles.shape[1]
        want, want_off, _ = tn.png_encode(tiles)
        got, off = gpu(eng, tiles)
        assert np.array_equal(off, want_off) and np.array_equal(got, want)
        per_tile = eng.png_encode_scratch(1, px).numel()
        assert eng.png_encode_scratch(len(tiles), px).numel() == len(tiles) * per_tile
        assert eng.png_encode_scratch(300, px).numel() == 128 * per_tile
        small = torch.empty(7 * per_tile + 5, dtype=torch.uint8, device='cuda')
        for scratch in (small, small[:per_tile]):
            got, off = gpu(eng, tiles, scratch=scratch)
            assert np.array_equal(off, want_off) and np.array_equal(got, want)


def test_cap_status_and_retry(eng):
    tiles = pc.mixed(12, px=17)
    want, want_off, _ = tn.png_encode(tiles)
    # the raw entry with a buffer one byte short: bit 1 for the last tile only, the earlier files intact, the offsets exact
    d = torch.from_numpy(tiles).cuda()
    cap = int(want_off[-1]) - 1
    out = torch.zeros(cap, dtype=torch.uint8, device='cuda')
    off = torch.zeros(13, dtype=torch.int64, device='cuda')
    status = torch.full((12,), -1, dtype=torch.int32, device='cuda')
    scratch = eng.png_encode_scratch(12, 17)

    def call(o, cap):
        return eng._lib.bq_png_encode(eng._ctx, C.c_void_p(d.data_ptr()), 12, 17, C.c_void_p(o.data_ptr()) if o is not None else None, cap,
                                      C.c_void_p(off.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                      scratch.numel(), eng._stream())
    assert call(out, cap) == 0
    assert status.cpu().tolist() == [0] * 11 + [1]
    assert np.array_equal(off.cpu().numpy(), want_off)
    got = out.cpu().numpy()
    assert np.array_equal(got[:want_off[11]], want[:want_off[11]]) and not got[want_off[11]:].any()
    # the sizing call: no buffer at all
    off.zero_()
    assert call(None, 0) == 0
    assert status.cpu().tolist() == [1] * 12 and np.array_equal(off.cpu().numpy(), want_off)
    # Engine.png_encode with a first guess that is too small: one more call with the exact total
    got, off2 = gpu(eng, tiles, cap=100)
    assert eng.png_encode_calls == 2
    assert np.array_equal(off2, want_off) and np.array_equal(got, want)
    got, off2 = gpu(eng, tiles)
    assert eng.png_encode_calls == 1 and np.array_equal(got, want)


def test_empty_batch_profile_classes_and_refusals(eng):
    from biscuit_amd.engine import BiscuitHipError
    eng.profile_enable(True)
    buf, off = eng.png_encode(torch.empty((0, 33, 33, 3), dtype=torch.uint8, device='cuda'))
    assert buf.numel() == 0 and off.tolist() == [0]
    assert not [e for e in eng.profile_read() if e.name.startswith('png_encode')]       # nothing was launched
    tiles = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device='cuda')
    eng.png_encode(tiles)
    assert sorted(e.name for e in eng.profile_read() if e.name.startswith('png_encode')) == [
        'png_encode_code', 'png_encode_filter', 'png_encode_match', 'png_encode_pack']
    eng.profile_enable(False)
    with pytest.raises(BiscuitHipError, match='subset'):
        eng.png_encode(torch.zeros((1, 0, 0, 3), dtype=torch.uint8, device='cuda'))
    with pytest.raises(BiscuitHipError, match='scratch'):
        eng.png_encode(tiles, scratch=torch.empty(64, dtype=torch.uint8, device='cuda'))
    assert eng._lib.bq_png_encode(eng._ctx, None, 1, 8, None, 0, None, None, None, 0, eng._stream()) != 0        # null pointers


def test_close_releases_the_scratch():
    from biscuit_amd.engine import Engine
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    try:
        e.png_encode(torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device='cuda'))
        assert e._tool_ws['png_encode'].is_cuda
    finally:
        e.close()
    assert e._tool_ws == {} and e._ws is None


@pytest.mark.parametrize('px', [5, 74, 299])
def test_the_device_decoder_reads_the_files_back(eng, px):
    """bq_png_inflate + bq_png_unfilter_strided over the encoder's files: status 0 and the original tiles -- stored, fixed and
    dynamic blocks, one IDAT and several."""
    names = list(pc.CONTENTS) if px != 299 else ['noise', 'gradient', 'synthetic']
    tiles = np.stack([pc.tile(px, w) for w in names])
    got, off = gpu(eng, tiles)
    z, zoff, zlen = pc.pack_streams([pc.zstream(raw) for raw in pc.split(got, off)])
    rows, status = eng.png_inflate(torch.from_numpy(z).cuda(), torch.from_numpy(zoff).cuda(), torch.from_numpy(zlen).cuda(), px)
    assert not status.cpu().numpy().any()
    back = eng.png_unfilter_strided(rows, px)
    assert np.array_equal(back.cpu().numpy(), tiles)
