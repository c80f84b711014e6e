"""The device JPEG encoder (csrc/kernels_jpeg_encode.hip, ``bq_jpeg_encode`` through ``Engine.jpeg_encode``) against the CPU build
of the same routines (``bqio_jpeg_encode``) and therefore against Pillow, which tests/test_jpeg_encode.py holds that build to:
complete files byte for byte, offset for offset, over tests/_jpeg_encode_cases.py.  ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import tfrecord as tfr
from biscuit_amd import tfrecord_native as tn
from biscuit_amd.weights import synthetic_weights
from tests import _jpeg_cases as jc
from tests import _jpeg_encode_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    return Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)


def gpu(eng, tiles, q=95, s='4:2:0', **kw):
    buf, off = eng.jpeg_encode(torch.from_numpy(np.ascontiguousarray(tiles)).cuda(), q, s, **kw)
    return buf.cpu().numpy(), off.numpy()


@pytest.mark.parametrize('px', ec.SIZES)
def test_same_files_as_the_cpu_build_and_pillow(eng, px):
    for q, s in ec.settings():
        for names in ec.batches(px):
            tiles = np.stack([ec.tile(px, w) for w in names])
            want, want_off, _ = tn.jpeg_encode(tiles, q, s)
            got, off = gpu(eng, tiles, q, s)
            assert np.array_equal(off, want_off), (px, q, s, names)
            assert np.array_equal(got, want), (px, q, s, names)
            for w, raw in zip(names, ec.split(got, off)):
                assert raw == ec.pillow(px, w, q, s), (px, q, s, w)


def test_rounds_and_a_large_batch(eng):
    """300 mixed tiles of 33 px: more than one wave of workgroups and more than 256 tiles (the scratch ``jpeg_encode_scratch``
    asks for holds 256: two rounds); then a scratch of 7 tiles (43 rounds).  The same bytes every way."""
    tiles = ec.mixed(300)
    want, want_off, _ = tn.jpeg_encode(tiles, 95, '4:2:0')
    got, off = gpu(eng, tiles)
    assert np.array_equal(off, want_off) and np.array_equal(got, want)
    per_tile = eng.jpeg_encode_scratch(1, 33).numel()
    assert eng.jpeg_encode_scratch(300, 33).numel() == 256 * per_tile
    small = torch.empty(7 * per_tile + 5, dtype=torch.uint8, device='cuda')
    got7, off7 = gpu(eng, tiles, scratch=small)
    assert np.array_equal(off7, want_off) and np.array_equal(got7, want)
    got4, off4 = gpu(eng, tiles[:50], 100, '4:4:4', scratch=small[:eng.jpeg_encode_scratch(1, 33, '4:4:4').numel()])
    want4, want_off4, _ = tn.jpeg_encode(tiles[:50], 100, '4:4:4')
    assert np.array_equal(off4, want_off4) and np.array_equal(got4, want4)


def test_cap_status_and_retry(eng):
    tiles = ec.mixed(12, px=17)
    want, want_off, _ = tn.jpeg_encode(tiles)
    # the raw entry with a buffer one byte short: bit 1 for the last tile only, the earlier files intact, the offsets exact
    d = torch.from_numpy(tiles).cuda()
    cap = int(want_off[-1]) - 1
    out = torch.zeros(cap, dtype=torch.uint8, device='cuda')
    off = torch.zeros(13, dtype=torch.int64, device='cuda')
    status = torch.full((12,), -1, dtype=torch.int32, device='cuda')
    scratch = eng.jpeg_encode_scratch(12, 17)
    rc = eng._lib.bq_jpeg_encode(eng._ctx, C.c_void_p(d.data_ptr()), 12, 17, 95, 2, C.c_void_p(out.data_ptr()), cap,
                                 C.c_void_p(off.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                 scratch.numel(), eng._stream())
    assert rc == 0
    assert status.cpu().tolist() == [0] * 11 + [1]
    assert np.array_equal(off.cpu().numpy(), want_off)
    got = out.cpu().numpy()
    assert np.array_equal(got[:want_off[11]], want[:want_off[11]]) and not got[want_off[11]:].any()
    # Engine.jpeg_encode with a first guess that is too small: one more call with the exact total
    got, off = gpu(eng, tiles, cap=100)
    assert eng.jpeg_encode_calls == 2
    assert np.array_equal(off, want_off) and np.array_equal(got, want)
    got, off = gpu(eng, tiles)
    assert eng.jpeg_encode_calls == 1 and np.array_equal(got, want)


def test_empty_batch_and_refusals(eng):
    from biscuit_amd.engine import BiscuitHipError
    eng.profile_enable(True)
    buf, off = eng.jpeg_encode(torch.empty((0, 33, 33, 3), dtype=torch.uint8, device='cuda'))
    assert buf.numel() == 0 and off.tolist() == [0]
    assert not [e for e in eng.profile_read() if e.name.startswith('jpeg_encode')]       # nothing was launched
    tiles = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device='cuda')
    eng.jpeg_encode(tiles)
    assert sorted(e.name for e in eng.profile_read() if e.name.startswith('jpeg_encode')) == [
        'jpeg_encode_pack', 'jpeg_encode_pixel', 'jpeg_encode_size', 'jpeg_encode_stuff']
    eng.profile_enable(False)
    for q in (0, 101):
        with pytest.raises(BiscuitHipError, match='subset'):
            eng.jpeg_encode(tiles, quality=q)
    with pytest.raises(ValueError):
        eng.jpeg_encode(tiles, subsampling='4:2:2')
    with pytest.raises(BiscuitHipError, match='subset'):
        eng.jpeg_encode(torch.zeros((1, 0, 0, 3), dtype=torch.uint8, device='cuda'))
    with pytest.raises(BiscuitHipError, match='scratch'):
        eng.jpeg_encode(tiles, scratch=torch.empty(64, dtype=torch.uint8, device='cuda'))


def test_the_device_decoder_reads_the_files_back(eng, tmp_path):
    """bq_jpeg_decode of the encoder's output equals Pillow's decode of it."""
    for s in ec.SUBSAMPLINGS:
        tiles = ec.mixed(9, px=33, seed=11)
        got, off = gpu(eng, tiles, 95, s)
        raws = ec.split(got, off)
        path = str(tmp_path / f'e{s[-1]}.tfrecords')
        tfr.write_slide(path, 'e', raws, np.zeros((len(raws), 2), np.int64))
        scan, desc, tables = jc.extract(path, 0, len(raws), 33)
        dec, status = eng.jpeg_decode(torch.from_numpy(scan).cuda(), torch.from_numpy(desc.view(np.int32)).cuda(),
                                      torch.from_numpy(tables).cuda(), 33)
        assert not status.cpu().numpy().any()
        dec = dec.cpu().numpy()
        for i, raw in enumerate(raws):
            assert np.array_equal(dec[i], ec.pillow_pixels(raw)), (s, i)
