"""``Engine.jpeg_decode_canvas`` and ``Engine.j2k_decode_canvas`` over the grid of places and clip rectangles of
tests/_canvas_place_cases.py, against the CPU decoders' canvases (which tests/test_canvas_place.py holds to the window rule of
csrc/canvas_place.h) byte for byte, with guard rows around the device canvas: ``-m gpu``."""
import numpy as np
import pytest
import torch

from tests import _canvas_place_cases as cp

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 2, 0xA5              # rows in front of and behind the device canvas


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    yield e
    e.close()


@pytest.mark.parametrize('codec', cp.CODECS)
def test_device_canvases_equal_the_cpu_decoders(eng, codec):
    dev = eng.device
    arrays = cp.packed(codec)
    if codec == 'jpeg':
        arrays = (arrays[0], arrays[1].view(np.int32), arrays[2])
    arrays = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    decode = eng.jpeg_decode_canvas if codec == 'jpeg' else eng.j2k_decode_canvas
    row = cp.W * 3
    buf = torch.empty((cp.H + 2 * GUARD) * row, dtype=torch.uint8, device=dev)
    canvas = buf[GUARD * row:(GUARD + cp.H) * row].view(cp.H, cp.W, 3)
    for pi, place in enumerate(cp.PLACES):
        d_place = torch.tensor([place], dtype=torch.int32, device=dev)
        for ci, clip in enumerate(cp.CLIPS):
            for fill in (0, 255):
                buf.fill_(GUARD_BYTE)
                canvas.fill_(fill)
                status = decode(*arrays, cp.SEG, cp.SEG, d_place, canvas, clip)
                flat = buf.cpu().numpy()
                assert status.cpu().tolist() == [0]
                assert (flat[:GUARD * row] == GUARD_BYTE).all() and (flat[(GUARD + cp.H) * row:] == GUARD_BYTE).all(), ('guard rows touched', place, clip)
                got = flat[GUARD * row:(GUARD + cp.H) * row].reshape(cp.H, cp.W, 3)
                assert np.array_equal(got, cp.cpu_canvases(codec)[pi, ci, fill]), (place, clip, fill)
