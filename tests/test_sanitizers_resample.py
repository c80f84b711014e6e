"""tools/fuzz/resample_check.cpp -- ``bqio_resample_taps`` and ``bqio_tile_resample``, the CPU build of the routines the tile
resampling kernel is compiled from (csrc/resample_device.h) -- under AddressSanitizer + UndefinedBehaviorSanitizer with
exact-size heap buffers, over the case matrix of tests/test_resample.py (every source width, windows inside, partly and wholly
outside the canvas) against Pillow's bytes; built like tests/test_sanitizers_jpeg_extract.py, skipped where the compiler has
no sanitizer runtime."""
import subprocess

import numpy as np
import pytest

from tests import _resample_ref as R
from tests.test_sanitizers import _build


def test_tile_resample_under_sanitizers(tmp_path):
    pytest.importorskip('PIL')
    files = []
    for src in R.WIDTHS:
        canvas, origin = R.case(src)
        want = R.pillow_tiles(canvas, origin, src)
        path = tmp_path / f'case_{src}.bin'
        with open(path, 'wb') as f:
            f.write(np.array([canvas.shape[0], canvas.shape[1], len(origin), src, R.PX], np.int32).tobytes())
            f.write(canvas.tobytes())
            f.write(origin.astype(np.int32).tobytes())
            f.write(want.tobytes())
        files.append(str(path))
    exe = str(tmp_path / 'resample_check')
    _build('resample_check.cpp', exe)
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])        # a sanitizer report aborts with a non-zero status
    assert p.stdout.strip() == f'tiles {10 * len(R.WIDTHS)} mismatches 0', p.stdout[-500:]
