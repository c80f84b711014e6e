"""tools/fuzz/jpeg_extract_fuzz.cpp -- ``bqio_extract_jpeg`` and the device JPEG decoder's routines (csrc/jpeg_device.h) run on
the CPU -- under AddressSanitizer + UndefinedBehaviorSanitizer with exact-size heap buffers, in the pattern of
tests/test_sanitizers.py: a short run per test invocation (the long run is quoted in DESIGN.md); skipped where the compiler
has no sanitizer runtime."""
import os
import subprocess
import sys

import pytest

from tests.test_sanitizers import ROOT, _build


def test_jpeg_extractor_and_device_routines_under_sanitizers(tmp_path):
    pytest.importorskip('PIL')
    corpus = str(tmp_path / 'corpus')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'fuzz', 'make_jpeg_corpus.py'), corpus], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    files = sorted(os.path.join(corpus, f) for f in os.listdir(corpus))
    assert len(files) >= 10
    exe = str(tmp_path / 'jpeg_extract_fuzz')
    _build('jpeg_extract_fuzz.cpp', exe, ['-lz', '-lpthread'])
    p = subprocess.run([exe, '3000'] + files, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])        # a sanitizer report aborts with a non-zero status
    assert 'decoded' in p.stdout and 'with a status' in p.stdout and 'refused' in p.stdout
