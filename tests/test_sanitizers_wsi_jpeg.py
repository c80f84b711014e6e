"""tools/fuzz/wsi_jpeg_fuzz.cpp -- ``bqio_extract_jpeg_segments`` and ``bqio_jpeg_decode_canvas``, the routines the device canvas decoder
is compiled from (csrc/jpeg_device.h) -- under AddressSanitizer + UndefinedBehaviorSanitizer with exact-size heap buffers, in the
pattern of tests/test_sanitizers_jpeg_extract.py.  The case files (tools/fuzz/make_wsi_jpeg_corpus.py) are the pages of
tests/test_wsi_jpeg_segments.py -- every sampling and tile shape, both stream forms, a segment with its own quantiser, the five
refusals -- each with Pillow's page or the index to refuse, so the harness first repeats those comparisons under the sanitizers and
then mutates: segments and tables, places, clip rectangles, canvas sizes, with guard rows around the canvas."""
import os
import re
import subprocess
import sys

import pytest

from tests.test_sanitizers import ROOT, _build


def test_segment_extractor_and_canvas_decode_under_sanitizers(tmp_path):
    pytest.importorskip('PIL')
    corpus = str(tmp_path / 'corpus')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'fuzz', 'make_wsi_jpeg_corpus.py'), corpus], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    files = sorted(os.path.join(corpus, f) for f in os.listdir(corpus))
    assert len(files) == 12 + 2 + 5
    exe = str(tmp_path / 'wsi_jpeg_fuzz')
    _build('wsi_jpeg_fuzz.cpp', exe, ['-lz', '-lpthread'])
    p = subprocess.run([exe, '400'] + files, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])        # a sanitizer report aborts with a non-zero status
    m = re.search(r'(\d+) pages equal to the case files, (\d+) refusals as expected; 400 mutations: (\d+) decoded, (\d+) with a status, '
                  r'(\d+) refused', p.stdout)
    assert m, p.stdout[-500:]
    pages, refusals, ok, status, refused = map(int, m.groups())
    assert pages == 14 and refusals == 5 and ok + status + refused == 400
    assert ok > 20 and status > 5 and refused > 20, p.stdout                # every outcome really occurs
