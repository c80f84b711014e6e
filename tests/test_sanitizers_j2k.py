"""tools/fuzz/j2k_fuzz.cpp -- ``bqio_j2k_extract`` (tier 2 of the JPEG 2000 decoder) and ``bqio_j2k_decode_canvas``, the routines the device
decoder is compiled from (csrc/j2k_device.h) -- under AddressSanitizer + UndefinedBehaviorSanitizer with exact-size heap buffers, in
the pattern of tests/test_sanitizers_wsi_jpeg.py: a stand-alone program, nothing inside ``python``.  The case files
(tools/fuzz/make_j2k_corpus.py) hold Pillow's codestreams across the subset's axes and the streams outside it, each with the
status and the pixels that must come out, so the harness first repeats the comparisons of tests/test_j2k.py under the sanitizers
and then mutates: headers, packet bytes, block rows and descriptors, places, clip rectangles, canvas sizes, with guard rows."""
import os
import re
import subprocess
import sys

import pytest

from tests.test_sanitizers import ROOT, _build


def test_extractor_and_canvas_decode_under_sanitizers(tmp_path):
    pytest.importorskip('PIL')
    corpus = str(tmp_path / 'corpus')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'fuzz', 'make_j2k_corpus.py'), corpus], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    files = sorted(os.path.join(corpus, f) for f in os.listdir(corpus))
    assert len(files) == 4 + 2 + 5
    exe = str(tmp_path / 'j2k_fuzz')
    _build('j2k_fuzz.cpp', exe, ['-lpthread'])
    p = subprocess.run([exe, '600'] + files, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])        # a sanitizer report aborts with a non-zero status
    m = re.search(r'(\d+) segments equal to the case files, (\d+) refusals as expected; 600 mutations: (\d+) decoded, (\d+) with a status, '
                  r'(\d+) refused', p.stdout)
    assert m, p.stdout[-500:]
    decoded, refusals, ok, status, refused = map(int, m.groups())
    assert decoded == 2 * 7 + 2 + 1 + 10 and refusals == 10 and ok + status + refused == 600
    assert ok > 30 and status > 30 and refused > 30, p.stdout                # every outcome really occurs
