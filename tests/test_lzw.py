"""TIFF LZW on the host (``bqio_lzw_decode``, ``bqio_lzw_decode_canvas``; csrc/lzw_device.h) against libtiff, byte for byte.  The
oracle wraps every segment in a one-page TIFF and opens it with Pillow -- that is libtiff's decoder: where it returns pixels the
decoder returns the same bytes with status 0; where it raises, the status is not 0.  The streams: libtiff's own (noise, flat,
smooth, 1 x 1, 1 x 700; predictor 1 and 2), the encoder's of tests/_lzw_cases.py for what libtiff never writes (a final string cut
at the segment's end, no EndOfInformation, early and doubled ClearCodes) and hand-built malformed ones.  Then the canvas entry's
placement (the pattern of tests/test_canvas_place.py) and the selfcheck program under ASan and UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from biscuit_amd import tfrecord_native as tn
from tests import _lzw_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not tn.available(), reason='libbiscuit_io.so not built')

VALID = lc.valid_cases()
MALFORMED = lc.malformed_cases()


@pytest.fixture(scope='module')
def verdicts():
    """name -> libtiff's pixels or None, computed once for the malformed streams."""
    return {name: lc.oracle(raw, w, rows) for name, raw, w, rows in MALFORMED}


@pytest.mark.parametrize('case', VALID, ids=lambda c: c[0])
def test_valid_streams_decode_as_libtiff_decodes_them(case):
    name, raw, w, rows, pred, a = case
    want = lc.oracle(raw, w, rows, pred)
    assert want is not None and np.array_equal(want, a), 'the oracle does not read the case'
    got, status = tn.lzw_decode(raw, rows, w, pred)
    assert status == 0 and np.array_equal(got, want)


def test_the_valid_streams_exercise_what_they_are_there_for():
    """Noise: several ClearCodes and all four widths (a table beyond 2047 entries); flat: KwKwK codes and strings far longer than
    a wave's 64 bytes.  Counted with a plain walk over the codes."""
    def walk(raw, need):
        val, nbits, pos, n, fresh, out, prev = int.from_bytes(raw, 'big'), len(raw) * 8, 0, lc.FIRST, True, 0, 0
        clears = kwkwk = longest = top = 0
        lens = {}
        while out < need:
            w = lc.width_for(n)
            c = (val >> (nbits - pos - w)) & ((1 << w) - 1)
            pos += w
            if c == lc.CLEAR:
                clears, n, fresh, lens = clears + 1, lc.FIRST, True, {}
                continue
            ln = 1 if c < 256 else lens[c] if c < n else prev + 1
            kwkwk += c == n and not fresh
            if not fresh:
                lens[n] = prev + 1
                n += 1
            fresh, prev, out, longest, top = False, ln, out + ln, max(longest, ln), max(top, n)
        return clears, kwkwk, longest, top
    by_name = {c[0]: c for c in VALID}
    clears, _, _, top = walk(by_name['noise-p1'][1], 96 * 80 * 3)
    assert clears >= 6 and top > 4090
    clears, kwkwk, longest, _ = walk(by_name['flat-p1'][1], 96 * 80 * 3)
    assert kwkwk > 100 and longest > 64
    clears, kwkwk, longest, _ = walk(by_name['white-p1'][1], 96 * 80 * 3)
    assert kwkwk > 200 and longest > 3 * 64


@pytest.mark.parametrize('case', MALFORMED, ids=lambda c: c[0])
def test_malformed_streams_get_the_oracles_verdict(case, verdicts):
    name, raw, w, rows = case
    want = verdicts[name]
    got, status = tn.lzw_decode(raw, rows, w, 1)
    if want is None:
        assert status != 0
    else:
        assert status == 0 and np.array_equal(got, want)


def test_the_verdicts_are_the_expected_ones(verdicts):
    """What libtiff 4.7 says about the malformed streams, so that the test above cannot pass because the oracle refuses (or
    takes) everything: it reads on past a full table up to its own table's end, and refuses the rest."""
    took = {name for name, v in verdicts.items() if v is not None}
    assert {'no-clear-line-1313', 'no-clear-line-1316', 'no-clear-line-1672'} <= took
    refused = set(verdicts) - took
    assert {'no-lead-clear', 'garbage', 'old-style', 'empty', 'clear-only', 'eoi-early', 'beyond-after-clear', 'beyond-by-one', 'beyond-far',
            'truncated-1', 'truncated-100', 'no-clear-80', 'no-clear-line-1675'} <= refused
    # ... and the status says which refusal it was
    status = {name: tn.lzw_decode(raw, rows, w, 1)[1] for name, raw, w, rows in MALFORMED}
    assert status['no-lead-clear'] == status['garbage'] == status['old-style'] == tn.LZW_HEAD
    assert status['beyond-after-clear'] == status['beyond-by-one'] == status['beyond-far'] == tn.LZW_CODE
    assert status['empty'] == status['truncated-1'] == status['truncated-100'] == status['clear-only'] == status['eoi-early'] == tn.LZW_SHORT
    assert status['no-clear-80'] == status['no-clear-line-1675'] == tn.LZW_FULL


def test_predictor_two_is_the_running_sum_modulo_256():
    a = lc.content('noise', 33, 5, 4)
    raw = lc.encode(lc.difference(a).tobytes())
    got, status = tn.lzw_decode(raw, 5, 33, 2)
    assert status == 0 and np.array_equal(got, a)
    plain, status = tn.lzw_decode(raw, 5, 33, 1)
    assert status == 0 and np.array_equal(np.cumsum(plain, axis=1, dtype=np.uint8), a)
    with pytest.raises(ValueError):
        tn.lzw_decode(raw, 5, 33, 3)


# ---- the canvas entry: placement ------------------------------------------------------------------------------------------------------------
def _canvas_case(predictor):
    """Five 24 x 16 segments around and inside a 40 x 60 canvas with a clip inside it: negative places, places that reach past
    the canvas, one segment outside the clip altogether, one refused."""
    sw, sh, H, W = 24, 16, 40, 60
    tiles = [lc.content(k, sw, sh, i) for i, k in enumerate(['noise', 'smooth', 'flat', 'noise', 'smooth'])]
    enc = (lambda t: lc.encode(lc.difference(t).tobytes())) if predictor == 2 else (lambda t: lc.encode(t.tobytes()))
    raws = [enc(t) for t in tiles]
    raws[3] = raws[3][:40]                                               # refused: the data ends
    place = np.array([[-5, -7], [50, 30], [10, 12], [30, 2], [100, 100]], np.int32)
    clip = (2, 3, 57, 38)
    return sw, sh, H, W, tiles, raws, place, clip


@pytest.mark.parametrize('predictor', [1, 2])
def test_canvas_windows_and_nothing_else(predictor):
    sw, sh, H, W, tiles, raws, place, clip = _canvas_case(predictor)
    ln = [len(r) for r in raws]
    packed, desc = tn.lzw_pack(np.frombuffer(b''.join(raws), np.uint8), np.cumsum([0] + ln[:-1]), ln)
    assert (desc[:, 0] % 16 == 0).all() and desc[:, 1].tolist() == ln
    assert all(packed[o:o + k].tobytes() == r and not packed[o + k:o + k + 16].any() for (o, k), r in zip(desc.tolist(), raws))
    canvas = np.full((H, W, 3), 77, np.uint8)
    status = tn.lzw_decode_canvas(packed, desc, sw, sh, place, canvas, clip, predictor=predictor)
    assert status.tolist() == [0, 0, 0, tn.LZW_SHORT, 0]
    want = np.full((H, W, 3), 77, np.uint8)
    for i, t in enumerate(tiles):
        if i == 3:
            continue
        for y in range(sh):
            for x in range(sw):
                cx, cy = place[i, 0] + x, place[i, 1] + y
                if clip[0] <= cx < clip[2] and clip[1] <= cy < clip[3] and 0 <= cx < W and 0 <= cy < H:
                    want[cy, cx] = t[y, x]
    assert np.array_equal(canvas, want)
    # a descriptor the decoder does not take: an offset that is no multiple of 16
    bad = desc.copy()
    bad[2, 0] += 1
    canvas2 = np.full((H, W, 3), 77, np.uint8)
    status = tn.lzw_decode_canvas(packed, bad, sw, sh, place, canvas2, clip, predictor=predictor)
    assert status.tolist() == [0, 0, tn.LZW_DESC, tn.LZW_SHORT, 0]
    want[12:28, 10:34] = 77
    assert np.array_equal(canvas2, want)
    # one thread and many give the same canvas; no segments: nothing happens
    canvas3 = np.full((H, W, 3), 77, np.uint8)
    tn.lzw_decode_canvas(packed, desc, sw, sh, place, canvas3, clip, predictor=predictor, threads=1)
    assert np.array_equal(canvas3, canvas)
    assert len(tn.lzw_decode_canvas(packed[:0], desc[:0], sw, sh, place[:0], canvas3, clip)) == 0 and np.array_equal(canvas3, canvas)


def test_canvas_entry_refuses_bad_arguments():
    canvas = np.zeros((8, 8, 3), np.uint8)
    packed, desc = tn.lzw_pack(np.frombuffer(lc.encode(b'\0' * 12), np.uint8), [0], [len(lc.encode(b'\0' * 12))])
    for sw, sh, pred in [(0, 2, 1), (2, 0, 1), (tn.LZW_MAX_SIDE + 1, 2, 1), (2, tn.LZW_MAX_SIDE + 1, 1), (2, 2, 0), (2, 2, 3)]:
        with pytest.raises(ValueError):
            tn.lzw_decode_canvas(packed, desc, sw, sh, [[0, 0]], canvas, (0, 0, 8, 8), predictor=pred)
    assert tn.lib().bqio_lzw_max_side() == tn.LZW_MAX_SIDE


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_selfcheck_under_the_sanitizers(tmp_path):
    """tests/lzw_selfcheck.cpp -- lzw_device.h over valid streams from a built-in encoder and tens of thousands of seeded
    mutations and truncations, in exact-size heap buffers -- built with AddressSanitizer and UBSan as a program of its own and run."""
    exe = str(tmp_path / 'lzw_selfcheck')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-I', os.path.join(ROOT, 'biscuit_amd', 'csrc'), os.path.join(ROOT, 'tests', 'lzw_selfcheck.cpp'),
                            '-o', exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert 'ok' in run.stdout
