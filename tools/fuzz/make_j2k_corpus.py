"""Case files for tools/fuzz/j2k_fuzz.cpp: python tools/fuzz/make_j2k_corpus.py OUTDIR

One file per row of JPEG 2000 segments as a slide reader would hand them to ``bqio_j2k_extract``: raw codestreams Pillow (OpenJPEG)
writes -- both transforms, MCT on and off, the five progressions, small and rectangular code blocks, explicit precincts, several
layers, rate-limited streams with truncated blocks, an all-white tile -- and streams the extractor has to refuse (several tiles, one
and four components, 16 bits, a code-block style, SOP, EPH, a truncated stream, a tile-part length past the end).  With each segment:
the status the extractor must give it, and the pixels that must come out -- Pillow's decode, through its YCbCr conversion where
the segments are read as compression 33003 -- or white for a refused one.  Little-endian uint32 fields:

    'BQJK' seg_w seg_h n ycc exact | lengths[n] | status[n] | segments | n * seg_h * seg_w * 3 bytes

``exact`` = 1: the pixels must be equal; 0 (irreversible streams): within one level."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _j2k_cases as jc                          # noqa: E402  (the forge the tests use)
from tests._j2k_cases import content, j2k                   # noqa: E402


def picture(w, h, seed, kind='photo'):
    return content(kind, w, h, seed)


def pillow(raw, ycc):
    return jc.pillow_ycc(raw) if ycc else jc.pillow(raw)


def write(path, w, h, segs, status, ycc, exact):
    with open(path, 'wb') as f:
        f.write(b'BQJK' + struct.pack('<5I', w, h, len(segs), int(ycc), int(exact)))
        f.write(struct.pack(f'<{len(segs)}I', *[len(s) for s in segs]) + struct.pack(f'<{len(segs)}I', *status))
        f.write(b''.join(segs))
        for s, st in zip(segs, status):
            f.write((np.full((h, w, 3), 255, np.uint8) if st else pillow(s, ycc)).tobytes())


def patched(raw, offset, value):
    return jc.patched(raw, b'\xff\x52', offset, value)             # a byte of COD


def main(out):
    os.makedirs(out, exist_ok=True)
    n = 0

    def name(kind):
        nonlocal n
        n += 1
        return os.path.join(out, f'case{n:02d}_{kind}.bqjk')
    rev = [dict(num_resolutions=1), dict(num_resolutions=6, mct=1, progression='RPCL'), dict(num_resolutions=3, codeblock_size=(4, 4), progression='CPRL'),
           dict(num_resolutions=4, mct=1, codeblock_size=(16, 64), progression='PCRL', precinct_size=(32, 32), quality_layers=[40, 10, 0])]
    irr = [dict(num_resolutions=1, mct=1), dict(num_resolutions=6, mct=1, quality_mode='rates', quality_layers=[20, 8], progression='RLCP'),
           dict(num_resolutions=3, mct=0, codeblock_size=(32, 32), quality_mode='dB', quality_layers=[30, 45])]
    for (w, h) in ((65, 64), (100, 70)):
        kinds = ('photo', 'noise', 'white', 'photo')
        write(name(f'rev_{w}x{h}'), w, h, [j2k(picture(w, h, 3 + k, kinds[k]), irreversible=False, **kw) for k, kw in enumerate(rev)], [0] * 4, False, True)
        write(name(f'irr_{w}x{h}'), w, h, [j2k(picture(w, h, 5 + k, kinds[k]), irreversible=True, **kw) for k, kw in enumerate(irr)], [0] * 3, False, False)
    ycc = [jc.ycc_of(picture(48, 40, 9 + k)) for k in range(2)]
    write(name('ycc'), 48, 40, [j2k(ycc[0], irreversible=False, mct=0, num_resolutions=3), j2k(ycc[1], irreversible=False, mct=0)], [0, 0], True, True)
    write(name('tiny'), 1, 1, [j2k(picture(1, 1, 2, 'noise'), irreversible=False, num_resolutions=1)], [0], False, True)
    a = picture(64, 64, 3)
    good = j2k(a, irreversible=False, num_resolutions=3)
    sot = good.index(b'\xff\x90')
    bad = [(j2k(a, irreversible=False, tile_size=(32, 32)), 32), (j2k(np.ascontiguousarray(a[:, :, 0]), irreversible=False), 32),
           (j2k(np.dstack([a, a[:, :, :1]]), irreversible=False), 32), (j2k(a[:, :, 0].astype(np.uint16) * 257, irreversible=False), 32),
           (patched(good, 8, 1), 32), (patched(good, 0, 2), 32), (patched(good, 0, 4), 32),
           (good[:sot + 14 + (len(good) - sot - 14) // 2], 64), (good[:sot + 6] + struct.pack('>I', len(good)) + good[sot + 10:], 64),
           (j2k(picture(96, 64, 3), irreversible=False), 32)]
    for k in range(0, len(bad), 2):
        write(name('refuse'), 64, 64, [good, bad[k][0], bad[k + 1][0], good], [0, bad[k][1], bad[k + 1][1], 0], False, True)
    print(n, 'files in', out)


if __name__ == '__main__':
    main(sys.argv[1])
