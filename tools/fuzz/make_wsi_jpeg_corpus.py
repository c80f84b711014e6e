"""Case files for tools/fuzz/wsi_jpeg_fuzz.cpp: python tools/fuzz/make_wsi_jpeg_corpus.py OUTDIR

One file per tiled JPEG page, as a slide reader would hand it to ``bqio_extract_jpeg_segments``: the page's ``JPEGTables`` and its
segments as Pillow writes them (abbreviated or complete streams; 4:4:4 / 4:2:2 / 4:2:0; square, Aperio-sized and rectangular tiles; a
page size that is no multiple of the tile, border tiles padded with 7, not white), and what must come out: the page as Pillow
decodes those streams, or the index of the first segment the extractor has to refuse.  Little-endian uint32 fields:

    'BQSG' seg_w seg_h page_w page_h across n tables_len expect_bad | lengths[n] | tables | segments | page_w * page_h * 3 bytes

``expect_bad`` = 0xFFFFFFFF: every segment decodes and the last field is present; otherwise it is absent."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

NONE = 0xFFFFFFFF


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(xx / 37 + seed), 128 + 80 * np.cos(yy / 29), 128 + 60 * np.sin((xx + yy) / 53)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def jpeg(t, quality=85, **kw):
    b = io.BytesIO()
    Image.fromarray(t).save(b, format='JPEG', quality=quality, **kw)
    return b.getvalue()


def tiles_of(a, tw, th):
    h, w = a.shape[:2]
    for ty in range(-(-h // th)):
        for tx in range(-(-w // tw)):
            t = np.full((th, tw, 3), 7, np.uint8)
            blk = a[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            t[:blk.shape[0], :blk.shape[1]] = blk
            yield t


def pillow_page(w, h, tw, th, tables, segs):
    """The page as a TIFF reader shows it: every segment read as tables-without-EOI + segment-without-SOI, cut to the image."""
    out = np.zeros((h, w, 3), np.uint8)
    across = -(-w // tw)
    for i, sg in enumerate(segs):
        raw = sg
        if tables:
            t = tables[:-2] if tables.endswith(b'\xff\xd9') else tables
            raw = t + (sg[2:] if sg[:2] == b'\xff\xd8' else sg)
        im = np.asarray(Image.open(io.BytesIO(raw)).convert('RGB'))
        ty, tx = divmod(i, across)
        part = im[:min(th, h - ty * th), :min(tw, w - tx * tw)]
        out[ty * th:ty * th + part.shape[0], tx * tw:tx * tw + part.shape[1]] = part
    return out


def write(path, w, h, tw, th, tables, segs, expect_bad=NONE):
    with open(path, 'wb') as f:
        f.write(b'BQSG' + struct.pack('<8I', tw, th, w, h, -(-w // tw), len(segs), len(tables), expect_bad))
        f.write(struct.pack(f'<{len(segs)}I', *[len(s) for s in segs]))
        f.write(tables + b''.join(segs))
        if expect_bad == NONE:
            f.write(pillow_page(w, h, tw, th, tables, segs).tobytes())


def main(out):
    os.makedirs(out, exist_ok=True)
    n = 0

    def name(kind):
        nonlocal n
        n += 1
        return os.path.join(out, f'case{n:02d}_{kind}.bqsg')
    for (w, h, tw, th) in [(40, 23, 16, 16), (100, 70, 64, 64), (500, 300, 240, 240), (600, 420, 256, 128)]:
        a = picture(w, h, 11)
        for ss in (0, 1, 2):
            tables = jpeg(np.zeros((th, tw, 3), np.uint8), subsampling=ss, streamtype=1)
            write(name(f'{tw}x{th}_ss{ss}'), w, h, tw, th, tables, [jpeg(t, subsampling=ss, streamtype=2) for t in tiles_of(a, tw, th)])
    a = picture(200, 150, 12)
    write(name('complete'), 200, 150, 64, 64, b'', [jpeg(t, subsampling=2) for t in tiles_of(a, 64, 64)])
    tables = jpeg(np.zeros((64, 64, 3), np.uint8), subsampling=1, streamtype=1)
    segs = [jpeg(t, subsampling=1, streamtype=2) for t in tiles_of(picture(128, 128, 13), 64, 64)]
    segs[2] = jpeg(picture(64, 64, 14), quality=40, subsampling=1)                # a complete stream with its own quantiser
    write(name('own_tables'), 128, 128, 64, 64, tables, segs)
    t = picture(64, 64, 14)
    tables = jpeg(np.zeros((64, 64, 3), np.uint8), subsampling=2, streamtype=1)
    good = jpeg(t, subsampling=2, streamtype=2)
    for k, (kind, bad) in enumerate([('restart', jpeg(t, subsampling=2, streamtype=2, restart_marker_blocks=2)),
                                     ('rgb', jpeg(t, subsampling=0, keep_rgb=True)), ('grey', jpeg(np.ascontiguousarray(t[:, :, 0]))),
                                     ('progressive', jpeg(t, subsampling=2, progressive=True))]):
        segs = [good] * 4
        segs[k % 4] = bad
        write(name('refuse_' + kind), 128, 128, 64, 64, tables, segs, expect_bad=k % 4)
    # a 256 x 256 frame in a 240 x 240 page
    tables = jpeg(np.zeros((240, 240, 3), np.uint8), subsampling=2, streamtype=1)
    segs = [jpeg(picture(240, 240, 15), subsampling=2, streamtype=2), jpeg(picture(256, 256, 15), subsampling=2, streamtype=2)]
    write(name('refuse_frame'), 480, 240, 240, 240, tables, segs, expect_bad=1)
    print(n, 'files in', out)


if __name__ == '__main__':
    main(sys.argv[1])
