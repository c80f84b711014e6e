"""Shared by tests/test_jpeg_encode.py (CPU) and tests/test_gpu_jpeg_encode.py: the encoder's inputs (seeded) and Pillow's files
for them, each computed once.

Sizes: 1 and 7 (a lone partial block; at 4:2:0 three dummy luma blocks), 8 (one whole block, dummy blocks to the right and
below), 15 (odd chroma width, partial blocks, no dummies), 16 (exactly one MCU at 4:2:0), 17 (a second MCU one pixel wide: a
dummy column and a dummy row), 33 (odd chroma width 17, dummies) and 299 (the workload: 38 x 38 luma and 19 x 19 chroma blocks)."""
import functools
import io

import numpy as np

SIZES = (1, 7, 8, 15, 16, 17, 33, 299)
QUALITIES = (1, 25, 50, 75, 95, 100)
SUBSAMPLINGS = ('4:2:0', '4:4:4')
CONTENTS = ('zeros', 'grey', 'white', 'noise', 'checker', 'gradient', 'corner', 'synthetic')
BATCH_299 = 3                            # tiles of 299 px in one call, at most


@functools.lru_cache(maxsize=None)
def tile(px, what):
    """uint8 [px, px, 3], read-only."""
    rng = np.random.default_rng(1000 * px + CONTENTS.index(what))
    y, x = np.mgrid[0:px, 0:px]
    if what in ('zeros', 'grey', 'white'):               # EOB only, DC differences of zero
        t = np.full((px, px, 3), {'zeros': 0, 'grey': 128, 'white': 255}[what], np.uint8)
    elif what == 'noise':                                # long codes, many 0xFF bytes to stuff
        t = rng.integers(0, 256, (px, px, 3), dtype=np.uint8)
    elif what == 'checker':                              # 8-pixel black / white blocks: the largest DC categories, both signs
        t = np.repeat((((y // 8) + (x // 8)) % 2 * 255).astype(np.uint8)[..., None], 3, -1)
    elif what == 'gradient':                             # smooth: long zero runs, ZRL
        d = max(2 * px - 2, 1)
        t = np.stack([(y + x) * 255 // d, (y + px - 1 - x) * 200 // d + 20, 255 - (y + x) * 255 // d], -1).astype(np.uint8)
    elif what == 'corner':                               # one bright pixel in the last column and row: edge replication
        t = np.full((px, px, 3), 40, np.uint8)
        t[px - 1, px - 1] = (255, 240, 10)
    else:
        from biscuit_amd.synthetic import make_tiles
        t = make_tiles(1, seed=7, grain=4.0)[0][:px, :px]
    t = np.ascontiguousarray(t)
    t.flags.writeable = False
    return t


def batches(px):
    """The contents of one size as lists of names, one list per encoder call."""
    if px != 299:
        return [list(CONTENTS)]
    return [list(CONTENTS[i:i + BATCH_299]) for i in range(0, len(CONTENTS), BATCH_299)]


@functools.lru_cache(maxsize=None)
def pillow(px, what, quality, subsampling):
    """The file Pillow writes for the tile: the oracle."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(tile(px, what)).save(b, 'JPEG', quality=quality, subsampling=subsampling)
    return b.getvalue()


def pillow_pixels(raw):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)).convert('RGB'))


def settings():
    return [(q, s) for q in QUALITIES for s in SUBSAMPLINGS]


def mixed(n, px=33, seed=5):
    """n tiles of px with different contents: the named ones in turn, every one disturbed by its own noise."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, px, px, 3), np.uint8)
    for i in range(n):
        base = tile(px, CONTENTS[i % len(CONTENTS)]).astype(np.int16)
        out[i] = np.clip(base + rng.integers(-(i % 7) * 6, (i % 7) * 6 + 1, base.shape), 0, 255).astype(np.uint8)
    return out


def split(buf, off):
    """The files of an encoder call as a list of bytes."""
    buf = np.asarray(buf)
    return [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
