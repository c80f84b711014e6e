"""Time the whole-slide heatmap (``Heatmap.from_slide``) and its input stage on one GPU.

    python tools/bench_heatmap.py --out DIR                      # this tree, the streamed path
    python tools/bench_heatmap.py --out DIR --resample host      # this tree, tiles read and resampled on the host
    python tools/bench_heatmap.py --out DIR --root OTHER_TREE --resample default --no-kernel
                                                                 # another checkout (e.g. the parent commit), its default path

The slide file is generated from ``--seed`` (deflate tiles of 256 px, two pyramid levels, 1 um per pixel: 302 um tiles are 302
level-0 pixels, ``--grid`` cells at stride_div 1) into ``--slide`` once and reused by later calls, so two trees are timed on
the same bytes.  Per ``--stride-div`` value: ``--runs`` timed calls of ``from_slide`` (wall clock around a call that ends with
every result on the host) after one untimed call; the logits / uncertainty arrays are written to ``DIR/arrays_<tag>.npz`` so
that runs of two trees can be compared.  Then (unless ``--no-kernel``) the resample kernel alone at 302 -> 299 and 604 -> 299 and
``Engine.mc_infer`` alone, in tiles a second (device events around 20 launches of one batch).  One JSON object per line on
stdout and in ``DIR/bench_heatmap_<tag>.jsonl``."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_slide(path, gw, gh, seed, tile=256, px=302):
    """A two-level tiled deflate TIFF with an Aperio description (MPP = 1.0): level 0 of gw x gh tiles' worth of pixels plus
    a ragged border, level 1 at a quarter of it.  Smooth colour gradients plus seeded noise, a white margin on the right."""
    w, h = gw * px + 57, gh * px + 31
    rng = np.random.default_rng(seed)

    def level(lw, lh, f):
        segs = []
        xx = np.arange(-(-lw // tile) * tile, dtype=np.float32)[None, :] * f
        for ty in range(-(-lh // tile)):
            yy = (np.arange(tile, dtype=np.float32)[:, None] + ty * tile) * f
            row = np.stack([150 + 70 * np.sin(xx / 211 + seed) + 0 * yy, 110 + 60 * np.cos(yy / 173) + 0 * xx,
                            160 + 50 * np.sin((xx + yy) / 307)], -1)
            row += rng.normal(0, 4, row.shape).astype(np.float32)
            row = np.clip(row, 0, 255).astype(np.uint8)
            row[:, int(0.8 * lw):] = 255
            for tx in range(-(-lw // tile)):
                segs.append(zlib.compress(row[:, tx * tile:(tx + 1) * tile].tobytes(), 1))
        return segs

    with open(path, 'wb') as f:
        f.write(b'II' + struct.pack('<HHHQ', 43, 8, 0, 0))                  # BigTIFF
        ptr_at = 8
        for li, (lw, lh, fac) in enumerate(((w, h, 1.0), (w // 4, h // 4, 4.0))):
            segs = level(lw, lh, fac)
            offs = []
            for s in segs:
                offs.append(f.tell())
                f.write(s)
            desc = (b'Aperio synthetic |MPP = 1.0' if li == 0 else b'level') + b'\0'
            blobs = {}
            for tag, data in ((270, desc), (324, struct.pack(f'<{len(offs)}Q', *offs)), (325, struct.pack(f'<{len(segs)}Q', *map(len, segs))),
                              (258, struct.pack('<3H', 8, 8, 8))):
                blobs[tag] = (f.tell(), data)
                f.write(data + b'\0' * (-len(data) % 8))
            ents = [(256, 4, 1, lw), (257, 4, 1, lh), (258, 3, 3, None), (259, 3, 1, 8), (262, 3, 1, 2), (270, 2, len(desc), None),
                    (277, 3, 1, 3), (284, 3, 1, 1), (322, 4, 1, tile), (323, 4, 1, tile), (324, 16, len(offs), None), (325, 16, len(segs), None)]
            ifd = f.tell()
            f.write(struct.pack('<Q', len(ents)))
            for tag, typ, cnt, val in ents:
                size = {2: 1, 3: 2, 4: 4, 16: 8}[typ] * cnt
                f.write(struct.pack('<HHQ', tag, typ, cnt))
                if val is not None:
                    f.write(struct.pack('<Q', val))
                elif size <= 8:
                    f.write(blobs[tag][1] + b'\0' * (8 - size))
                else:
                    f.write(struct.pack('<Q', blobs[tag][0]))
            nxt = f.tell()
            f.write(struct.pack('<Q', 0))
            f.seek(ptr_at)
            f.write(struct.pack('<Q', ifd))
            f.seek(0, 2)
            ptr_at = nxt
    return w, h


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', required=True)
    ap.add_argument('--root', default=HERE, help='the checkout whose biscuit_amd is timed (default: this one)')
    ap.add_argument('--tag', default=None)
    ap.add_argument('--slide', default=None, help='slide file to generate / reuse (default: OUT/bench_slide.svs)')
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--grid', default='36x28', help='grid cells at stride_div 1 (columns x rows; at least 1 000 cells by default)')
    ap.add_argument('--resample', default='gpu', choices=['gpu', 'host', 'default'], help="'default': pass no resample argument")
    ap.add_argument('--stride-div', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--mc', type=int, default=30)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--no-kernel', action='store_true')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    tag = args.tag or args.resample
    slide = args.slide or os.path.join(args.out, 'bench_slide.svs')
    gw, gh = (int(v) for v in args.grid.lower().split('x'))
    if not os.path.exists(slide):
        t0 = time.perf_counter()
        write_slide(slide, gw, gh, args.seed)
        print(json.dumps({'slide': slide, 'bytes': os.path.getsize(slide), 'written_in_s': round(time.perf_counter() - t0, 2)}), flush=True)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from biscuit_amd.engine import Engine
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.weights import synthetic_weights
    log = open(os.path.join(args.out, f'bench_heatmap_{tag}.jsonl'), 'a')

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=args.batch, max_mc=args.mc)
    kw = dict(mc_n=args.mc, seed=0, batch=args.batch)
    if args.resample != 'default':
        kw['resample'] = args.resample
    arrays = {}
    for sd in args.stride_div:
        times = []
        for r in range(args.runs + 1):                                      # the first call is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hm = Heatmap.from_slide(eng, slide, stride_div=sd, **kw)
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        cells = int(hm.logits.shape[0] * hm.logits.shape[1])
        arrays[f'logits_{sd}'], arrays[f'uncertainty_{sd}'] = hm.logits, hm.uncertainty
        emit({'what': 'from_slide', 'tag': tag, 'root': os.path.abspath(args.root), 'stride_div': sd, 'cells': cells,
              'seconds': [round(t, 4) for t in times], 'median_s': round(float(np.median(times)), 4),
              'spread': round((max(times) - min(times)) / float(np.median(times)), 4), 'tiles_per_s': round(cells / float(np.median(times)), 1)})
    np.savez(os.path.join(args.out, f'arrays_{tag}.npz'), **arrays)
    if not args.no_kernel:
        rng = np.random.default_rng(args.seed)
        n = args.batch

        def rate(fn, reps=20):
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            return n * reps / (a.elapsed_time(b) * 1e-3)

        for src in (302, 604):
            for sdiv in (1, 2):                                             # a band of the grid: sdiv = 2 overlaps the windows
                step, cols = src // sdiv, 16 * sdiv
                rows = -(-n // cols)
                canvas = torch.from_numpy(rng.integers(0, 256, ((rows - 1) * step + src, (cols - 1) * step + src, 3), dtype=np.uint8)).to(eng.device)
                org = np.array([[x * step, y * step] for y in range(rows) for x in range(cols)][:n], np.int32)
                origin = torch.from_numpy(org).to(eng.device)
                out = torch.empty((n, 299, 299, 3), dtype=torch.uint8, device=eng.device)
                emit({'what': 'tile_resample', 'src_px': src, 'stride_div': sdiv, 'batch': n,
                      'tiles_per_s': round(rate(lambda: eng.tile_resample(canvas, origin, src, out=out)), 1)})
        tiles = torch.from_numpy(rng.integers(0, 256, (n, 299, 299, 3), dtype=np.uint8)).to(eng.device)
        emit({'what': 'tile_grayspace', 'batch': n, 'tiles_per_s': round(rate(lambda: eng.tile_grayspace(tiles)), 1)})
        emit({'what': 'mc_infer', 'batch': n, 'mc': args.mc, 'tiles_per_s': round(rate(lambda: eng.mc_infer(tiles, args.mc, 0), reps=10), 1)})
    eng.close()


if __name__ == '__main__':
    main()
