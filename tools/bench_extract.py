"""Time tile extraction (``biscuit_amd/extract.py``) and its JPEG and PNG encoders on one GPU.

    python tools/bench_extract.py --out DIR [--img-format jpg|png|both]

1. The encoder alone: ``Engine.jpeg_encode``'s kernels on a resident batch of ``--tiles`` (256) tiles of 299 px -- photo-like
   synthetic tiles, ``synthetic.make_tiles(grain=4)`` -- at the default setting (quality 95, 4:2:0) and at quality 100, 4:4:4:
   device events around ``--launches`` calls of ``bq_jpeg_encode`` into a buffer sized beforehand (no host read in the timed
   region), ``--runs`` times, tiles a second with the per-stage share from ``bq_profile_*``.
2. The host's figure, in the same process on the same tiles: ``tfrecord.encode_image(tile, 'JPEG')`` (Pillow, quality 95, 4:2:0)
   over the batch on ``--threads`` (16) host threads, ``--runs`` times, tiles a second.
3. ``extract_slide`` on the synthetic pyramidal slide ``tools/bench_heatmap.py`` builds (deflate tiles, ``--grid`` cells), wall
   clock per call after one untimed call, with the device time per stage (``bq_profile_*``: tile_resample and the four
   jpeg_encode stages) next to it; what is left of the wall clock is the host: reading and inflating the bands, the uploads, the
   copy of the streams to the host, framing the records.

With ``--img-format png`` (or ``both``, the default) the same three legs for PNG records: ``Engine.png_encode`` on the resident
batch with its four stages (png_encode_filter / _match / _code / _pack) and the bytes per tile next to Pillow's;
``tfrecord.encode_image(tile, 'PNG')`` (Pillow's default, zlib level 6) and Pillow's ``compress_level=1`` on the same host threads;
``extract_slide(img_format='png')``.

One JSON object per line on stdout and in ``DIR/bench_extract.jsonl``."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def encoder_leg(args, eng, tiles, emit):
    import ctypes as C

    import torch
    from biscuit_amd import tfrecord_native as tn
    d = torch.from_numpy(tiles).to(eng.device)
    n, px = tiles.shape[0], tiles.shape[1]
    for quality, sub in ((95, '4:2:0'), (100, '4:4:4')):
        buf, off = eng.jpeg_encode(d, quality, sub)                         # sizes the output; also the warm-up
        cap = int(off[-1])
        want, _, _ = tn.jpeg_encode(tiles[:2], quality, sub)
        assert bytes(buf[:int(off[2])].cpu().numpy()) == want.tobytes()
        out = torch.empty(cap, dtype=torch.uint8, device=eng.device)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
        status = torch.zeros(n, dtype=torch.int32, device=eng.device)
        scratch = eng.jpeg_encode_scratch(n, px, sub)
        ptr = lambda t: C.c_void_p(t.data_ptr())                            # noqa: E731

        def launch():
            eng._check(eng._lib.bq_jpeg_encode(eng._ctx, ptr(d), n, px, quality, tn.jpeg_subsampling(sub), ptr(out), cap, ptr(d_off),
                                               ptr(status), ptr(scratch), scratch.numel(), eng._stream()))
        rates = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                launch()
            b.record()
            torch.cuda.synchronize()
            rates.append(n * args.launches / (a.elapsed_time(b) / 1e3))
        assert int(status.sum()) == 0
        eng.profile_enable(True)
        for _ in range(args.launches):
            launch()
        torch.cuda.synchronize()
        stages = {e.name: round(e.ms / e.launches, 4) for e in eng.profile_read() if e.name.startswith('jpeg_encode')}
        eng.profile_enable(False)
        emit({'leg': 'encoder', 'quality': quality, 'subsampling': sub, 'tiles': n, 'px': px, 'bytes_per_tile': round(cap / n),
              'tiles_per_s': [round(r) for r in rates], 'median_tiles_per_s': round(float(np.median(rates))),
              'ms_per_call_by_stage': stages})


def png_encoder_leg(args, eng, tiles, emit):
    import ctypes as C

    import torch
    from biscuit_amd import tfrecord_native as tn
    d = torch.from_numpy(tiles).to(eng.device)
    n, px = tiles.shape[0], tiles.shape[1]
    buf, off = eng.png_encode(d)                                            # sizes the output; also the warm-up
    cap = int(off[-1])
    want, _, _ = tn.png_encode(tiles[:2])
    assert bytes(buf[:int(off[2])].cpu().numpy()) == want.tobytes()
    out = torch.empty(cap, dtype=torch.uint8, device=eng.device)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
    status = torch.zeros(n, dtype=torch.int32, device=eng.device)
    scratch = eng.png_encode_scratch(n, px)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731

    def launch():
        eng._check(eng._lib.bq_png_encode(eng._ctx, ptr(d), n, px, ptr(out), cap, ptr(d_off), ptr(status), ptr(scratch), scratch.numel(),
                                          eng._stream()))
    rates = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            launch()
        b.record()
        torch.cuda.synchronize()
        rates.append(n * args.launches / (a.elapsed_time(b) / 1e3))
    assert int(status.sum()) == 0
    eng.profile_enable(True)
    for _ in range(args.launches):
        launch()
    torch.cuda.synchronize()
    stages = {e.name: round(e.ms / e.launches, 4) for e in eng.profile_read() if e.name.startswith('png_encode')}
    eng.profile_enable(False)
    emit({'leg': 'png_encoder', 'tiles': n, 'px': px, 'bytes_per_tile': round(cap / n), 'tiles_per_s': [round(r) for r in rates],
          'median_tiles_per_s': round(float(np.median(rates))), 'ms_per_round_by_stage': stages,
          'rounds_per_call': -(-n // 128)})


def png_host_leg(args, tiles, emit):
    import io

    from PIL import Image

    def save(t, **kw):
        b = io.BytesIO()
        Image.fromarray(t).save(b, 'PNG', **kw)
        return b.getbuffer().nbytes
    with ThreadPoolExecutor(args.threads) as pool:
        for name, kw in (('host_pillow_png', {}), ('host_pillow_png_level1', {'compress_level': 1})):
            list(pool.map(lambda t: save(t, **kw), tiles[:args.threads]))                     # warm-up
            rates = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                sizes = list(pool.map(lambda t: save(t, **kw), tiles))
                rates.append(len(tiles) / (time.perf_counter() - t0))
            emit({'leg': name, 'threads': args.threads, 'tiles': len(tiles), 'bytes_per_tile': round(sum(sizes) / len(sizes)),
                  'tiles_per_s': [round(r) for r in rates], 'median_tiles_per_s': round(float(np.median(rates)))})


def host_leg(args, tiles, emit):
    from biscuit_amd import tfrecord as tfr
    rates = []
    with ThreadPoolExecutor(args.threads) as pool:
        list(pool.map(lambda t: tfr.encode_image(t, 'JPEG'), tiles[:args.threads]))          # warm-up
        for _ in range(args.runs):
            t0 = time.perf_counter()
            sizes = list(pool.map(lambda t: len(tfr.encode_image(t, 'JPEG')), tiles))
            rates.append(len(tiles) / (time.perf_counter() - t0))
    emit({'leg': 'host_pillow', 'threads': args.threads, 'tiles': len(tiles), 'bytes_per_tile': round(sum(sizes) / len(sizes)),
          'tiles_per_s': [round(r) for r in rates], 'median_tiles_per_s': round(float(np.median(rates)))})


def slide_leg(args, eng, emit, img_format='jpg'):
    import torch
    from biscuit_amd.extract import extract_slide
    sys.path.insert(0, os.path.join(HERE, 'tools'))
    import bench_heatmap
    gw, gh = (int(v) for v in args.grid.split('x'))
    slide = args.slide or os.path.join(args.out, 'bench_slide.svs')
    if not os.path.exists(slide):
        bench_heatmap.write_slide(slide, gw, gh, args.seed)
    out = os.path.join(args.out, 'tfrecords_' + img_format)
    extract_slide(eng, slide, out, batch=args.batch, img_format=img_format)     # untimed: taps, buffers, the file cache
    walls = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = extract_slide(eng, slide, out, batch=args.batch, img_format=img_format)
        walls.append(time.perf_counter() - t0)
    eng.profile_enable(True)
    extract_slide(eng, slide, out, batch=args.batch, img_format=img_format)
    torch.cuda.synchronize()
    stages = {e.name: round(e.ms, 3) for e in eng.profile_read() if e.name.startswith(('jpeg_encode', 'png_encode', 'tile_'))}
    eng.profile_enable(False)
    emit({'leg': 'extract_slide', 'img_format': img_format, 'grid_shape': s['grid_shape'], 'tiles_written': s['tiles_written'], 'bytes_written': s['bytes_written'],
          'seconds': [round(w, 3) for w in walls], 'median_seconds': round(float(np.median(walls)), 3),
          'tiles_per_s': round(s['tiles_written'] / float(np.median(walls))), 'device_ms_by_stage': stages,
          'device_ms_total': round(sum(stages.values()), 3)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', required=True)
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--grid', default='36x28')
    ap.add_argument('--slide', default=None, help='slide file to generate / reuse (default: OUT/bench_slide.svs)')
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--no-slide', action='store_true', help='the encoder and the host figure only')
    ap.add_argument('--img-format', default='both', choices=['jpg', 'png', 'both'])
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    os.makedirs(args.out, exist_ok=True)
    from biscuit_amd.engine import Engine
    from biscuit_amd.synthetic import make_tiles
    from biscuit_amd.weights import synthetic_weights
    log = open(os.path.join(args.out, 'bench_extract.jsonl'), 'a')

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()
    tiles = make_tiles(args.tiles, seed=args.seed, grain=4.0)
    eng = Engine(synthetic_weights(1), max_batch=8, max_mc=2)              # (no network runs here)
    try:
        for fmt in ('jpg', 'png') if args.img_format == 'both' else (args.img_format,):
            if fmt == 'jpg':
                encoder_leg(args, eng, tiles, emit)
                host_leg(args, tiles, emit)
            else:
                png_encoder_leg(args, eng, tiles, emit)
                png_host_leg(args, tiles, emit)
            if not args.no_slide:
                slide_leg(args, eng, emit, fmt)
    finally:
        eng.close()


if __name__ == '__main__':
    main()
