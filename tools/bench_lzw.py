"""LZW tile decode, device against host: python tools/bench_lzw.py [--tiles 256] [--launches 5] [--out profiles/lzw_decode.txt]

Three legs, one JSON line each (and the same lines in --out):
  decoder   --tiles resident 256 x 256 tiles (32 distinct pictures, repeated) as libtiff writes them, photo-like with predictor 2 and
            noise with predictor 1, through Engine.lzw_decode_canvas: tiles per second over --launches calls (a warm-up call
            first, three repetitions) and milliseconds per call by stage from bq_profile_*; the host's packing (numpy) beside it;
  host      the same tiles through this library's host decoder (tfrecord_native.lzw_decode_canvas) on 16 threads, and through
            libtiff -- Pillow, every segment wrapped in a one-strip TIFF -- on a pool of 16 worker processes (started before the
            GPU is touched): the comparator, what sixteen host cores deliver with the decoder everyone has;
  slide     Heatmap.from_slide on a synthetic two-level LZW slide (predictor 2) with decode='host' and decode='gpu'.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from biscuit_amd import tfrecord_native as tn   # noqa: E402
from tests import _lzw_cases as lc              # noqa: E402

PX = 256


def pil_decode(page):
    return np.asarray(Image.open(io.BytesIO(page))).shape


def streams(n):
    """name -> (predictor, n LZW segments of PX x PX, 32 distinct pictures repeated)"""
    out = {}
    for name, kind, pred in (('photo_predictor2', 'smooth', 2), ('noise', 'noise', 1)):
        distinct = [lc.libtiff_stream(lc.content(kind, PX, PX, k), pred) for k in range(32)]
        out[name] = (pred, [distinct[i % 32] for i in range(n)])
    return out


def libtiff_processes(tiles, workers=16):
    """name -> tiles/s of libtiff's decode (through Pillow) on a pool of ``workers`` fresh processes (spawned: none inherits a GPU)."""
    import multiprocessing as mp
    rates = {}
    with mp.get_context('spawn').Pool(workers) as pool:
        for name, (pred, raws) in tiles.items():
            pages = [lc.strip_page(r, PX, PX, pred) for r in raws]
            pool.map(pil_decode, pages[:4 * workers], chunksize=4)      # every worker started and warm
            best = 0.0
            for _ in range(3):
                t0 = time.perf_counter()
                pool.map(pil_decode, pages, chunksize=4)
                best = max(best, len(pages) / (time.perf_counter() - t0))
            rates[name] = round(best)
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    tiles = streams(args.tiles)
    process_rates = libtiff_processes(tiles)                 # before the engine exists: the workers never see the GPU
    from biscuit_amd.engine import Engine
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.weights import synthetic_weights
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=64, max_mc=2)
    dev, lines = eng.device, []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    n = args.tiles
    for name, (pred, raws) in tiles.items():
        data = np.frombuffer(b''.join(raws), np.uint8)
        ln = np.array([len(r) for r in raws], np.uint64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
        t0 = time.perf_counter()
        for _ in range(3):
            packed, desc = tn.lzw_pack(data, off, ln)
        pack_s = (time.perf_counter() - t0) / 3
        place = np.array([[(i % 16) * PX, (i // 16) * PX] for i in range(n)], np.int32)
        H, W = -(-n // 16) * PX, 16 * PX
        canvas = torch.full((H, W, 3), 255, dtype=torch.uint8, device=dev)
        up = [torch.from_numpy(x).to(dev) for x in (packed, desc.view(np.int32), place)]
        scratch = eng.lzw_canvas_scratch(n, PX, PX)

        def launch():
            return eng.lzw_decode_canvas(up[0], up[1], PX, PX, up[2], canvas, (0, 0, W, H), predictor=pred, scratch=scratch)
        status = launch()
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        cpu = np.full((H, W, 3), 255, np.uint8)
        host_rates = []
        for _ in range(4):                                                # (the first pass warms the threads' pages)
            t0 = time.perf_counter()
            cpu_status = tn.lzw_decode_canvas(packed, desc, PX, PX, place, cpu, (0, 0, W, H), predictor=pred, threads=16)
            host_rates.append(n / (time.perf_counter() - t0))
        assert not cpu_status.any() and np.array_equal(canvas.cpu().numpy(), cpu)
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                launch()
            b.record()
            torch.cuda.synchronize()
            rates.append(n * args.launches / (a.elapsed_time(b) / 1e3))
        eng.profile_enable(True)
        for _ in range(args.launches):
            launch()
        torch.cuda.synchronize()
        stages = {e.name: round(e.ms / e.launches, 3) for e in eng.profile_read() if e.name.startswith('lzw_')}
        eng.profile_enable(False)
        emit({'leg': 'decoder', 'stream': name, 'predictor': pred, 'tiles': n, 'px': PX, 'bytes_per_tile': int(ln.mean()),
              'device_tiles_per_s': [round(r) for r in rates], 'median_device_tiles_per_s': round(float(np.median(rates))),
              'ms_per_call_by_stage': stages, 'pack_host_ms_per_call': round(pack_s * 1e3, 2)})
        emit({'leg': 'host', 'stream': name, 'tiles': n, 'threads': 16, 'this_library_tiles_per_s': [round(r) for r in host_rates[1:]],
              'median_this_library_tiles_per_s': round(float(np.median(host_rates[1:]))), 'processes': 16,
              'libtiff_tiles_per_s_processes': process_rates[name]})
        del canvas, scratch, up
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        path, _, _ = lc.slide_file(pathlib.Path(tmp), 0.5045, w=2400, h=1800, tile=256, predictor=2, libtiff=True)
        for decode in ('host', 'gpu', 'host', 'gpu'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hm = Heatmap.from_slide(eng, path, decode=decode, mc_n=2, seed=3, batch=16)
            torch.cuda.synchronize()
            emit({'leg': 'slide', 'decode': decode, 'wall_s': round(time.perf_counter() - t0, 3), 'tiles': int(hm.grid.shape[0]),
                  'decode_stats': hm.decode_stats})
    eng.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
