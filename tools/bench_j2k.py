"""JPEG 2000 tile decode, device against host: python tools/bench_j2k.py [--tiles 256] [--launches 5] [--out profiles/j2k_decode.txt]

Three legs, one JSON line each (and the same lines in --out):
  decoder   --tiles resident 256 x 256 tiles (32 distinct pictures, repeated), reversible and irreversible at about 10:1, through
            Engine.j2k_decode_canvas: tiles per second over --launches calls, milliseconds per call by stage from bq_profile_*,
            and the host's share -- tier 2 (tfrecord_native.j2k_extract) on the process's threads;
  pillow    the same tiles through Pillow's OpenJPEG: on a 16-thread pool of this process -- what a Python caller gets without more
            ado, and a ONE-CORE figure, since Pillow's JPEG 2000 decoder holds the interpreter lock while it decodes -- and on a
            pool of 16 worker processes (started before the GPU is touched), which is what sixteen host cores deliver;
  slide     Heatmap.from_slide on a synthetic two-level JPEG 2000 slide (reversible tiles) with decode='host' and decode='gpu'.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from biscuit_amd import tfrecord_native as tn   # noqa: E402
from tests import _j2k_cases as jc              # noqa: E402


def pil_decode(raw):
    return np.asarray(Image.open(io.BytesIO(raw))).shape


def streams(n, px=256):
    """name -> n codestreams of px x px (32 distinct pictures, repeated), 6 resolutions, MCT on."""
    pictures = [jc.content('photo', px, px, k) for k in range(32)]
    out = {}
    for name, kw in (('reversible', dict(irreversible=False)), ('irreversible_10to1', dict(irreversible=True, quality_mode='rates', quality_layers=[10]))):
        distinct = [jc.j2k(a, num_resolutions=6, mct=1, **kw) for a in pictures]
        out[name] = [distinct[i % 32] for i in range(n)]
    return out


def pillow_processes(tiles, workers=16):
    """name -> tiles/s of Pillow's decode on a pool of ``workers`` fresh processes (spawned: none of them inherits a GPU)."""
    import multiprocessing as mp
    rates = {}
    with mp.get_context('spawn').Pool(workers) as pool:
        for name, raws in tiles.items():
            pool.map(pil_decode, raws[:4 * workers], chunksize=4)       # every worker started and warm
            t0 = time.perf_counter()
            pool.map(pil_decode, raws, chunksize=4)
            rates[name] = round(len(raws) / (time.perf_counter() - t0))
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    tiles = streams(args.tiles)
    process_rates = pillow_processes(tiles)                  # before the engine exists: the workers never see the GPU
    from biscuit_amd.engine import Engine
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.weights import synthetic_weights
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=64, max_mc=2)
    dev, lines = eng.device, []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    n, px = args.tiles, 256
    for name, raws in tiles.items():
        data = np.frombuffer(b''.join(raws), np.uint8)
        ln = np.array([len(r) for r in raws], np.uint64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
        t0 = time.perf_counter()
        for _ in range(3):
            desc, blocks, cw = tn.j2k_extract(data, off, ln, px, px)
        tier2 = (time.perf_counter() - t0) / 3
        place = np.array([[(i % 16) * px, (i // 16) * px] for i in range(n)], np.int32)
        H, W = -(-n // 16) * px, 16 * px
        canvas = torch.full((H, W, 3), 255, dtype=torch.uint8, device=dev)
        up = [torch.from_numpy(x).to(dev) for x in (desc, blocks, cw, place)]
        scratch = eng.j2k_canvas_scratch(n, px, px)

        def launch():
            return eng.j2k_decode_canvas(up[0], up[1], up[2], px, px, up[3], canvas, (0, 0, W, H), scratch=scratch)
        status = launch()
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        cpu = np.full((px, px, 3), 255, np.uint8)
        one = tn.j2k_extract(data[:int(ln[0])], [0], ln[:1], px, px)
        tn.j2k_decode_canvas(*one, px, px, [[0, 0]], cpu, (0, 0, px, px))
        assert np.array_equal(canvas[:px, :px].cpu().numpy(), cpu)
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
        stages = {e.name: round(e.ms / e.launches, 3) for e in eng.profile_read() if e.name.startswith('j2k_')}
        eng.profile_enable(False)
        emit({'leg': 'decoder', 'stream': name, 'tiles': n, 'px': px, 'bytes_per_tile': int(ln.mean()), 'code_blocks': int(len(blocks)),
              'device_tiles_per_s': [round(r) for r in rates], 'median_device_tiles_per_s': round(float(np.median(rates))),
              'ms_per_call_by_stage': stages, 'tier2_host_ms_per_call': round(tier2 * 1e3, 2), 'tier2_tiles_per_s': round(n / tier2),
              'host_threads': tn.default_threads()})

        with ThreadPoolExecutor(16) as pool:
            list(pool.map(pil_decode, raws[:16]))
            t0 = time.perf_counter()
            list(pool.map(pil_decode, raws))
            wall = time.perf_counter() - t0
        emit({'leg': 'pillow', 'stream': name, 'tiles': n, 'threads_one_process': 16, 'tiles_per_s_threads': round(n / wall),
              'processes': 16, 'tiles_per_s_processes': process_rates[name]})
        del canvas, scratch, up
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        path, _, _ = jc.slide_file(pathlib.Path(tmp), 0.5045, w=2400, h=1800, tile=256, num_resolutions=6, mct=1)
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
