"""The device JPEG decoder (``Engine.jpeg_decode``, csrc/kernels_jpeg.hip) measured: the kernels alone on 16 / 32 decode CUs and on
the whole chip, and ``evaluate()`` over JPEG TFRecords end to end.  profiles/jpeg_decode.txt holds the results.

    python tools/bench_jpeg_decode.py kernel [--tiles 4096] [--cus 16 32 0] [--quality 75 95 100] [--sampling 0 2]
    python tools/bench_jpeg_decode.py e2e [--root DIR] [--reserve 0|16|32] [--slides 64] [--per 1024] [--quality 95] [--sampling 0]

``e2e --reserve 0`` is the host decoder (what a tree without the device path does); ``--root DIR`` imports ``biscuit_amd`` from
another checkout (built), so that the parent commit's ``evaluate()`` runs over the same files on the same box.  One measurement
per process: alternate the processes and take medians.  Under ``rocprofv3 --kernel-trace --stats -- python tools/... kernel``
the entropy and pixel kernels show separately.
"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np


def jpeg_tiles(n_base, quality, sampling):
    from PIL import Image
    from biscuit_amd.synthetic import make_tiles
    out = []
    for t in make_tiles(n_base, seed=21, grain=4.0):                 # photograph-like
        b = io.BytesIO()
        Image.fromarray(t).save(b, format='JPEG', quality=quality, subsampling=sampling)
        out.append(b.getvalue())
    return out


def kernel(args):
    import torch
    from biscuit_amd import tfrecord, tfrecord_native as tn
    from biscuit_amd.engine import EnginePool
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    d = tempfile.mkdtemp(prefix='bq_jd_')
    try:
        for cus in args.cus:
            pool = EnginePool(w, n_streams=1, reserve_cus=cus, decode_streams=1, dtype='f16', max_batch=8, max_mc=2)
            eng = pool.engines[0]
            stream = pool.decode_streams[0] if cus else torch.cuda.current_stream()
            for q in args.quality:
                for ss in args.sampling:
                    base = jpeg_tiles(32, q, ss)
                    p = os.path.join(d, 'k.tfrecords')
                    tfrecord.write_slide(p, 'k', [base[i % 32] for i in range(args.tiles)], np.zeros((args.tiles, 2), np.int64))
                    with tn.NativeReader(p) as r:
                        used, nt, _ = r.extract_jpeg(0, args.tiles, 299, None, None, None)
                        scan, desc = np.zeros(used, np.uint8), np.zeros((args.tiles, 4), np.uint32)
                        tables = np.zeros((nt, tn.jpeg_table_bytes()), np.uint8)
                        t0 = time.perf_counter()
                        r.extract_jpeg(0, args.tiles, 299, scan, desc, tables)
                        t_ex = time.perf_counter() - t0
                    dev = [torch.from_numpy(a).cuda() for a in (scan, desc.view(np.int32), tables)]
                    ms = []
                    with torch.cuda.stream(stream):
                        scratch = eng.jpeg_scratch(args.tiles, 299)
                        for _ in range(args.reps + 1):
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record(stream)
                            _, status = eng.jpeg_decode(*dev, 299, scratch=scratch)
                            b.record(stream)
                            b.synchronize()
                            ms.append(a.elapsed_time(b))
                    assert not status.cpu().numpy().any()
                    med = sorted(ms[1:])[len(ms[1:]) // 2]
                    print(json.dumps({'mode': 'kernel', 'cus': cus or 'all', 'quality': q, 'sampling': {0: '4:4:4', 1: '4:2:2', 2: '4:2:0'}[ss],
                                      'tiles': args.tiles, 'bytes_per_tile': int(np.mean([len(x) for x in base])), 'ms': round(med, 2),
                                      'tiles_per_s': round(args.tiles / med * 1e3), 'host_extract_tiles_per_s': round(args.tiles / t_ex),
                                      'host_threads': tn.default_threads()}), flush=True)
            pool.synchronize(); pool.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def e2e(args):
    from biscuit_amd import tfrecord, tfrecord_native as tn
    from biscuit_amd.engine import EnginePool
    from biscuit_amd.inference import evaluate, slides_from_tfrecords
    from biscuit_amd.weights import synthetic_weights
    w = synthetic_weights(1)
    n = args.slides * args.per
    d = tempfile.mkdtemp(prefix='bq_je_')
    try:
        base = jpeg_tiles(32, args.quality[0], args.sampling[0])
        paths = []
        for s in range(args.slides):
            p = os.path.join(d, f'j{s}.tfrecords')
            if s < 8:
                tfrecord.write_slide(p, f'j{s}', [base[(i + s) % 32] for i in range(args.per)], np.zeros((args.per, 2), np.int64))
            else:
                os.symlink(os.path.join(d, f'j{s % 8}.tfrecords'), p)          # (the same bytes again: the page cache holds 8 files)
            paths.append(p)
        lab = {f'j{s}': s % 2 for s in range(args.slides)}
        rc = args.reserve
        pool = EnginePool(w, n_streams=1, dtype='f16', max_batch=256, max_mc=args.mc, **({'reserve_cus': rc, 'decode_streams': 2} if rc else {}))
        batch = (256 - rc) // 16 * 16
        slides = slides_from_tfrecords(paths, lab, **({'gpu_decode': True} if rc else {}))
        evaluate(pool, slides[:8], mc_n=args.mc, seed=1, batch=batch, keep_tiles=False)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = evaluate(pool, slides, mc_n=args.mc, seed=1, batch=batch, keep_tiles=False)
            ts.append(time.perf_counter() - t0)
        pool.synchronize(); pool.close()
        print(json.dumps({'mode': 'e2e', 'root': args.root or '.', 'decode': f'device, {rc} CUs' if rc else 'host', 'tiles': n,
                          'quality': args.quality[0], 'sampling': args.sampling[0], 'host_threads': tn.default_threads(),
                          'tiles_per_s': round(n / sorted(ts)[len(ts) // 2]), 'runs_s': [round(t, 3) for t in ts],
                          'slide_pred_sum': float(np.nansum(r.slide_pred))}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'e2e'])
    ap.add_argument('--root', help='import biscuit_amd from this checkout instead of the one this file lies in')
    ap.add_argument('--tiles', type=int, default=4096)
    ap.add_argument('--cus', type=int, nargs='*', default=[16, 32, 0], help='decode CUs (0: the whole chip)')
    ap.add_argument('--quality', type=int, nargs='*', default=[75, 95, 100])
    ap.add_argument('--sampling', type=int, nargs='*', default=[0, 2], help='Pillow subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0')
    ap.add_argument('--reserve', type=int, default=16)
    ap.add_argument('--slides', type=int, default=64)
    ap.add_argument('--per', type=int, default=1024)
    ap.add_argument('--mc', type=int, default=30)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    (kernel if args.mode == 'kernel' else e2e)(args)


if __name__ == '__main__':
    main()
