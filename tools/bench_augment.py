"""Measure the training augmentation on an MI355X (DESIGN.md section 7 "Training augmentation"; the record is profiles/augment.txt):

    python tools/bench_augment.py [--out profiles/augment.txt] [--tiles 256] [--launches 20] [--runs 5] [--threads 16]

In one run, on ``--tiles`` resident 299-px tiles (``synthetic.make_tiles(grain=4)``):

* tiles per second of ``Engine.augment`` (``bq_augment``) for four parameter tables -- ``xyr`` only, ``j`` on every tile at quality
  75, ``b`` on every tile at sigma = 2, and the natural ``xyrjb`` draw of ``augment.draw`` --: device events around ``--launches``
  back-to-back calls after a warm-up call, ``--runs`` times, with the per-stage times of the library's profiling classes;
* ``Engine.backbone_u8`` on the same batch, timed the same way, and each table's time as a share of it;
* ``augment.apply_host`` (``bqio_augment``, the same routines on the CPU) on ``--threads`` host threads for the same tables;
* ``train.cache_features`` over a resident synthetic cohort (``--cohort-slides`` x ``--cohort-tiles``) with ``augment='xyrjb'``,
  ``views=1`` against the same call without augmentation, wall clock with a synchronisation at the end, alternating.

Records, not bars.  Prints one JSON line per measurement and writes them, with a header, to ``--out``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from biscuit_amd import augment as A                    # noqa: E402
from biscuit_amd import train as T                      # noqa: E402
from biscuit_amd.engine import Engine                   # noqa: E402
from biscuit_amd.feed import Slide                      # noqa: E402
from biscuit_amd.synthetic import make_tiles            # noqa: E402
from biscuit_amd.weights import synthetic_weights       # noqa: E402


def tables(n, seed):
    xyr = A.draw(n, 'xyr', seed, 0)
    j = np.zeros((n, 4), np.uint8); j[:, 2] = 75
    b = np.zeros((n, 4), np.uint8); b[:, 3] = 4
    return {'xyr': xyr, 'j_q75_all': j, 'b_sigma2_all': b, 'xyrjb_natural': A.draw(n, 'xyrjb', seed, 0)}


def timed(fn, launches, runs):
    """ms per call of ``fn`` by device events: a warm-up call, then ``runs`` windows of ``launches`` back-to-back calls."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return out


def bench_device(eng, tiles, args, emit):
    n = len(tiles)
    d = torch.from_numpy(tiles).to(eng.device)
    out, status = torch.empty_like(d), torch.empty(n, dtype=torch.int32, device=eng.device)
    scratch = eng.augment_scratch(n)
    bb = timed(lambda: eng.backbone_u8(d), args.launches, args.runs)
    bb_ms = float(np.median(bb))
    emit({'measure': 'backbone_u8', 'tiles': n, 'ms_per_call_runs': [round(x, 3) for x in bb], 'ms_per_call_median': round(bb_ms, 3),
          'tiles_per_s': round(n / bb_ms * 1e3)})
    for name, table in tables(n, args.seed).items():
        p = torch.from_numpy(table).to(eng.device)
        call = lambda: eng.augment(d, p, out=out, status=status, scratch=scratch)      # noqa: E731
        want, _ = A.apply_host(tiles[:4], table[:4])
        call()
        assert np.array_equal(out[:4].cpu().numpy(), want) and int(status.abs().sum()) == 0
        ms = timed(call, args.launches, args.runs)
        eng.profile_enable(True)
        for _ in range(args.launches):
            call()
        torch.cuda.synchronize()
        stages = {e.name: round(e.ms / e.launches, 4) for e in eng.profile_read() if e.name.startswith('augment_')}
        eng.profile_enable(False)
        med = float(np.median(ms))
        emit({'measure': 'augment', 'table': name, 'tiles': n, 'jpeg_tiles': int((table[:, 2] > 0).sum()), 'blur_tiles': int((table[:, 3] > 0).sum()),
              'ms_per_call_runs': [round(x, 3) for x in ms], 'ms_per_call_median': round(med, 3), 'tiles_per_s': round(n / med * 1e3),
              'share_of_backbone_u8': round(med / bb_ms, 4), 'ms_per_call_by_stage': stages})


def bench_host(tiles, args, emit):
    for name, table in tables(len(tiles), args.seed).items():
        A.apply_host(tiles[:16], table[:16], threads=args.threads)
        walls = []
        for _ in range(max(args.runs // 2, 2)):
            t0 = time.perf_counter()
            A.apply_host(tiles, table, threads=args.threads)
            walls.append(time.perf_counter() - t0)
        emit({'measure': 'apply_host', 'table': name, 'tiles': len(tiles), 'threads': args.threads, 'wall_s_runs': [round(w, 4) for w in walls],
              'tiles_per_s': round(len(tiles) / float(np.median(walls)))})


def bench_cache(eng, args, emit):
    tiles = make_tiles(args.cohort_tiles, seed=7)
    slides = [Slide(f's{i}', tiles, args.cohort_tiles, y_true=i % 2) for i in range(args.cohort_slides)]
    kinds = {'plain': {}, 'xyrjb_views1': {'augment': 'xyrjb', 'views': 1, 'seed': args.seed}}
    for kw in kinds.values():
        T.cache_features(eng, slides[:2], **kw)
    walls = {k: [] for k in kinds}
    for _ in range(3):
        for k, kw in kinds.items():
            torch.cuda.synchronize(eng.device)
            t0 = time.perf_counter()
            cache = T.cache_features(eng, slides, **kw)
            torch.cuda.synchronize(eng.device)
            walls[k].append(time.perf_counter() - t0)
            del cache
    med = {k: float(np.median(w)) for k, w in walls.items()}
    emit({'measure': 'cache_features', 'slides': args.cohort_slides, 'tiles_per_slide': args.cohort_tiles,
          'wall_s_runs': {k: [round(x, 3) for x in w] for k, w in walls.items()}, 'wall_s_median': {k: round(v, 3) for k, v in med.items()},
          'augmented_over_plain': round(med['xyrjb_views1'] / med['plain'], 3),
          'note': 'resident host tiles, upload included, no decode, no stain normaliser; one view doubles the backbone passes'})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'augment.txt'))
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--cohort-slides', type=int, default=64)
    ap.add_argument('--cohort-tiles', type=int, default=200)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment: no GPU; a CPU run measures nothing')
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
    tiles = make_tiles(args.tiles, seed=args.seed, grain=4.0)
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=max(args.tiles, 256), max_mc=2)
    try:
        bench_device(eng, tiles, args, emit)
        bench_host(tiles, args, emit)
        bench_cache(eng, args, emit)
    finally:
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('Training augmentation (DESIGN.md section 7 "Training augmentation"): python tools/bench_augment.py on one MI355X, f16 engine,\n'
                f'synthetic weights, {args.tiles} resident 299-px tiles, device events around {args.launches} back-to-back calls, {args.runs} windows.\n'
                'Records, not bars.\n\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
