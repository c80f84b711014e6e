"""Cost of the UQ calibration data (DESIGN.md section 7 "UQ calibration").  python tools/bench_calibration.py [--out FILE] [--sizes 1000,200000,1600000]

Per table size (1 600 000 rows is BASELINE config 3's cohort-wide table), grid 200: the device entries ``Engine.uq_kde`` and
``Engine.uq_loess`` -- kernel time by the profiling classes' HIP events, and the whole call by the host clock from host arrays
(upload, launch, read-back) -- and the numpy path of ``biscuit_amd/calibration.py`` on the cores this process may use.  One warm-up
call each, then repeats; the median and the spread (min .. max) of the repeats.  profiles/calibration.txt holds what was measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd import calibration                        # noqa: E402
from biscuit_amd.engine import Engine                      # noqa: E402
from biscuit_amd.weights import synthetic_weights          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='1000,200000,1600000')
ap.add_argument('--grid', type=int, default=200)
ap.add_argument('--out')
ap.add_argument('--no-host', action='store_true')
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def spread(ms):
    return f'{statistics.median(ms):10.3f} ms  ({min(ms):.3f} .. {max(ms):.3f}, {len(ms)} calls)'


def host_clock(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
say(f'grid {args.grid}; device {torch.cuda.get_device_name(eng.device)}; host threads {torch.get_num_threads()}, '
    f'cores usable {len(os.sched_getaffinity(0))}')
for n in (int(s) for s in args.sizes.split(',')):
    rng = np.random.default_rng(0)
    x = np.abs(rng.normal(0.05, 0.03, n)).astype(np.float32).astype(np.float64)
    c = rng.random(n) < 1.0 / (1.0 + np.exp(-(0.07 - x) / 0.02))
    reps = 20 if n <= 200000 else 10
    say(f'N = {n}  (chunks of {eng.uq_chunk_rows(n)} rows)')
    for name, fn in (('uq_kde', lambda: eng.uq_kde(x, c, grid=args.grid)), ('uq_loess', lambda: eng.uq_loess(x, c, grid=args.grid))):
        whole = host_clock(fn, reps)
        kern = []
        for _ in range(reps):
            eng.profile_enable(True)
            fn()
            kern.append(sum(p.ms for p in eng.profile_read() if p.name == name))
        eng.profile_enable(False)
        say(f'  {name:9s} kernels {spread(kern)}   whole call {spread(whole)}')
    if not args.no_host:
        hreps = 5 if n <= 200000 else 3
        say(f'  numpy kde      {spread(host_clock(lambda: calibration.kde_host(x, c, grid=args.grid), hreps))}')
        say(f'  numpy loess    {spread(host_clock(lambda: calibration.loess_host(x, c, grid=args.grid), hreps))}')
eng.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
