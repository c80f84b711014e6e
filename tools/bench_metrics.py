"""Cost of DeLong's covariance (DESIGN.md section 7 "Prediction metrics").  python tools/bench_metrics.py [--out FILE] [--sizes 1000,200000,1600000]

Per table size (1 600 000 rows is BASELINE config 3's cohort-wide table) and k = 1, 2 classifiers: the device entry
``Engine.delong`` -- kernel time by the profiling class's HIP events, and the whole call by the host clock from host arrays
(upload, launch, read-back) -- and ``metrics.delong_host`` on the cores this process may use.  One warm-up call each, then repeats;
the median and the spread (min .. max) of the repeats.  Last, the bound the measurement gives ``metrics.DEFAULT_MIN_ROWS``: the
smallest measured n at which the whole device call is faster than the host call at k = 1.  profiles/metrics.txt holds what was
measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd import metrics                            # noqa: E402
from biscuit_amd.engine import Engine                      # noqa: E402
from biscuit_amd.weights import synthetic_weights          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='1000,200000,1600000')
ap.add_argument('--out')
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
say(f'device {torch.cuda.get_device_name(eng.device)}; host threads {torch.get_num_threads()}, cores usable {len(os.sched_getaffinity(0))}')
wins = []
for n in (int(s) for s in args.sizes.split(',')):
    rng = np.random.default_rng(0)
    y = (rng.random(n) < 0.4).astype(np.int64)
    P = (0.4 + 0.2 * y[None, :] + 0.25 * rng.normal(size=(2, n))).astype(np.float32).astype(np.float64)      # a tile table's y_pred: float32 values
    reps = 20 if n <= 200000 else 10
    say(f'N = {n}  (chunks of {eng.delong_chunk_rows(n)} rows)')
    for k in (1, 2):
        S = P[:k]
        whole = host_clock(lambda: eng.delong(y, S), reps)
        kern = []
        for _ in range(reps):
            eng.profile_enable(True)
            eng.delong(y, S)
            kern.append(sum(p.ms for p in eng.profile_read() if p.name == 'delong'))
        eng.profile_enable(False)
        host = host_clock(lambda: metrics.delong_host(y, S), 10)
        say(f'  k = {k}  kernels {spread(kern)}   whole call {spread(whole)}   delong_host {spread(host)}')
        if k == 1 and statistics.median(whole) < statistics.median(host):
            wins.append(n)
eng.close()
say(f'DEFAULT_MIN_ROWS by the rule (smallest measured n where the whole device call beats delong_host at k = 1): {min(wins) if wins else "none -- the device never wins at k = 1"}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
