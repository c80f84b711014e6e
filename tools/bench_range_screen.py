"""Cost of the f16 range screen (evaluate(range_screen=True); bq_range_screen).  python tools/bench_range_screen.py [--slides 51
--tiles 1000 --pairs 6]

evaluate() at config 2's shape -- 1 000-tile slides on the device, batch 256, MC 30, f16, one stream, the tile table written --
with the screen off and on, alternated A/B/A/B in this one process; tiles/s per run (host clock around work that ends in a
synchronise), then the median cost of the screen.  51 slides = 199 batches: one interval of the default headroom_every=200, so a
run pays the screen's per-batch kernels and ONE tap of the candidates, the steady state of a long run.  The kernels' own times: run this under
``rocprofv3 --kernel-trace --stats -- python tools/bench_range_screen.py --slides 2 --pairs 1``, separately."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd.engine import EnginePool                 # noqa: E402
from biscuit_amd.inference import Slide, evaluate         # noqa: E402
from biscuit_amd.synthetic import make_tiles              # noqa: E402
from biscuit_amd.weights import synthetic_weights         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--slides', type=int, default=51)
ap.add_argument('--tiles', type=int, default=1000)
ap.add_argument('--pairs', type=int, default=6)
args = ap.parse_args()

w = synthetic_weights(1)
base = torch.from_numpy(make_tiles(64, seed=31, slide_bias=[40.0, -35.0, 25.0], grain=4.0)).cuda()
pool = EnginePool(w, n_streams=1, dtype='f16', max_batch=256, max_mc=30)
slides = []
for s in range(args.slides):
    idx = torch.arange(args.tiles, device='cuda') % 64
    t = base[idx].to(torch.int16) + int((s * 7) % 21 - 10)
    slides.append(Slide(f's{s:02d}', t.clamp_(0, 255).to(torch.uint8).contiguous(), args.tiles, y_true=s % 2))
out = tempfile.mkdtemp(prefix='bench_range_screen_')
try:
    for on in (False, True):                                        # warm-up of both paths
        evaluate(pool, slides[:1], mc_n=30, seed=1, batch=256, keep_tiles=False, save_dir=out, range_screen=on)
    runs = {'off': [], 'on': []}
    n = args.slides * args.tiles
    for rep in range(args.pairs):
        for mode in ('off', 'on'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = evaluate(pool, slides, mc_n=30, seed=1, batch=256, keep_tiles=False, save_dir=out, range_screen=mode == 'on')
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            runs[mode].append(round(n / dt, 1))
            print(json.dumps({'mode': mode, 'rep': rep, 'tiles': n, 's': round(dt, 4), 'tiles_per_s': round(n / dt, 1),
                              'f16_checks': r.f16_checks, 'f16_screen_checks': r.f16_screen_checks, 'f16_screened': r.f16_screened,
                              'f16_screen_headroom': round(r.f16_screen_headroom, 3), 'f16_screen_max_key': r.f16_screen_max_key}),
                  flush=True)
finally:
    shutil.rmtree(out, ignore_errors=True)
    pool.close()
# per pair: the cost of the screen relative to the run without it next to it
rel = [(a - b) / a for a, b in zip(runs['off'], runs['on'])]
print(json.dumps({'evaluate_tiles_per_s': runs, 'median_off': float(np.median(runs['off'])), 'median_on': float(np.median(runs['on'])),
                  'cost_per_pair_pct': [round(100 * x, 3) for x in rel], 'median_cost_pct': round(100 * float(np.median(rel)), 3)}))
