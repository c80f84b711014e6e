"""Cost of the Macenko stain normaliser (bq_stain_macenko).  python tools/bench_macenko.py [--slides 16 --tiles 1000 --reps 2]

1. the normaliser alone: ms per batch of 256 photo-like tiles (HIP events, 20 repetitions after a warm-up);
2. evaluate() on device-resident tiles at config 2 (MC 30, batch 256, f16): no normaliser, reinhard_fast and macenko,
   alternated A/B/C/A/B/C in this one process; tiles/s per run (host clock around work that ends in a synchronise)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd import stain                             # noqa: E402
from biscuit_amd.engine import Engine, EnginePool         # noqa: E402
from biscuit_amd.inference import Slide, evaluate         # noqa: E402
from biscuit_amd.synthetic import make_tiles              # noqa: E402
from biscuit_amd.weights import synthetic_weights         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--slides', type=int, default=16)
ap.add_argument('--tiles', type=int, default=1000)
ap.add_argument('--reps', type=int, default=2)
args = ap.parse_args()

w = synthetic_weights(1)
base = torch.from_numpy(make_tiles(64, seed=31, slide_bias=[40.0, -35.0, 25.0], grain=4.0)).cuda()
big = base.repeat(4, 1, 1, 1).contiguous()                      # 256 tiles
he, mc = stain.MACENKO_HE_REF, stain.MACENKO_MAXC_REF
eng = Engine(w, dtype='f16', max_batch=8, max_mc=2)
out = torch.empty_like(big)
st = torch.empty(256, dtype=torch.int32, device='cuda')
res = {}
for name, fn in (('macenko', lambda: eng.macenko(big, he, mc, out=out, status=st)),
                 ('reinhard_fast', lambda: eng.reinhard_fast(big, [65.0, 12.0, -8.0], [14.0, 7.0, 6.0], out=out))):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        fn()
    b.record()
    b.synchronize()
    res[f'{name}_ms_per_256'] = round(a.elapsed_time(b) / 20, 4)
res['macenko_passthrough_of_256'] = int((st != 0).sum())
print(json.dumps(res), flush=True)
eng.close()

# config 2: tiles resident on the device, each slide its own shift of the 64 base tiles' colours
pool = EnginePool(w, n_streams=1, dtype='f16', max_batch=256, max_mc=30)
slides = []
for s in range(args.slides):
    idx = torch.arange(args.tiles, device='cuda') % 64
    t = base[idx].to(torch.int16) + int((s * 7) % 21 - 10)
    slides.append(Slide(f's{s:02d}', t.clamp_(0, 255).to(torch.uint8).contiguous(), args.tiles, y_true=s % 2))
modes = {'none': dict(norm_fit=None),
         'reinhard_fast': dict(normalizer='reinhard_fast', norm_fit={'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, 6.0]}),
         'macenko': dict(normalizer='macenko', norm_fit={'stain_matrix_target': [list(r) for r in he], 'target_concentrations': list(mc)})}
evaluate(pool, slides[:1], mc_n=30, seed=1, batch=256, keep_tiles=False, **modes['macenko'])       # warm-up
runs = {m: [] for m in modes}
n = args.slides * args.tiles
for rep in range(args.reps):
    for m, kw in modes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = evaluate(pool, slides, mc_n=30, seed=1, batch=256, keep_tiles=False, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        runs[m].append(round(n / dt, 1))
        print(json.dumps({'mode': m, 'rep': rep, 'tiles': n, 's': round(dt, 4), 'tiles_per_s': round(n / dt, 1),
                          'stain_passthrough': r.stain_passthrough}), flush=True)
print(json.dumps({'evaluate_tiles_per_s': runs, **res}))
