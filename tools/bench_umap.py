"""Cost of the feature map's stages (DESIGN.md "Feature map (Figure 6)").  python tools/bench_umap.py [--n 10000 --d 2048 --k 50 --epochs 20]

On ``n`` synthetic cluster points of ``d`` columns: the neighbour search (bq_knn, and how many rows it ranked again over all
rows), the membership weights (bq_umap_smooth), the
host's graph assembly, the host's PCA start, ``--epochs`` epochs of the layout (bq_umap_epoch) and the projected end-to-end time
at the map's own number of epochs.  Device stages by HIP events after one warm-up call, host stages by the host clock.  One JSON
line; profiles/umap.txt holds what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd import umap                               # noqa: E402
from biscuit_amd.engine import Engine                      # noqa: E402
from biscuit_amd.weights import synthetic_weights          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=10000)
ap.add_argument('--d', type=int, default=2048)
ap.add_argument('--k', type=int, default=50)
ap.add_argument('--epochs', type=int, default=20)
args = ap.parse_args()

rng = np.random.default_rng(0)
latent = rng.normal(0.0, 4.0, (12, 8))[np.arange(args.n) % 12] + rng.normal(0.0, 1.0, (args.n, 8))
x_host = np.maximum(latent @ (rng.normal(0.0, 1.0, (8, args.d)) / np.sqrt(8.0)), 0.0).astype(np.float32)
eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
x = torch.from_numpy(x_host).to(eng.device)


def device_ms(fn, reps=1):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, out


res = {'n': args.n, 'd': args.d, 'k': args.k}
res['knn_ms'], (idx, dist) = device_ms(lambda: eng.knn(x, args.k))
res['knn_rows_ranked_again'] = int(eng.knn_exhaustive_rows(args.n).sum())      # (the rows the pruning pass could not prove)
res['smooth_ms'], (_, _, w) = device_ms(lambda: eng.umap_smooth(idx, dist), 5)
n_epochs = umap.n_epochs_for(args.n)
t0 = time.perf_counter()
indptr, nbr, eps = umap.fuzzy_graph(idx.cpu().numpy(), w.cpu().numpy(), n_epochs)
res['graph_host_ms'] = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
init = umap.pca_init(x_host)
res['pca_host_ms'] = (time.perf_counter() - t0) * 1e3
a, b = umap.fit_ab(0.1)
graph = umap.graph_to_device(eng, args.n, indptr, nbr, eps)
cur, other = torch.from_numpy(init).to(eng.device), torch.empty((args.n, 2), dtype=torch.float32, device=eng.device)
eng.umap_epoch(cur, graph, 1, 1.0, a, b, 0, out=other)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for ep in range(2, 2 + args.epochs):
    cur, other = other, cur
    eng.umap_epoch(cur, graph, ep, 1.0 - (ep - 1) / n_epochs, a, b, 0, out=other)
ev[1].record()
ev[1].synchronize()
res['epoch_ms'] = ev[0].elapsed_time(ev[1]) / args.epochs
res['edges'] = int(len(nbr))
res['n_epochs'] = n_epochs
res['end_to_end_ms_projected'] = res['knn_ms'] + res['smooth_ms'] + res['graph_host_ms'] + res['pca_host_ms'] + n_epochs * res['epoch_ms']
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
eng.close()
