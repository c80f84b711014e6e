"""Measure head training on an MI355X (DESIGN.md section 7 "Head training"; the record is profiles/train_head.txt):

    python tools/bench_train.py [--steps 200] [--batch 128] [--cache-slides 8] [--cache-tiles 512] [--cv-slides 64] [--cv-tiles 200]

* microseconds per training step at the given batch (wall time of ``Engine.head_train_steps`` over ``--steps`` steps after a warm-up
  call, one synchronisation at the end), and the split between the launches from the library's own profiling classes;
* one validation check of 32 x batch rows in the middle of a training (``Engine.head_validate``), the same rows through
  ``train.head_engine`` + ``mc_head`` -- the only way to score a head before it --, and the share a check adds to 32 steps;
* the feature-cache rate: ``train.cache_features`` over resident synthetic slides, tiles per second (host decode is not part of it:
  the tiles are in memory, as in ``bench.py``);
* wall time of ``train_nested_cv`` (3 x (1 + 5) trainings with their validation tables) and ``thresholds_from_nested_cv`` over a
  synthetic cohort of cached features.

Records, not bars: nothing of the kind exists to compare with.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from biscuit_amd import train as T                      # noqa: E402
from biscuit_amd.engine import Engine                   # noqa: E402
from biscuit_amd.feed import Slide                      # noqa: E402
from biscuit_amd.synthetic import make_tiles            # noqa: E402
from biscuit_amd.weights import synthetic_weights       # noqa: E402


def bench_steps(eng, steps, batch):
    dev = eng.device
    rng = np.random.default_rng(1)
    feats = torch.from_numpy(np.abs(rng.standard_normal((8192, 2048))).astype(np.float32)).to(dev)
    rows = torch.from_numpy(rng.integers(0, 8192, steps * batch)).to(dev)
    labels = torch.from_numpy(rng.integers(0, 2, steps * batch).astype(np.uint8)).to(dev)
    w = torch.from_numpy(T.flatten_head(T.glorot_head(1))).to(dev)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    lr = [1e-4] * steps
    eng.head_train_steps(w, m, v, feats, rows, labels, batch, 0, 1, lr)
    torch.cuda.synchronize(dev)
    walls = []
    for r in range(3):
        t0 = time.perf_counter()
        eng.head_train_steps(w, m, v, feats, rows, labels, batch, (r + 1) * steps, 1, lr)
        torch.cuda.synchronize(dev)
        walls.append((time.perf_counter() - t0) / steps * 1e6)
    eng.profile_enable(True)
    eng.head_train_steps(w, m, v, feats, rows, labels, batch, 4 * steps, 1, lr)
    torch.cuda.synchronize(dev)
    split = {p.name: round(p.ms / max(p.launches, 1) * 1e3, 2) for p in eng.profile_read() if p.name.startswith('head_train_')}
    eng.profile_enable(False)
    grad = sum(us for name, us in split.items() if name != 'head_train_adam')
    return {'measure': 'train_step', 'batch': batch, 'steps': steps, 'us_per_step_wall_median': round(float(np.median(walls)), 1),
            'us_per_step_wall_runs': [round(x, 1) for x in walls], 'us_per_launch_by_class': split, 'us_grad_launches': round(grad, 1),
            'us_adam_launch': split.get('head_train_adam')}


def bench_validate(eng, batch, val_steps=32, window=32, repeats=20):
    """One validation check of ``val_steps * batch`` rows through ``Engine.head_validate`` (the 16 bytes read back, as ``fit_head``
    does), the same rows through the only route there was before it -- ``train.head_engine`` + ``mc_head`` with one pass, the engine's
    construction included --, and what a check adds to a window of ``window`` training steps."""
    dev = eng.device
    n = val_steps * batch
    rng = np.random.default_rng(2)
    feats = torch.from_numpy(np.abs(rng.standard_normal((8192, 2048))).astype(np.float32)).to(dev)
    rows = torch.from_numpy(rng.permutation(8192)[:n].astype(np.int64)).to(dev)
    labels = torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).to(dev)
    head = T.glorot_head(1)
    w = torch.from_numpy(T.flatten_head(head)).to(dev)
    check = lambda: eng.head_validate(w, feats, rows, labels, 7, 1, rate=0.0)[0].cpu()
    check()
    walls = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        check()
        walls.append((time.perf_counter() - t0) * 1e6)
    eng.profile_enable(True)
    check()
    split = {p.name: round(p.ms / max(p.launches, 1) * 1e3, 2) for p in eng.profile_read() if p.name.startswith('head_validate_')}
    eng.profile_enable(False)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    train_rows, train_labels, lr = rows[:window * batch].contiguous(), labels[:window * batch].contiguous(), [1e-4] * window
    eng.head_train_steps(w.clone(), m, v, feats, train_rows, train_labels, batch, 0, 1, lr)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    eng.head_train_steps(w.clone(), m, v, feats, train_rows, train_labels, batch, window, 1, lr)
    torch.cuda.synchronize(dev)
    window_us = (time.perf_counter() - t0) * 1e6
    old = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        other = T.head_engine(eng, head)
        try:
            for a in range(0, n, other.max_batch):
                r = rows[a:a + other.max_batch].contiguous()
                mean, _ = other.mc_head(feats.index_select(0, r).contiguous(), 1, 1, tile_idx0=0, tile_idx=r)
                mean.cpu()
        finally:
            other.close()
        old.append((time.perf_counter() - t0) * 1e6)
    us = float(np.median(walls))
    return {'measure': 'validation_check', 'rows': n, 'batch': batch, 'us_head_validate_wall_median': round(us, 1),
            'us_head_validate_wall_min_max': [round(min(walls), 1), round(max(walls), 1)], 'us_per_launch_by_class': split,
            'us_head_engine_mc_head_wall_median': round(float(np.median(old)), 1), 'us_head_engine_mc_head_runs': [round(x, 1) for x in old],
            'window_steps': window, 'us_window_wall': round(window_us, 1), 'check_share_of_window_and_check': round(us / (us + window_us), 3)}


def bench_cache(eng, n_slides, n_tiles):
    tiles = make_tiles(n_tiles, seed=7)
    slides = [Slide(f's{i}', tiles, n_tiles, y_true=i % 2) for i in range(n_slides)]
    T.cache_features(eng, slides[:1])
    torch.cuda.synchronize(eng.device)
    t0 = time.perf_counter()
    cache = T.cache_features(eng, slides)
    torch.cuda.synchronize(eng.device)
    wall = time.perf_counter() - t0
    return {'measure': 'feature_cache', 'slides': n_slides, 'tiles': len(cache), 'wall_s': round(wall, 3),
            'tiles_per_s': round(len(cache) / wall, 1), 'note': 'resident host tiles, upload included, no decode, no stain normaliser'}


def bench_cv(eng, n_slides, n_tiles, mc_n):
    rng = np.random.default_rng(3)
    slides = [f's{i:03d}' for i in range(n_slides)]
    labels = {s: i % 2 for i, s in enumerate(slides)}
    sidx = np.repeat(np.arange(n_slides), n_tiles).astype(np.int64)
    f = np.abs(rng.standard_normal((len(sidx), 2048))).astype(np.float32)
    f[sidx % 2 == 1] += np.float32(0.05) * (np.arange(2048) % 2 == 0)
    loc = np.stack([np.arange(len(sidx)), np.zeros(len(sidx), np.int64)], 1).astype(np.int64)
    cache = T.FeatureCache(torch.from_numpy(f).to(eng.device), sidx, loc, slides)
    trainer = T.HeadTrainer(eng, cache, labels, init='glorot', mc_n=mc_n)
    with tempfile.TemporaryDirectory() as out:
        t0 = time.perf_counter()
        dirs = T.train_nested_cv(cache, labels, out, 'EXP', trainer, outer_k=3, inner_k=5, seed=1)
        torch.cuda.synchronize(eng.device)
        t_train = time.perf_counter() - t0
        t0 = time.perf_counter()
        try:
            _, th = T.thresholds_from_nested_cv(out, 'EXP', outer_k=3, inner_k=5)
            th = {k: (None if v is None else float(v)) for k, v in th.items()}
        except Exception as e:                                  # noqa: BLE001 -- a record of what happened, not a test
            th = repr(e)
        t_th = time.perf_counter() - t0
    return {'measure': 'nested_cv', 'slides': n_slides, 'tiles_per_slide': n_tiles, 'trainings': len(dirs), 'mc_n': mc_n,
            'steps_total': int(sum(len(x) for x in trainer.losses)), 'train_and_tables_wall_s': round(t_train, 2),
            'thresholds_wall_s': round(t_th, 2), 'thresholds': th}


# the share of these figures that ``--exit`` reports (profiles/train_exit.txt): the MI355X's f32 matrix peak and HBM bandwidth
F32_MATRIX_PEAK, HBM_BYTES_PER_S = 157.3e12, 8.0e12
EXIT_GEMMS = ('pw1', 'pw2', 'dp1', 'du1', 'dp2', 'du2', 'dfeat')
EXIT_DEPTHWISE = ('dw1', 'dw2', 'dd1', 'dd2', 'dh1')
EXIT_BN = ('stat1', 'stat2', 'bnfix1', 'bnfix2', 'bnmove')            # what --bn batch adds to a step


def bench_exit_steps(eng, steps, batch, tiles=512, store='f32', bn='frozen'):
    """One exit-flow training step (``Engine.exit_train_steps``: block 14 and the head under one Adam) at ``batch``: wall time per
    step, the library's time per launch class, and from each class's own flop and byte counts the GEMMs' share of the f32 matrix
    peak and the depthwise kernels' share of the HBM bandwidth.  ``store`` (``--act-cache``): the cache as float32 on the device,
    as the engine's 16-bit type there (``packed``), or that in pinned host memory (``host``: the gather's time and rate beside it).
    ``bn`` (``--bn``): 'batch' measures the training-mode step -- the statistics, the two in-place passes over dz and the moving
    update beside the frozen step's launches -- and reports their classes' share of the HBM bandwidth as well."""
    dev = eng.device
    rng = np.random.default_rng(1)
    acts = torch.rand((tiles,) + eng.EXIT_ACT_SHAPE, dtype=torch.float32, device=dev)
    if store != 'f32':
        acts = acts.to(eng._elt)
    if store == 'host':
        acts = torch.empty(acts.shape, dtype=acts.dtype, pin_memory=True).copy_(acts)
    rows = torch.from_numpy(rng.integers(0, tiles, steps * batch)).to(dev)
    labels = torch.from_numpy(rng.integers(0, 2, steps * batch).astype(np.uint8)).to(dev)
    w = torch.from_numpy(np.concatenate([T.flatten_exit(eng.weights), T.flatten_head(T.glorot_head(1))])).to(dev)
    stats = torch.from_numpy(T.exit_bn_stats(eng.weights)).to(dev)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    lr = [1e-4] * steps
    eng.exit_train_steps(w, m, v, stats, acts, rows, labels, batch, 0, 1, lr, bn=bn)
    torch.cuda.synchronize(dev)
    walls, extra = [], {}
    for r in range(3):
        t0 = time.perf_counter()
        eng.exit_train_steps(w, m, v, stats, acts, rows, labels, batch, (r + 1) * steps, 1, lr, bn=bn)
        torch.cuda.synchronize(dev)
        walls.append((time.perf_counter() - t0) / steps * 1e6)
    eng.profile_enable(True)
    eng.exit_train_steps(w, m, v, stats, acts, rows, labels, batch, 4 * steps, 1, lr, bn=bn)
    torch.cuda.synchronize(dev)
    prof = {p.name: p for p in eng.profile_read() if p.name.startswith(('exit_train_', 'head_train_', 'exit_gather'))}
    eng.profile_enable(False)
    us = {name: round(p.ms / max(p.launches, 1) * 1e3, 2) for name, p in prof.items()}
    per_s = lambda p: p.ms / max(p.launches, 1) * 1e-3
    peak = {k: round(prof['exit_train_' + k].flops / per_s(prof['exit_train_' + k]) / F32_MATRIX_PEAK, 3) for k in EXIT_GEMMS}
    hbm = {k: round(prof['exit_train_' + k].bytes / per_s(prof['exit_train_' + k]) / HBM_BYTES_PER_S, 3) for k in EXIT_DEPTHWISE}
    if bn == 'batch':
        extra = {'bn_us_per_step': round(sum(us['exit_train_' + k] for k in EXIT_BN), 1),
                 'bn_share_of_hbm_bandwidth': {k: round(prof['exit_train_' + k].bytes / per_s(prof['exit_train_' + k]) / HBM_BYTES_PER_S, 3)
                                               for k in EXIT_BN[:4]}}
    if store == 'host':          # the gather's class counts the bytes it reads and writes: half of them cross the link
        g = prof['exit_gather']
        extra.update({'gather_GB_per_s_over_the_link': round(g.bytes / 2 / per_s(g) / 1e9, 1),
                      'gather_share_of_step': round(us['exit_gather'] / float(np.median(walls)), 3)})
    return {'measure': 'exit_train_step', 'act_cache': store, 'bn': bn, **extra, 'batch': batch, 'steps': steps,
            'us_per_step_wall_median': round(float(np.median(walls)), 1),
            'us_per_step_wall_runs': [round(x, 1) for x in walls], 'us_per_launch_by_class': us, 'us_launches_total': round(sum(us.values()), 1),
            'gemm_share_of_f32_matrix_peak': peak, 'depthwise_share_of_hbm_bandwidth': hbm,
            'workspace_MB': round((eng._exit_bn_need(batch, acts.dtype if store == 'host' else None) if bn == 'batch' else
                                   eng._exit_need(True, batch, acts.dtype if store == 'host' else None)) / 1e6, 1)}


def bench_trunk(eng, batch=256, repeats=9):
    """Cache construction's device call at ``batch``: ``Engine.trunk`` against ``Engine.trunk(packed=True)``, which leaves out the
    widening copy and the scale pass -- the median of ``repeats`` event-timed calls of each, taken in turns."""
    tiles = torch.randint(0, 256, (batch, 299, 299, 3), dtype=torch.uint8, device=eng.device)
    ms = {False: [], True: []}
    for r in range(repeats + 2):
        for packed in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.trunk(tiles, packed=packed)
            b.record()
            b.synchronize()
            if r >= 2:
                ms[packed].append(a.elapsed_time(b))
    return {'measure': 'trunk', 'batch': batch, 'trunk_ms_median': round(float(np.median(ms[False])), 3),
            'trunk_packed_ms_median': round(float(np.median(ms[True])), 3)}


def bench_exit_cv(eng, n_slides, n_tiles, mc_n, batch):
    """Wall time of a toy ``train_nested_cv`` with ``trainable='exit'`` over a synthetic activation cache (3 x (1 + 2) trainings)."""
    rng = np.random.default_rng(3)
    slides = [f's{i:03d}' for i in range(n_slides)]
    labels = {s: i % 2 for i, s in enumerate(slides)}
    sidx = np.repeat(np.arange(n_slides), n_tiles).astype(np.int64)
    acts = torch.rand((len(sidx),) + eng.EXIT_ACT_SHAPE, dtype=torch.float32, device=eng.device)
    acts[torch.from_numpy(sidx % 2 == 1).to(eng.device)] += 0.05
    loc = np.stack([np.arange(len(sidx)), np.zeros(len(sidx), np.int64)], 1).astype(np.int64)
    e, stats = (torch.from_numpy(a).to(eng.device) for a in (T.flatten_exit(eng.weights), T.exit_bn_stats(eng.weights)))
    feats = eng.exit_features_all(e, stats, acts, torch.arange(len(sidx), device=eng.device))
    cache = T.ActivationCache(feats, sidx, loc, slides, acts=acts)
    trainer = T.HeadTrainer(eng, cache, labels, params=T.TrainParams(batch_size=batch, trainable='exit'), init='glorot', mc_n=mc_n)
    with tempfile.TemporaryDirectory() as out:
        t0 = time.perf_counter()
        dirs = T.train_nested_cv(cache, labels, out, 'EXP', trainer, outer_k=3, inner_k=2, seed=1)
        torch.cuda.synchronize(eng.device)
        wall = time.perf_counter() - t0
    return {'measure': 'exit_nested_cv', 'slides': n_slides, 'tiles_per_slide': n_tiles, 'trainings': len(dirs), 'mc_n': mc_n, 'batch': batch,
            'steps_total': int(sum(len(x) for x in trainer.losses)), 'train_and_tables_wall_s': round(wall, 2),
            'activation_cache_MB': round(T.activation_cache_bytes(len(sidx)) / 1e6, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--exit', action='store_true', help="measure exit-flow fine-tuning (trainable='exit') instead: one step at --batch, "
                    'and a toy nested CV (profiles/train_exit.txt)')
    ap.add_argument('--act-cache', default='f32', choices=['f32', 'packed', 'host'], help='with --exit: the store of the activation cache '
                    'the step reads (train.ACT_STORES); other than f32 also times trunk against trunk(packed=True) at batch 256 and skips the CV')
    ap.add_argument('--bn', default='frozen', choices=list(T.BN_MODES), help="with --exit: block 14's batch norm in the measured step "
                    "(train.BN_MODES); 'batch' skips the CV")
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--cache-slides', type=int, default=8)
    ap.add_argument('--cache-tiles', type=int, default=512)
    ap.add_argument('--cv-slides', type=int, default=64)
    ap.add_argument('--cv-tiles', type=int, default=200)
    ap.add_argument('--mc', type=int, default=30)
    args = ap.parse_args(argv)
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=256, max_mc=args.mc)
    try:
        if args.exit:
            print(json.dumps(bench_exit_steps(eng, min(args.steps, 20), args.batch, store=args.act_cache, bn=args.bn)), flush=True)
            if args.bn != 'frozen':
                return
            if args.act_cache != 'f32':
                print(json.dumps(bench_trunk(eng)), flush=True)
            elif args.cv_slides > 0:
                print(json.dumps(bench_exit_cv(eng, min(args.cv_slides, 12), min(args.cv_tiles, 64), args.mc, args.batch)), flush=True)
            return
        print(json.dumps(bench_steps(eng, args.steps, args.batch)), flush=True)
        if args.batch * 32 <= Engine.HEAD_VALIDATE_MAX_ROWS:
            print(json.dumps(bench_validate(eng, args.batch)), flush=True)
        if args.cache_slides > 0:
            print(json.dumps(bench_cache(eng, args.cache_slides, args.cache_tiles)), flush=True)
        if args.cv_slides > 0:
            print(json.dumps(bench_cv(eng, args.cv_slides, args.cv_tiles, args.mc)), flush=True)
    finally:
        eng.close()


if __name__ == '__main__':
    main()
