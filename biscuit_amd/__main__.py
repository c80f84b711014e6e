"""Command-line entry to the hot path: MC-dropout inference over slides, tile table on disk,
slide-level table and (optionally) thresholded metrics -- what ``Project.evaluate(...,
save_predictions=True)`` followed by ``threshold.apply`` does in the reference
(``biscuit/experiment.py:917-922``, ``705-720``).

    python -m biscuit_amd --tfrecords DIR --labels labels.csv --weights model.npz --out eval_dir
    python -m biscuit_amd --synthetic 16x64 --out eval_dir          # random-init weights, synthetic tiles

labels.csv: columns ``slide,label[,patient]`` (label 0/1).  Needs an MI355X; there is no CPU path.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np
import pandas as pd


def model_hp(params):
    """(ModelParams, norm_fit) from what ``keras_import.read_params`` found in a model's params.json: the dropout
    rate (and ``uq_n`` when stored) drive the MC statistics, so they come from the model, never from the defaults;
    a stain normaliser other than the ones this path takes (`reinhard_fast`, hp.py:19, the masked forms of the Reinhard family
    and `macenko`) is an error -- among them plain `reinhard`, which the library implements (``stain.Reinhard``, every driver's
    ``normalizer='reinhard'``) but the command lines go on refusing by name, as tests/test_host.py pins --, and
    its fit is used only when that normaliser is the model's and the fit is one of that method."""
    from .stain import METHODS, REINHARD_FLAGS, macenko_fit, reinhard_fit
    from .hp import ModelParams
    hp = ModelParams()
    if not params:
        return hp, None
    raw = params.get('hp') or {}
    if raw.get('dropout') is not None:
        hp.dropout = float(raw['dropout'])
    if raw.get('uq_n') is not None:
        hp.uq_n = int(raw['uq_n'])
    normalizer = params.get('normalizer')
    if normalizer is None and params.get('norm_fit'):
        raise SystemExit(f"{params.get('path', 'params.json')}: a norm_fit block but no hp.normalizer: cannot tell which stain "
                         f"normaliser the model was trained with")
    hp.normalizer = normalizer
    hp.validate()
    if normalizer is not None and (normalizer not in METHODS or normalizer == 'reinhard'):
        raise SystemExit(f"{params.get('path', 'params.json')}: the model was trained with normalizer={normalizer!r}; this "
                         f"path takes 'reinhard_fast' (biscuit/hp.py:19), 'reinhard_mask', 'reinhard_fast_mask', 'macenko' or none"
                         + ("; plain 'reinhard' runs through the Python drivers only (evaluate(..., normalizer='reinhard'))"
                            if normalizer == 'reinhard' else ''))
    if normalizer == 'macenko':
        fit = params.get('norm_fit')
        try:
            macenko_fit(fit)
        except ValueError as e:
            raise SystemExit(f"{params.get('path', 'params.json')}: normalizer='macenko' but {e}") from None
        return hp, fit
    fit = params.get('norm_fit') if normalizer in REINHARD_FLAGS else None
    if normalizer in REINHARD_FLAGS and not fit:
        raise SystemExit(f"{params.get('path', 'params.json')}: normalizer={normalizer!r} but no norm_fit block")
    if normalizer in REINHARD_FLAGS and normalizer != 'reinhard_fast':
        try:
            reinhard_fit(fit)
        except ValueError as e:
            raise SystemExit(f"{params.get('path', 'params.json')}: normalizer={normalizer!r} but {e}") from None
    return hp, fit


def load_model_weights(model=None, weights=None):
    """(weights, params or None) of ``--model DIR`` (a Slideflow model directory: SavedModel weights plus params.json),
    ``--weights FILE``, or neither (seeded random init): what both command lines load."""
    if model:
        from .keras_import import load_model_dir
        return load_model_dir(model)
    if weights:
        from .keras_import import load_weights
        return load_weights(weights), None
    from .weights import synthetic_weights
    return synthetic_weights(1), None


def model_hp_from(model_params, params_path=None):
    """``model_hp`` of the model directory's params, or -- when ``--params FILE`` is given -- of that params.json, which must
    carry a norm_fit block."""
    hp, norm_fit = model_hp(model_params)
    if not params_path:
        return hp, norm_fit
    with open(params_path) as f:
        raw = json.load(f)
    hp, norm_fit = model_hp({'hp': raw.get('hp') or {}, 'normalizer': (raw.get('hp') or {}).get('normalizer', raw.get('normalizer', 'reinhard_fast')),
                             'norm_fit': raw.get('norm_fit'), 'path': params_path})
    if not norm_fit:
        raise SystemExit(f'{params_path}: no norm_fit block')
    return hp, norm_fit


def _first_tiles(slide, n):
    """The first ``n`` decoded tiles of a slide as a uint8 array, reading no more than those: through the slide's chunk source
    when it has one (TFRecords: ``n`` records, not the slide -- a 10^4-tile slide is 2.7 GB decoded), with the PNG filters
    reversed on the host whatever mode the run itself uses."""
    if slide is None:
        return None
    cnt = min(int(n), slide.n_tiles)
    src = getattr(slide, 'source', None)
    if src is not None and hasattr(src, 'path'):
        from .inference import TFRecordSource
        one = TFRecordSource(src.path, slide.n_tiles, src.tile_px, rows=False)
        buf = np.empty(one.chunk_shape(cnt), np.uint8)
        try:
            one.read(0, cnt, buf)
        finally:
            one.close()
        return buf
    t = slide.load()
    if hasattr(t, 'rows'):          # filtered PNG scanlines without a chunk source: not tiles yet
        return None
    t = t[:cnt]
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, 'cpu') else t)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--tfrecords', help='directory of Slideflow *.tfrecords (one per slide)')
    src.add_argument('--synthetic', help='SxT: S synthetic slides of T tiles; or a comma list of tile counts (9,3,0,7)')
    ap.add_argument('--labels', help='CSV with slide,label[,patient]')
    ap.add_argument('--weights', help='weights: .npz / .safetensors under Keras variable names, a TensorFlow checkpoint '
                                      'prefix, or a Keras SavedModel directory (default: seeded random init)')
    ap.add_argument('--model', help='Slideflow model directory (find_model, biscuit/utils.py:233-272): SavedModel weights '
                                    'plus params.json (norm_fit, outcome labels); replaces --weights and --params')
    ap.add_argument('--outcome', default='cohort')
    ap.add_argument('--out', required=True)
    ap.add_argument('--mc', type=int, default=None, help='MC-dropout passes (default: uq_n of the model, 30)')
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--dtype', default='f16', choices=['f16', 'bf16', 'f32'])
    ap.add_argument('--streams', type=int, default=1,
                    help='batches in flight, each on its share of the chip (1 measured fastest through evaluate(): 25.8 k vs 25.4 k tiles/s)')
    ap.add_argument('--params', help="Slideflow params.json: its hp.normalizer ('reinhard_fast', the default, 'reinhard_mask', "
                                     "'reinhard_fast_mask' or 'macenko') and "
                                     "norm_fit switch on that stain normaliser (hp.py:19)")
    ap.add_argument('--tile-uq', type=float, default=0.0, help='tile-level uncertainty threshold (0 = off)')
    ap.add_argument('--slide-uq', type=float, default=0.0, help='slide-level uncertainty threshold (0 = off)')
    ap.add_argument('--gpu-decode', type=int, default=0, metavar='CUS',
                    help='decode PNG and baseline-JPEG tiles on the GPU: the host only copies their zlib streams / entropy-coded scans, CUS '
                         'compute units (16-32) kept out of the inference streams decode them; slides outside both device subsets '
                         '(progressive, grey or restart-interval JPEG, ...) stay on the host.  PNG: for hosts with few free cores per GPU '
                         'and runs of >= 30 k tiles; slower than 16 host threads otherwise (profiles/r05_inflate.txt).  JPEG at quality '
                         '<= 95: faster than the host decoder on hosts with 16 free cores per GPU or fewer (20 k tiles/s on 16 CUs, 29 k '
                         'on 32, against 17 k); not at quality 100, and not needed with ~28 or more free cores per GPU '
                         '(profiles/jpeg_decode.txt).  Pins 3 x up to 1 GiB of host memory per rank for the compressed ring (4 096-tile '
                         'chunks) and allocates ~3 GB on the device per chunk in flight; JPEG adds 1.14 GB of coefficient scratch per '
                         'decode stream (554 KB per 299-px tile, rounds of 2 048 tiles)')
    ap.add_argument('--skip-existing', action='store_true',
                    help='do nothing when OUT already holds tile_predictions_eval.csv (the idempotence of the reference\'s Step 6: '
                         'utils.eval_exists, biscuit/experiment.py:913-914)')
    ap.add_argument('--detect', action='store_true',
                    help='also run threshold.detect on the tile table (Youden thresholds over every tile of the cohort, threshold.py:364-475)')
    ap.add_argument('--dist-backend', default=None, help='process-group backend for WORLD_SIZE > 1 (default nccl = RCCL; gloo for a rehearsal '
                                                          'of several ranks on one GPU)')
    ap.add_argument('--local-device', type=int, default=None, help='HIP device of this rank (default LOCAL_RANK)')
    ap.add_argument('--unfilter', default='auto', choices=['auto', 'host', 'gpu'],
                    help="where the PNG scanline filters of TFRecord tiles are reversed: 'auto' (default) decodes 48 tiles of the first "
                         "slide both ways and takes the GPU where the host alone cannot feed it (same bytes either way; 28.8 k -> 31.9 k "
                         "tiles/s on 16 cores)")
    ap.add_argument('--no-calibrate', action='store_true',
                    help='f16 with external weights: skip the activation-exponent calibration on the first tiles (the headroom check stays)')
    ap.add_argument('--range-screen', action=argparse.BooleanOptionalAction, default=False,
                    help='f16: screen every tile for the f16 range limit -- each tile is ranked on the GPU by how far its standardised '
                         'input reaches and the riskiest of each interval go through the range taps; a run that would clamp stops with '
                         'an error.  Off by default: it costs 0.9 %% of throughput against a bar of 0.5 %% (DESIGN.md section 4)')
    args = ap.parse_args(argv)

    if args.skip_existing and os.path.exists(os.path.join(args.out, 'tile_predictions_eval.csv')):
        # (every rank sees the same directory and takes the same way out, before any rendezvous)
        if int(os.environ.get('RANK', '0')) == 0:
            print(json.dumps({'skipped': True, 'tile_table': os.path.join(args.out, 'tile_predictions_eval.csv')}))
        return
    from . import distributed as D, threshold
    from .engine import EnginePool
    from .inference import Slide, evaluate, slides_from_tfrecords
    from .synthetic import make_slides

    rank, world, local = D.init_from_env('cuda', backend=args.dist_backend, local_device=args.local_device)
    D.pin_rank(int(os.environ.get('LOCAL_RANK', rank)), int(os.environ.get('LOCAL_WORLD_SIZE', world)), device_index=local)     # before any thread pool exists
    w, model_params = load_model_weights(args.model, args.weights)
    patients = None
    if args.tfrecords:
        lab = pd.read_csv(args.labels, dtype={'slide': str}) if args.labels else pd.DataFrame(columns=['slide', 'label'])
        labels = dict(zip(lab['slide'], lab['label']))
        patients = dict(zip(lab['slide'], lab['patient'])) if 'patient' in lab.columns else None
        paths = sorted(glob.glob(os.path.join(args.tfrecords, '*.tfrecords')))
        slides = slides_from_tfrecords(paths, labels, patients, gpu_decode=args.gpu_decode > 0,
                                       gpu_unfilter={'auto': 'auto', 'host': False, 'gpu': True}[args.unfilter])
    else:
        if 'x' in args.synthetic.lower():
            s, t = (int(x) for x in args.synthetic.lower().split('x'))
            tiles, sidx, y = make_slides(s, t, seed=0)
            slides = [Slide(f'slide{i:03d}', tiles[sidx == i], t, y_true=int(y[i])) for i in range(s)]
        else:                                                     # explicit (ragged) tile counts: 9,3,0,7
            from .synthetic import make_tiles
            counts = [int(x) for x in args.synthetic.split(',')]
            slides = [Slide(f'slide{i:03d}', make_tiles(c, seed=500 + i, slide_bias=[(i % 2) * 60.0 - 30.0, 0.0, (i % 3) * 10.0]), c,
                            y_true=i % 2) for i, c in enumerate(counts)]
    hp, norm_fit = model_hp_from(model_params, args.params)
    if args.mc is None:
        args.mc = hp.uq_n
    act_exp, probe = None, None
    if args.dtype == 'f16' and (args.model or args.weights) and slides:
        # IEEE half ends at 65504 and every f16 kernel clamps there without a signal (MODE.FP16_OVFL).  With weights from outside
        # the storage is kept in range by construction: the first tiles go through the fp32 kernels once, every stored tensor's
        # peak is measured, and power-of-two activation exponents are folded into the BatchNorm constants (weights.py).  Every
        # rank reads the same 16 tiles of the same slide, so every rank packs the same blob.
        probe = _first_tiles(next((s for s in slides if s.n_tiles), None), 16)
        if probe is not None and not args.no_calibrate:
            from .engine import Engine
            act_exp, peaks = Engine.calibrate(w, probe, hp=hp, device=local, norm_fit=norm_fit, normalizer=hp.normalizer)
            if rank == 0 and any(act_exp.values()):
                big = {t: k for t, k in act_exp.items() if k}
                print(f'f16: activation exponents from the first {len(probe)} tiles (peak {max(peaks.values()):.3g}): {big}', flush=True)
    pool = EnginePool(w, n_streams=args.streams, hp=hp, dtype=args.dtype, max_batch=args.batch, max_mc=args.mc, device=local,
                      act_exp=act_exp, reserve_cus=max(0, args.gpu_decode))
    if probe is not None:
        import torch
        from .stain import normalise
        t = torch.from_numpy(probe[:8]).to(pool.engines[0].device)
        t = normalise(pool.engines[0], t, hp.normalizer, norm_fit)
        hr = pool.engines[0].f16_headroom(t)                      # the check behind the construction
        if any(hr['saturated'].values()):
            raise SystemExit(f'f16 storage saturates with these weights ({hr["saturated"]}): run with --dtype bf16 or f32')
        if hr['headroom'] < 8 and rank == 0:
            print(f'warning: f16 headroom only {hr["headroom"]:.1f}x on the first tiles ({hr["max_abs"]}); '
                  f'consider --dtype bf16', flush=True)
    # the tile table streams to disk while the GPU works (every rank its shard; rank 0 splices them after the gather): the frame
    # is not kept in memory, the consumer reads the file -- as biscuit does (experiment.py:688-699)
    res = evaluate(pool, slides, outcome=args.outcome, mc_n=args.mc, seed=args.seed, batch=args.batch,
                   save_dir=args.out, rank=rank, world=world, norm_fit=norm_fit, keep_tiles=False, normalizer=hp.normalizer,
                   range_screen=args.range_screen)
    if res.stain_passthrough:
        print(f'rank {rank}: the {hp.normalizer} normaliser left {res.stain_passthrough} degenerate tile(s) un-normalised '
              f'(too little tissue, one colour or too dark)', file=sys.stderr, flush=True)
    if rank == 0:
        from .predictions import load_tile_predictions
        sf, _ = res.slide_frame(0.5)
        sf.to_csv(os.path.join(args.out, f'slide_predictions_{args.outcome}_eval.csv'), index=False)
        summary = {'slides': int((res.slide_count > 0).sum()), 'tiles': int(res.slide_count.sum()), 'world': world,
                   'tile_table': res.table_path}
        # the consumer on THE table, at any world size: rank 0 holds every tile of the cohort once the shards are spliced
        # (threshold.detect takes Youden's J over all of them, threshold.py:417-426)
        df = load_tile_predictions(res.table_path, args.outcome)
        if args.detect:
            try:
                found, auc = threshold.detect(df.copy(), patients=patients)
                summary['detected'] = {k: (None if v is None else float(v)) for k, v in found.items()}
                summary['detect_auc'] = None if auc is None or np.isnan(auc) else float(auc)
            except ValueError as e:                               # (a cohort whose tiles are all correct / of one class)
                summary['detected'], summary['detect_error'] = None, str(e)
        metrics, _ = threshold.apply(df, tile_uq=args.tile_uq, slide_uq=args.slide_uq, patients=patients)
        summary.update({k: (None if v is None or (isinstance(v, float) and np.isnan(v)) else float(v))
                        for k, v in metrics.items()})
        print(json.dumps(summary))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
