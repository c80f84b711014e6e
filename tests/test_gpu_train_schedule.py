"""The training schedule on the GPU (biscuit_amd/train.py; DESIGN.md section 7 "Training schedule"): validation checks that change
nothing, early stopping against ``steps_per_epoch_override``, the per-fold ``results_log.csv``, ``find_cv_early_stop`` into
``train_full``, and the command line.  A cohort of 12 slides x 40 tiles of synthetic features, batch 16, a check of 32 rows every
2 steps, ``ema_observations=2``.  ``-m gpu``."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from biscuit_amd import tfrecord as tfr
from biscuit_amd import train as T
from biscuit_amd.synthetic import make_tiles

pytestmark = pytest.mark.gpu

SEED = 4
BASE = dict(batch_size=16, learning_rate=1e-4, validate_on_batch=2, validation_steps=2, ema_observations=2)


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=4)
    yield e
    e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


@pytest.fixture(scope='module')
def cohort(eng):
    """``(cache, labels, train rows, their labels, validation rows, their labels)``: two classes whose features differ in mean on
    every other unit; slides 0-7 train, 8-11 validate."""
    rng = np.random.default_rng(12)
    slides = [f's{i:02d}' for i in range(12)]
    labels = {s: i % 2 for i, s in enumerate(slides)}
    sidx = np.repeat(np.arange(12), 40).astype(np.int64)
    f = np.abs(rng.standard_normal((480, 2048))).astype(np.float32)
    f[sidx % 2 == 1] += np.float32(0.04) * (np.arange(2048) % 2 == 0)
    cache = T.FeatureCache(up(eng, f), sidx, np.stack([np.arange(480), np.zeros(480, np.int64)], 1).astype(np.int64), slides)
    rows, val = np.flatnonzero(sidx < 8), np.flatnonzero(sidx >= 8)
    return cache, labels, rows, sidx[rows] % 2, val, sidx[val] % 2


def same_head(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k, _ in T.HEAD_TENSORS)


def same_f32(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope='module')
def plain(eng, cohort):
    """Two epochs without validation or balancing."""
    cache, _, rows, y, _, _ = cohort
    return T.fit_head(eng, cache, rows, y, init='glorot', params=T.TrainParams(epochs=[2], **BASE), seed=SEED)


@pytest.fixture(scope='module')
def stopped(eng, cohort):
    """One epoch of 20 steps under the early-stopping rule."""
    cache, _, rows, y, val, vy = cohort
    return T.fit_head(eng, cache, rows, y, val_rows=val, val_labels=vy, init='glorot', params=T.TrainParams(early_stop=True, **BASE), seed=SEED)


def test_fit_head_without_a_schedule_is_the_epoch_loop_it_replaced(eng, cohort, plain):
    """``train_head`` as it was: per epoch one permutation and one ``head_train_steps`` call, restated here."""
    cache, _, rows, y, _, _ = cohort
    p = T.TrainParams(epochs=[2], **BASE)
    w = up(eng, T.flatten_head(T.glorot_head(SEED)))
    m, v, losses, step = torch.zeros_like(w), torch.zeros_like(w), [], 0
    for epoch in range(2):
        order = np.random.default_rng([SEED, epoch]).permutation(len(rows))
        lr = [p.learning_rate_at(step + i) for i in range(20)]
        losses.append(eng.head_train_steps(w, m, v, cache.feats, up(eng, rows[order]), up(eng, y[order].astype(np.uint8)), 16, step, SEED, lr,
                                           rate=p.dropout, b1=T.ADAM_BETA_1, b2=T.ADAM_BETA_2, eps=T.ADAM_EPSILON).cpu().numpy())
        step += 20
    assert plain.steps == 40 and plain.checks == [] and plain.early_stop_batch is None
    assert same_head(plain.head, T.unflatten_head(w.cpu().numpy())) and same_f32(plain.losses, np.concatenate(losses))
    head, losses = T.train_head(eng, cache, rows, y, init='glorot', params=p, seed=SEED)
    assert same_head(head, plain.head) and same_f32(losses, plain.losses)


def test_validation_perturbs_nothing(eng, cohort, plain):
    cache, _, rows, y, val, vy = cohort
    p = T.TrainParams(epochs=[2], early_stop=True, early_stop_patience=100, **BASE)
    fit = T.fit_head(eng, cache, rows, y, val_rows=val, val_labels=vy, init='glorot', params=p, seed=SEED)
    assert fit.early_stop_batch is None and fit.steps == 40 and [c[0] for c in fit.checks] == list(range(2, 41, 2))
    assert same_head(fit.head, plain.head) and same_f32(fit.losses, plain.losses)
    assert all(np.isfinite(c[1]) and 0.0 <= c[2] <= 1.0 for c in fit.checks) and len({c[1] for c in fit.checks}) > 1


def test_a_stopped_run_is_a_run_of_that_many_steps(eng, cohort, stopped):
    cache, _, rows, y, _, _ = cohort
    s = stopped.early_stop_batch
    print('stopped at step', s, 'checks', stopped.checks)
    assert s is not None and s % 2 == 0 and 6 <= s < 20 and stopped.steps == s and stopped.checks[-1][0] == s
    fit = T.fit_head(eng, cache, rows, y, init='glorot', params=T.TrainParams(steps_per_epoch_override=s, **BASE), seed=SEED)
    assert fit.steps == s and same_head(fit.head, stopped.head) and same_f32(fit.losses, stopped.losses)


def test_every_check_is_head_validate_on_the_rows_the_definition_names(eng, cohort, stopped):
    cache, _, rows, y, val, vy = cohort
    p = T.TrainParams(early_stop=True, **BASE)
    order = np.random.default_rng([SEED, 0]).permutation(len(rows))
    walk = np.random.default_rng([SEED, 0x76616c]).permutation(len(val))
    w = up(eng, T.flatten_head(T.glorot_head(SEED)))
    m, v, rule = torch.zeros_like(w), torch.zeros_like(w), T.EarlyStop.of(p)
    for c, (step, val_loss, val_acc, ema) in enumerate(stopped.checks):
        seg = order[(step - 2) * 16:step * 16]
        eng.head_train_steps(w, m, v, cache.feats, up(eng, rows[seg]), up(eng, y[seg].astype(np.uint8)), 16, step - 2, SEED,
                             [p.learning_rate_at(step - 2), p.learning_rate_at(step - 1)], rate=p.dropout)
        at = walk[(32 * c + np.arange(32)) % len(val)]
        stats, _, hit = eng.head_validate(w, cache.feats, up(eng, val[at]), up(eng, vy[at].astype(np.uint8)), step, SEED, rate=0.0, hit=True)
        stats = stats.cpu().numpy()
        assert step == 2 * (c + 1) and val_loss == stats[0] / 32 and val_acc == stats[1] / 32 == float(hit.sum()) / 32
        fired = rule.update(val_acc, 0)
        assert ema == rule.ema and fired == (c == len(stopped.checks) - 1)


@pytest.fixture(scope='module')
def folds(eng, cohort, tmp_path_factory):
    """``train_cv`` over the cohort, three folds, under the early-stopping rule -> ``(out, trainer, directories)``."""
    cache, labels, _, _, _, _ = cohort
    out = str(tmp_path_factory.mktemp('cv'))
    trainer = T.HeadTrainer(eng, cache, labels, params=T.TrainParams(early_stop=True, **BASE), init='glorot', mc_n=2)
    return out, trainer, T.train_cv(cache, labels, out, 'EXP', 3, trainer, seed=2)


def test_train_cv_writes_the_results_log(eng, cohort, folds):
    cache, labels, _, _, _, _ = cohort
    out, trainer, dirs = folds
    assert len(trainer.fits) == 3 and all(len(f.checks) >= 3 for f in trainer.fits)
    for d, fit in zip(dirs, trainer.fits):
        df = pd.read_csv(os.path.join(d, T.RESULTS_FILE))
        assert len(df) == 1 and df['model_name'][0] == os.path.basename(d) + '-epoch1' and df['steps'][0] == fit.steps
        assert df['val_loss'][0] == pytest.approx(fit.checks[-1][1], rel=1e-12) and df['val_acc'][0] == fit.checks[-1][2]
        assert ('early_stop_batch' in df.columns) == (fit.early_stop_batch is not None)
        if fit.early_stop_batch is not None:
            assert df['early_stop_batch'][0] == fit.early_stop_batch == fit.steps
        assert os.path.exists(os.path.join(d, T.HEAD_FILE))
    # a rule that may never fire leaves the column out; without early_stop the trainer validates nothing
    patient = T.HeadTrainer(eng, cache, labels, params=T.TrainParams(early_stop=True, early_stop_patience=100, **BASE), init='glorot', mc_n=2)
    for d, fit in zip(T.train_cv(cache, labels, out, 'LATE', 3, patient, seed=2), patient.fits):
        df = pd.read_csv(os.path.join(d, T.RESULTS_FILE))
        assert 'early_stop_batch' not in df.columns and fit.early_stop_batch is None and df['steps'][0] == 20 and len(fit.checks) == 10
    assert T.find_cv_early_stop(out, 'LATE') is None


def test_the_folds_stop_batch_trains_the_full_model(eng, cohort, folds):
    cache, labels, _, _, _, _ = cohort
    out, trainer, _ = folds
    stops = [f.early_stop_batch for f in trainer.fits]
    print('the folds stopped at', stops)
    assert all(s is not None for s in stops), 'the cohort is chosen so that every fold stops within its one epoch'
    stop = T.find_cv_early_stop(out, 'EXP')
    assert stop == round(sum(stops) / 3)
    d = T.train_full(cache, labels, out, 'EXP', stop_batch=stop, trainer=trainer, seed=7)
    assert d == os.path.join(out, 'EXP_FULL') and json.load(open(os.path.join(d, T.MANIFEST_FILE)))['training'] == cache.slides
    df = pd.read_csv(os.path.join(d, T.RESULTS_FILE))
    assert df['steps'][0] == stop and 'early_stop_batch' not in df.columns and df['model_name'][0] == 'EXP_FULL-epoch1'
    rows = np.arange(len(cache))
    fit = T.fit_head(eng, cache, rows, cache.slide_idx % 2, init='glorot', params=T.TrainParams(steps_per_epoch_override=stop, **BASE), seed=7)
    assert fit.steps == stop and len(fit.losses) == stop and same_head(T.load_head(os.path.join(d, T.HEAD_FILE)), fit.head)


def test_balanced_training_runs_on_the_device(eng, cohort):
    cache, _, rows, y, _, _ = cohort
    keep = np.flatnonzero((cache.slide_idx[rows] % 2 == 1) | (cache.slide_idx[rows] == 0))       # one slide of class 0, four of class 1
    p = T.TrainParams(training_balance='category', epochs=[2], **BASE)
    fit = T.fit_head(eng, cache, rows[keep], y[keep], init='glorot', params=p, seed=SEED)
    assert fit.steps == 2 * -(-len(keep) // 16) and np.isfinite(fit.losses).all()
    again = T.fit_head(eng, cache, rows[keep], y[keep], init='glorot', params=p, seed=SEED)
    assert same_head(fit.head, again.head) and same_f32(fit.losses, again.losses)


def test_command_line_early_stop_balance_full(tmp_path, capsys):
    """Self-written TFRecords and a model directory through ``--early-stop --balance category --full``: 12 slides x 6 tiles, so an
    epoch is one step and one check; the full model is trained exactly when every outer fold stopped early."""
    from biscuit_amd import keras_import as K
    from biscuit_amd.weights import synthetic_weights
    d = str(tmp_path)
    recs, rows = [], ['slide,label']
    for i in range(12):
        t = make_tiles(6, seed=80 + i, slide_bias=[(i % 2) * 40.0 - 20.0, 0.0, 0.0])
        recs.append(f'{d}/s{i:02d}.tfrecords')
        tfr.write_slide(recs[-1], f's{i:02d}', t, np.stack([np.arange(6) * 299 + 150, np.full(6, 150)], 1).astype(np.int64))
        rows.append(f's{i:02d},{"wt" if i % 2 else "mut"}')
    open(f'{d}/labels.csv', 'w').write('\n'.join(rows) + '\n')
    mdir = f'{d}/00001-cohort-HP0/cohort-HP0_epoch1'
    K.export_bundle(mdir + '/variables/variables', synthetic_weights(1), optimizer_slots=True)
    json.dump({'norm_fit': {'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, 6.0]},
               'hp': {'model': 'xception', 'tile_px': 299, 'hidden_layers': 2, 'hidden_layer_width': 1024, 'dropout': 0.1,
                      'normalizer': 'reinhard_fast'}}, open(mdir + '/params.json', 'w'))
    out = f'{d}/out'
    argv = recs + ['--labels', f'{d}/labels.csv', '--model', mdir, '--out', out, '--inner-k', '2', '--epochs', '26', '--mc', '2', '--seed', '3',
                   '--early-stop', '--balance', 'category', '--full', '--validate-on-batch', '1', '--validation-steps', '1']
    try:
        T.main(argv)
    except SystemExit as e:                                     # (a toy cohort may leave threshold.from_cv without a threshold)
        assert 'no thresholds' in str(e), e
    printed = capsys.readouterr().out
    logs = [pd.read_csv(os.path.join(T.fold_dir(out, 'EXP', j), T.RESULTS_FILE)) for j in (1, 2, 3)]
    assert all(len(df) == 1 and df['model_name'][0].endswith('epoch26') and 1 <= df['steps'][0] <= 26 for df in logs)
    for j in (1, 2, 3):
        assert os.path.exists(os.path.join(T.fold_dir(out, 'EXP-k1', 1 + j % 2), T.RESULTS_FILE))
    stop = T.find_cv_early_stop(out, 'EXP')
    full = os.path.join(out, 'EXP_FULL')
    if stop is None:
        assert 'no full model is trained' in printed and not os.path.exists(full)
    else:
        assert all('early_stop_batch' in df.columns for df in logs)
        assert pd.read_csv(os.path.join(full, T.RESULTS_FILE))['steps'][0] == 26 * stop and os.path.exists(os.path.join(full, T.HEAD_FILE))
