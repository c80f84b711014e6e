"""Head training on the host side (biscuit_amd/train.py; DESIGN.md section 7 "Head training"): the float64 yardstick of the GPU tests
against finite differences, the float32 twin's distance from it (what the GPU tolerance is derived from), the schedule, the k-fold
split, nested cross-validation down to the thresholds with a stub trainer, and the command line's refusals.  No GPU."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from biscuit_amd import predictions, threshold
from biscuit_amd import train as T
from tests import _train_ref as R


# ------------------------------------------------------------------------------------------------ 1. the yardstick itself
def test_float64_gradients_match_central_differences():
    """20 random elements of each of the six tensors at rate 0.1 with fixed masks, n = 5, h = 1e-6: the central difference of the
    float64 loss agrees with the float64 gradient within 1e-6 of the tensor's largest gradient entry."""
    rng = np.random.default_rng(8)
    f, w = R.cache(), R.tensors(R.head())
    rows = np.array([3, 7, 11, 19, 30], np.int64)
    labels = np.array([0, 1, 1, 0, 1])
    keeps = R.keep_masks(R.SEED, rows, 2, 0.1)
    _, g = R.loss_and_grad(f[rows], labels, w, keeps, 0.1)
    h = 1e-6
    for name in R.TENSORS:
        scale = np.abs(g[name]).max()
        assert scale > 0
        flat = w[name].reshape(-1)                              # a view: the perturbation reaches ``w``
        for e in rng.choice(flat.size, min(20, flat.size), replace=False):     # (logits/bias has two)
            keep = flat[e]
            flat[e] = keep + h
            up, _ = R.loss_and_grad(f[rows], labels, w, keeps, 0.1, want_grad=False)
            flat[e] = keep - h
            down, _ = R.loss_and_grad(f[rows], labels, w, keeps, 0.1, want_grad=False)
            flat[e] = keep
            fd = (up - down) / (2 * h)
            assert abs(fd - g[name].reshape(-1)[e]) <= 1e-6 * scale, (name, int(e), fd, g[name].reshape(-1)[e])


# ------------------------------------------------------------------------------------------------ 2. the float32 twin
@pytest.mark.parametrize('n', R.GRAD_N)
def test_float32_twin_error_on_the_gpu_cases(n):
    """Per tensor max|g32 - g64| / max|g64| of every GPU gradient case: computed, never stored -- tests/test_gpu_train.py allows the
    device 8 x this number.  Here: it is a rounding-level number, neither 0 nor large."""
    for rate in R.GRAD_RATES:
        for kind in R.GRAD_LABELS:
            rows, labels, l64, g64, twin = R.grad_reference(n, rate, kind)
            assert np.isfinite(l64) and len(rows) == n
            for name in R.TENSORS + ('loss',):
                print(f'n={n} rate={rate} {kind} {name}: {twin[name]:.3e}')
                assert 0 < twin[name] < 1e-5, (n, rate, kind, name, twin[name])
            assert (g64['hidden_0/kernel'][:, -8:] == 0).all() and (g64['hidden_0/bias'][-8:] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the schedule
def test_learning_rate_schedule_values():
    p = T.TrainParams()
    assert (p.batch_size, p.epochs, p.optimizer, p.learning_rate, p.learning_rate_decay, p.learning_rate_decay_steps, p.dropout) == \
        (128, [1], 'Adam', 1e-4, 0.98, 512, 0.1)
    assert (T.ADAM_BETA_1, T.ADAM_BETA_2, T.ADAM_EPSILON, T.LR_STAIRCASE) == (0.9, 0.999, 1e-7, True)
    assert p.learning_rate_at(0) == 1e-4 and p.learning_rate_at(511) == 1e-4
    assert p.learning_rate_at(512) == 1e-4 * 0.98 and p.learning_rate_at(1024) == 1e-4 * 0.98 ** 2
    for step in (0, 511, 512, 1024):
        assert p.learning_rate_at(step) == R.learning_rate(step)
    with pytest.raises(ValueError):
        T.TrainParams(optimizer='SGD').validate()
    with pytest.raises(ValueError):
        T.TrainParams(batch_size=2048).validate()


def test_head_vector_round_trip_and_glorot():
    w = R.head()
    vec = T.flatten_head(w)
    assert vec.shape == (T.HEAD_PARAMS,) == (3149826,) and vec.dtype == np.float32
    back = T.unflatten_head(vec)
    assert all(np.array_equal(back[k], w[k]) for k in R.TENSORS)
    assert vec[2048 * 1024 + 5] == w['hidden_0/bias'][5] and vec[-2] == w['logits/bias'][0]
    g = T.glorot_head(4)
    assert all(np.array_equal(g[k], T.glorot_head(4)[k]) for k in R.TENSORS) and not np.array_equal(g['logits/kernel'], T.glorot_head(5)['logits/kernel'])
    lim = np.sqrt(6.0 / (2048 + 1024))
    assert np.abs(g['hidden_0/kernel']).max() <= lim and np.abs(g['hidden_0/kernel']).max() > 0.99 * lim and not g['hidden_1/bias'].any()
    with pytest.raises(ValueError):
        T.unflatten_head(vec[:-1])


# ------------------------------------------------------------------------------------------------ 4. kfold
def test_kfold_split():
    patients = [f'p{i:02d}' for i in range(23)]
    labels = {p: int(i % 3 == 0) for i, p in enumerate(patients)}          # 8 of class 1, 15 of class 0
    folds = T.kfold(patients, labels, 3, 7)
    assert len(folds) == 3 and sorted(p for f in folds for p in f) == patients
    assert all(len(set(a) & set(b)) == 0 for i, a in enumerate(folds) for b in folds[i + 1:])
    assert all({labels[p] for p in f} == {0, 1} for f in folds)
    assert max(len(f) for f in folds) - min(len(f) for f in folds) <= 1
    assert T.kfold(list(reversed(patients)), labels, 3, 7) == folds and T.kfold(patients, labels, 3, 8) != folds
    with pytest.raises(ValueError):
        T.kfold(patients[:4], labels, 3, 7)                                 # class 1 has two patients


class _Stub:
    """A trainer that returns canned tables: per validation tile a prediction that leans to its slide's label."""

    def __init__(self, cache, labels):
        self.cache, self.labels, self.calls = cache, labels, []

    def __call__(self, train_rows, val_rows, seed):
        self.calls.append((train_rows, val_rows, seed))
        rng = np.random.default_rng(seed)
        sidx = self.cache.slide_idx[val_rows]
        y = np.array([self.labels[self.cache.slides[i]] for i in sidx])
        lean = rng.normal(0, 0.3, len(self.cache.slides))[sidx]                # per slide: some slides come out wrong
        p1 = np.clip(0.5 + (y - 0.5) * 0.2 + lean + rng.normal(0, 0.25, len(y)), 0.01, 0.99).astype(np.float32)
        unc = (0.02 + 0.2 * np.abs(rng.normal(0, 1, len(y))) * (1.2 - np.abs(p1 - 0.5))).astype(np.float32)
        mean, std = np.stack([1 - p1, p1], 1), np.stack([unc, unc], 1)
        return predictions.tile_frame('cohort', [self.cache.slides[i] for i in sidx], y, mean, std, self.cache.loc[val_rows]), None


def _cohort(n_patients=18, tiles=15):
    """Two slides for every third patient, one for the others; ``tiles`` tiles per slide."""
    slides, patients, labels = [], {}, {}
    for i in range(n_patients):
        for j in range(2 if i % 3 == 0 else 1):
            s = f's{i:02d}{"ab"[j]}'
            slides.append(s)
            patients[s] = f'p{i:02d}'
            labels[s] = i % 2
    slide_idx = np.repeat(np.arange(len(slides)), tiles).astype(np.int64)
    loc = np.stack([np.arange(len(slide_idx)), np.zeros(len(slide_idx), np.int64)], 1).astype(np.int64)
    return T.FeatureCache(None, slide_idx, loc, slides), labels, patients


def test_two_slides_of_one_patient_never_separate(tmp_path):
    cache, labels, patients = _cohort()
    stub = _Stub(cache, labels)
    T.train_cv(cache, labels, str(tmp_path), 'EXP', 3, stub, patients=patients, seed=1)
    assert len(stub.calls) == 3
    seen = []
    for train_rows, val_rows, _ in stub.calls:
        tr = {patients[cache.slides[i]] for i in cache.slide_idx[train_rows]}
        va = {patients[cache.slides[i]] for i in cache.slide_idx[val_rows]}
        assert tr and va and not tr & va and len(tr | va) == 18
        seen += sorted(va)
    assert sorted(seen) == sorted(set(patients.values()))


# ------------------------------------------------------------------------------------------------ 5. nested CV with a stub trainer
def _hand_thresholds(out, label, outer, inner_k, pmap):
    dfs = []
    for j in range(1, inner_k + 1):
        df = predictions.load_tile_predictions(os.path.join(out, f'{label}-k{outer}-kfold{j}', predictions.VAL_NAME), 'cohort')
        df['patient'] = df['slide'].map(pmap)
        dfs.append(df)
    kw = dict(tile_pred='detect', slide_pred='detect', plot=False, patients=pmap)
    tile_uq = threshold.from_cv(dfs, tile_uq='detect', slide_uq=None, **kw)['tile_uq']
    return threshold.from_cv(dfs, tile_uq=tile_uq, slide_uq='detect', **kw)


def test_nested_cv_directories_frame_and_thresholds(tmp_path):
    cache, labels, patients = _cohort()
    out = str(tmp_path)
    stub = _Stub(cache, labels)
    dirs = T.train_nested_cv(cache, labels, out, 'EXP', stub, outer_k=3, inner_k=2, patients=patients, seed=5)
    want = [f'EXP-kfold{k}' for k in (1, 2, 3)] + [f'EXP-k{k}-kfold{j}' for k in (1, 2, 3) for j in (1, 2)]
    assert [os.path.basename(d) for d in dirs] == want and sorted(os.listdir(out)) == sorted(want)
    assert len(stub.calls) == 3 * (1 + 2)
    for d in dirs:
        assert sorted(os.listdir(d)) == ['slides.json', predictions.VAL_NAME]            # (the stub returns no head)
        df = pd.read_csv(os.path.join(d, predictions.VAL_NAME), dtype={'slide': str})
        assert list(df.columns) == ['slide', 'loc_x', 'loc_y', 'cohort-y_true0', 'cohort-y_pred0', 'cohort-y_pred1', 'cohort-uncertainty0',
                                    'cohort-uncertainty1']
    # an inner fold trains and validates inside its outer fold's training slides
    for k in (1, 2, 3):
        outer = json.load(open(os.path.join(out, f'EXP-kfold{k}', 'slides.json')))
        for j in (1, 2):
            inner = json.load(open(os.path.join(out, f'EXP-k{k}-kfold{j}', 'slides.json')))
            assert sorted(inner['training'] + inner['validation']) == sorted(outer['training'])
            assert not set(inner['validation']) & set(outer['validation'])

    frame, th = T.thresholds_from_nested_cv(out, 'EXP', patients=patients, outer_k=3, inner_k=2)
    assert list(frame.columns) == ['id', 'n_slides', 'fold', 'uq', 'patient_auc', 'patient_uq_perc', 'slide_auc', 'slide_uq_perc']
    assert frame['fold'].tolist() == [1, 2, 3] and set(frame['id']) == {'EXP'} and set(frame['uq']) == {'include'}
    assert frame['n_slides'].tolist() == [len(cache.slides)] * 3
    hand = [_hand_thresholds(out, 'EXP', k, 2, patients) for k in (1, 2, 3)]
    assert th['tile_uq'] == np.mean([h['tile_uq'] for h in hand]) and th['slide_uq'] == np.mean([h['slide_uq'] for h in hand])
    assert th['slide_pred'] == np.mean([h['slide_pred'] for h in hand])
    assert all(v is not None and not np.isnan(v) for v in th.values())
    # the applied metrics of fold 1, by hand
    tile_df = predictions.load_tile_predictions(os.path.join(out, 'EXP-kfold1', predictions.VAL_NAME), 'cohort')
    res, _ = threshold.apply(tile_df, plot=False, patients=patients, level='patient', **hand[0])
    assert frame['patient_auc'][0] == res['auc'] and frame['patient_uq_perc'][0] == res['percent_incl']

    # a missing inner fold: its outer fold is skipped, as experiment.py:956-966 skips it
    os.remove(os.path.join(out, 'EXP-k2-kfold1', predictions.VAL_NAME))
    frame2, th2 = T.thresholds_from_nested_cv(out, 'EXP', patients=patients, outer_k=3, inner_k=2)
    assert frame2['fold'].tolist() == [1, 3]
    assert th2['tile_uq'] == np.mean([hand[0]['tile_uq'], hand[2]['tile_uq']])
    # nothing at all: the reference's Nones
    frame3, th3 = T.thresholds_from_nested_cv(out, 'OTHER', patients=patients)
    assert len(frame3) == 0 and th3 == {'tile_uq': None, 'slide_uq': None, 'slide_pred': None}


def test_feature_cache_rows_and_file(tmp_path):
    cache, _, _ = _cohort(4, 3)
    cache.feats = np.arange(len(cache) * 2048, dtype=np.float32).reshape(-1, 2048)
    assert cache.rows_of(['s01a', 's00b']).tolist() == [3, 4, 5, 6, 7, 8]
    path = str(tmp_path / 'cache.npz')
    cache.save(path)
    back = T.FeatureCache.load(path)
    assert back.slides == cache.slides and np.array_equal(back.feats, cache.feats) and back.feats.dtype == np.float32
    assert np.array_equal(back.slide_idx, cache.slide_idx) and np.array_equal(back.loc, cache.loc)


# ------------------------------------------------------------------------------------------------ 6. command-line refusals
def test_command_line_refusals(tmp_path):
    model = tmp_path / 'model'
    model.mkdir()
    rec = tmp_path / 'a.tfrecords'
    rec.write_bytes(b'')
    good = tmp_path / 'labels.csv'
    good.write_text('slide,label\na,wt\nb,mut\n')
    base = [str(rec), '--labels', str(good), '--model', str(model), '--out', str(tmp_path / 'out')]
    for argv in ([], base[:1], base + ['--init', 'zeros'], base + ['--outer-k', '1'], base + ['--epochs', '0']):
        with pytest.raises(SystemExit):
            T.main(argv)
    with pytest.raises(SystemExit, match='not a directory'):
        T.main(base[:3] + ['--model', str(tmp_path / 'none'), '--out', 'x'])
    with pytest.raises(SystemExit, match='no such file'):
        T.main([str(tmp_path / 'missing.tfrecords')] + base[1:])
    one = tmp_path / 'one.csv'
    one.write_text('slide,label\na,wt\nb,wt\n')
    with pytest.raises(SystemExit, match='exactly two label values'):
        T.main([str(rec), '--labels', str(one), '--model', str(model), '--out', 'x'])
    cols = tmp_path / 'cols.csv'
    cols.write_text('name,class\na,wt\n')
    with pytest.raises(SystemExit, match='slide and label'):
        T.main([str(rec), '--labels', str(cols), '--model', str(model), '--out', 'x'])
    other = tmp_path / 'other.csv'
    other.write_text('slide,label\nb,wt\nc,mut\n')
    with pytest.raises(SystemExit, match='no label for slide'):
        T.main([str(rec), '--labels', str(other), '--model', str(model), '--out', 'x'])
    with pytest.raises(SystemExit, match='fewer than k'):                   # one slide cannot make three folds of both classes
        T.main(base)
    # six patients of each class make three outer folds, but the four left of a class do not make five inner ones: refused before any work
    recs, rows = [], ['slide,label']
    for i in range(12):
        p = tmp_path / f'r{i:02d}.tfrecords'
        p.write_bytes(b'')
        recs.append(str(p))
        rows.append(f'r{i:02d},{"wt" if i % 2 else "mut"}')
    twelve = tmp_path / 'twelve.csv'
    twelve.write_text('\n'.join(rows) + '\n')
    with pytest.raises(SystemExit, match='inner split of outer fold 1'):
        T.main(recs + ['--labels', str(twelve), '--model', str(model), '--out', str(tmp_path / 'out')])
    T.check_nested_split({f'r{i:02d}': i % 2 for i in range(12)}, None, 3, 2, 0)
    assert not (tmp_path / 'out').exists()
