"""The training schedule's host side (biscuit_amd/train.py; DESIGN.md section 7 "Training schedule"): the early-stopping rule against a
sequence worked by hand, balanced draws, epochs of an overridden length, ``find_cv_early_stop`` over written fold directories, and
the row arithmetic of ``fit_head`` with a stub in the engine's place.  No GPU."""
import os

import numpy as np
import pandas as pd
import pytest

from biscuit_amd import train as T


# ------------------------------------------------------------------------------------------------ 1. EarlyStop
def test_early_stop_against_a_hand_worked_sequence():
    """ema_observations = 2, smoothing 2: k = 2 / 3.  Values 0.5, 0.7 seed 0.6; 0.9 -> 0.9 * 2/3 + 0.6 / 3 = 0.8 (only one prior:
    no decision); 0.3 -> 0.2 + 0.8 / 3 = 0.4667 <= 0.6, the average of two checks back: stop."""
    s = T.EarlyStop('accuracy', 0, ema_observations=2, ema_smoothing=2)
    assert s.update(0.5, 0) is False and s.ema is None                      # no average before the seed
    assert s.update(0.7, 0) is False and s.ema == pytest.approx(0.6, abs=1e-15) and s.two is None
    assert s.update(0.9, 0) is False and s.ema == pytest.approx(0.8, abs=1e-15) and s.two == pytest.approx(0.6, abs=1e-15)
    assert s.update(0.3, 0) is True and s.ema == pytest.approx(0.2 + 0.8 / 3, abs=1e-15)
    # a rising accuracy never stops; the same rising values as a loss stop at the first check with two priors
    up = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    s = T.EarlyStop('accuracy', 0, 2, 2)
    assert [s.update(v, 0) for v in up] == [False] * 6
    s = T.EarlyStop('loss', 0, 2, 2)
    assert [s.update(v, 0) for v in up[:4]] == [False, False, False, True]
    s = T.EarlyStop('loss', 0, 2, 2)
    assert [s.update(v, 0) for v in up[::-1]] == [False] * 6                # a falling loss goes on
    # an average that stands still has not improved, for either method
    for method in ('accuracy', 'loss'):
        s = T.EarlyStop(method, 0, 1, 2)
        assert [s.update(0.5, 0) for _ in range(3)] == [False, False, True]


def test_early_stop_respects_patience():
    s = T.EarlyStop('accuracy', 2, 2, 2)
    falling = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    assert [s.update(v, e) for v, e in zip(falling, (0, 0, 0, 1, 1, 2))] == [False, False, False, False, False, True]
    p = T.TrainParams(early_stop=True, early_stop_method='loss', early_stop_patience=3, ema_observations=5, ema_smoothing=4)
    s = T.EarlyStop.of(p)
    assert (s.method, s.patience, s.observations, s.k) == ('loss', 3, 5, 4 / 6)
    with pytest.raises(ValueError):
        T.EarlyStop('auc')


def test_params_defaults_and_the_reference_setting():
    p = T.TrainParams()
    assert (p.early_stop, p.early_stop_method, p.early_stop_patience, p.ema_observations, p.ema_smoothing) == (False, 'accuracy', 0, 20, 2)
    assert (p.validate_on_batch, p.validation_steps, p.validation_dropout, p.training_balance, p.steps_per_epoch_override) == \
        (32, 32, False, 'none', None)
    n = T.TrainParams.nature2022(dropout=0.2).validate()
    assert n.early_stop and n.early_stop_method == 'accuracy' and n.training_balance == 'category' and n.dropout == 0.2
    for bad in (dict(training_balance='class'), dict(early_stop_method='auc'), dict(validate_on_batch=0), dict(validation_steps=0),
                dict(steps_per_epoch_override=0), dict(ema_observations=0), dict(early_stop=True, batch_size=256)):
        with pytest.raises(ValueError):
            T.TrainParams(**bad).validate()
    T.TrainParams(batch_size=256).validate()                               # (the 4096-row limit binds only where checks run)


# ------------------------------------------------------------------------------------------------ 2. balanced draws
def _cohort():
    """3 slides of class 0 and 9 of class 1, of unequal size; slides 2k and 2k + 1 share a patient."""
    sizes = [5, 40, 17, 8, 30, 3, 12, 25, 9, 50, 7, 21]
    slide_idx = np.repeat(np.arange(12) + 100, sizes).astype(np.int64)      # (slide ids need not start at 0)
    labels = (slide_idx - 100 >= 3).astype(np.int64)
    rows = np.arange(len(slide_idx), dtype=np.int64) * 3 + 1                # (rows are cache rows, not positions)
    return rows, slide_idx, labels, (slide_idx - 100) // 2, sizes


def _within(share, p, n, what):
    assert abs(share - p) <= 5 * np.sqrt(p * (1 - p) / n), (what, share, p)


@pytest.mark.parametrize('balance', ['category', 'slide', 'patient'])
def test_balanced_shares_lie_within_five_sigma(balance):
    rows, slide_idx, labels, patients, sizes = _cohort()
    n = 20000
    pos = T.balanced_rows(rows, slide_idx, labels, patients, balance, n, 3, 0)
    assert pos.dtype == np.int64 and pos.shape == (n,) and pos.min() >= 0 and pos.max() < len(rows)
    slides, p = T.slide_probabilities(slide_idx, labels, patients, balance)
    assert slides.tolist() == list(range(100, 112)) and p.sum() == pytest.approx(1.0, abs=1e-12)
    want = {'category': [1 / 6] * 3 + [1 / 18] * 9, 'slide': [1 / 12] * 12, 'patient': [1 / 12] * 12}[balance]
    assert np.allclose(p, want, rtol=0, atol=1e-15)
    for s, ps in zip(slides, p):
        _within(float((slide_idx[pos] == s).mean()), ps, n, ('slide', s))
    if balance == 'category':
        _within(float(labels[pos].mean()), 0.5, n, 'class')
        assert abs(labels.mean() - 0.5) > 0.2                                # (the tiles themselves are far from balanced: 73 % class 1)


def test_patient_balance_weighs_patients_not_slides():
    rows, slide_idx, labels, _, _ = _cohort()
    patients = np.where(slide_idx < 103, 0, slide_idx)                       # the first three slides are one patient
    _, p = T.slide_probabilities(slide_idx, labels, patients, 'patient')
    assert np.allclose(p, [1 / 30] * 3 + [1 / 10] * 9, rtol=0, atol=1e-15)
    _, p = T.slide_probabilities(slide_idx, labels, None, 'patient')         # no patients: every slide is its own
    assert np.allclose(p, 1 / 12, rtol=0, atol=1e-15)


def test_no_tile_of_a_slide_repeats_within_a_cycle_and_the_walk_carries_over():
    rows, slide_idx, labels, patients, sizes = _cohort()
    state = {}
    first = T.balanced_rows(rows, slide_idx, labels, patients, 'category', 1500, 3, 0, state)
    second = T.balanced_rows(rows, slide_idx, labels, patients, 'category', 1500, 3, 1, state)
    both = np.concatenate([first, second])
    for s, size in zip(range(100, 112), sizes):
        mine = both[slide_idx[both] == s]                                    # the slide's draws in order, across the two epochs
        assert len(mine) > size
        for a in range(0, len(mine), size):
            cycle = mine[a:a + size]
            assert len(set(cycle.tolist())) == len(cycle), (s, a)
        assert set(mine[:size].tolist()) == set(np.flatnonzero(slide_idx == s).tolist())
        assert np.array_equal(mine[size:2 * size], mine[:size][:len(mine[size:2 * size])])      # the same permutation again
        assert state[s] == len(mine) % size
    # the same seed gives the same rows; another seed or epoch does not; without a state every epoch starts its walks afresh
    again = T.balanced_rows(rows, slide_idx, labels, patients, 'category', 1500, 3, 0, {})
    assert np.array_equal(again, first)
    assert not np.array_equal(T.balanced_rows(rows, slide_idx, labels, patients, 'category', 1500, 4, 0), first)
    fresh = T.balanced_rows(rows, slide_idx, labels, patients, 'category', 1500, 3, 1)
    assert not np.array_equal(fresh, second) and np.array_equal(slide_idx[fresh], slide_idx[second])


def test_none_and_tile_are_todays_permutation():
    rows, slide_idx, labels, patients, _ = _cohort()
    for balance in ('none', 'tile'):
        for epoch in (0, 3):
            got = T.balanced_rows(rows, slide_idx, labels, patients, balance, len(rows), 9, epoch, {})
            assert np.array_equal(got, np.random.default_rng([9, epoch]).permutation(len(rows)))
    with pytest.raises(ValueError):
        T.balanced_rows(rows, slide_idx[:-1], labels, patients, 'slide', 5, 0, 0)


# ------------------------------------------------------------------------------------------------ 3. steps_per_epoch_override
def test_epoch_order_below_and_above_the_natural_length():
    k0 = np.random.default_rng([5, 2]).permutation(10)
    assert np.array_equal(T.epoch_order(10, 10, 5, 2), k0)                   # today's stream
    assert np.array_equal(T.epoch_order(10, 6, 5, 2), k0[:6])
    long = T.epoch_order(10, 27, 5, 2)
    assert np.array_equal(long, np.concatenate([k0, np.random.default_rng([5, 2, 1]).permutation(10),
                                                np.random.default_rng([5, 2, 2]).permutation(10)[:7]]))
    assert len(T.epoch_order(10, 0, 5, 2)) == 0


# ------------------------------------------------------------------------------------------------ 4. find_cv_early_stop
def _fold(out, label, j, stop, steps=40):
    d = T.fold_dir(out, label, j)
    os.makedirs(d, exist_ok=True)
    fit = T.FitResult({}, np.zeros(steps, np.float32), [(steps - 2, 0.7, 0.5, None), (steps, 0.65, 0.625, 0.6)], stop, steps)
    T.write_results_log(os.path.join(d, T.RESULTS_FILE), os.path.basename(d), fit, 1)
    return d


def test_find_cv_early_stop_over_written_folds(tmp_path):
    out = str(tmp_path)
    for j, stop in enumerate((10, 11, 13), 1):
        d = _fold(out, 'EXP', j, stop)
    df = pd.read_csv(os.path.join(d, T.RESULTS_FILE))
    assert list(df.columns) == ['model_name', 'steps', 'val_loss', 'val_acc', 'early_stop_batch'] and len(df) == 1
    assert df['model_name'][0] == 'EXP-kfold3-epoch1' and df['steps'][0] == 40 and df['val_loss'][0] == 0.65 and df['val_acc'][0] == 0.625
    assert T.find_cv_early_stop(out, 'EXP') == 11                            # round(34 / 3)
    assert T.find_cv_early_stop(out, 'EXP', k=2) == 10                       # round(10.5): Python's round, to the even neighbour
    _fold(out, 'ODD', 1, 11), _fold(out, 'ODD', 2, 12)
    assert T.find_cv_early_stop(out, 'ODD', k=2) == 12                       # round(11.5)
    # one fold never triggered: its file has no such column, and the answer is None
    for j, stop in enumerate((10, None, 13), 1):
        d = _fold(out, 'TWO', j, stop)
        assert ('early_stop_batch' in pd.read_csv(os.path.join(d, T.RESULTS_FILE)).columns) == (stop is not None)
    assert T.find_cv_early_stop(out, 'TWO') is None
    assert T.find_cv_early_stop(out, 'EXP', k=4) is None and T.find_cv_early_stop(out, 'NONE') is None       # a fold is missing
    # a training without checks: the columns stay, empty
    T.write_results_log(str(tmp_path / 'r.csv'), 'EXP_FULL', T.FitResult({}, np.zeros(3, np.float32), [], None, 3), 2)
    df = pd.read_csv(tmp_path / 'r.csv')
    assert list(df.columns) == ['model_name', 'steps', 'val_loss', 'val_acc'] and df['model_name'][0] == 'EXP_FULL-epoch2'
    assert df['val_loss'].isna().all()


def test_results_log_bytes(tmp_path):
    """The file's bytes, with and without checks and with and without a stop batch."""
    path = str(tmp_path / 'r.csv')
    want = {(True, 40): b'model_name,steps,val_loss,val_acc,early_stop_batch\nEXP-kfold2-epoch3,40,0.65,0.625,40\n',
            (True, None): b'model_name,steps,val_loss,val_acc\nEXP-kfold2-epoch3,40,0.65,0.625\n',
            (False, 40): b'model_name,steps,val_loss,val_acc,early_stop_batch\nEXP-kfold2-epoch3,40,,,40\n',
            (False, None): b'model_name,steps,val_loss,val_acc\nEXP-kfold2-epoch3,40,,\n'}
    for (checked, stop), text in want.items():
        checks = [(38, 0.7, 0.5, None), (40, 0.65, 0.625, 0.6)] if checked else []
        T.write_results_log(path, 'EXP-kfold2', T.FitResult({}, np.zeros(40, np.float32), checks, stop, 40), 3)
        with open(path, 'rb') as f:
            assert f.read() == text, (checked, stop)


# ------------------------------------------------------------------------------------------------ 5. fit_head's row arithmetic
class _Stub:
    """In the engine's place: records what ``fit_head`` asks for; the validation accuracy of check c is ``accs[c]``."""

    def __init__(self, accs=()):
        import torch
        self.torch, self.device, self.weights = torch, torch.device('cpu'), T.glorot_head(0)
        self.train, self.val, self.accs = [], [], list(accs)

    def head_train_steps(self, w, m, v, feats, rows, labels, batch, step, seed, lr, **kw):
        self.train.append((rows.numpy().copy(), labels.numpy().copy(), batch, step, list(lr), kw['rate']))
        return self.torch.zeros(len(lr))

    def head_validate(self, params, feats, rows, labels, pass_, seed, rate=0.0, **kw):
        acc = self.accs[len(self.val)] if len(self.val) < len(self.accs) else 0.5
        self.val.append((feats, rows.numpy().copy(), labels.numpy().copy(), pass_, seed, rate))
        return self.torch.tensor([0.25 * len(rows), acc * len(rows)], dtype=self.torch.float64), None, None


def _stub_cache(n=60):
    feats = np.zeros((n, 2048), np.float32)
    return T.FeatureCache(feats, np.arange(n, dtype=np.int64) // 5, np.zeros((n, 2), np.int64), [f's{i}' for i in range(n // 5)])


def test_fit_head_segments_steps_and_validation_walk():
    cache = _stub_cache()
    rows, labels = np.arange(0, 46, dtype=np.int64), (np.arange(46) % 2).astype(np.int64)          # 46 rows, batch 4: 12 steps
    val_rows, val_labels = np.arange(46, 60, dtype=np.int64), (np.arange(14) % 3 == 0).astype(np.int64)
    p = T.TrainParams(batch_size=4, epochs=[2], validate_on_batch=5, validation_steps=2, ema_observations=2, dropout=0.2,
                      learning_rate_decay_steps=7)
    eng = _Stub()
    fit = T.fit_head(eng, cache, rows, labels, val_rows=val_rows, val_labels=val_labels, params=p, seed=5)
    # segments of 5, 5 and 2 steps per epoch, each starting at the global step, the learning rates per step
    assert [t[3] for t in eng.train] == [0, 5, 10, 12, 17, 22] and [len(t[4]) for t in eng.train] == [5, 5, 2, 5, 5, 2]
    assert fit.steps == 24 and fit.losses.shape == (24,) and fit.early_stop_batch is None
    for e in range(2):
        order = np.random.default_rng([5, e]).permutation(46)
        got = np.concatenate([t[0] for t in eng.train[3 * e:3 * e + 3]])
        assert np.array_equal(got, rows[order]) and np.array_equal(np.concatenate([t[1] for t in eng.train[3 * e:3 * e + 3]]), labels[order])
    assert [len(t[0]) for t in eng.train] == [20, 20, 6, 20, 20, 6] and all(t[2] == 4 and t[5] == 0.2 for t in eng.train)
    assert eng.train[1][4] == [p.learning_rate_at(s) for s in range(5, 10)] and eng.train[1][4][2] != eng.train[1][4][1]
    # one check after every segment: pass = the steps done, rate 0, the unaugmented features, 8 rows of the cyclic walk
    assert [v[3] for v in eng.val] == [5, 10, 12, 17, 22, 24] == [c[0] for c in fit.checks]
    assert all(v[0] is cache.feats and v[4] == 5 and v[5] == 0.0 and len(v[1]) == 8 for v in eng.val)
    walk = np.random.default_rng([5, 0x76616c]).permutation(val_rows)
    assert np.array_equal(walk, val_rows[np.random.default_rng([5, 0x76616c]).permutation(14)])
    label_of = dict(zip(val_rows.tolist(), val_labels.tolist()))
    for c, v in enumerate(eng.val):
        want = walk[(8 * c + np.arange(8)) % 14]
        assert np.array_equal(v[1], want) and v[2].tolist() == [label_of[r] for r in want.tolist()], c
    assert [c[1:3] for c in fit.checks] == [(0.25, 0.5)] * 6 and [c[3] for c in fit.checks] == [None, 0.5, 0.5, 0.5, 0.5, 0.5]
    # with validation_dropout the checks draw masks at the training rate
    eng = _Stub()
    T.fit_head(eng, cache, rows, labels, val_rows=val_rows, val_labels=val_labels, seed=5,
               params=T.TrainParams(batch_size=4, validate_on_batch=5, validation_steps=2, dropout=0.2, validation_dropout=True))
    assert [v[5] for v in eng.val] == [0.2] * 3
    # fewer validation rows than a check asks for: all of them, every time
    eng = _Stub()
    T.fit_head(eng, cache, rows, labels, val_rows=val_rows[:3], val_labels=val_labels[:3], seed=5,
               params=T.TrainParams(batch_size=4, validate_on_batch=6, validation_steps=2))
    assert [sorted(v[1].tolist()) for v in eng.val] == [[46, 47, 48]] * 2


def test_fit_head_stops_where_the_rule_says_and_override_sets_the_epoch():
    cache = _stub_cache()
    rows, labels = np.arange(0, 46, dtype=np.int64), (np.arange(46) % 2).astype(np.int64)
    val = dict(val_rows=np.arange(46, 60), val_labels=np.zeros(14, np.int64))
    accs = [0.5, 0.7, 0.9, 0.3, 0.9, 0.9]                                                  # the hand-worked sequence: stop at check 4
    p = T.TrainParams(batch_size=4, epochs=[3], early_stop=True, validate_on_batch=2, validation_steps=1, ema_observations=2)
    eng = _Stub(accs)
    fit = T.fit_head(eng, cache, rows, labels, params=p, seed=1, **val)
    assert fit.early_stop_batch == 8 == fit.steps and len(fit.checks) == 4 and len(eng.train) == 4 and fit.losses.shape == (8,)
    assert fit.checks[-1][3] == pytest.approx(0.2 + 0.8 / 3, abs=1e-15)
    # the same values without early_stop: recorded, never acted on
    eng = _Stub(accs)
    fit = T.fit_head(eng, cache, rows, labels, params=T.TrainParams(batch_size=4, validate_on_batch=2, validation_steps=1, ema_observations=2),
                     seed=1, **val)
    assert fit.early_stop_batch is None and fit.steps == 12 and len(fit.checks) == 6
    # by loss the stub's constant 0.25 has not improved at the first check with two priors
    eng = _Stub()
    fit = T.fit_head(eng, cache, rows, labels, seed=1, **val, params=T.TrainParams(
        batch_size=4, early_stop=True, early_stop_method='loss', validate_on_batch=1, validation_steps=1, ema_observations=1))
    assert fit.early_stop_batch == 3
    # steps_per_epoch_override: S = 8 steps of the first permutation, all full; S = 14 continues into the stream k = 1
    for S in (8, 14):
        eng = _Stub()
        fit = T.fit_head(eng, cache, rows, labels, params=T.TrainParams(batch_size=4, epochs=[2], steps_per_epoch_override=S), seed=1)
        assert fit.steps == 2 * S and [t[3] for t in eng.train] == [0, S] and fit.checks == []
        for e, t in enumerate(eng.train):
            assert np.array_equal(t[0], rows[T.epoch_order(46, 4 * S, 1, e)]) and len(t[0]) == 4 * S
    assert np.array_equal(eng.train[1][0][:46], rows[np.random.default_rng([1, 1]).permutation(46)])
    # balanced: the epoch's draws are balanced_rows', its offsets carried from epoch to epoch
    eng = _Stub()
    T.fit_head(eng, cache, rows, labels, params=T.TrainParams(batch_size=4, epochs=[2], training_balance='slide'), seed=1)
    state, sidx = {}, cache.slide_idx[rows]
    for e, t in enumerate(eng.train):
        want = T.balanced_rows(rows, sidx, labels, None, 'slide', 46, 1, e, state)
        assert np.array_equal(t[0], rows[want]) and np.array_equal(t[1], labels[want])
    with pytest.raises(ValueError):
        T.fit_head(_Stub(), cache, rows, labels, val_rows=np.array([60]), val_labels=np.array([0]), seed=1)
    with pytest.raises(ValueError, match='4096'):                          # a check of 5 x 1024 rows, and that many to walk
        T.fit_head(_Stub(), cache, rows, labels, seed=1, val_rows=np.arange(5200) % 60, val_labels=np.zeros(5200, np.int64),
                   params=T.TrainParams(batch_size=1024, validation_steps=5))


def test_train_cv_writes_the_results_log_of_a_trainer_that_returns_a_fit(tmp_path):
    from tests.test_train import _Stub as TableStub, _cohort as cohort
    cache, labels, patients = cohort()
    table = TableStub(cache, labels)
    stops = iter((6, None, 9))

    def trainer(train_rows, val_rows, seed):
        return (*table(train_rows, val_rows, seed), T.FitResult({}, np.zeros(9, np.float32), [(9, 0.5, 0.75, 0.7)], next(stops), 9))
    dirs = T.train_cv(cache, labels, str(tmp_path), 'EXP', 3, trainer, patients=patients, seed=1)
    cols = [list(pd.read_csv(os.path.join(d, T.RESULTS_FILE)).columns) for d in dirs]
    assert ['early_stop_batch' in c for c in cols] == [True, False, True] and T.find_cv_early_stop(str(tmp_path), 'EXP') is None
    T.train_cv(cache, labels, str(tmp_path), 'OLD', 3, table, patients=patients, seed=1)             # a trainer of two values: no log
    assert not os.path.exists(os.path.join(T.fold_dir(str(tmp_path), 'OLD', 1), T.RESULTS_FILE))


def test_command_line_refuses_full_without_early_stop(tmp_path):
    base = ['a.tfrecords', '--labels', 'l.csv', '--model', str(tmp_path), '--out', str(tmp_path / 'out')]
    with pytest.raises(SystemExit, match='--early-stop'):
        T.main(base + ['--full'])
    with pytest.raises(SystemExit, match='--validation-steps'):
        T.main(base + ['--early-stop', '--validation-steps', '0'])
    with pytest.raises(SystemExit):
        T.main(base + ['--balance', 'class'])
    assert not (tmp_path / 'out').exists()
