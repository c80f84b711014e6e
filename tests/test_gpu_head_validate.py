"""``bq_head_validate`` (csrc/kernels_train.hip; DESIGN.md section 7 "Training schedule") against the float64 restatement of
tests/_validate_ref.py: 4096 half-normal feature rows (one all zeros), ``_train_ref.head()``, the first n rows of one fixed order.
The tolerance is the rule of tests/test_gpu_train.py: 8 x the float32 twin's own distance from float64 for the same case.
``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from biscuit_amd import train as T
from tests import _poison as P
from tests import _train_ref as R
from tests import _validate_ref as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    e = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    yield e
    e.close()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


@pytest.fixture(scope='module')
def dev(eng):
    """The inputs on the device: ``(feats, params, rows, labels)``."""
    f, w, rows, labels = V.inputs()
    return up(eng, f), up(eng, T.flatten_head(w)), up(eng, rows), up(eng, labels)


@pytest.fixture(scope='module')
def refs():
    return {rate: V.reference(rate) for rate in V.RATES}


_RUNS = {}


def run(eng, dev, n, rate, **kw):
    """``(stats [2], rowloss [n], hit [n])`` of the first n rows on the host, one call per case."""
    if (n, rate) not in _RUNS or kw:
        feats, params, rows, labels = dev
        out = eng.head_validate(params, feats, rows[:n].contiguous(), labels[:n].contiguous(), V.PASS, V.SEED, rate=rate, rowloss=True,
                                hit=True, **kw)
        got = tuple(t.cpu().numpy() for t in out)
        if kw:
            return got
        _RUNS[n, rate] = got
    return _RUNS[n, rate]


def same_bits(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize('n', V.NS)
def test_losses_within_eight_twin_errors(eng, dev, refs, n):
    for rate in V.RATES:
        ref = refs[rate]
        stats, rowloss, _ = run(eng, dev, n, rate)
        twin, floor = V.twin(ref, n), V.twin_floor(ref, n)
        err = (R.rel_err(rowloss, ref['loss64'][:n]), R.rel_err(stats[0] / n, ref['loss64'][:n].mean()))
        for what, e, t, f in zip(('rowloss', 'mean'), err, twin, floor):
            print(f'n={n} rate={rate} {what}: device {e:.3e} twin {t:.3e} ratio {e / t:.2f} (the twin\'s floor {f:.3e})')
        for what, e, t, f in zip(('rowloss', 'mean'), err, twin, floor):
            assert t >= f, (n, rate, what, 'the twin\'s figure is no sample of float32\'s error', t, f)
            assert e <= 8 * t, (n, rate, what, e, t)


# ------------------------------------------------------------------------------------------------ 2. hits
@pytest.mark.parametrize('n', V.NS)
def test_hits_equal_float64_beyond_the_margin(eng, dev, refs, n):
    for rate in V.RATES:
        ref = refs[rate]
        stats, _, hit = run(eng, dev, n, rate)
        sure = ref['margin'][:n] > V.MARGIN
        print(f'n={n} rate={rate}: {int((~sure).sum())} rows within the margin, {int(hit.sum())} hits, class 1 predicted for '
              f'{ref["pred1"]:.3f} of all rows')
        assert (~sure).sum() <= 0.01 * n
        assert np.array_equal(hit[sure], ref['hit'][:n][sure])
        assert set(np.unique(hit)) <= {0, 1} and stats[1] == float(hit.sum())
    assert 0.4 < refs[0.0]['pred1'] < 0.6                       # (neither class alone: the count is not trivial)


# ------------------------------------------------------------------------------------------------ 3. a row is a row
@pytest.mark.parametrize('rate', (0.0, 0.1))
def test_a_row_does_not_depend_on_its_call(eng, dev, rate):
    feats, params, rows, labels = dev
    _, loss_all, hit_all = run(eng, dev, 4096, rate)
    for a, b in ((0, 1), (4000, 4001), (100, 165), (4031, 4096)):                     # calls of 1 and of 65 rows
        _, loss, hit = (t.cpu().numpy() for t in eng.head_validate(params, feats, rows[a:b].contiguous(), labels[a:b].contiguous(), V.PASS,
                                                                  V.SEED, rate=rate, rowloss=True, hit=True))
        assert same_bits((loss, hit), (loss_all[a:b], hit_all[a:b])), (rate, a, b)
    for n in (1, 65):
        _, loss, hit = run(eng, dev, n, rate)
        assert same_bits((loss, hit), (loss_all[:n], hit_all[:n])), (rate, n)


# ------------------------------------------------------------------------------------------------ 4. the training kernel's loss
@pytest.mark.parametrize('n', (1, 33, 128))
def test_mean_loss_is_head_grads_loss(eng, dev, n):
    feats, params, rows, labels = dev
    for rate in V.RATES:
        r, y = rows[:n].contiguous(), labels[:n].contiguous()
        _, loss = eng.head_grad(params, feats, r, y, V.PASS, V.SEED, rate=rate)
        stats, _, _ = eng.head_validate(params, feats, r, y, V.PASS, V.SEED, rate=rate)
        want, got = np.float32(loss.cpu().numpy()[0]), np.float32(float(stats[0]) / n)
        assert abs(float(got) - float(want)) <= float(np.spacing(np.abs(want))), (n, rate, got, want)


# ------------------------------------------------------------------------------------------------ 5. the contract
def test_same_bits_again_and_on_poisoned_scratch(eng, dev):
    feats, params, rows, labels = dev
    before = params.clone()
    for n, rate in ((65, 0.0), (65, 0.1), (1025, 0.1)):
        first = run(eng, dev, n, rate)
        assert same_bits(first, run(eng, dev, n, rate, scratch=None))
        need = int(eng._lib.bq_head_validate_workspace_bytes(n))
        assert eng.validate_scratch(n).numel() == need > 0
        for fill in P.BYTE_FILLS:
            scratch, check = P.guarded(need, fill, eng.device)
            got = run(eng, dev, n, rate, scratch=scratch)
            torch.cuda.synchronize(eng.device)
            check()
            assert same_bits(first, got), (n, rate, hex(fill))
    assert torch.equal(params.view(torch.int32), before.view(torch.int32))              # only read
    assert 'validate' in eng._tool_ws and eng.HEAD_VALIDATE_MAX_ROWS == 4096


def test_sizes_and_refusals(eng, dev):
    from biscuit_amd.engine import BiscuitHipError
    feats, params, rows, labels = dev
    lib = eng._lib
    assert lib.bq_head_validate_workspace_bytes(0) == 0 and lib.bq_head_validate_workspace_bytes(4097) == 0
    assert lib.bq_head_validate_workspace_bytes(4096) > 0 and lib.bq_head_train_workspace_bytes(1025) == 0
    need = int(lib.bq_head_validate_workspace_bytes(64))
    with pytest.raises(BiscuitHipError, match='workspace'):
        eng.head_validate(params, feats, rows[:64].contiguous(), labels[:64].contiguous(), 0, 1, scratch=eng._bytes(need - 256))
    stats = torch.full((2,), 7.0, dtype=torch.float64, device=eng.device)
    ws = eng.validate_scratch(64)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = lambda n, nbytes: lib.bq_head_validate(eng._ctx, ptr(params), ptr(feats), int(feats.shape[0]), ptr(rows), ptr(labels), n, 0, 1, 0.0,
                                                  ptr(stats), None, None, ptr(ws), nbytes, eng._stream())
    assert call(0, ws.numel()) == -1 and call(4097, ws.numel()) == -1            # BQ_ERR_ARG
    assert call(64, need - 1) == -4                                               # BQ_ERR_WORKSPACE
    torch.cuda.synchronize(eng.device)
    assert stats.tolist() == [7.0, 7.0]                                           # nothing was enqueued
    assert call(64, ws.numel()) == 0
    al = lambda b: (b + 255) & ~255                 # include/biscuit_hip.h: h0 | h1, each [n][1024] f32 | rowloss f64 [n] | hit u8 [n]
    for n in (1, 63, 64, 65, 1024, 1025, 4096):
        assert lib.bq_head_validate_workspace_bytes(n) == 2 * al(n * 1024 * 4) + al(n * 8) + al(n), n

    def refused(code, text, params_at=params.data_ptr(), n_feat=int(feats.shape[0]), n=64, pass_=0, rate=0.0, rowloss_at=0, nbytes=ws.numel()):
        """One refused call, a branch of the argument check each: the code and the text of ``bq_last_error``."""
        rc = lib.bq_head_validate(eng._ctx, C.c_void_p(params_at), ptr(feats), n_feat, ptr(rows), ptr(labels), n, pass_, 1, rate, ptr(stats),
                                  C.c_void_p(rowloss_at), None, ptr(ws), nbytes, eng._stream())
        assert (rc, lib.bq_last_error(eng._ctx).decode()) == (code, 'bq_head_validate: ' + text)

    stats.fill_(7.0)
    pointers = ('bad argument (null pointer, params or feats not 16-byte, rows, stats or rowloss not 8-byte or the workspace not 256-byte '
                'aligned)')
    refused(-1, '1 <= n <= 4096', n=0)
    refused(-1, '1 <= n <= 4096', n=4097)
    refused(-1, 'an empty feature cache, or a pass outside 0 .. 2^32 - 1', n_feat=0)
    refused(-1, 'an empty feature cache, or a pass outside 0 .. 2^32 - 1', pass_=1 << 32)
    refused(-1, 'the rate must lie in [0, 1)', rate=1.0)
    refused(-1, pointers, params_at=params.data_ptr() + 4)
    refused(-1, pointers, rowloss_at=stats.data_ptr() + 4)
    refused(-4, 'workspace below bq_head_validate_workspace_bytes(n)', nbytes=need - 1)
    torch.cuda.synchronize(eng.device)
    assert stats.tolist() == [7.0, 7.0]                                           # nothing was enqueued
    with pytest.raises(ValueError):
        eng.head_validate(params, feats, rows[:0], labels[:0], 0, 1)
    with pytest.raises(ValueError):
        eng.head_validate(params, feats, torch.cat([rows, rows[:1]]), torch.cat([labels, labels[:1]]), 0, 1)
    with pytest.raises(ValueError):
        eng.head_validate(params, feats, rows[:4].contiguous(), labels[:4].contiguous(), 0, 1, rate=1.0)


@pytest.mark.parametrize('rate', (0.0, 0.1))
def test_a_bad_row_is_nan_and_the_others_are_unchanged(eng, dev, rate):
    feats, params, rows, labels = dev
    n, at = 65, 40
    r, y = rows[:n].contiguous(), labels[:n].contiguous()
    _, loss0, hit0 = run(eng, dev, n, rate)
    others = np.arange(n) != at

    def check(feats_, r_, y_, why):
        stats, loss, hit = (t.cpu().numpy() for t in eng.head_validate(params, feats_, r_, y_, V.PASS, V.SEED, rate=rate, rowloss=True, hit=True))
        assert np.isnan(stats[0]) and np.isnan(loss[at]) and hit[at] == 0, why
        assert same_bits((loss[others], hit[others]), (loss0[others], hit0[others])), why
        assert stats[1] == float(hit.sum()), why

    for value in (float('nan'), float('inf')):
        for unit in range(4):                       # kept or dropped: every unit of a Philox group
            bad = feats.clone()
            bad[int(r[at]), 100 + unit] = value
            check(bad, r, y, (value, unit))
    far = r.clone()
    far[at] = feats.shape[0]                        # outside the cache: never read
    check(feats, far, y, 'row')
    two = y.clone()
    two[at] = 2
    check(feats, r, two, 'label')
