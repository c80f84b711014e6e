"""SHA-256 of head training's results on fixed synthetic inputs -- ``head_grad``, ``head_adam``, ``head_train_steps``,
``head_validate`` and ``train.fit_head`` -- : run before and after a change to csrc/kernels_train.hip, the engine's head calls or
train.py that must be bit-identical (GPU only).  usage: python tools/train_hash.py"""
import hashlib, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from biscuit_amd import train as T
from biscuit_amd.engine import Engine
from biscuit_amd.weights import synthetic_weights
from tests import _train_ref as R
from tests import _validate_ref as V


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p.cpu().numpy().tobytes() if torch.is_tensor(p) else p.tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()[:16]


eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
feats, params = up(R.cache()), up(T.flatten_head(R.head()))
for n in (1, 3, 33, 128):
    for rate in (0.0, 0.1):
        rows, labels = R.grad_case(n, 'mixed')
        g, loss = eng.head_grad(params, feats, up(rows), up(labels), 3, R.SEED, rate=rate)
        print(f'head_grad n={n} rate={rate} {sha(g, loss)}')
w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
for step in (0, 1000):                                                  # (g: n = 128 at rate 0.1)
    eng.head_adam(w, m, v, g, step, 1e-3)
    print(f'head_adam step={step} {sha(w, m, v)}')

rng = np.random.default_rng(3)                                          # the seven steps of tests/test_gpu_train.py, the last batch short
rows = np.concatenate([rng.permutation(R.CACHE_ROWS) for _ in range(3)])[:6 * 16 + 8].astype(np.int64)
labels = rng.integers(0, 2, len(rows)).astype(np.uint8)
w, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
losses = eng.head_train_steps(w, m, v, feats, up(rows), up(labels), 16, 0, 9, [1e-3 * 0.98 ** i for i in range(7)], rate=0.1)
print(f'head_train_steps {sha(w, m, v, losses)}')

f, head, rows, labels = V.inputs()
feats, params, rows, labels = up(f), up(T.flatten_head(head)), up(rows), up(labels)
for n in (1, 65, 1025, 4096):
    for rate in (0.0, 0.1):
        out = eng.head_validate(params, feats, rows[:n].contiguous(), labels[:n].contiguous(), V.PASS, V.SEED, rate=rate, rowloss=True, hit=True)
        print(f'head_validate n={n} rate={rate} {sha(*out)}')

rng = np.random.default_rng(8)                                          # 12 slides x 40 tiles, the classes apart in mean; two views
sidx = np.repeat(np.arange(12), 40).astype(np.int64)
f = np.abs(rng.standard_normal((3, 480, 2048))).astype(np.float32)
f[:, sidx % 2 == 1] += np.float32(0.05) * (np.arange(2048) % 2 == 0)
loc = np.stack([np.arange(480), np.zeros(480, np.int64)], 1).astype(np.int64)
plain = T.FeatureCache(up(f[0]), sidx, loc, [f's{i:02d}' for i in range(12)])
viewed = T.FeatureCache(up(f[0]), sidx, loc, plain.slides, up(f[1:]), 'xy', 1)
train, val = np.flatnonzero(sidx < 9).astype(np.int64), np.flatnonzero(sidx >= 9).astype(np.int64)
held = {'val_rows': val, 'val_labels': sidx[val] % 2}
for name, cache, p, kw in (
        ('plain', plain, T.TrainParams(batch_size=32, epochs=[2]), {}),
        ('early_stop', plain, T.TrainParams(batch_size=32, epochs=[2], early_stop=True, validate_on_batch=4, validation_steps=2,
                                            ema_observations=2), held),
        ('category_views', viewed, T.TrainParams(batch_size=32, epochs=[2], training_balance='category', augment='xy'), {})):
    fit = T.fit_head(eng, cache, train, sidx[train] % 2, init='glorot', params=p, seed=6, **kw)
    print(f'fit_head {name} steps={fit.steps} stop={fit.early_stop_batch} checks={len(fit.checks)} '
          f'{sha(*(fit.head[k] for k, _ in T.HEAD_TENSORS), fit.losses, fit.checks)}')
eng.close()
