"""The stain normaliser alone (bq_stain_reinhard_fast: hp.py:19's `reinhard_fast`, results.py:251-252): ms per batch of 256 tiles
(HIP events, 20 repetitions after a warm-up) and the uint8 result against oracle/stain.py on 6 tiles; then, in the same run, the
four flag values of the Reinhard family (bq_stain_reinhard: 0 reinhard_fast, 1 reinhard, 2 reinhard_fast_mask, 3 reinhard_mask) on
256 resident tiles a user would run -- synthetic H&E-like tiles, a third of them half glass -- with reinhard_fast's kernel timed on
the same tiles next to them, alternating, three rounds (the median is reported).  python tools/bench_stain.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from biscuit_amd.engine import Engine                     # noqa: E402
from biscuit_amd.synthetic import make_tiles              # noqa: E402
from biscuit_amd.weights import synthetic_weights         # noqa: E402
from oracle import stain                                  # noqa: E402

eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
g = torch.Generator(device='cuda').manual_seed(1)
big = torch.randint(0, 256, (256, 299, 299, 3), dtype=torch.uint8, device='cuda', generator=g)
out = torch.empty_like(big)
tm, ts = [65.0, 12.0, -8.0], [14.0, 7.0, 6.0]
for _ in range(3):
    eng.reinhard_fast(big, tm, ts, out=out)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(20):
    eng.reinhard_fast(big, tm, ts, out=out)
b.record(); b.synchronize()
ms = a.elapsed_time(b) / 20
small = np.concatenate([make_tiles(3, seed=5, grain=4.0, slide_bias=[30, -40, 20]), big[:3].cpu().numpy()])
want = stain.reinhard_fast(small, np.float32(tm), np.float32(ts))
got = eng.reinhard_fast(torch.from_numpy(small).cuda(), tm, ts).cpu().numpy()
d = np.abs(got.astype(int) - want.astype(int))
st = eng.lab_stats(torch.from_numpy(small).cuda()).cpu().numpy()
L, A, B = stain.rgb_to_lab(small)
mu, sd = stain.lab_stats(L, A, B)
print(f'reinhard_fast: {ms:.4f} ms per 256 tiles ({256 * 89401 / ms / 1e6:.1f} G pixels/s; 137 MB in + out: {0.137 / ms * 1e3:.0f} GB/s); '
      f'vs oracle on 6 tiles: max |d| {d.max()}, differing bytes {int((d != 0).sum())} of {d.size}; '
      f'stats max |d| {max(np.abs(st[:, :3] - mu).max(), np.abs(st[:, 3:] - sd).max()):.2e}')


# ---- the Reinhard family next to reinhard_fast, same tiles, same run
from biscuit_amd.stain import REINHARD_FLAGS              # noqa: E402


def _ms(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / reps


he = make_tiles(256, seed=9, grain=4.0)
he[::3, :, 150:] = np.random.default_rng(9).integers(240, 256, he[::3, :, 150:].shape, dtype=np.uint8)      # every third tile: half glass
for label, tiles in (('uniform noise', big), ('synthetic tissue, a third half glass', torch.from_numpy(he).cuda())):
    runs = {'reinhard_fast (bq_stain_reinhard_fast)': lambda: eng.reinhard_fast(tiles, tm, ts, out=out)}
    for name, flags in sorted(REINHARD_FLAGS.items(), key=lambda kv: kv[1]):
        runs[f'flags {flags} {name} (bq_stain_reinhard)'] = lambda flags=flags: eng.reinhard(tiles, tm, ts, flags, out=out)
    times = {k: [] for k in runs}
    for _ in range(3):
        for k, fn in runs.items():
            times[k].append(_ms(fn))
    base = float(np.median(times['reinhard_fast (bq_stain_reinhard_fast)']))
    st = torch.empty(256, dtype=torch.int32, device='cuda')
    eng.reinhard(tiles, tm, ts, 3, out=out, status=st)
    print(f'{label}: 256 tiles of 299 px, ms per batch (median of 3 rounds of 20; all rounds); status != 0 under flags 3: {int(st.ne(0).sum())}')
    for k, v in times.items():
        med = float(np.median(v))
        print(f'  {k:48s} {med:.4f} ms  x{med / base:.2f}  ({", ".join(f"{x:.4f}" for x in v)})')
assert torch.equal(eng.reinhard(big[:8], tm, ts, 0), eng.reinhard_fast(big[:8], tm, ts))
