"""BASELINE.json configs 3, 4 and 5 and the parity stress set, on the MI355X (``-m gpu``).

* config 3 (slides sharded over ranks, one gather): two ranks on ONE GPU -- the real ``Engine`` in each,
  an explicit local device 0 + a gloo process group -- must reproduce the single-rank result exactly; and
  ``bench.py --gpus 2`` must start its own two ranks.
* config 4 (MC sweep N in {1,5,10,30,50}): the fused on-device Welford ('head') is bit-identical to N separate
  complete passes ('full') at every N, and matches the CPU oracle at N <= 10.
* config 5 (TFRecords + checkpoint + params.json -> CLI -> CSV -> threshold.apply): the harness on self-written
  records and an exported Keras-format checkpoint (no TCGA data exists here), equal to the in-memory path.
* stress weights (``synthetic_weights(hard=True)``): O(1) logits, BatchNorm statistics far from identity.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from biscuit_amd.synthetic import make_slides, make_tiles
from biscuit_amd.weights import synthetic_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------------------------------------ config 3
# [9, 4, 0, 7, 5, 3] partitions into contiguous runs of slides; [9, 3, 7, 4, 5] does not (rank 0 gets slides 0 and 3, rank 1
# slides 1, 2 and 4): rank 0's second batch is tile 8 of slide 0 + the four tiles of slide 3, two runs of Philox tile indices --
# one bq_mc_infer call with the indices as an array (bq_set_tile_index_array; round 4: features once, one head call per run):
# the same kernels as the single-run batches of the one-rank reference, so the same bits
@pytest.mark.parametrize('counts,dtype', [([9, 4, 0, 7, 5, 3], 'bf16'), ([9, 3, 7, 4, 5], 'f16'), ([9, 3, 7, 4, 5], 'bf16')])
def test_two_ranks_on_one_gpu_equal_single_rank(tmp_path, counts, dtype):
    from _rank_worker import build_slides
    from biscuit_amd import distributed as D
    from biscuit_amd.engine import Engine
    from biscuit_amd.inference import evaluate
    mc_n, batch = 6, 8
    if len(counts) == 5:
        parts = D.partition_slides(counts, 2)
        assert parts == [[0, 3], [1, 2, 4]], parts          # the case exists: rank 0's slides are not neighbours
    out = str(tmp_path / 'res')
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), BQ_TEST_SAVE_DIR=str(tmp_path / 'multi'))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', '_rank_worker.py'), out, dtype,
                                       str(mc_n), str(batch), ','.join(map(str, counts)), '0', 'gloo'], env=env, cwd=ROOT))
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    eng = Engine(synthetic_weights(1), dtype=dtype, max_batch=batch, max_mc=mc_n)
    single = evaluate(eng, build_slides(counts), mc_n=mc_n, seed=77, batch=batch, save_dir=str(tmp_path / 'single'))
    # THE product of the path (experiment.py:688-699 reads ONE tile_predictions_eval.csv): each rank streamed its shard while its
    # GPU worked and closed it before the gather, rank 0 spliced them -- the single-rank file byte for byte, which is also
    # to_csv of the frame; the consumer finds the same thresholds on it (threshold.detect: Youden over every tile, threshold.py:417-426)
    from biscuit_amd import predictions as P, threshold
    whole = os.path.join(str(tmp_path / 'multi'), P.EVAL_NAME)
    assert open(whole, 'rb').read() == open(single.table_path, 'rb').read()
    assert open(P.save_tile_predictions(single.tile_df, str(tmp_path / 'pandas')), 'rb').read() == open(whole, 'rb').read()
    assert len(P.find_shards(str(tmp_path / 'multi'))) == 2
    df_m, df_s = P.load_tile_predictions(str(tmp_path / 'multi'), 'cohort'), P.load_tile_predictions(single.table_path, 'cohort')
    assert df_m.equals(df_s) and len(df_s) == sum(counts)
    assert threshold.detect(df_m.copy())[0] == threshold.detect(df_s.copy())[0]
    r0, r1 = (np.load(f'{out}.rank{r}.npz') for r in range(2))
    # both ranks hold the whole gathered slide table, equal to the single-rank one bit for bit
    for r in (r0, r1):
        assert np.array_equal(r['slide_pred'], single.slide_pred, equal_nan=True)
        assert np.array_equal(r['slide_unc'], single.slide_unc, equal_nan=True)
        assert list(r['slide_count']) == counts
    assert sorted(list(r0['local']) + list(r1['local'])) == list(range(len(counts)))
    # tile rows stay rank-local; together they are the single-rank table (Philox counters are global tile indices)
    got = pd.DataFrame({'slide': np.concatenate([r0['tile_slide'], r1['tile_slide']]),
                        'p': np.concatenate([r0['tile_pred'], r1['tile_pred']]),
                        'u': np.concatenate([r0['tile_unc'], r1['tile_unc']])})
    want = single.tile_df
    for name in set(want['slide']):
        a = got[got['slide'] == name]; b = want[want['slide'] == name]
        assert np.array_equal(a['p'].to_numpy(), b['cohort-y_pred1'].to_numpy())
        assert np.array_equal(a['u'].to_numpy(), b['cohort-uncertainty1'].to_numpy())
    eng.close()


def test_rccl_communicator_carries_the_gather(tmp_path):
    """The `nccl` branch of the N > 1 path on hardware, as far as a one-GPU box allows (RCCL refuses two ranks on one device):
    a real RCCL communicator of ONE rank carries `gather_slide_results`' all-gather (a float64 CUDA buffer through
    ncclAllGather) and the closing barrier; the result equals the group-less run bit for bit."""
    from _rank_worker import build_slides
    from biscuit_amd.engine import Engine
    from biscuit_amd.inference import evaluate
    counts = [5, 0, 9, 3]
    mc_n, batch = 4, 8
    out = str(tmp_path / 'res')
    env = dict({k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')},
               RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_rank_worker.py'), out, 'f16', str(mc_n), str(batch),
                        ','.join(map(str, counts)), '0', 'nccl', 'group1'], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    g = np.load(f'{out}.group.npz')
    assert str(g['backend']) == 'nccl' and int(g['size']) == 1
    r0 = np.load(f'{out}.rank0.npz')
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=batch, max_mc=mc_n)
    single = evaluate(eng, build_slides(counts), mc_n=mc_n, seed=77, batch=batch)
    assert np.array_equal(r0['slide_pred'], single.slide_pred, equal_nan=True)
    assert np.array_equal(r0['slide_unc'], single.slide_unc, equal_nan=True)
    assert list(r0['slide_count']) == counts
    eng.close()


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no torchrun environment: the parent spawns two ranks before touching the
    GPU and relays rank 0's JSON line (here both ranks share GPU 0: --local-device 0 --dist-backend gloo)."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    common = ['--local-device', '0', '--dist-backend', 'gloo', '--steps', '2', '--warmup', '1', '--batch', '16', '--mc', '5', '--streams', '1', '--no-extras',
              '--no-cpu-baseline', '--no-profile']
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'] + common, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['scaling'] == 'weak' and line['value'] > 0 and line['steps'] == 2
    # the collective really spanned both ranks (gloo here, so it is not counted as RCCL)
    assert line['collective'] == {'backend': 'gloo', 'ranks_seen': 2, 'rccl_ranks': 0} and line['rccl_ranks'] == 0
    # the strong-scaling form of config 3 (scaled down): slides LPT-sharded through inference.evaluate
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--workload', 'cfg3', '--slides', '6',
                        '--tiles-per-slide', '40'] + common, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['scaling'] == 'strong' and line['config']['slides_per_rank'] == [3, 3]
    # a WORLD_SIZE / --gpus mismatch is an error, not a silent single-rank run
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'] + common,
                         env=dict(env, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0'), cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode != 0 and 'WORLD_SIZE' in bad.stderr


def _json_line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])


def test_plain_bench_run_times_only_the_headline(tmp_path):
    """`python bench.py --gpus 1` without --full: the headline, its dumped outputs and nothing that takes runs of its own;
    --full (here without the TFRecord / storage-type / CPU legs) still adds the other MC mode and the per-kernel roofline."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'LOCAL_WORLD_SIZE')}
    common = ['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '16', '--mc', '5']
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *common, *a], env=env, cwd=ROOT,     # noqa: E731
                                    capture_output=True, text=True, timeout=600)
    legs = {'full_mode_value', 'with_reinhard_value', 'bf16_value', 'f32_value', 'b1_latency', 'tfrecords', 'host_tiles',
            'cpu_baseline', 'roofline', 'kernels', 'entry_side_ms', 'leg_seconds'}
    plain = _json_line(run('--dump-outputs', str(tmp_path)))
    assert plain['value'] > 0 and plain['steps'] == 2 and plain['warmup'] == 1 and plain['dtype'] == 'f16'
    assert abs(plain['ms_per_step'] - 16 / plain['value'] * 1e3) < 1e-9 * plain['ms_per_step']     # one batch of 16 per step
    assert not legs & set(plain), legs & set(plain)
    assert sorted(os.listdir(tmp_path)) == sorted(f'{n}.npy' for n in ('tile_mean', 'tile_std', 'slide_pred', 'slide_unc', 'slide_count'))
    full = _json_line(run('--full', '--no-extras', '--no-cpu-baseline'))
    assert full['full_mode_value'] > 0 and full['kernels'] and full['roofline']['kernel'] and 'leg_seconds' in full


# Ranks of the multi-rank rehearsal.  The suite keeps at most six processes on the GPU at a time, and this test's own process
# holds it too: five ranks.  (Eight ranks -- BASELINE config 3's world -- run in tests/test_distributed.py
# with stand-in engines, on the CPU.)
REHEARSAL_WORLD = 5


def test_multi_rank_rehearsal_on_one_gpu(tmp_path):
    """What the driver runs at N > 1, end to end with real engines on the ONE GPU of this box (REHEARSAL_WORLD HIP contexts on
    device 0, a gloo group: RCCL refuses several ranks on one device): ``bench.py --gpus N`` on config 2 and on a ragged config 3
    with the tile table, and the CLI at world N with the shards spliced and the consumer run by rank 0 -- rank 0's results equal
    to the single-rank run bit for bit (digests of the slide table and of tile_predictions_eval.csv, the printed metrics)."""
    n = REHEARSAL_WORLD
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'LOCAL_WORLD_SIZE')}
    common = ['--local-device', '0', '--dist-backend', 'gloo', '--batch', '16', '--mc', '5', '--streams', '1', '--no-extras',
              '--no-cpu-baseline', '--no-profile']
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *a, *common], env=env, cwd=ROOT,     # noqa: E731
                                    capture_output=True, text=True, timeout=1500)
    wn = _json_line(run('--gpus', str(n), '--steps', '2', '--warmup', '1'))
    assert wn['n_gpus'] == n and wn['scaling'] == 'weak' and wn['value'] > 0
    assert wn['collective'] == {'backend': 'gloo', 'ranks_seen': n, 'rccl_ranks': 0}
    assert wn['host_cores_of_rank0'] >= 1                       # pin_rank against this box's sysfs: a share, never empty
    # the DRIVER's form of the same: torchrun starts the ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from its environment)
    tr = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4', '--master-addr', '127.0.0.1',
                         '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '2', '--warmup', '1',
                         *common], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    w4 = _json_line(tr)
    assert w4['n_gpus'] == 4 and w4['steps'] == 2 and w4['collective']['ranks_seen'] == 4 and w4['value'] > 0
    cfg3 = ['--workload', 'cfg3', '--slides', '19', '--tiles-per-slide', '24', '--ragged', '--full']     # --full: the tile-table run
    sn, s1 = _json_line(run('--gpus', str(n), *cfg3)), _json_line(run('--gpus', '1', *cfg3))
    assert sn['n_gpus'] == n and sn['config']['ragged'] and sum(sn['config']['slides_per_rank']) == 19
    assert sn['slide_table_sha256'] == s1['slide_table_sha256']
    assert sn['tile_table']['sha256'] == s1['tile_table']['sha256'] and sn['tile_table']['rows'] == s1['tile_table']['rows'] > 0
    # the CLI: n ranks, shards spliced by rank 0, threshold.detect / apply on THE table
    counts = '9,3,7,4,5,0,11,6,2,8,1,10'
    cli = [sys.executable, '-m', 'biscuit_amd', '--synthetic', counts, '--batch', '8', '--mc', '5', '--detect', '--local-device', '0',
           '--dist-backend', 'gloo']
    port = _free_port()
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1',
                 MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cli + ['--out', str(tmp_path / 'wn')], env=e, cwd=ROOT, text=True,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE if r == 0 else None))
    out0, err0 = procs[0].communicate(timeout=900)
    assert [p.wait(timeout=300) for p in procs] == [0] * n, err0[-3000:]
    one = subprocess.run(cli + ['--out', str(tmp_path / 'w1')], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    a = json.loads([ln for ln in out0.splitlines() if ln.startswith('{')][-1])
    b = _json_line(one)
    assert a.pop('world') == n and b.pop('world') == 1
    ta, tb = a.pop('tile_table'), b.pop('tile_table')
    assert a == b and a['tiles'] == 66 and 'auc' in a and 'detected' in a, (a, b)
    assert open(ta, 'rb').read() == open(tb, 'rb').read()
    name = 'slide_predictions_cohort_eval.csv'
    assert open(tmp_path / 'wn' / name, 'rb').read() == open(tmp_path / 'w1' / name, 'rb').read()


def test_config3_one_ranks_share_at_real_size():
    """BASELINE.json config 3 at its real size, the part one GPU runs: rank 0's share of 1 600 slides x 1 000 tiles over 8
    ranks = 200 slides x 1 000 tiles (200 000 tiles, batches of 256 that span slides), through ``inference.evaluate``
    exactly as ``bench.py --workload cfg3`` drives it.  No oracle at this size: counts, the partition, bit-exact
    re-run, independence of the batches in flight, and per-slide means equal to direct ``mc_infer`` calls with the
    slide's global tile indices."""
    from biscuit_amd import distributed as D
    from biscuit_amd.engine import EnginePool
    from biscuit_amd.inference import Slide, evaluate
    S, T, world, B, mc_n = 1600, 1000, 8, 256, 30
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(3)
    pool_t = torch.randint(0, 256, (1024, 299, 299, 3), dtype=torch.uint8, device=dev, generator=g)   # resident tiles, cycled

    def tiles_of(i):
        def load():
            return pool_t.index_select(0, (torch.arange(T, device=dev) * 7 + i * 131) % pool_t.shape[0])
        return load
    slides = [Slide(f's{i:04d}', tiles_of(i), T, y_true=i % 2) for i in range(S)]
    parts = D.partition_slides([T] * S, world)
    assert [len(p) for p in parts] == [200] * world and sorted(sum(parts, [])) == list(range(S))
    mine = parts[0]
    pool = EnginePool(synthetic_weights(1), n_streams=2, dtype='f16', max_batch=B, max_mc=mc_n)
    runs = []
    for in_flight in (1, 2):
        pool.set_in_flight(in_flight)
        runs.append(evaluate(pool, slides, mc_n=mc_n, seed=1234, batch=B, keep_tiles=True, rank=0, world=world))
        pool.synchronize()
    a, b = runs
    # the gather did not run (this process is one rank of eight): slides of other ranks are unreported
    assert sorted(a.local_slides) == mine
    cnt = np.asarray(a.slide_count)
    assert cnt[mine].tolist() == [T] * 200 and int(cnt.sum()) == 200 * T
    assert len(a.tile_df) == 200 * T and a.tile_df['slide'].nunique() == 200
    # bit-exact whatever the number of batches in flight
    assert np.array_equal(a.slide_pred[mine], b.slide_pred[mine]) and np.array_equal(a.slide_unc[mine], b.slide_unc[mine])
    assert a.tile_df.equals(b.tile_df)
    assert np.isfinite(a.slide_pred[mine]).all() and (a.slide_unc[mine] > 0).all()
    yp = a.tile_df['cohort-y_pred1'].to_numpy(); un = a.tile_df['cohort-uncertainty1'].to_numpy()
    assert np.allclose(a.tile_df['cohort-y_pred0'].to_numpy() + yp, 1.0, atol=1e-6) and (un > 0).all() and (un < 0.5).all()
    # slide means = plain float64 means of the slide's tile rows (the consumer's groupby, threshold.py:191-192) ...
    names = a.tile_df['slide'].to_numpy()
    for si in (mine[0], mine[57], mine[-1]):
        rows = names == f's{si:04d}'
        assert rows.sum() == T
        assert abs(a.slide_pred[si] - yp[rows].mean()) < 1e-9 and abs(a.slide_unc[si] - un[rows].mean()) < 1e-9
    # ... and a slide's tile rows = direct calls on that slide alone with its GLOBAL tile indices (slide si starts at
    # tile si * T of the dataset: batches that span slides and the sharding change nothing)
    eng = pool.engines[0]
    si = mine[57]
    t = tiles_of(si)()
    m = torch.cat([eng.mc_infer(t[o:o + B].contiguous(), mc_n, 1234, tile_idx0=si * T + o)[0] for o in range(0, T, B)])
    assert np.array_equal(m[:, 1].double().cpu().numpy(), yp[names == f's{si:04d}'])
    pool.close()


# ------------------------------------------------------------------------------------------------ config 4
@pytest.fixture(scope='module')
def sweep_engines():
    from biscuit_amd.engine import Engine
    w = synthetic_weights(1)
    e = {'f32': Engine(w, dtype='f32', max_batch=8, max_mc=50), 'bf16': Engine(w, dtype='bf16', max_batch=8, max_mc=50),
         'f16': Engine(w, dtype='f16', max_batch=8, max_mc=50)}
    yield e
    for x in e.values():
        x.close()


@pytest.mark.parametrize('mc_n', [1, 5, 10, 30, 50])
def test_mc_sweep_fused_equals_separate_passes(sweep_engines, mc_n):
    tiles = make_tiles(5, seed=31)
    d = dev(tiles)
    for dtype in ('f32', 'bf16', 'f16'):
        eng = sweep_engines[dtype]
        m_h, s_h = eng.mc_infer(d, mc_n, 1234, tile_idx0=40, mc_mode='head')
        m_f, s_f = eng.mc_infer(d, mc_n, 1234, tile_idx0=40, mc_mode='full')
        assert torch.equal(m_h, m_f) and torch.equal(s_h, s_f), (dtype, mc_n)
        if mc_n == 1:
            assert torch.all(s_h == 0)
        else:
            assert torch.all(s_h > 0)
    if mc_n <= 10:
        from oracle.xception_ref import XceptionOracle
        rm, rs = XceptionOracle(synthetic_weights(1)).mc_predict(tiles, mc_n, 1234, tile_index0=40, mode='head')
        m, s = sweep_engines['f32'].mc_infer(d, mc_n, 1234, tile_idx0=40)
        assert np.abs(m.cpu().numpy() - rm).max() < 1e-5 and np.abs(s.cpu().numpy() - rs).max() < 1e-5


# ------------------------------------------------------------------------------------------------ config 5
def test_config5_harness_tfrecords_checkpoint_cli_threshold(tmp_path):
    """Self-written PNG TFRecords (configure.py:118-124) + a Keras-format checkpoint + params.json
    -> `python -m biscuit_amd --model` -> tile_predictions_eval.csv -> threshold.apply, against the in-memory path."""
    from biscuit_amd import keras_import as K, tfrecord as tfr, threshold
    from biscuit_amd.engine import Engine
    from biscuit_amd.inference import Slide, evaluate
    from biscuit_amd.predictions import rename_cols
    d = str(tmp_path)
    n_slides, per = 6, 7
    tiles, sidx, y = make_slides(n_slides, per, seed=3)
    rows = []
    for i in range(n_slides):
        t = tiles[sidx == i]
        tfr.write_slide(f'{d}/s{i}.tfrecords', f's{i}', t, np.arange(2 * len(t)).reshape(-1, 2))
        rows.append(f's{i},{int(y[i])},p{i // 2}')
    open(f'{d}/labels.csv', 'w').write('slide,label,patient\n' + '\n'.join(rows) + '\n')
    fit = {'target_means': [65.0, 12.0, -8.0], 'target_stds': [14.0, 7.0, 6.0]}
    w = synthetic_weights(1, hard=True)
    mdir = f'{d}/00001-cohort-HP0/cohort-HP0_epoch1'
    K.export_bundle(mdir + '/variables/variables', w, optimizer_slots=True)
    json.dump({'norm_fit': fit, 'hp': {'model': 'xception', 'tile_px': 299, 'hidden_layers': 2, 'hidden_layer_width': 1024,
                                        'dropout': 0.2, 'normalizer': 'reinhard_fast'}}, open(mdir + '/params.json', 'w'))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, '-m', 'biscuit_amd', '--tfrecords', d, '--labels', f'{d}/labels.csv', '--out',
                        f'{d}/eval', '--mc', '8', '--batch', '16', '--model', mdir, '--seed', '1234'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    summary = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert summary['slides'] == n_slides and summary['tiles'] == n_slides * per
    df = pd.read_csv(f'{d}/eval/tile_predictions_eval.csv', dtype={'slide': str})
    assert list(df.columns[:2]) == ['slide', 'cohort-y_true0'] or 'cohort-y_pred1' in df.columns
    # the in-memory path on the same tiles, the same model hyper-parameters (dropout 0.2 from params.json)
    from biscuit_amd.hp import ModelParams
    eng = Engine(w, hp=ModelParams(dropout=0.2), dtype='f16', max_batch=16, max_mc=8)
    slides = [Slide(f's{i}', tiles[sidx == i], per, y_true=int(y[i])) for i in range(n_slides)]
    mem = evaluate(eng, slides, outcome='cohort', mc_n=8, seed=1234, batch=16, norm_fit=fit)
    np.testing.assert_allclose(df['cohort-y_pred1'].to_numpy(), mem.tile_df['cohort-y_pred1'].to_numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(df['cohort-uncertainty1'].to_numpy(), mem.tile_df['cohort-uncertainty1'].to_numpy(), rtol=0, atol=1e-7)
    assert list(df['slide']) == list(mem.tile_df['slide'])
    # dropout 0.2 really was used: the default-rate engine gives other uncertainties
    eng01 = Engine(w, dtype='f16', max_batch=16, max_mc=8)
    other = evaluate(eng01, slides, outcome='cohort', mc_n=8, seed=1234, batch=16, norm_fit=fit)
    assert not np.allclose(other.tile_df['cohort-uncertainty1'].to_numpy(), df['cohort-uncertainty1'].to_numpy(), atol=1e-4)
    # consumer: the CSV through the reference's surface
    rename_cols(df, 'cohort')
    patients = {f's{i}': f'p{i // 2}' for i in range(n_slides)}
    metrics, _ = threshold.apply(df, tile_uq=0.0, slide_uq=0.0, patients=patients)
    assert set(metrics) >= {'auc', 'percent_incl', 'acc', 'sensitivity', 'specificity'}
    assert metrics['percent_incl'] == 1.0
    for k in ('auc', 'acc'):
        assert summary[k] is None or abs(summary[k] - float(metrics[k])) < 1e-12
    sl = pd.read_csv(f'{d}/eval/slide_predictions_cohort_eval.csv', dtype={'slide': str})
    np.testing.assert_allclose(sl['y_pred'].to_numpy(), mem.slide_pred, atol=1e-9)
    eng.close(); eng01.close()
    # the same command as THREE ranks (one GPU, gloo): every rank imports the model, calibrates on the same 16 tiles, decodes its
    # slides' TFRecords and streams its shard; rank 0 splices the table and runs the consumer -- the one-rank run's bytes and numbers
    port = _free_port()
    procs = []
    for r in range(3):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='3', LOCAL_WORLD_SIZE='3', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, '-m', 'biscuit_amd', '--tfrecords', d, '--labels', f'{d}/labels.csv', '--out',
                                       f'{d}/eval3', '--mc', '8', '--batch', '16', '--model', mdir, '--seed', '1234', '--local-device', '0',
                                       '--dist-backend', 'gloo'], cwd=ROOT, env=e, text=True,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE if r == 0 else None))
    out0, err0 = procs[0].communicate(timeout=900)
    assert [q.wait(timeout=300) for q in procs] == [0, 0, 0], err0[-3000:]
    s3 = json.loads([ln for ln in out0.splitlines() if ln.startswith('{')][-1])
    assert s3.pop('world') == 3 and summary.pop('world') == 1
    t3, t1 = s3.pop('tile_table'), summary.pop('tile_table')
    assert s3 == summary and open(t3, 'rb').read() == open(t1, 'rb').read()
    assert open(f'{d}/eval3/slide_predictions_cohort_eval.csv', 'rb').read() == open(f'{d}/eval/slide_predictions_cohort_eval.csv', 'rb').read()


def test_jpeg_tfrecords_feed_the_same_tiles(tmp_path):
    """Slideflow's other tile format: JPEG TFRecords through the reader's own baseline decoder (csrc/jpeg_baseline.h) and
    `evaluate` give exactly what the Pillow-decoded tiles give in memory -- the decoder is held to libjpeg's bytes
    (tests/test_jpeg.py), so the network sees the same image."""
    from biscuit_amd import tfrecord as tfr
    from biscuit_amd.engine import Engine
    from biscuit_amd.inference import Slide, evaluate, slides_from_tfrecords
    d = str(tmp_path)
    n_slides, per = 3, 9
    tiles, sidx, y = make_slides(n_slides, per, seed=5)
    paths, mem_slides = [], []
    for i in range(n_slides):
        p = f'{d}/j{i}.tfrecords'
        tfr.write_slide(p, f'j{i}', tiles[sidx == i], fmt='JPEG')
        paths.append(p)
        dec = np.stack([tfr.decode_image(tfr.parse_example(r)['image_raw']) for r in tfr.read_records(p)])   # Pillow
        assert not np.array_equal(dec, tiles[sidx == i])                 # lossy: the decoded tiles are their own images
        mem_slides.append(Slide(f'j{i}', dec, per, y_true=int(y[i])))
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=5)
    from_files = evaluate(eng, slides_from_tfrecords(paths, {f'j{i}': int(y[i]) for i in range(n_slides)}), outcome='cohort',
                          mc_n=5, seed=7, batch=16)
    in_memory = evaluate(eng, mem_slides, outcome='cohort', mc_n=5, seed=7, batch=16)
    for col in ('cohort-y_pred1', 'cohort-uncertainty1'):
        assert np.array_equal(from_files.tile_df[col].to_numpy(), in_memory.tile_df[col].to_numpy()), col
    assert np.array_equal(from_files.slide_pred, in_memory.slide_pred)
    eng.close()


def test_host_tiles_through_the_pinned_ring_equal_resident_tiles(monkeypatch):
    """The chunk-source contract of `evaluate` (chunk_shape / read / rows / close) on the simplest source there is -- decoded tiles
    in pageable host memory, bench.py's PCIe-inclusive leg -- with chunks smaller than a slide, so that slides span ring slots
    and batches span chunks: the tile table and the slide table equal those of the same tiles handed over whole."""
    import biscuit_amd.inference as inf
    from bench import _HostTiles
    from biscuit_amd import feed
    from biscuit_amd.engine import Engine
    monkeypatch.setattr(feed, 'CHUNK_TILES', 7)
    calls, read = [], _HostTiles.read

    def counted(self, *a):
        calls.append(id(self))
        return read(self, *a)
    monkeypatch.setattr(_HostTiles, 'read', counted)
    n_slides, per = 3, 19
    tiles, sidx, y = make_slides(n_slides, per, seed=9)
    whole = [inf.Slide(f'h{i}', tiles[sidx == i], per, y_true=int(y[i])) for i in range(n_slides)]
    ring = [inf.Slide(f'h{i}', tiles[sidx == i], per, y_true=int(y[i]), source=_HostTiles(np.ascontiguousarray(tiles[sidx == i])))
            for i in range(n_slides)]
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=16, max_mc=5)
    a = inf.evaluate(eng, whole, outcome='cohort', mc_n=5, seed=7, batch=16)
    b = inf.evaluate(eng, ring, outcome='cohort', mc_n=5, seed=7, batch=16)
    # the run really was cut up: the first chunks of a run are the ramp's and hold a slide each, the last slide's 19 tiles meet CHUNK_TILES
    assert calls.count(id(ring[-1].source)) > 1
    for col in ('cohort-y_pred1', 'cohort-uncertainty1'):
        assert np.array_equal(a.tile_df[col].to_numpy(), b.tile_df[col].to_numpy()), col
    assert np.array_equal(a.slide_pred, b.slide_pred) and np.array_equal(a.slide_count, b.slide_count)
    eng.close()


# ------------------------------------------------------------------------------------------------ stress weights
@pytest.fixture(scope='module')
def hard():
    from biscuit_amd.engine import Engine
    from oracle.xception_ref import XceptionOracle
    w = synthetic_weights(1, hard=True)
    e = {'w': w, 'f32': Engine(w, dtype='f32', max_batch=64, max_mc=30), 'bf16': Engine(w, dtype='bf16', max_batch=64, max_mc=30),
         'f16': Engine(w, dtype='f16', max_batch=64, max_mc=30), 'oracle': XceptionOracle(w)}
    yield e
    e['f32'].close(); e['bf16'].close(); e['f16'].close()


def test_hard_weights_fp32_kernels_against_both_oracles(hard):
    from oracle import xception_nn as NN
    tiles = make_tiles(4, seed=19)
    rm, rs = hard['oracle'].mc_predict(tiles, 10, 1234, mode='head')
    nm, ns = NN.mc_predict(NN.XceptionNN(hard['w']), tiles, 10, 1234)
    m, s = hard['f32'].mc_infer(dev(tiles), 10, 1234)
    m, s = m.cpu().numpy(), s.cpu().numpy()
    print('hard weights, fp32 kernels: vs oracle 1 %.2e / %.2e, vs oracle 2 %.2e / %.2e; pred %s std %s' % (
        np.abs(m - rm).max(), np.abs(s - rs).max(), np.abs(m - nm).max(), np.abs(s - ns).max(), m[:, 1], s[:, 1]))
    assert np.abs(m - rm).max() < 2e-5 and np.abs(s - rs).max() < 2e-5
    assert np.abs(m - nm).max() < 2e-5 and np.abs(s - ns).max() < 2e-5
    assert np.abs(m[:, 1] - 0.5).max() > 0.05           # O(1) logits: predictions leave the 0.35-0.65 band of the default set


def test_hard_weights_every_layer_fp32(hard):
    from oracle.xception_ref import standardize
    from test_gpu_parity import TAPS
    t2 = make_tiles(2, seed=19)
    taps = {}
    hard['oracle'].backbone(standardize(t2), taps)
    eng = hard['f32']
    staged = eng.stage(dev(t2))
    for name, shp in TAPS:
        got = eng.debug_activation(name, staged, shp).cpu().numpy()
        ref = taps[name].permute(0, 2, 3, 1).numpy()
        assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), name


def _hard_deltas(hard, dtype):
    """16-bit kernels against the exact fp32 kernels (= both oracles to 2e-5) on the stress set: 4 slides x 16 tiles,
    MC = 30.  Returns tile max|d mean|, tile max|d std|, slide max|d pred|, slide max|d unc|."""
    tiles, sidx, _ = make_slides(4, 16, seed=7)
    d = dev(tiles)
    m32, s32 = hard['f32'].mc_infer(d, 30, 1234)
    m16, s16 = hard[dtype].mc_infer(d, 30, 1234)
    sl = dev(sidx).long()

    def smean(x):
        return torch.zeros(4, device='cuda', dtype=torch.float64).index_add_(0, sl, x.double()) / 16
    return (float((m32 - m16).abs().max()), float((s32 - s16).abs().max()),
            float((smean(m32[:, 1]) - smean(m16[:, 1])).abs().max()), float((smean(s32[:, 1]) - smean(s16[:, 1])).abs().max()))


def test_hard_weights_throughput_mode_holds_tolerance(hard):
    """THE parity claim of the headline mode.  BASELINE.json north_star: tile- and slide-level mean and sigma within
    1e-3 of the reference.  f16 storage + f16 MFMAs (fp32 accumulation, fp32 folded BN, fp32 head) on weights with O(1)
    logits and BatchNorm statistics far from the identity: measured 2.5e-4 / 1.0e-4 at tile level, 1.0e-4 / 1.1e-5 at
    slide level -- a quarter of the budget."""
    dm, ds, dsp, dsu = _hard_deltas(hard, 'f16')
    print(f'hard weights, f16 vs fp32 kernels: tile max|dmean|={dm:.3e} max|dstd|={ds:.3e}; slide pred {dsp:.3e} unc {dsu:.3e}')
    assert dm < NORTH_STAR_TOL and ds < NORTH_STAR_TOL and dsp < NORTH_STAR_TOL and dsu < NORTH_STAR_TOL


@pytest.mark.parametrize('weight_seed', [4, 7])
def test_hard_weights_other_draws_hold_the_tolerance(weight_seed):
    """The same claim on other draws of the stress weights: of eight seeds (tools/parity_seeds.py, profiles/r03_parity_seeds.log:
    f16 tile max|d mean| 2.2e-4 .. 4.6e-4, slide 4e-5 .. 2.1e-4; bf16 1.5e-3 .. 3.9e-3) these two are the worst for f16."""
    from biscuit_amd.engine import Engine
    w = synthetic_weights(weight_seed, hard=True)
    tiles, sidx, _ = make_slides(4, 16, seed=100 + weight_seed)
    d, sl = dev(tiles), dev(sidx).long()
    e32, e16 = Engine(w, dtype='f32', max_batch=64, max_mc=30), Engine(w, dtype='f16', max_batch=64, max_mc=30)
    (m32, s32), (m16, s16) = e32.mc_infer(d, 30, 1234), e16.mc_infer(d, 30, 1234)

    def smean(x):
        return torch.zeros(4, device='cuda', dtype=torch.float64).index_add_(0, sl, x.double()) / 16
    deltas = (float((m32 - m16).abs().max()), float((s32 - s16).abs().max()),
              float((smean(m32[:, 1]) - smean(m16[:, 1])).abs().max()), float((smean(s32[:, 1]) - smean(s16[:, 1])).abs().max()))
    print(f'hard weights seed {weight_seed}, f16 vs fp32 kernels: tile {deltas[0]:.3e} / {deltas[1]:.3e}; slide {deltas[2]:.3e} / {deltas[3]:.3e}')
    assert max(deltas) < NORTH_STAR_TOL
    e32.close(); e16.close()


def test_hard_weights_bf16_kernels_reported(hard):
    """The same figure for the bf16 mode, which BASELINE config 2 names: with O(1) logits it does NOT stay inside 1e-3
    (measured 2.7e-3 on the tile mean, 9e-4 on the tile std, 1.4e-3 on the slide mean of 16 tiles): the error is the
    2^-9 relative rounding of every activation, depthwise result and weight, not a kernel defect -- which is why the
    headline mode is f16 (test above).  The bounds below only guard against a regression of that figure."""
    dm, ds, dsp, dsu = _hard_deltas(hard, 'bf16')
    print(f'hard weights, bf16 vs fp32 kernels: tile max|dmean|={dm:.3e} max|dstd|={ds:.3e}; slide pred {dsp:.3e} unc {dsu:.3e}')
    assert dm < BF16_HARD_TILE_BOUND and ds < BF16_HARD_TILE_BOUND and dsp < 3e-3 and dsu < 1e-3


def test_f16_range_by_construction_with_activation_exponents():
    """IEEE half ends at 65504 and the f16 kernels clamp there silently.  `equivalent_rescaled(w, 3e4)` is the stress classifier
    with every stored tensor 30 000 times larger -- the same function in real arithmetic, raw activations up to ~1e6 --: without
    activation exponents the f16 path saturates and its predictions are wrong; with the exponents `Engine.calibrate` measures on
    eight tiles (fp32 kernels, powers of two folded into the BatchNorm constants, weights.py) it holds the north-star tolerance
    of 1e-3 against the fp32 CPU oracle at tile and slide level.  Default weights calibrate to all-zero exponents and the blob
    they always had; forced exponents on them change no result beyond the last place (a power of two only moves exponents)."""
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import equivalent_rescaled, pack_blob, tensor_plan
    from oracle.xception_ref import XceptionOracle
    base = synthetic_weights(3, hard=True)
    big = equivalent_rescaled(base, 3.0e4)
    tiles, sidx, _ = make_slides(2, 8, seed=41)
    d, sl = dev(tiles), dev(sidx).long()
    mc_n, seed = 30, 1234
    rm, rs = XceptionOracle(base).mc_predict(tiles, mc_n, seed)                 # the function both weight sets compute
    bm, bs = XceptionOracle(big).mc_predict(tiles[:4], mc_n, seed)
    assert np.abs(bm - rm[:4]).max() < 2e-5 and np.abs(bs - rs[:4]).max() < 2e-5     # (the rescaling is an equivalence)

    def deltas(m, s):
        m, s = m.cpu().numpy(), s.cpu().numpy()
        sm = lambda x: np.array([x[sidx == k].mean() for k in range(2)])
        return (np.abs(m - rm).max(), np.abs(s - rs).max(), np.abs(sm(m[:, 1]) - sm(rm[:, 1])).max(),
                np.abs(sm(s[:, 1]) - sm(rs[:, 1])).max())
    # 1. as it is: clipped
    e0 = Engine(big, dtype='f16', max_batch=16, max_mc=mc_n)
    hr0 = e0.f16_headroom(d)
    bad = deltas(*e0.mc_infer(d, mc_n, seed))
    assert any(hr0['saturated'].values()) and max(bad) > 1e-2, (hr0['saturated'], bad)
    e0.close()
    # 2. exponents from a calibration batch
    act_exp, peaks = Engine.calibrate(big, tiles[:8])
    assert max(peaks.values()) > 3e5 and max(act_exp.values()) >= 5, (max(peaks.values()), act_exp)
    e1 = Engine(big, dtype='f16', max_batch=16, max_mc=mc_n, act_exp=act_exp)
    hr1 = e1.f16_headroom(d)
    good = deltas(*e1.mc_infer(d, mc_n, seed))
    print(f'weights x 3e4 (peak activation {max(peaks.values()):.3g}): f16 without exponents tile {bad[0]:.2e}; with {act_exp}: '
          f'tile {good[0]:.2e} / {good[1]:.2e}, slide {good[2]:.2e} / {good[3]:.2e}, headroom {hr1["headroom"]:.1f}x')
    assert not any(hr1['saturated'].values()) and hr1['headroom'] >= 8
    assert max(good) < NORTH_STAR_TOL, good
    # taps come back at true scale: the stored tensor times 2^k
    k = act_exp['block4_out']
    a = e1.debug_activation_u8('block8_out', d[:2].contiguous(), (19, 19, 728))
    b = e1.debug_activation_u8('block8_out', d[:2].contiguous(), (19, 19, 728), true_scale=False)
    assert k > 0 and torch.equal(a, b * float(2 ** k)) and float(b.abs().max()) <= 4096 * 4
    e1.close()
    # 3. weights that fit as they are: no exponents, the same blob.  Forced exponents on them: a power of two moves exponents only,
    # so every NORMAL value keeps its mantissa; what differs is the handful of values in IEEE half's subnormal range (|x| < 6.1e-5:
    # 42 of 2.8 M in block1_conv2), which the scaled-up run stores with more bits -- tools/dbg_exp.py shows the first differences
    # there, then the one-ulp rounding flips they seed downstream.  The two runs agree like any two roundings of the network do:
    # well inside the f16 mode's distance from fp32 (2-3e-4), nowhere near the tolerance.
    act0, _ = Engine.calibrate(base, tiles[:8])
    assert not any(act0.values()) and pack_blob(base, 'f16', act0) == pack_blob(base, 'f16')
    e2 = Engine(base, dtype='f16', max_batch=16, max_mc=mc_n)
    e3 = Engine(base, dtype='f16', max_batch=16, max_mc=mc_n, act_exp={t: -2 for _, _, t in tensor_plan()})
    (m2, s2), (m3, s3) = e2.mc_infer(d, mc_n, seed), e3.mc_infer(d, mc_n, seed)
    assert float((m2 - m3).abs().max()) < 3e-4 and float((s2 - s3).abs().max()) < 3e-4
    assert max(deltas(m3, s3)) < NORTH_STAR_TOL
    a2 = e2.debug_activation_u8('block1_conv2', d[:2].contiguous(), (147, 147, 64))
    a3 = e3.debug_activation_u8('block1_conv2', d[:2].contiguous(), (147, 147, 64))
    differ = a2 != a3
    assert int(differ.sum()) < 1000 and (not bool(differ.any()) or float(a2.abs()[differ].max()) < 6.2e-5)   # subnormals only
    e2.close(); e3.close()


NORTH_STAR_TOL = 1e-3
BF16_HARD_TILE_BOUND = 5e-3
