"""The per-slide MC-dropout inference loop -- what ``Project.evaluate(model, outcome,
filters, save_predictions=True)`` (``biscuit/experiment.py:917-922``) and the validation
step of ``Project.train(..., save_predictions=True)`` (``experiment.py:1042-1051``) do for
BISCUIT: stream every slide's 299x299 tiles, run the classifier with dropout active for
``uq_n`` passes, keep per-tile mean/std, and reduce to slide-level prediction/uncertainty.

Slides are sharded over ranks (one process per GPU); tiles stream in batches of
``batch`` that may span slide boundaries (a per-tile slide index drives the device-side
segmented reduce); each tile's Philox counter is its GLOBAL index in dataset order, so
results do not depend on batch size, sharding or rank count.
"""
import contextlib
import os
import queue
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import distributed as D
from .feed import CHUNK_TILES, PngRows, Slide, TFRecordSource, _DeviceDecode, _Feeder, pick_unfilter_mode, slides_from_tfrecords  # noqa: F401
from .predictions import (EVAL_NAME, TableWriter, assemble_shards, remove_stale_shards, save_tile_predictions, shard_name,
                          tile_frame, write_shard_index)


@dataclass
class EvalResult:
    tile_df: Optional[pd.DataFrame]          # this rank's tile rows (Slideflow headers)
    slide_names: List[str]
    slide_pred: np.ndarray                   # float64 [S], all slides (after the gather)
    slide_unc: np.ndarray
    slide_count: np.ndarray
    slide_y_true: np.ndarray
    local_slides: List[int] = field(default_factory=list)
    table_path: Optional[str] = None         # the tile table on disk: THE table (world 1; rank 0 after the splice) or this rank's shard
    table_rows: int = 0                      # rows this rank wrote
    f16_headroom: float = float('inf')       # minimum over the run's range checks of 65504 / max |stored activation| (f16 engines)
    f16_checks: int = 0
    stain_passthrough: int = 0               # tiles of this rank the normaliser did not normalise (degenerate: a status other than 0; stain.STATUS_METHODS)
    f16_screen_checks: int = 0               # range screen (evaluate(range_screen=True)): tap runs on the screened candidates
    f16_screen_headroom: float = float('inf')    # ... the minimum of 65504 / max |stored activation| over them
    f16_screened: int = 0                    # ... tiles of this rank that went through the key (0: the screen did not run)
    f16_screen_max_key: float = 0.0          # ... the largest key among the candidates looked at

    def slide_frame(self, pred_thresh=0.5, level='slide'):
        """Group table in ``process_group_predictions`` form from the device-reduced means."""
        from .threshold import group_frame
        keep = self.slide_count > 0
        names = [n for n, k in zip(self.slide_names, keep) if k]
        return group_frame(names, self.slide_pred[keep], self.slide_y_true[keep].astype(np.uint8),
                           self.slide_unc[keep], pred_thresh, level)


def _take_front(parts, k, size=len, cut=lambda t, a, b: t[a:b]):
    """(the pieces that make up the first k rows of the arrays in ``parts``, what is left of the list): whole arrays and views, no copy."""
    out, i = [], 0
    while k > 0:
        t = parts[i]
        if size(t) <= k:
            out.append(t); k -= size(t); i += 1
        else:
            out.append(cut(t, 0, k)); parts = parts[:i] + [cut(t, k, size(t))] + parts[i + 1:]; k = 0
    return out, parts[i:]


class _Pending:
    """The tiles that wait for a batch, in dataset order: the device tensors they lie in and, per run of tiles of one slide, every
    tile's local slide index (int32, device) and global index (int64, host) and the table's segment (si, name, y_true, loc, count)."""

    def __init__(self):
        self.tiles, self.sidx, self.gidx, self.segs = [], [], [], []
        self.n = 0

    def push(self, tiles, sidx, gidx, segs):                # one tensor; per slide in it one entry of each list (``segs``: empty without a table)
        self.tiles.append(tiles)
        self.sidx += sidx
        self.gidx += gidx
        self.segs += segs
        self.n += tiles.shape[0]

    def take(self, k):
        """The first ``k`` tiles: (tiles, slide indices, global indices, table segments)."""
        # the first `k` rows of what is pending: a VIEW when they lie in one tensor, one batch-sized copy when the batch spans
        # two (round 4 concatenated everything pending -- a 1 000-tile slide behind a 200-tile remainder: 330 MB copied to cut 256
        # tiles off the front, 0.11 ms per batch in config 3's trace)
        cur, self.tiles = _take_front(self.tiles, k)
        cs, self.sidx = _take_front(self.sidx, k)
        cg, self.gidx = _take_front(self.gidx, k)
        segs = []
        if self.segs:
            segs, self.segs = _take_front(self.segs, k, size=lambda seg: seg[4],
                                          cut=lambda seg, a, b: (*seg[:3], None if seg[3] is None else seg[3][a:b], b - a))
        self.n -= k
        return (cur[0] if len(cur) == 1 else torch.cat(cur), cs[0] if len(cs) == 1 else torch.cat(cs),
                cg[0] if len(cg) == 1 else np.concatenate(cg), segs)


def _to_device(t, device):
    if torch.is_tensor(t):
        return t.to(device=device, dtype=torch.uint8, non_blocking=True).contiguous()
    return torch.from_numpy(np.ascontiguousarray(t)).to(device, non_blocking=True)


def _device_tiles(chunk, eng, dev, decoder):
    """One of the feeder's chunks -> its tiles on the device (uint8 NHWC), ordered before the current stream's work that follows."""
    if chunk.fmt is not None:                            # compressed: decoded on the decode CUs
        return decoder.decode(chunk)
    if chunk.event is None:                              # as the slide's loader left them
        tiles = _to_device(chunk.data, dev)
    else:                                                # made on the copy stream: order it before this stream's work
        torch.cuda.current_stream(dev).wait_event(chunk.event)
        chunk.data.record_stream(torch.cuda.current_stream(dev))
        tiles = chunk.data.contiguous()
    return eng.png_unfilter(tiles) if chunk.rows else tiles      # (filtered PNG scanlines: the filters are reversed on the device)


class _TableStream:
    """The tile table written WHILE the GPU works (round 6; Slideflow -- and rounds 1-5 here -- wrote it with one
    ``DataFrame.to_csv`` after the last batch: 1.75 s per 200 000 rows, serial, behind 6 s of GPU time).  ``submit`` takes a
    batch's results as they were enqueued -- one device tensor [2, n, 2] (mean | std), the event behind the batch's last kernel,
    and the runs of tiles per slide it holds --; a host thread waits for the event on a side stream, copies the 4 KB to pinned
    memory there and appends the rows through ``TableWriter`` (libbiscuit_io; the GIL is released while it formats and writes).
    Batches are written in submission order, so the rows are in dataset order however many batches are in flight.  For a shard
    of a multi-rank run it also notes every slide's byte range (``write_shard_index``)."""

    def __init__(self, path, outcome, with_loc, dev, max_batch, shard=None):
        self.writer = TableWriter(path, outcome, with_loc)
        self.path, self.outcome, self.with_loc, self.shard = path, outcome, with_loc, shard
        self.dev = torch.device(dev)
        self.cuda = self.dev.type == 'cuda'
        self.side = torch.cuda.Stream(device=self.dev) if self.cuda else None
        self.host = torch.empty((2 * max_batch * 2,), dtype=torch.float32, pin_memory=self.cuda)
        self.q = queue.Queue(maxsize=64)
        self.error = None
        self.index = []                      # [global slide index, name, rows, offset, length]
        self.rows = 0
        self.th = threading.Thread(target=self._work, name='bq-table-writer', daemon=True)
        self.th.start()

    def _work(self):
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                if self.error is not None:
                    continue                 # (drain: the producer must never block on a dead writer)
                out2, ev, segs = item
                n = out2.shape[1]
                if self.cuda:
                    host = self.host[:4 * n].view(2, n, 2)
                    with torch.cuda.stream(self.side):
                        if ev is not None:
                            self.side.wait_event(ev)
                        host.copy_(out2, non_blocking=True)
                    self.side.synchronize()
                    arr = host.numpy()
                else:
                    arr = out2.numpy()
                at = 0
                for si, name, y_true, loc, count in segs:
                    t0 = self.writer.tell()
                    self.writer.rows(name, y_true, arr[0, at:at + count], arr[1, at:at + count], loc)
                    t1 = self.writer.tell()
                    if self.index and self.index[-1][0] == si:
                        self.index[-1][2] += count
                        self.index[-1][4] += t1 - t0
                    else:
                        self.index.append([si, name, count, t0, t1 - t0])
                    at += count
                    self.rows += count
                del out2, item
        except BaseException as e:           # noqa: BLE001 -- re-raised by the producer
            self.error = e
            while self.q.get() is not None:  # keep draining until the producer says stop
                pass

    def submit(self, out2, ev, segs):
        if self.error is not None:
            self.finish()
        if self.cuda:
            out2.record_stream(self.side)
        self.q.put((out2, ev, segs))

    def abort(self):
        """The run failed elsewhere: stop the thread and close the file (what is on disk stays, without an index)."""
        if self.th is not None:
            self.q.put(None)
            self.th.join()
            self.th = None
        self.error = None
        try:
            self.writer.close()
        except IOError:
            pass

    def finish(self):
        """Everything submitted is on disk and the file is closed when this returns; raises what the writer thread met."""
        if self.th is not None:
            self.q.put(None)
            self.th.join()
            self.th = None
        err, self.error = self.error, None
        if err is not None:
            try:
                self.writer.close()
            finally:
                raise err
        rows, _ = self.writer.close()
        if self.shard is not None:
            write_shard_index(self.path, self.shard[0], self.shard[1], self.outcome, self.with_loc, self.index)
        return rows


def _f16_verdict(a, headroom_min):
    """One [8, 2] result of ``Engine.f16_headroom_async`` (per tap: peak |activation| as stored, values at the clamp) ->
    (headroom = 65504 / peak, None or what is wrong: a value at the clamp, or less than ``headroom_min`` x of range left)."""
    worst = int(np.argmax(a[:, 0]))
    hr = 65504.0 / max(float(a[worst, 0]), 1e-30)
    if not (a[:, 1].sum() > 0 or hr < float(headroom_min)):
        return hr, None
    from .engine import Engine
    sat = {Engine.HEADROOM_TAPS[i][0]: int(a[i, 1]) for i in range(a.shape[0]) if a[i, 1] > 0}
    return hr, (f'{sat} values clamped at +-65504' if sat else f'only {hr:.2f}x of range left at {Engine.HEADROOM_TAPS[worst][0]} '
                f'(peak {float(a[worst, 0]):.4g}; headroom_min {headroom_min})')


class _RangeWatch:
    """``evaluate``'s sampling monitor (the first tiles of a batch) and range screen (the riskiest tiles of an engine's interval): the
    eight f16 range taps run behind the batches and are looked at later, with no host synchronisation in between.  Taps in flight, per
    engine: (batch number, first global tile index or None, pinned [8, 2] result [+ the candidates' keys, global indices], event)."""

    def __init__(self, n_engines, headroom_min, dev, slides, offsets):
        self.pending = [[] for _ in range(n_engines)]
        self.headroom_min, self.dev, self.slides, self.offsets = headroom_min, dev, slides, offsets
        self.min, self.checks, self.max_key = float('inf'), 0, 0.0

    def tap(self, k, eng, tiles, batch_no, g0=None, candidates=()):
        """Enqueue the taps on ``tiles`` and the copies out on the current stream (engine ``k``'s); reported on failure: ``g0`` / ``candidates``."""
        parts = (eng.f16_headroom_async(tiles), *candidates)
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in parts]
        for h, t in zip(host, parts):
            h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.pending[k].append((batch_no, g0, host, ev))

    def look(self, ks=None):
        """Wait for the taps in flight (of engines ``ks``; default: all) and judge them: ``F16RangeError`` at the first that fails.  (Engine
        by engine, not in batch order: every tap is preceded by a look, so an engine has one in flight at most and the order cannot matter.)"""
        for k in range(len(self.pending)) if ks is None else ks:
            while self.pending[k]:
                nb, g0, host, ev = self.pending[k].pop(0)
                ev.synchronize()
                self.checks += 1
                if len(host) > 1:
                    self.max_key = max(self.max_key, float(host[1].numpy().max()))
                hr, wrong = _f16_verdict(host[0].numpy(), self.headroom_min)
                self.min = min(self.min, hr)
                if wrong is not None:
                    raise self._error(k, nb, g0, host[1:], wrong)

    def _tile_name(self, g):
        for si in range(len(self.slides) - 1, -1, -1):
            if self.slides[si].n_tiles and self.offsets[si] <= g:
                return f'{self.slides[si].name} tile {g - self.offsets[si]}'
        return '?'

    def _error(self, k, nb, g0, candidates, wrong):
        from .engine import F16RangeError
        if not candidates:
            where = f'in batch {nb} (global tile {g0} on): '
            then = '; the results from there on would be plausible and wrong.'
        else:
            keys, gidx = (h.numpy() for h in candidates)
            order = sorted(range(len(keys)), key=lambda i: (-keys[i], gidx[i]))
            cands = '; '.join(f'{self._tile_name(int(gidx[i]))} (global tile {int(gidx[i])}, key {float(keys[i]):.4g})' for i in order)
            where = f'on the riskiest tiles of stream {k}\'s interval ending at batch {nb}: '
            then = (f'; candidates looked at, largest standardised input first: {cands}.  The results of these tiles would be '
                    'plausible and wrong.')
        return F16RangeError(f'f16 storage at its range limit {where}{wrong}{then}  Re-run with Engine.calibrate() on tiles like '
                             'these, or with dtype bf16 / f32')


class _Batches:
    """``evaluate``'s batches, round-robin over the engines (a pool's: each on its own stream): accumulators, range watches, table hand-over."""

    def __init__(self, pool, engines, table, dev, n_local, slides, offsets, stain, *, batch, mc_n, seed, mc_mode, tile_uq, normalizer, norm_fit,
                 keep_tiles, headroom_every, headroom_min, range_screen):
        self.pool, self.engines, self.table, self.dev, self.n_local, self.stain = pool, engines, table, dev, n_local, stain
        self.streams = getattr(pool, 'streams', None) if pool else None
        self.mc_n, self.seed, self.mc_mode, self.tile_uq = mc_n, seed, mc_mode, tile_uq
        self.normalizer, self.norm_fit, self.keep_tiles = normalizer, norm_fit, keep_tiles
        self.n = 0                                       # batches enqueued
        self.acc = [None] * len(engines)
        self.passthrough = [None] * len(engines)         # per stream: int64 device count of the tiles whose stain status is not 0
        self.rows = []                                   # keep_tiles: the batches' (mean | std), on the device; copied to the host at the end
        f16 = all(getattr(e, 'dtype', None) == 'f16' and hasattr(e, 'f16_headroom_async') for e in engines)
        self.every = int(headroom_every or 0) if f16 else 0      # batches between range checks (0: neither monitor nor mid-run screen taps)
        self.monitor = _RangeWatch(len(engines), headroom_min, dev, slides, offsets)
        self.screen = _RangeWatch(len(engines), headroom_min, dev, slides, offsets)
        self.screens = []
        if range_screen and f16:
            from .engine import RangeScreen
            self.screens = [RangeScreen(e, k=min(8, e.max_batch), max_batch=batch) for e in engines]
        self.sc_count = [0] * len(engines)

    def _screen_tap(self, k, eng, batch_no):
        scr = self.screens[k]
        if scr.filled:
            self.screen.tap(k, eng, scr.tiles, batch_no, candidates=scr.candidates())
            scr.reset()

    def _work(self, eng, k, cur, cs, g0, gdev, mean, std):
        if self.norm_fit is not None:
            if self.normalizer in self.stain.STATUS_METHODS:
                st = torch.empty(cur.shape[0], dtype=torch.int32, device=self.dev)
                cur = self.stain.normalise(eng, cur, self.normalizer, self.norm_fit, status=st)
                cnt = st.ne(0).sum()
                self.passthrough[k] = cnt if self.passthrough[k] is None else self.passthrough[k].add_(cnt)
            else:
                cur = self.stain.normalise(eng, cur, self.normalizer, self.norm_fit)
        if self.screens:                                 # the tiles exactly as the network sees them
            self.screens[k].update(cur, tile_idx0=g0 if gdev is None else 0, tile_idx=gdev)
        if gdev is None:
            eng.mc_infer(cur, self.mc_n, self.seed, tile_idx0=g0, mc_mode=self.mc_mode, out=(mean, std))
        else:
            eng.mc_infer(cur, self.mc_n, self.seed, tile_idx0=0, mc_mode=self.mc_mode, out=(mean, std), tile_idx=gdev)
        self.acc[k] = eng.slide_reduce(mean, std, cs, max(self.n_local, 1), tile_uq=self.tile_uq, acc=self.acc[k])
        if self.every and self.n % self.every == 0:
            self.monitor.tap(k, eng, cur, self.n, g0=g0)
        if self.screens:
            self.sc_count[k] += 1
            if self.every and self.sc_count[k] % self.every == 0:
                self._screen_tap(k, eng, self.n)

    def run(self, cur, cs, cg, segs):
        """Enqueue one batch: the tiles, every tile's local slide index and global index (host), the table segments of its slides."""
        n, k = cur.shape[0], self.n % len(self.engines)
        cur, cs = cur.contiguous(), cs.contiguous()
        out2 = torch.empty((2, n, 2), dtype=torch.float32, device=self.dev)       # mean | std: ONE device-to-host copy per batch
        # a batch that spans slides holds tiles whose global indices are not one consecutive run: the backbone does not care,
        # the head's Philox counter does -- it takes the indices as an array then (bq_set_tile_index_array): ONE launch sequence
        # per batch whatever its composition (round 4: one head call per run, 4 x the head time with 64-tile slides), and a
        # tile's result does not depend on batch size, sharding or rank count
        gdev = None
        if (np.diff(cg) != 1).any():
            gdev = torch.from_numpy(np.ascontiguousarray(cg)).to(self.dev, non_blocking=True)
        if self.every and self.n % self.every == 0:
            self.monitor.look()                      # the previous check: one interval old, long finished -- a run fails one interval late at most
        if self.screens and self.every and (self.sc_count[k] + 1) % self.every == 0:
            self.screen.look([k])                    # this engine's previous screen tap, one of its intervals old
        if self.pool:
            # these tensors were allocated on the caller's stream and are read on the pool's: tell the
            # caching allocator, or the next batch's temporaries may reuse their memory while this
            # batch's kernels are still in flight
            if self.streams and cur.is_cuda:
                for t in (cur, cs, out2) + ((gdev,) if gdev is not None else ()):
                    t.record_stream(self.streams[k])
            self.pool.run(self.n, lambda eng: self._work(eng, k, cur, cs, int(cg[0]), gdev, out2[0], out2[1]), wait_for_current=True)
        else:
            self._work(self.engines[0], k, cur, cs, int(cg[0]), gdev, out2[0], out2[1])
        if self.table is not None:
            ev = None
            if out2.is_cuda:
                ev = torch.cuda.Event()
                ev.record(self.streams[k] if self.streams else torch.cuda.current_stream(self.dev))
            self.table.submit(out2, ev, segs)
        self.n += 1
        if self.keep_tiles:
            self.rows.append(out2)

    def final_looks(self):
        if self.every:
            self.monitor.look()
        if self.screens:
            # the last, partial interval of every engine: tapped here, on the engine's stream, and looked at at once
            for k, eng in enumerate(self.engines):
                if self.pool:
                    self.pool.run(k, lambda e, k=k: self._screen_tap(k, e, self.n - 1))
                else:
                    self._screen_tap(k, eng, self.n - 1)
            self.screen.look()


def evaluate(engine, slides: Sequence[Slide], outcome='cohort', mc_n=None, seed=None, batch=256,
             mc_mode='head', tile_uq=None, save_dir=None, keep_tiles=True, rank=0, world=1, norm_fit=None,
             table_name=EVAL_NAME, table_writer='native', headroom_every=200, headroom_min=2.0, normalizer='reinhard_fast',
             range_screen=False):
    """Run MC-dropout inference over ``slides`` and return tile- and slide-level results.

    Every rank passes the SAME slide list; rank r processes ``partition_slides(...)[r]``.
    The slide-level arrays are all-gathered (one collective).

    ``save_dir``: the tile table -- the product ``biscuit.threshold`` reads (experiment.py:688-699) -- is written there as
    ``table_name`` WHILE the GPU works (``_TableStream``; ``keep_tiles`` is not needed for it).  With ``world`` > 1 every rank
    streams its shard ``tile_predictions_eval.rankR.csv`` (+ a byte index of its slides) and closes it BEFORE the all-gather, so
    the gather doubles as "all shards complete"; rank 0 then splices them into the ONE table in dataset order -- byte for byte
    the file a single-rank run writes.  ``table_writer='pandas'`` (or a ``.parquet.gzip`` name) writes with pandas after the run
    instead: the checker of the native writer, and the parquet form.

    ``headroom_every`` (f16 engines only; 0 / None: off): every that many batches -- and on the first -- the eight range taps of
    ``Engine.f16_headroom`` run on up to eight tiles of the batch, behind it on its stream, with no host synchronisation: the
    maxima are copied out asynchronously and looked at when the next check is due (and at the end).  A value at the clamp, or
    less than ``headroom_min`` x of range left, raises ``F16RangeError``: the calibration batch at the start of a run says
    nothing about the 10^5 tiles behind it, and f16's clamp is silent.  ``EvalResult.f16_headroom`` = the minimum seen.

    ``range_screen`` (f16 engines only): every tile of the run -- as the network sees it, after the stain
    normaliser -- is ranked on the device by ``Engine.range_key`` (how far its standardised input reaches), each engine keeps the
    eight riskiest of its interval in a ``RangeScreen``, and the same eight range taps run on THOSE tiles every ``headroom_every``
    batches of that engine (0 / None: once, at the end) and on what is left at the end; the results are looked at one interval
    late, like the sampling monitor's, and raise ``F16RangeError`` the same way, naming the candidates' slides, global tile indices
    and keys.  No host synchronisation per batch, no result changes.  ``EvalResult.f16_screen_*`` / ``f16_screened`` report it.
    With another dtype, or False, nothing is launched or allocated.

    ``norm_fit`` (``{'target_means': [3], 'target_stds': [3]}``, the block of that name in the model's
    params.json) switches on the `reinhard_fast` stain normaliser of hp.py:19 in front of the staging
    kernel, where results.py:251-252 applies it.  ``normalizer='macenko'`` takes a Macenko fit instead
    (``{'stain_matrix_target': 3x2, 'target_concentrations': 2}``); the tiles it passes through unchanged (degenerate: no
    tissue, one colour) are counted on the device and read once at the end: ``EvalResult.stain_passthrough`` (this rank's).
    ``normalizer='reinhard'``, ``'reinhard_mask'`` and ``'reinhard_fast_mask'`` take ``reinhard_fast``'s fit; the tiles they report
    as too dark or without tissue (``stain.REINHARD_*``) are counted in the same place."""
    from . import stain
    stain.check(normalizer, norm_fit)
    mc_n = int(mc_n or engine.hp.uq_n)
    seed = int(engine.hp.seed if seed is None else seed)
    counts = [s.n_tiles for s in slides]
    parts = D.partition_slides(counts, world)
    mine = parts[rank]
    offsets = D.global_tile_offsets(counts)
    dev = engine.device
    cuda = torch.device(dev).type == 'cuda'
    n_local = len(mine)
    # an EnginePool alternates batches over independent contexts / HIP streams
    pool = engine if hasattr(engine, 'engines') else None
    engines = pool.engines[:len(pool)] if pool else [engine]      # len(pool) = batches in flight
    rows_slide, rows_true, rows_loc = [], [], []
    with_loc = any(s.n_tiles for s in slides) and all(s.loc is not None for s in slides if s.n_tiles)    # (every rank decides the same: one header)
    native = save_dir is not None and table_writer == 'native' and table_name.endswith('.csv')
    if table_writer not in ('native', 'pandas'):
        raise ValueError(f"table_writer must be 'native' or 'pandas', not {table_writer!r}")
    if save_dir is not None and not native and not keep_tiles:
        raise ValueError('the pandas writer needs keep_tiles=True (it writes the frame after the run)')
    if save_dir is not None and rank == 0 and os.path.isdir(save_dir):
        remove_stale_shards(save_dir, world if world > 1 else 0, table_name)      # (a one-rank run leaves THE table only)
    table = None
    if native:
        tpath = os.path.join(save_dir, table_name if world == 1 else shard_name(table_name, rank))
        table = _TableStream(tpath, outcome, with_loc, dev, batch, shard=None if world == 1 else (rank, world))
    # from here to table.finish() a failure, wherever it surfaces, stops the writer thread and closes the file before it goes on up
    try:
        run = _Batches(pool, engines, table, dev, n_local, slides, offsets, stain, batch=batch, mc_n=mc_n, seed=seed, mc_mode=mc_mode,
                       tile_uq=tile_uq, normalizer=normalizer, norm_fit=norm_fit, keep_tiles=keep_tiles,
                       headroom_every=headroom_every, headroom_min=headroom_min, range_screen=range_screen)
        pending = _Pending()
        decoder = _DeviceDecode(engines[0], pool, dev, slides)
        # With a pool, everything this function itself enqueues (H2D copies, concatenations, a device-side loader) goes to
        # a side stream, not to the default stream: the pool's CU-masked streams are ordinary (blocking) HIP streams, and
        # an operation on the legacy default stream is a barrier across all of those -- one such operation per batch and
        # the batches in flight never overlap (measured: 14.9 k tiles/s instead of 24 k through this function).
        prep = torch.cuda.Stream(device=dev) if (pool and cuda) else None
        if prep is not None:
            prep.wait_stream(torch.cuda.current_stream(dev))        # the caller's tensors were made there
        copy_stream = torch.cuda.Stream(device=dev) if cuda else None
        with (torch.cuda.stream(prep) if prep is not None else contextlib.nullcontext()), \
                contextlib.closing(iter(_Feeder(slides, mine, dev, copy_stream))) as chunks:
            for chunk in chunks:
                tiles = _device_tiles(chunk, engines[0], dev, decoder)
                sidx, gidx, segs = [], [], []
                for li, si, first, count in chunk.segs:
                    s = slides[si]
                    if count == 0:
                        continue
                    sidx.append(torch.full((count,), li, dtype=torch.int32, device=dev))
                    gidx.append(offsets[si] + first + np.arange(count, dtype=np.int64))
                    if table is not None:
                        segs.append((si, s.name, int(s.y_true), np.asarray(s.loc)[first:first + count] if with_loc else None, count))
                    if keep_tiles:
                        rows_slide += [s.name] * count
                        rows_true += [s.y_true] * count
                        if s.loc is not None:
                            rows_loc.append(np.asarray(s.loc)[first:first + count])
                if sidx:
                    assert tiles.shape[0] == sum(len(g) for g in gidx), (chunk.segs, tiles.shape)
                    pending.push(tiles, sidx, gidx, segs)
                while pending.n >= batch:
                    run.run(*pending.take(batch))
            if pending.n:
                run.run(*pending.take(pending.n))
        if prep is not None:
            torch.cuda.current_stream(dev).wait_stream(prep)
        if pool:
            pool.synchronize()
        run.final_looks()
        decoder.check(block=True)                        # what is left: the last chunks
        live = [a for a in run.acc if a is not None]
        if live:
            # per-stream fixed-point accumulators are integers: their sum is exact and order-free
            tot = live[0] if len(live) == 1 else tuple(sum(a[j] for a in live[1:]) + live[0][j] for j in range(3))
            mp, mu, cnt = engines[0].slide_finish(tot)
            mp, mu, cnt = mp.cpu().numpy(), mu.cpu().numpy(), cnt.cpu().numpy()
        else:
            mp = mu = np.zeros(0); cnt = np.zeros(0, dtype=np.int64)
    except BaseException:
        if table is not None:
            table.abort()
        raise
    # this rank's rows are on disk and its file closed BEFORE the collective: whoever leaves the gather knows every shard is complete
    table_path, table_rows = None, 0
    if table is not None:
        table_rows = table.finish()
        table_path = table.path
    cap = max(len(p) for p in parts) if parts else 0
    g_pred, g_unc, g_cnt = D.gather_slide_results(mine, mp[:n_local], mu[:n_local], cnt[:n_local],
                                                  len(slides), cap)
    if table is not None and world > 1 and rank == 0:
        table_path = assemble_shards(save_dir, table_name)
    tile_df = None
    if keep_tiles:
        mean, std = torch.cat(run.rows, 1).cpu().numpy() if run.rows else np.zeros((2, 0, 2), np.float32)
        loc = np.concatenate(rows_loc) if rows_loc and sum(len(x) for x in rows_loc) == len(rows_slide) else None
        tile_df = tile_frame(outcome, rows_slide, rows_true, mean, std, loc if (with_loc or table is None) else None)
        if save_dir is not None and table is None:
            table_path = save_tile_predictions(tile_df, save_dir, table_name if world == 1 else shard_name(table_name, rank))
            table_rows = len(tile_df)
            if world > 1:                        # (pandas shards carry the same index, without byte ranges: row counts order them)
                order = [[si, slides[si].name, slides[si].n_tiles, 0, 0] for si in mine if slides[si].n_tiles]
                write_shard_index(table_path, rank, world, outcome, 'loc_x' in tile_df.columns, order)
    n_pass = sum(int(c) for c in run.passthrough if c is not None)
    return EvalResult(tile_df, [s.name for s in slides], g_pred, g_unc, g_cnt,
                      np.array([s.y_true for s in slides]), list(mine), table_path, table_rows, run.monitor.min, run.monitor.checks,
                      n_pass, f16_screen_checks=run.screen.checks, f16_screen_headroom=run.screen.min,
                      f16_screened=sum(s.screened for s in run.screens), f16_screen_max_key=run.screen.max_key)
