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
from .predictions import (EVAL_NAME, TableWriter, assemble_shards, remove_stale_shards, save_tile_predictions, shard_name,
                          tile_frame, write_shard_index)


@dataclass
class Slide:
    """One slide = one TFRecord's worth of tiles.  ``tiles`` is either a uint8 array
    [T,299,299,3] (host or device) or a zero-argument callable returning one.  ``source`` (optional): an object with
    ``read(first, count, out)`` that decodes tiles [first, first + count) into a caller-supplied uint8 buffer and a
    ``rows`` flag (``TFRecordSource``): ``evaluate`` then streams the slide in fixed chunks through a ring of reusable
    pinned buffers instead of calling ``tiles``."""
    name: str
    tiles: object
    n_tiles: int
    y_true: int = 0
    patient: Optional[str] = None
    loc: Optional[np.ndarray] = None
    source: Optional[object] = None

    def load(self):
        t = self.tiles() if callable(self.tiles) else self.tiles
        return t


class PngRows:
    """A slide's tiles as the tile reader leaves them when the GPU reverses the PNG scanline filters: uint8
    [T,px,1+3*px] (host, usually pinned).  ``evaluate`` copies them to the device and calls ``Engine.png_unfilter``."""
    def __init__(self, rows):
        self.rows = rows


class TFRecordSource:
    """Chunk-wise decoder of one slide's TFRecord for ``evaluate``'s pinned ring: ``read(first, count, out)`` decodes
    tiles [first, first + count) into ``out`` (a uint8 numpy view, usually of page-locked memory) on the reader's thread
    pool.  ``rows``: stop at the inflated PNG scanlines ([count,px,1+3*px]; the GPU reverses the filters).  A slide with
    a record outside the native decoders' subset is decoded whole with Pillow once and served from memory."""
    def __init__(self, path, n_tiles, tile_px=299, rows=False, z=False):
        self.path, self.n_tiles, self.tile_px, self.rows = path, int(n_tiles), int(tile_px), bool(rows)
        # z: hand the tiles over COMPRESSED (``read_z``: the records' zlib streams, packed; the device inflates them -- bq_png_inflate;
        # ``read_jpeg``: the entropy-coded segments of baseline-JPEG tiles; the device decodes them -- bq_jpeg_decode);
        # decided per slide before its first chunk: a slide with a record outside both device subsets stays on ``read``
        self.z = bool(z)
        self._reader = None
        self._fallback = None
        self._probed = False                    # the once-per-slide decoder decision (``read``) has been taken

    def z_ok(self):
        """True when the whole slide can go the compressed way (every record an 8-bit RGB, non-interlaced PNG of the tile size)."""
        from . import tfrecord_native as tn
        # (larger tiles: the un-filter kernel takes rows of up to 1 024 bytes = 341 px; those slides stay on the host decoder)
        if not (self.z and tn.available() and self.n_tiles and self.tile_px <= 341):
            return False
        if self._reader is None:
            self._reader = tn.NativeReader(self.path)
        probe = np.zeros(1, np.uint8)
        off, ln = np.zeros(CHUNK_TILES_Z, np.uint32), np.zeros(CHUNK_TILES_Z, np.uint32)
        for first in range(0, self.n_tiles, CHUNK_TILES_Z):      # (chunk-wise: the offsets of one call are 32-bit)
            try:
                self._reader.extract_z(first, min(CHUNK_TILES_Z, self.n_tiles - first), self.tile_px, probe, off, ln)
            except MemoryError:
                continue                                 # (headers fine, only the buffer was too small: as intended)
            except (tn.UnsupportedImage, ValueError, IOError):
                return False
        return True

    def read_z(self, first, count, z, off, length):
        """The zlib streams of tiles [first, first + count) packed into ``z`` (uint8), offsets / lengths into ``off`` / ``length``
        (uint32 [count]).  Returns the bytes used; MemoryError (bytes needed in ``.args[1]``) when ``z`` is too small."""
        return self._reader.extract_z(first, count, self.tile_px, z, off, length)[0]

    def jpeg_ok(self):
        """True when the whole slide can go to the device JPEG decoder: every record a baseline JPEG of the tile size inside
        ``NativeReader.extract_jpeg``'s subset -- the host decoder's (8-bit, Huffman, one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0)
        WITHOUT grey tiles and WITHOUT restart intervals; a slide with one such record, or one progressive record, stays on
        ``read`` whole (host decoder or Pillow, as its probe decides).  One pass over the slide's bytes, nothing decoded."""
        from . import tfrecord_native as tn
        if not (self.z and tn.available() and self.n_tiles):
            return False
        if self._reader is None:
            self._reader = tn.NativeReader(self.path)
        for first in range(0, self.n_tiles, CHUNK_TILES_Z):      # (chunk-wise: the offsets of one call are 32-bit)
            try:
                self._reader.extract_jpeg(first, min(CHUNK_TILES_Z, self.n_tiles - first), self.tile_px, None, None, None)
            except (tn.UnsupportedImage, ValueError, IOError):
                return False
        return True

    def read_jpeg(self, first, count, scan, desc, tables):
        """The entropy-coded segments of tiles [first, first + count) packed into ``scan`` (uint8), descriptors into ``desc`` (uint32
        [count, 4]), the distinct table sets into ``tables``.  Returns (bytes used, table sets used); MemoryError (bytes and sets
        needed in ``.args[1:]``) when ``scan`` or ``tables`` is too small."""
        return self._reader.extract_jpeg(first, count, self.tile_px, scan, desc, tables)[:2]

    def chunk_shape(self, count):
        px = self.tile_px
        return (count, px, 1 + 3 * px) if self.rows else (count, px, px, 3)

    def read(self, first, count, out):
        from . import tfrecord, tfrecord_native as tn
        if self._fallback is None and tn.available():
            if self._reader is None:
                self._reader = tn.NativeReader(self.path)
            if not self._probed:
                # ONE decoder per slide, decided before its first chunk: a record the native decoders refuse (a progressive
                # JPEG, ...) sends the WHOLE slide to Pillow -- as the whole-slide loader does (Slide.load) -- instead of the chunks
                # from that record on: the native islow IDCT and Pillow's libjpeg-turbo are not bound to agree to the last bit.
                # (Its own flag: ``z_ok`` may have opened the reader already -- round 5 skipped the probe then.)
                self._probed = True
                if self._reader.probe(self.tile_px) is not None:
                    self._reader.close()
                    self._reader = None
                    self._fallback = tfrecord.read_slide(self.path, self.tile_px, rows=self.rows)[1]
            if self._reader is not None:
                try:
                    self._reader.decode(first, count, self.tile_px, out=out, rows=self.rows)
                    return
                except tn.UnsupportedImage:
                    # behind a clean probe only a damaged entropy-coded stream ends here; chunks of this slide went out already
                    if first > 0:
                        raise
        if self._fallback is None:                      # Pillow (or the pure-Python reader), the whole slide once
            self._fallback = tfrecord.read_slide(self.path, self.tile_px, rows=self.rows)[1]
        out[...] = self._fallback[first:first + count]

    def close(self):
        if self._reader is not None:
            self._reader.close()
            self._reader = None
        self._fallback = None
        self._probed = False


def pick_unfilter_mode(path, tile_px=299, sample=48):
    """'auto' for ``slides_from_tfrecords``: decode the first ``sample`` tiles of one slide both ways and keep the GPU
    un-filter only where it pays -- the host alone is slower than the GPU consumes tiles (~28 k/s) AND stopping at the
    scanlines makes it at least 8 % faster (noise-like synthetic tiles: Sub / Up rows, cheap on the host; photo-like
    tiles: +20-30 %).  Returns (use_gpu_unfilter, host tiles/s, rows tiles/s)."""
    import time
    from . import tfrecord_native as tn
    if not tn.available():
        return False, 0.0, 0.0
    try:
        with tn.NativeReader(path) as r:
            n = min(sample, len(r))
            if n == 0:
                return False, 0.0, 0.0
            r.decode(0, n, tile_px)                      # page cache, thread pool warm
            t0 = time.perf_counter(); r.decode(0, n, tile_px); t_full = time.perf_counter() - t0
            t0 = time.perf_counter(); r.decode(0, n, tile_px, rows=True); t_rows = time.perf_counter() - t0
    except (tn.UnsupportedImage, ValueError, IOError):
        return False, 0.0, 0.0
    full, rows = n / max(t_full, 1e-9), n / max(t_rows, 1e-9)
    return (full < 26000.0 and rows > 1.08 * full), full, rows


def slides_from_tfrecords(paths, labels, patients=None, tile_px=299, pinned=None, gpu_unfilter=None, gpu_decode=False):
    """One ``Slide`` per ``*.tfrecords`` file (Slideflow writes one file per slide).  Tiles are
    decoded lazily when the slide's turn comes (``evaluate`` decodes one slide ahead on a host thread);
    only the record headers are scanned up front.  labels: {slide name (file stem): 0/1}.
    ``pinned`` (default: when a GPU is present) decodes into page-locked memory so the H2D copy is
    asynchronous and overlaps the next slide's decode.  ``gpu_unfilter`` (default off; tiles up to 341 px): the host stops at
    the inflated PNG scanlines and the GPU reverses their filters (``Engine.png_unfilter``) -- 12-30 % more tiles per host
    core for 0.4-0.6 ms of GPU time per launch of up to 512 tiles (host side): for hosts whose cores,
    not the GPU, bound the run."""
    from . import tfrecord
    if pinned is None:
        pinned = torch.cuda.is_available()
    if gpu_unfilter == 'auto':                          # a short measurement on the first slide decides
        gpu_unfilter = bool(paths) and tile_px <= 341 and torch.cuda.is_available() and pick_unfilter_mode(paths[0], tile_px)[0]
    gpu_unfilter = bool(gpu_unfilter)
    # gpu_decode (round 5): the host only walks the record framing and copies the PNG tiles' zlib streams; the GPU inflates them
    # (one stream per lane, on compute units an ``EnginePool(reserve_cus=...)`` keeps out of the inference streams' masks) and
    # reverses the scanline filters.  For hosts with few cores per GPU: 16 CUs inflate 27-39 k tiles/s (profiles/r05_inflate.txt).
    # Baseline-JPEG slides go the same way: the host parses the markers and copies the scan bytes, the GPU does the entropy decode,
    # the IDCT, the upsampling and the colour conversion (``Engine.jpeg_decode``; profiles/jpeg_decode.txt) -- the same bytes.
    gpu_decode = bool(gpu_decode) and bool(pinned)
    out = []
    for path in paths:
        name = os.path.splitext(os.path.basename(path))[0]
        count = tfrecord.count_records(path)

        def loader(pth=path, n=count):
            if gpu_unfilter and n:
                t = torch.empty((n, tile_px, 1 + 3 * tile_px), dtype=torch.uint8, pin_memory=bool(pinned))
                tfrecord.read_slide(pth, tile_px, out=t.numpy(), rows=True)
                return PngRows(t)
            if pinned and n:
                t = torch.empty((n, tile_px, tile_px, 3), dtype=torch.uint8, pin_memory=True)
                tfrecord.read_slide(pth, tile_px, out=t.numpy())
                return t
            return tfrecord.read_slide(pth, tile_px)[1]
        out.append(Slide(name, loader, count, y_true=int(labels.get(name, 0)),
                         patient=(patients or {}).get(name),
                         source=TFRecordSource(path, count, tile_px, rows=gpu_unfilter and not gpu_decode, z=gpu_decode) if pinned else None))
    return out


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
    stain_passthrough: int = 0               # tiles of this rank the Macenko normaliser passed through unchanged (degenerate)
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


CHUNK_TILES = 512        # tiles per pinned buffer: 137 MB at 299 px (a 10^4-tile slide is twenty chunks, never one allocation)
RAMP_CHUNKS = (128, 256) # the first chunks of a run are short: the GPU starts after 128 decoded tiles (4 ms of the decoder), not 512
CHUNK_TILES_Z = 4096     # compressed chunks (gpu_decode): one zlib stream per LANE, so a chunk is what keeps the decode CUs' waves full
RAMP_CHUNKS_Z = (512, 1024, 2048)
Z_SLOT_MAX = 1 << 30      # bytes of one pinned slot of the compressed ring at most (three slots are leased)
Z_FRACTION = 0.9         # pinned bytes per tile of a compressed chunk, as a fraction of the raw scanlines (a nearly incompressible 299-px
                         # PNG: 227 KB of 268 KB = 0.85; a photograph-like one 0.58); a chunk that does not fit is cut in two
JPEG_SETS = 16           # table sets (Huffman lookups + quantisers, 21 KB each) a compressed JPEG chunk carries at most; a slide's tiles share one
RING_SLOTS = 3
PREFETCH_CHUNKS = 2      # decoded chunks waiting for the GPU (plus the one being decoded)


class _PinnedRing:
    """RING_SLOTS reusable page-locked buffers (page-locking 137 MB costs tens of milliseconds, which round 3 paid per slide).  A
    slot is free again when the event recorded behind its last host-to-device copy has completed.  Rings are LEASED: one
    ``evaluate`` call holds a ring from its first chunk to its last and hands it back, so calls that follow each other reuse the
    same pinned memory and calls that overlap (two threads of one process) never share slots.  A ring is sized for the larger
    of the two chunk layouts of its tile size -- decoded tiles (px * px * 3 bytes) and filtered PNG scanlines (px * (1 + 3 px))
    -- so alternating the two modes does not re-allocate it (round 4 did: one size in the cache at a time)."""
    _idle = []                       # rings not leased at the moment
    _lock = threading.Lock()
    MAX_IDLE = 2

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.bufs = [torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(RING_SLOTS)]
        self.events = [None] * RING_SLOTS
        self.next = 0

    @staticmethod
    def chunk_bytes(tile_px):
        return CHUNK_TILES * tile_px * (1 + 3 * tile_px)

    @classmethod
    def lease(cls, nbytes):
        with cls._lock:
            for i, r in enumerate(cls._idle):
                if r.nbytes >= nbytes:
                    return cls._idle.pop(i)
            cls._idle.clear()                        # (a larger tile size: the smaller buffers go)
        return cls(nbytes)

    def release(self):
        for i, ev in enumerate(self.events):
            if ev is not None:
                ev.synchronize()
                self.events[i] = None
        with self._lock:
            if len(self._idle) < self.MAX_IDLE:
                self._idle.append(self)

    def acquire(self):
        i = self.next
        self.next = (i + 1) % RING_SLOTS
        if self.events[i] is not None:
            self.events[i].synchronize()             # (the feeder thread waits, not the thread that launches kernels)
            self.events[i] = None
        return i


@dataclass
class _Chunk:
    """What the feeder hands over: tiles in dataset order, ``segs`` = [(li, si, first, count)] (local and global slide index, tile
    range; several only in a compressed chunk).  ``kind``: 'tiles' ([count,px,px,3]), 'rows' (PNG scanlines [count,px,1+3*px], filters to be
    reversed), 'z' (``_ZChunk``'s layout, ``cap`` slots) or 'j' (``_JChunk``'s layout, ``cap`` slots, ``sets`` table sets).  ``event``: behind
    the copy of ``data`` to the device; None: as the loader left it."""
    kind: str
    segs: list
    data: object
    event: object
    cap: int = 0
    sets: int = 0


class _ZChunk:
    """The compressed chunk being filled (gpu_decode): [off u32[cap] | len u32[cap] | packed zlib streams] in one pinned slot, one H2D copy.
    It runs ACROSS slides (the device inflates one stream per lane: a 1 000-tile slide alone would leave the decode CUs' waves mostly empty)."""
    kind = 'z'

    def __init__(self, ring, slot, cap, px):
        self.slot, self.cap, self.px = slot, cap, px
        self.buf = ring.bufs[slot].numpy()
        self.hdr = (8 * cap + 15) & ~15
        self.n = self.pos = 0                            # tiles in the chunk, bytes of their streams
        self.segs = []

    def add(self, src, li, si, first, left):
        """Pack tiles [first, ...) of ``src``, ``left`` at most, behind what is there; returns how many went in (0: the slot is full)."""
        cap = self.cap
        cnt = min(cap - self.n, left)
        off = self.buf[:4 * cap].view(np.uint32)[self.n:]
        ln = self.buf[4 * cap:8 * cap].view(np.uint32)[self.n:]
        room = self.buf[self.hdr + self.pos:]
        while cnt:
            try:
                used = src.read_z(first, cnt, room, off, ln)
                break
            except MemoryError:
                if cnt == 1 and not self.segs:
                    raise
                cnt //= 2                                # (tiles that compress worse than the slot was sized for)
        if cnt:
            off[:cnt] += np.uint32(self.pos)
            self.segs.append((li, si, first, cnt))
            self.n += cnt
            self.pos += used
        return cnt


class _JChunk:
    """The compressed JPEG chunk being filled (gpu_decode): [desc u32[cap][4] | JPEG_SETS table sets | packed entropy-coded segments] in
    one pinned slot, one H2D copy.  Like ``_ZChunk`` it runs across slides; the table sets of the slides in it are kept once each."""
    kind = 'j'

    def __init__(self, ring, slot, cap, px):
        from . import tfrecord_native as tn
        self.slot, self.cap, self.px = slot, cap, px
        self.buf = ring.bufs[slot].numpy()
        self.tb = tn.jpeg_table_bytes()
        self.tab0, self.hdr = self.layout(cap, self.tb)
        self.n = self.pos = 0                            # tiles in the chunk, bytes of their segments
        self.segs, self.sets = [], []                    # ..., the chunk's table sets (bytes)
        self.tmp = np.zeros((JPEG_SETS, self.tb), np.uint8)

    @staticmethod
    def layout(cap, tb):
        """(offset of the table sets, offset of the segments) in a chunk of ``cap`` slots."""
        tab0 = (16 * cap + 15) & ~15
        return tab0, (tab0 + JPEG_SETS * tb + 15) & ~15

    def add(self, src, li, si, first, left):
        """Pack tiles [first, ...) of ``src``, ``left`` at most, behind what is there; returns how many went in (0: the slot is full)."""
        cap = self.cap
        cnt = min(cap - self.n, left)
        desc = self.buf[:16 * cap].view(np.uint32).reshape(cap, 4)[self.n:]
        room = self.buf[self.hdr + self.pos:]
        while cnt:
            try:
                used, nt = src.read_jpeg(first, cnt, room, desc, self.tmp)
                break
            except MemoryError:
                if cnt == 1 and not self.segs:
                    raise
                cnt //= 2                                # (tiles larger than the slot was sized for, or more table sets than a chunk carries)
        if cnt:
            new = [b for b in dict.fromkeys(self.tmp[k].tobytes() for k in range(nt)) if b not in self.sets]
            if len(self.sets) + len(new) > JPEG_SETS:    # (no room for this slide's tables: it starts the next chunk)
                return 0
            for b in new:
                k = len(self.sets)
                self.buf[self.tab0 + k * self.tb:self.tab0 + (k + 1) * self.tb] = np.frombuffer(b, np.uint8)
                self.sets.append(b)
            remap = np.array([self.sets.index(self.tmp[k].tobytes()) for k in range(nt)], np.uint32)
            desc[:cnt, 0] += np.uint32(self.pos)
            desc[:cnt, 3] = remap[desc[:cnt, 3]]
            self.segs.append((li, si, first, cnt))
            self.n += cnt
            self.pos += used
        return cnt


class _FeederStopped(Exception):
    """The consumer has gone (its ``finally`` set the stop flag): the feeder thread unwinds."""


class _Feeder:
    """Iterable over this rank's slides in order: yields ``_Chunk``s.  Slides with a ``source`` are decoded chunk by chunk on a
    feeder thread into the pinned ring and copied to the device on ``copy_stream``; PREFETCH_CHUNKS chunks may wait decoded and copied
    while the GPU works -- with 512-tile chunks that is two 1 000-tile slides of lead; the native decoder releases the GIL, so decode,
    H2D copy and kernels overlap.  Other slides are loaded whole on the same thread and handed over as they are (event None)."""

    def __init__(self, slides, mine, dev, copy_stream):
        self.slides, self.mine, self.dev, self.copy_stream = slides, mine, dev, copy_stream
        self.q = queue.Queue(maxsize=PREFETCH_CHUNKS)
        self.stop = threading.Event()
        self.ring = None
        self.n_chunks = 0                                # chunks decoded so far in this run (over all slides)
        self.zc = None                                   # the compressed chunk being filled (gpu_decode), if any

    def __iter__(self):
        th = threading.Thread(target=self._work, name='bq-tile-feeder', daemon=True)
        th.start()
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            self.stop.set()
            th.join(timeout=30)

    def _put(self, item):
        while not self.stop.is_set():
            with contextlib.suppress(queue.Full):
                self.q.put(item, timeout=0.1)
                return
        raise _FeederStopped

    def _work(self):
        try:
            for li, si in enumerate(self.mine):
                s = self.slides[si]
                src = getattr(s, 'source', None)
                if src is None or s.n_tiles == 0 or self.copy_stream is None:
                    self._emit_z()
                    # a loader may launch GPU work of its own (tiles resident on the device): on this thread that must
                    # not be the legacy default stream -- a barrier across the pool's streams, and unordered against the
                    # consumer's -- but the copy stream, with an event for the consumer to wait on
                    ev = None
                    with (torch.cuda.stream(self.copy_stream) if self.copy_stream is not None else contextlib.nullcontext()):
                        loaded = s.load()
                        if self.copy_stream is not None and torch.is_tensor(loaded) and loaded.is_cuda:
                            ev = torch.cuda.Event()
                            ev.record(self.copy_stream)
                    rows = isinstance(loaded, PngRows)
                    self._put(_Chunk('rows' if rows else 'tiles', [(li, si, 0, s.n_tiles)], loaded.rows if rows else loaded, ev))
                    continue
                try:
                    if getattr(src, 'z', False) and src.z_ok():
                        self._compressed(li, si, s, src, _ZChunk)
                    elif getattr(src, 'z', False) and src.jpeg_ok():
                        self._compressed(li, si, s, src, _JChunk)
                    else:
                        self._emit_z()                   # (a slide that goes the decoded way: what is open goes first)
                        self._decoded(li, si, s, src)
                finally:
                    src.close()
            self._emit_z()
            self._put(None)
        except _FeederStopped:
            pass
        except BaseException as e:                       # noqa: BLE001 -- re-raised in the consumer
            with contextlib.suppress(_FeederStopped):
                self._put(e)
        finally:
            if self.ring is not None:
                self.ring.release()

    def _need_ring(self, need):
        """The leased ring's slots hold ``need`` bytes after this (an open compressed chunk sits in the ring that goes: it goes first)."""
        if self.ring is None or self.ring.nbytes < need:
            self._emit_z()
            if self.ring is not None:
                self.ring.release()
            self.ring = _PinnedRing.lease(need)

    def _upload(self, slot, host):
        """``host`` (a view of ring slot ``slot``) -> a new device tensor, on the copy stream; (tensor, the copy's event)."""
        with torch.cuda.stream(self.copy_stream):
            d = torch.empty(host.shape, dtype=torch.uint8, device=self.dev)
            d.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.ring.events[slot] = ev
        return d, ev

    def _emit_z(self):
        c, self.zc = self.zc, None
        if c is not None and c.segs:
            d, ev = self._upload(c.slot, self.ring.bufs[c.slot][:c.hdr + c.pos])
            self._put(_Chunk(c.kind, c.segs, d, ev, c.cap, len(getattr(c, 'sets', ()))))

    def _compressed(self, li, si, s, src, chunk_type):
        """A slide that goes to the device compressed: PNG (``_ZChunk``) or baseline JPEG (``_JChunk``).  A chunk holds one format."""
        px = src.tile_px
        from . import tfrecord_native as tn
        # (larger tiles: chunks of fewer; both layouts fit: 16 bytes of descriptor per tile and the table sets are the JPEG chunk's)
        self._need_ring(min(CHUNK_TILES_Z * (16 + int(Z_FRACTION * px * (1 + 3 * px))) + JPEG_SETS * tn.jpeg_table_bytes() + 64, Z_SLOT_MAX))
        first = 0
        while first < s.n_tiles:
            if self.zc is not None and (self.zc.px != px or type(self.zc) is not chunk_type):
                self._emit_z()
            if self.zc is None:
                cap = RAMP_CHUNKS_Z[self.n_chunks] if self.n_chunks < len(RAMP_CHUNKS_Z) else CHUNK_TILES_Z
                self.n_chunks += 1
                self.zc = chunk_type(self.ring, self.ring.acquire(), cap, px)
            cnt = self.zc.add(src, li, si, first, s.n_tiles - first)
            first += cnt
            if not cnt or self.zc.n == self.zc.cap:
                self._emit_z()

    def _decoded(self, li, si, s, src):
        per = int(np.prod(src.chunk_shape(1)))
        px = getattr(src, 'tile_px', None)
        self._need_ring(max(CHUNK_TILES * per, _PinnedRing.chunk_bytes(px) if px else 0))
        first = 0
        while first < s.n_tiles:
            size = RAMP_CHUNKS[self.n_chunks] if self.n_chunks < len(RAMP_CHUNKS) else CHUNK_TILES
            self.n_chunks += 1
            cnt = min(size, s.n_tiles - first)
            slot = self.ring.acquire()
            host = self.ring.bufs[slot][:cnt * per].view(src.chunk_shape(cnt))
            src.read(first, cnt, host.numpy())
            d, ev = self._upload(slot, host)
            self._put(_Chunk('rows' if src.rows else 'tiles', [(li, si, first, cnt)], d, ev))
            first += cnt


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


class _DeviceDecode:
    """gpu_decode: compressed chunks are decoded on the pool's decode streams (CU-masked: the compute units it keeps out of the
    inference streams; without a pool, the current stream), round-robin, each with its own scratch -- PNG chunks inflated
    (``decode``), baseline-JPEG chunks decoded to tiles (``decode_jpeg``); the status words are looked at one chunk late (``check``)."""

    def __init__(self, eng0, pool, dev, slides):
        self.eng0, self.dev, self.slides = eng0, dev, slides
        self.streams = getattr(pool, 'decode_streams', None) if pool else None
        self.k = 0                                       # chunks so far: the round-robin counter
        self.scratch = {}                                # decode stream -> its table scratch
        self.status = []                                 # in flight: (the chunk's segments, pinned status words, event, format)

    def check(self, block):
        while self.status and (block or self.status[0][2].query()):
            segs, status, ev, fmt = self.status.pop(0)
            ev.synchronize()
            bad = np.flatnonzero(status.numpy()).tolist()
            if bad:
                at, where = 0, None
                for (_, si, first, c) in segs:
                    if at <= bad[0] < at + c:
                        where = f'{self.slides[si].name}, tile {first + bad[0] - at}'
                    at += c
                what = 'inflate' if fmt == 'PNG' else 'JPEG decoder'
                raise IOError(f'the device {what} refused {len(bad)} tile(s) (first: {where}, status {int(status[bad[0]])}): damaged {fmt} '
                              f'data; decode on the host (gpu_decode=False) to see the decoder\'s own error')

    def decode(self, chunk, px):
        """A compressed PNG chunk -> its tiles' filtered scanlines, ordered before the current stream's work that follows."""
        eng0, buf, cap, count = self.eng0, chunk.data, chunk.cap, sum(c for *_, c in chunk.segs)
        off = buf[:4 * count].view(torch.int32)
        ln = buf[4 * cap:4 * cap + 4 * count].view(torch.int32)
        z = buf[(8 * cap + 15) & ~15:]

        def work(key):
            if key not in self.scratch or self.scratch[key].numel() < eng0._lib.bq_png_inflate_scratch_bytes(count):
                self.scratch[key] = eng0.inflate_scratch(max(count, CHUNK_TILES_Z))
            return eng0.png_inflate(z, off, ln, px=px, scratch=self.scratch[key])
        return self._on_decode_stream(chunk, work, 'PNG')

    def decode_jpeg(self, chunk, px):
        """A compressed JPEG chunk -> its tiles (uint8 NHWC), ordered before the current stream's work that follows."""
        from . import tfrecord_native as tn
        eng0, buf, cap, count = self.eng0, chunk.data, chunk.cap, sum(c for *_, c in chunk.segs)
        tb = tn.jpeg_table_bytes()
        tab0, hdr = _JChunk.layout(cap, tb)
        desc = buf[:16 * count].view(torch.int32).view(count, 4)
        tables = buf[tab0:tab0 + chunk.sets * tb].view(chunk.sets, tb)
        scan = buf[hdr:]

        def work(key):
            key = (key, 'jpeg')
            if key not in self.scratch or self.scratch[key].numel() < eng0._lib.bq_jpeg_scratch_bytes(count, px):
                self.scratch[key] = eng0.jpeg_scratch(max(count, CHUNK_TILES_Z), px)
            return eng0.jpeg_decode(scan, desc, tables, px=px, scratch=self.scratch[key])
        return self._on_decode_stream(chunk, work, 'JPEG')

    def _on_decode_stream(self, chunk, work, fmt):
        buf = chunk.data
        main = torch.cuda.current_stream(self.dev)
        dec = self.streams[self.k % len(self.streams)] if self.streams else main
        self.k += 1
        dec.wait_event(chunk.event)
        buf.record_stream(dec)
        with torch.cuda.stream(dec):
            rows, status = work(dec.cuda_stream)
            done = torch.cuda.Event()
            done.record(dec)
        main.wait_event(done)
        rows.record_stream(main)
        # the status words leave the device behind the decode (a few KB, pinned, on the decode stream) and are looked at when the NEXT
        # chunk arrives -- one chunk late, without stalling anything: a damaged stream stops the run there instead of after it
        host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
        with torch.cuda.stream(dec):
            host.copy_(status, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(dec)
        self.check(block=False)
        self.status.append((chunk.segs, host, ev, fmt))
        return rows


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
        self.passthrough = [None] * len(engines)         # per stream: int64 device count of the tiles the Macenko kernel passed through
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
            if self.normalizer == 'macenko':
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
    tissue, one colour) are counted on the device and read once at the end: ``EvalResult.stain_passthrough`` (this rank's)."""
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
                if chunk.kind == 'z':                    # a compressed chunk: inflate on the decode CUs, un-filter here
                    px = slides[chunk.segs[0][1]].source.tile_px
                    tiles = engines[0].png_unfilter_strided(decoder.decode(chunk, px), px=px)
                elif chunk.kind == 'j':                  # a compressed JPEG chunk: decoded to tiles on the decode CUs
                    tiles = decoder.decode_jpeg(chunk, slides[chunk.segs[0][1]].source.tile_px)
                elif chunk.event is None:                # as the slide's loader left them
                    tiles = _to_device(chunk.data, dev)
                else:                                    # made on the copy stream: order it before this stream's work
                    torch.cuda.current_stream(dev).wait_event(chunk.event)
                    chunk.data.record_stream(torch.cuda.current_stream(dev))
                    tiles = chunk.data.contiguous()
                if chunk.kind == 'rows':                 # filtered PNG scanlines: the filters are reversed on the device
                    tiles = engines[0].png_unfilter(tiles)
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
