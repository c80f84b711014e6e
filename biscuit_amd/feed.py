"""The feeding half of ``inference.evaluate``: slides and their chunk sources, the leased ring of pinned buffers, the feeder thread that reads,
packs and uploads ``_Chunk``s, and the compressed tile formats (``PNG_Z``, ``JPEG``), each described once from the host pack to the device decode."""
import contextlib
import os
import queue
import threading
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import tfrecord_native as tn

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
        return self.tiles() if callable(self.tiles) else self.tiles


class PngRows:
    """A slide's tiles as the tile reader leaves them when the GPU reverses the PNG scanline filters: uint8
    [T,px,1+3*px] (host, usually pinned).  ``evaluate`` copies them to the device and calls ``Engine.png_unfilter``."""
    def __init__(self, rows):
        self.rows = rows


def _align16(n):
    return (n + 15) & ~15


def _u32(buf):                   # the 32-bit view type of a slot: uint32 on the host (numpy), int32 on the device (torch) -- the same bytes
    return torch.int32 if torch.is_tensor(buf) else np.uint32


class _Format:
    """A compressed tile format, from the host pack to the device decode: which slides go this way (``ok``), where the arrays of a slot lie
    (``layout``), how tiles of a source get into the open chunk (``extract``), how the device decodes it (``scratch``, ``decode`` on a
    decode stream, ``finish`` on the consumer's) and the words of the error (``name``, ``what``).  Stateless: what it keeps of a chunk is that chunk's ``new_state``."""
    max_px = float('inf')

    def new_state(self, cap):                            # what ``extract`` keeps of a chunk while it fills; it travels with the chunk to ``decode``
        return cap

    def ok(self, src):
        """True when the whole slide of ``src`` (a ``TFRecordSource``) can go this way: one pass over the records, nothing decoded."""
        if not (src.z and tn.available() and src.n_tiles and src.tile_px <= self.max_px):
            return False
        reader = src._open()
        for first in range(0, src.n_tiles, CHUNK_TILES_Z):       # (chunk-wise: the offsets of one call are 32-bit)
            try:
                self.probe(reader, first, min(CHUNK_TILES_Z, src.n_tiles - first), src.tile_px)
            except (tn.UnsupportedImage, ValueError, IOError):
                return False
        return True

    def finish(self, eng, out, px):
        return out


class _PngZ(_Format):
    """PNG tiles as their zlib streams: [off u32[cap] | len u32[cap] | packed streams]; the device inflates one stream per lane
    (bq_png_inflate) and reverses the scanline filters."""
    name, what = 'PNG', 'inflate'
    max_px = 341             # the un-filter kernel takes rows of up to 1 024 bytes; slides of larger tiles stay on the host decoder

    def probe(self, reader, first, cnt, px):
        with contextlib.suppress(MemoryError):           # (headers fine, only the buffer was too small: as intended)
            reader.extract_z(first, cnt, px, np.zeros(1, np.uint8), np.zeros(cnt, np.uint32), np.zeros(cnt, np.uint32))

    def layout(self, buf, cap):
        """(offsets [cap], lengths [cap], the streams) of a slot of ``cap`` tiles."""
        return buf[:4 * cap].view(_u32(buf)), buf[4 * cap:8 * cap].view(_u32(buf)), buf[_align16(8 * cap):]

    def extract(self, c, src, first, cnt):
        off, ln, z = c.views
        used = src.read_z(first, cnt, z[c.pos:], off[c.n:], ln[c.n:])
        off[c.n:c.n + cnt] += np.uint32(c.pos)
        return used

    def scratch(self, eng, n, px):
        return eng.inflate_scratch(n)

    def decode(self, eng, buf, cap, count, px, scratch):
        off, ln, z = self.layout(buf, cap)
        return eng.png_inflate(z, off[:count], ln[:count], px=px, scratch=scratch)

    def finish(self, eng, rows, px):
        return eng.png_unfilter_strided(rows, px=px)


class _Jpeg(_Format):
    """Baseline-JPEG tiles as their entropy-coded segments: [desc u32[cap][4] | JPEG_SETS table sets | packed segments]; the table sets
    of the slides in a chunk are kept once each; the device decodes them to tiles (bq_jpeg_decode)."""
    name, what = 'JPEG', 'JPEG decoder'

    def probe(self, reader, first, cnt, px):
        reader.extract_jpeg(first, cnt, px, None, None, None)

    def layout(self, buf, cap):
        """(descriptors [cap, 4], table sets [JPEG_SETS, table bytes], the segments) of a slot of ``cap`` tiles."""
        tab0, tabs = _align16(16 * cap), JPEG_SETS * tn.jpeg_table_bytes()
        return buf[:16 * cap].view(_u32(buf)).reshape(cap, 4), buf[tab0:tab0 + tabs].reshape(JPEG_SETS, -1), buf[_align16(tab0 + tabs):]

    def new_state(self, cap):                            # ..., the chunk's table sets so far (bytes), room for those of one ``read_jpeg`` call
        return SimpleNamespace(cap=cap, sets=[], tmp=np.empty((JPEG_SETS, tn.jpeg_table_bytes()), np.uint8))

    def extract(self, c, src, first, cnt):
        (desc, tables, scan), sets, tmp = c.views, c.state.sets, c.state.tmp
        used, nt = src.read_jpeg(first, cnt, scan[c.pos:], desc := desc[c.n:], tmp)
        got = [tmp[k].tobytes() for k in range(nt)]
        new = [b for b in dict.fromkeys(got) if b not in sets]
        if len(sets) + len(new) > len(tables):           # (no room for this slide's tables: it starts the next chunk)
            return None
        for b in new:
            tables[len(sets)] = np.frombuffer(b, np.uint8)
            sets.append(b)
        desc[:cnt, 0] += np.uint32(c.pos)
        desc[:cnt, 3] = np.array([sets.index(b) for b in got], np.uint32)[desc[:cnt, 3]]
        return used

    def scratch(self, eng, n, px):
        return eng.jpeg_scratch(n, px)

    def decode(self, eng, buf, state, count, px, scratch):
        desc, tables, scan = self.layout(buf, state.cap)
        return eng.jpeg_decode(scan, desc[:count], tables[:len(state.sets)], px=px, scratch=scratch)


FORMATS = PNG_Z, JPEG = _PngZ(), _Jpeg()     # in the order a slide is offered them


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

    def _open(self):
        if self._reader is None:
            self._reader = tn.NativeReader(self.path)
        return self._reader

    def z_ok(self):
        """True when the whole slide can go the compressed way (every record an 8-bit RGB, non-interlaced PNG of the tile size)."""
        return PNG_Z.ok(self)

    def read_z(self, first, count, z, off, length):
        """The zlib streams of tiles [first, first + count) packed into ``z`` (uint8), offsets / lengths into ``off`` / ``length``
        (uint32 [count]).  Returns the bytes used; MemoryError (bytes needed in ``.args[1]``) when ``z`` is too small."""
        return self._reader.extract_z(first, count, self.tile_px, z, off, length)[0]

    def jpeg_ok(self):
        """True when the whole slide can go to the device JPEG decoder: every record a baseline JPEG of the tile size inside
        ``NativeReader.extract_jpeg``'s subset -- the host decoder's (8-bit, Huffman, one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0)
        WITHOUT grey tiles and WITHOUT restart intervals; a slide with one such record, or one progressive record, stays on
        ``read`` whole (host decoder or Pillow, as its probe decides).  One pass over the slide's bytes, nothing decoded."""
        return JPEG.ok(self)

    def read_jpeg(self, first, count, scan, desc, tables):
        """The entropy-coded segments of tiles [first, first + count) packed into ``scan`` (uint8), descriptors into ``desc`` (uint32
        [count, 4]), the distinct table sets into ``tables``.  Returns (bytes used, table sets used); MemoryError (bytes and sets
        needed in ``.args[1:]``) when ``scan`` or ``tables`` is too small."""
        return self._reader.extract_jpeg(first, count, self.tile_px, scan, desc, tables)[:2]

    def chunk_shape(self, count):
        px = self.tile_px
        return (count, px, 1 + 3 * px) if self.rows else (count, px, px, 3)

    def read(self, first, count, out):
        from . import tfrecord
        if self._fallback is None and tn.available():
            self._open()
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
    range; several only in a compressed chunk).  ``data``: the tiles ([count,px,px,3]); with ``rows`` their PNG scanlines ([count,px,1+3*px],
    filters to be reversed); with ``fmt`` a slot of ``px``-pixel tiles packed by that ``_Format``, whose ``state`` of it goes to its unpacker.  ``event``:
    behind the copy of ``data`` to the device; None: as the loader left it."""
    segs: list
    data: object
    event: object
    rows: bool = False
    fmt: Optional[_Format] = None
    px: int = 0
    state: object = None


class _Filling:
    """The compressed chunk being filled (gpu_decode): ``cap`` tiles of ``px`` pixels in ``fmt``'s layout in one slot ``buf`` (numpy uint8, usually pinned),
    one H2D copy.  It runs ACROSS slides (the device decodes one tile per lane: a 1 000-tile slide alone would leave the decode CUs' waves mostly empty)."""

    def __init__(self, fmt, slot, buf, cap, px):
        self.fmt, self.slot, self.cap, self.px, self.state = fmt, slot, cap, px, fmt.new_state(cap)
        self.views = fmt.layout(buf, cap)                # (..., the packed payload)
        self.hdr = buf.size - self.views[-1].size
        self.n, self.pos, self.segs = 0, 0, []           # tiles in the chunk, bytes of their payload, ...

    def add(self, src, li, si, first, left):
        """Pack tiles [first, ...) of ``src``, ``left`` at most, behind what is there; returns how many went in (0: the slot is full)."""
        cnt = min(self.cap - self.n, left)
        while cnt:
            try:
                used = self.fmt.extract(self, src, first, cnt)
                break
            except MemoryError:
                if cnt == 1 and not self.segs:
                    raise
                cnt //= 2                                # (tiles larger than the slot was sized for, or more table sets than a chunk carries)
        if not cnt or used is None:
            return 0
        self.segs.append((li, si, first, cnt))
        self.n, self.pos = self.n + cnt, self.pos + used
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
        self.ring = self.zc = None                       # the leased ring; the compressed chunk being filled (gpu_decode), if any
        self.n_chunks = 0                                # chunks decoded so far in this run (over all slides)

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
                src = s.source
                if src is None or s.n_tiles == 0 or self.copy_stream is None:
                    self._emit_z()
                    # a loader may launch GPU work of its own (tiles resident on the device): on this thread that must
                    # not be the legacy default stream -- a barrier across the pool's streams, and unordered against the
                    # consumer's -- but the copy stream, with an event for the consumer to wait on
                    ev = None
                    with (torch.cuda.stream(self.copy_stream) if self.copy_stream is not None else contextlib.nullcontext()):
                        loaded = s.load()
                        if self.copy_stream is not None and torch.is_tensor(loaded) and loaded.is_cuda:
                            ev = self.copy_stream.record_event()
                    rows = isinstance(loaded, PngRows)
                    self._put(_Chunk([(li, si, 0, s.n_tiles)], loaded.rows if rows else loaded, ev, rows))
                    continue
                try:
                    fmt = next((f for f in FORMATS if f.ok(src)), None) if getattr(src, 'z', False) else None    # (``z``: ``TFRecordSource``'s own)
                    if fmt is not None:
                        self._compressed(li, si, s, src, fmt)
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
            ev = self.copy_stream.record_event()
        self.ring.events[slot] = ev
        return d, ev

    def _emit_z(self):
        c, self.zc = self.zc, None
        if c is not None and c.segs:
            d, ev = self._upload(c.slot, self.ring.bufs[c.slot][:c.hdr + c.pos])
            self._put(_Chunk(c.segs, d, ev, fmt=c.fmt, px=c.px, state=c.state))

    def _compressed(self, li, si, s, src, fmt):
        """A slide that goes to the device compressed, in format ``fmt``.  A chunk holds one format and one tile size."""
        px = src.tile_px
        # (larger tiles: chunks of fewer; both layouts fit: 16 bytes of descriptor per tile and the table sets are the JPEG chunk's)
        self._need_ring(min(max(CHUNK_TILES_Z, *RAMP_CHUNKS_Z) * (16 + int(Z_FRACTION * px * (1 + 3 * px))) + JPEG_SETS * tn.jpeg_table_bytes() + 64, Z_SLOT_MAX))
        first = 0
        while first < s.n_tiles:
            if self.zc is not None and (self.zc.px != px or self.zc.fmt is not fmt):
                self._emit_z()
            if self.zc is None:
                cap = RAMP_CHUNKS_Z[self.n_chunks] if self.n_chunks < len(RAMP_CHUNKS_Z) else CHUNK_TILES_Z
                self.n_chunks += 1
                slot = self.ring.acquire()
                self.zc = _Filling(fmt, slot, self.ring.bufs[slot].numpy(), cap, px)
            cnt = self.zc.add(src, li, si, first, s.n_tiles - first)
            first += cnt
            if not cnt or self.zc.n == self.zc.cap:
                self._emit_z()

    def _decoded(self, li, si, s, src):
        per = int(np.prod(src.chunk_shape(1)))
        # (either layout of this tile size: see ``_PinnedRing``; no chunk of the ramp is larger than a slot)
        self._need_ring(max(CHUNK_TILES, *RAMP_CHUNKS) * max(per, src.tile_px * (1 + 3 * src.tile_px)))
        first = 0
        while first < s.n_tiles:
            size = RAMP_CHUNKS[self.n_chunks] if self.n_chunks < len(RAMP_CHUNKS) else CHUNK_TILES
            self.n_chunks += 1
            cnt = min(size, s.n_tiles - first)
            slot = self.ring.acquire()
            host = self.ring.bufs[slot][:cnt * per].view(src.chunk_shape(cnt))
            src.read(first, cnt, host.numpy())
            d, ev = self._upload(slot, host)
            self._put(_Chunk([(li, si, first, cnt)], d, ev, bool(src.rows)))
            first += cnt


class _DeviceDecode:
    """gpu_decode: compressed chunks are decoded on the pool's decode streams (CU-masked: the compute units it keeps out of the
    inference streams; without a pool, the current stream), round-robin, each with its own scratch per format; the status words
    are looked at one chunk late (``check``)."""

    def __init__(self, eng0, pool, dev, slides):
        self.eng0, self.dev, self.slides = eng0, dev, slides
        self.streams = getattr(pool, 'decode_streams', None) if pool else None
        self.k = 0                                       # chunks so far: the round-robin counter
        self.scratch = {}                                # (decode stream, format) -> (the tiles and tile size it is for, its scratch)
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
                raise IOError(f'the device {fmt.what} refused {len(bad)} tile(s) (first: {where}, status {int(status[bad[0]])}): damaged '
                              f'{fmt.name} data; decode on the host (gpu_decode=False) to see the decoder\'s own error')

    def decode(self, chunk):
        """A compressed chunk -> its tiles (uint8 NHWC), ordered before the current stream's work that follows."""
        eng0, fmt, buf, px, count = self.eng0, chunk.fmt, chunk.data, chunk.px, sum(c for *_, c in chunk.segs)
        main = torch.cuda.current_stream(self.dev)
        dec = self.streams[self.k % len(self.streams)] if self.streams else main
        self.k += 1
        dec.wait_event(chunk.event)
        buf.record_stream(dec)
        with torch.cuda.stream(dec):
            key = (dec.cuda_stream, fmt)
            n, for_px, scratch = self.scratch.get(key, (0, 0, None))
            if n < count or for_px < px:
                n = max(count, CHUNK_TILES_Z)
                self.scratch[key] = n, px, (scratch := fmt.scratch(eng0, n, px))
            out, status = fmt.decode(eng0, buf, chunk.state, count, px, scratch)
            done = dec.record_event()
        main.wait_event(done)
        out.record_stream(main)
        # the status words leave the device behind the decode (a few KB, pinned, on the decode stream) and are looked at when the NEXT
        # chunk arrives -- one chunk late, without stalling anything: a damaged stream stops the run there instead of after it
        host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
        with torch.cuda.stream(dec):
            host.copy_(status, non_blocking=True)
            ev = dec.record_event()
        self.check(block=False)
        self.status.append((chunk.segs, host, ev, fmt))
        return fmt.finish(eng0, out, px)                 # (PNG: inflated on the decode CUs, un-filtered here)
