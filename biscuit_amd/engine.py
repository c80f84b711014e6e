"""Host side of the MI355X MC-dropout inference path.

``Engine`` owns one ``bq_ctx`` (one process per GPU), the uploaded weights and a
workspace; PyTorch-ROCm tensors are used only as device-memory containers whose
``data_ptr()`` is handed to the C ABI, and ``torch.cuda.current_stream()`` supplies the
HIP stream.  All arithmetic happens in ``libbiscuit_hip.so``.

``UncertaintyInterface`` mirrors the callable the reference uses in
``results.py:234,257-258``: ``interface(batch) -> (mean[B,2], std[B,2])``.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .hp import ModelParams, nature2022
from .weights import DTYPE_CODE, choose_act_exponents, pack_blob, tensor_taps

TILE_PX = 299


class BiscuitHipError(RuntimeError):
    pass


class F16RangeError(RuntimeError):
    """The f16 storage type met activations at (or within the demanded margin of) its range limit during a run: every f16 kernel
    clamps at +-65504 without a signal, so the results from there on are plausible and wrong.  Raised by ``inference.evaluate``'s
    headroom monitor; re-run with ``Engine.calibrate`` on tiles like the offending ones, or with dtype bf16 / f32."""


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@dataclass
class ProfileEntry:
    name: str
    launches: int
    ms: float
    flops: float
    bytes: float


class Engine:
    """One MC-dropout inference context on one GPU.

    weights: dict of numpy arrays in Keras layout (``biscuit_amd.weights``).
    dtype: storage / matrix-core type of the backbone -- 'f16' (IEEE half: the throughput mode that holds the 1e-3
    tolerance; saturates beyond +-65504), 'bf16' (same rate, 8x coarser rounding) or 'f32' (exact fp32 matrix-core
    path, the parity mode).  Accumulation, folded BN and the MC head are fp32 in all three.
    """

    def __init__(self, weights, hp: ModelParams = None, dtype='f16', max_batch=256, max_mc=30,
                 device=None, act_exp=None):
        if not torch.cuda.is_available():
            raise BiscuitHipError('no HIP device visible: the MI355X path has no CPU fallback')
        self.hp = hp or nature2022()
        self.weights = weights           # the caller's dict, not a copy: host arrays that live as long as the engine does (``train`` starts a
                                         # head from them and builds the engine of a trained head around the same backbone)
        self.dtype = dtype
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self.max_batch, self.max_mc = int(max_batch), int(max_mc)
        self._lib = _lib.lib
        if dtype not in DTYPE_CODE:
            raise ValueError(f'dtype must be one of {sorted(DTYPE_CODE)}, not {dtype!r}')
        cfg = _lib.BqConfig(DTYPE_CODE[dtype],
                            self.hp.tile_px, 2, float(self.hp.dropout), self.max_batch, self.max_mc)
        self._ctx = self._lib.bq_create(self.device.index, C.byref(cfg))
        if not self._ctx:
            raise BiscuitHipError('bq_create: ' + self._lib.bq_last_error(None).decode())
        self._check(self._lib.bq_set_dropout(self._ctx, float(self.hp.dropout)))     # the contract's rate is a double
        # activation exponents (weights.py: choose_act_exponents / Engine.calibrate): the f16 mode's range by construction
        self.act_exp = {t: int(k) for t, k in (act_exp or {}).items() if int(k)} if dtype == 'f16' else {}
        self._tap_exp = {tap: self.act_exp.get(t, 0) for t, taps in tensor_taps().items() for tap in taps}
        blob = pack_blob(weights, dtype, self.act_exp)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._check(self._lib.bq_load_weights(self._ctx, C.cast(buf, C.c_void_p), len(blob)))
        self._drop_caches()
        self._elt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[dtype]

    # shapes of the stored tensors by debug-tap name
    TAP_SHAPES = dict([('block1_conv1', (149, 149, 32)), ('block1_conv2', (147, 147, 64))] +
                      [(f'block2_{n}', (147, 147, 128)) for n in ('sepconv1', 'sepconv2')] +
                      [(f'block2_{n}', (74, 74, 128)) for n in ('res', 'out')] +
                      [(f'block3_{n}', (74, 74, 256)) for n in ('sepconv1', 'sepconv2')] +
                      [(f'block3_{n}', (37, 37, 256)) for n in ('res', 'out')] +
                      [(f'block4_{n}', (37, 37, 728)) for n in ('sepconv1', 'sepconv2')] +
                      [(f'block4_{n}', (19, 19, 728)) for n in ('res', 'out')] +
                      [(f'block{b}_{n}', (19, 19, 728)) for b in range(5, 13) for n in ('sepconv1', 'sepconv2', 'out')] +
                      [('block13_sepconv1', (19, 19, 728)), ('block13_sepconv2', (19, 19, 1024)), ('block13_res', (10, 10, 1024)),
                       ('block13_out', (10, 10, 1024)), ('block14_sepconv1', (10, 10, 1536)), ('block14_sepconv2', (10, 10, 2048))])

    @staticmethod
    def calibrate(weights, tiles_u8, hp=None, device=None, target_log2=12, norm_fit=None, normalizer='reinhard_fast'):
        """Activation exponents for the f16 storage type, measured: up to 16 of ``tiles_u8`` (uint8 [n,299,299,3], host or
        device; the tiles the model will see -- stain-normalised here when ``norm_fit`` is given) go through the fp32 kernels
        of this library, which have no range limit, every stored tensor is tapped, and ``weights.choose_act_exponents`` turns
        the peaks into powers of two (``normalizer``: the method of ``norm_fit``, stain.METHODS).  Returns ``(act_exp, peaks)``; pass ``act_exp`` to ``Engine`` / ``EnginePool``.  A
        network whose activations fit IEEE half as they are gets all-zero exponents and the blob it always had."""
        from . import stain
        stain.check(normalizer, norm_fit)
        t = torch.as_tensor(np.asarray(tiles_u8[:16]) if not torch.is_tensor(tiles_u8) else tiles_u8[:16])
        eng = Engine(weights, hp=hp, dtype='f32', max_batch=max(1, int(t.shape[0])), max_mc=1, device=device)
        try:
            t = t.to(eng.device).contiguous()
            t = stain.normalise(eng, t, normalizer, norm_fit)
            staged = eng.stage(t)
            peaks = {}
            for tensor, taps in tensor_taps().items():
                peaks[tensor] = max(float(eng.debug_activation(tap, staged, Engine.TAP_SHAPES[tap]).abs().max()) for tap in taps)
        finally:
            eng.close()
        bad = [k for k, v in peaks.items() if not np.isfinite(v)]
        if bad:
            raise BiscuitHipError(f'calibration: non-finite activations in {bad[:4]}')
        return choose_act_exponents(weights, peaks, target_log2), peaks

    # ------------------------------------------------------------------ utils
    def close(self):
        if getattr(self, '_ctx', None):
            self._lib.bq_destroy(self._ctx)
            self._ctx = None
            self._drop_caches()

    def drop_scratch(self):
        """Lets go of every device buffer grown on demand -- the network's workspace and each tool's scratch -- and of nothing else;
        the next call that wants one allocates it again."""
        self._ws = None                  # the network's workspace (``_ws_for``)
        self._tool_ws = {}               # family -> a tool's scratch (``_scratch``): inflate, jpeg, j2k, lzw, jpeg_encode, png_encode, knn, umap, uq, delong, train, validate, augment, exit_features, exit_train, exit_validate, exit_features_staged, exit_train_staged

    def _drop_caches(self):
        """Every device tensor the engine keeps between calls, empty: how ``__init__`` declares them and ``close()`` lets them go."""
        self.drop_scratch()
        self._tables = {}                # (tool, key) -> the tool's table(s) of that key on the device (``_table``)
        self._host_held = []             # (event, host tables) of the calls the stream may not have passed yet (``_hold``)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc is not None and rc < 0:
            raise BiscuitHipError(f'libbiscuit_hip error {rc}: '
                                  + self._lib.bq_last_error(self._ctx).decode())
        return rc

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _hold(self, *host):
        """Keeps the host arrays a call just handed to ``hipMemcpyAsync`` alive until an event recorded behind the call has completed
        (queried, never waited for), so back-to-back calls do not release one another's."""
        done = torch.cuda.current_stream(self.device).record_event()
        self._host_held = [(e, t) for e, t in self._host_held if not e.query()] + [(done, host)]

    @staticmethod
    def _check_cells(T, col, row, h, w):
        """ValueError for a threshold outside 0 .. 255 and for a range of ``col`` / ``row`` that is empty or leaves the ``h`` x ``w`` plane."""
        if not 0 <= int(T) <= 255:
            raise ValueError(f'T must lie in 0 .. 255, not {T!r}')
        for name, r, n in (('col', col, w), ('row', row, h)):
            if (r[:, 0] < 0).any() or (r[:, 0] >= r[:, 1]).any() or (r[:, 1] > n).any():
                raise ValueError(f'a {name} range is empty or outside the {h} x {w} plane')

    def _on_device(self, name, t):
        if not t.is_cuda or t.device != self.device:
            raise ValueError(f'{name} must be on {self.device}, not {t.device}')

    def _thumb_hw(self, thumb, same_device=False):
        """(H, W) of a thumbnail, uint8 [H, W, 3] with ``H * W < 2^31``; ValueError otherwise (``same_device``: and for one elsewhere)."""
        if not (torch.is_tensor(thumb) and thumb.dtype == torch.uint8 and thumb.dim() == 3 and thumb.shape[2] == 3):
            raise ValueError('thumb must be uint8 [H, W, 3]')
        if same_device:
            self._on_device('thumb', thumb)
        assert thumb.is_cuda and thumb.is_contiguous()
        h, w = int(thumb.shape[0]), int(thumb.shape[1])
        if h < 1 or w < 1 or h * w >= 1 << 31:
            raise ValueError(f'a thumbnail has 1 <= H, W and H * W < 2^31, not {h} x {w}')
        return h, w

    def _plane_hw(self, name, plane, same_device=False):
        """(H, W) of a mask's plane, uint8 [H, W] and not empty; ValueError otherwise (``same_device``: and for one elsewhere)."""
        if not (torch.is_tensor(plane) and plane.dtype == torch.uint8 and plane.dim() == 2 and plane.numel() > 0):
            raise ValueError(f'{name} must be uint8 [H, W]')
        if same_device:
            self._on_device(name, plane)
        assert plane.is_cuda and plane.is_contiguous()
        return int(plane.shape[0]), int(plane.shape[1])

    @staticmethod
    def _cell_tables(col, row):
        """The cells' ranges as contiguous int32 [gw, 2] / [gh, 2] host arrays; ValueError for another shape."""
        col, row = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(row, np.int32)
        if col.ndim != 2 or col.shape[1] != 2 or row.ndim != 2 or row.shape[1] != 2 or len(col) < 1 or len(row) < 1:
            raise ValueError('col and row must be int32 [gw, 2] and [gh, 2]')
        return col, row

    def _scratch(self, name, need, given=None):
        """A call's scratch, ``need`` bytes: what the caller gave (launches that may overlap on different streams bring their own),
        or the cached device buffer of the family ``name`` (a torch uint8 tensor), where the old one goes before a larger one comes."""
        if given is not None:
            return given
        if name not in self._tool_ws or self._tool_ws[name].numel() < need:
            self._tool_ws.pop(name, None)
            self._tool_ws[name] = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        return self._tool_ws[name]

    def _table(self, tool, key, build):
        """A tool's table(s) on the device: ``build()`` -> numpy array(s), built and uploaded once per ``(tool, key)`` and kept; a
        ``build`` that refuses its key stores nothing.  Later calls are one lookup."""
        held = self._tables.get((tool, key))
        if held is None:
            host = build()
            held = (torch.from_numpy(host).to(self.device) if isinstance(host, np.ndarray)
                    else tuple(torch.from_numpy(a).to(self.device) for a in host))
            self._tables[(tool, key)] = held
        return held

    def _bytes(self, n):
        """``n`` bytes on this device that the caller owns: what the ``*_scratch`` methods hand out."""
        return torch.empty(int(n), dtype=torch.uint8, device=self.device)

    @staticmethod
    def _canvas_args(n, place, canvas, clip):
        """What the canvas decoders take alike: ``place`` int32 [n, 2], ``canvas`` uint8 [H, W, 3] -> the clip rectangle's four ints."""
        assert place.dtype == torch.int32 and place.is_cuda and place.is_contiguous() and tuple(place.shape) == (n, 2)
        assert canvas.dtype == torch.uint8 and canvas.is_cuda and canvas.is_contiguous() and canvas.dim() == 3 and canvas.shape[2] == 3
        return tuple(int(v) for v in clip)

    def _decode_canvas(self, entry, family, head_args, n, seg_w, seg_h, place, canvas, clip, scratch):
        """The canvas decoders' call: ``bq_<entry>_decode_canvas(ctx, *head_args, place, canvas, H, W, clip, status, scratch, bytes,
        stream)`` -- ``head_args`` the codec's own leading arguments in its header's order -- with the scratch of ``family`` sized by
        ``bq_<entry>_canvas_scratch_bytes(n, seg_w, seg_h)`` unless the caller brought one.  -> status int32 [n] on the device."""
        x0, y0, x1, y1 = self._canvas_args(n, place, canvas, clip)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        scratch = self._scratch(family, int(getattr(self._lib, f'bq_{entry}_canvas_scratch_bytes')(n, seg_w, seg_h)), scratch)
        assert scratch.is_cuda and scratch.is_contiguous()
        self._check(getattr(self._lib, f'bq_{entry}_decode_canvas')(self._ctx, *head_args, _ptr(place), _ptr(canvas), int(canvas.shape[0]),
                                                                    int(canvas.shape[1]), x0, y0, x1, y1, _ptr(status), _ptr(scratch),
                                                                    scratch.numel() * scratch.element_size(), self._stream()))
        return status

    def _encode(self, entry, counter_attr, tiles, cap, scratch, scratch_bytes, *mid_args):
        """The encoders' call: ``bq_<entry>(ctx, tiles, n, px, *mid_args, out, cap, off, status, scratch, ...)`` with ``cap`` bytes of
        output, and once more with the exact total -- which the first call's offsets state -- when the files did not fit (status
        bit 1).  The scratch is the family ``entry``'s; ``counter_attr`` counts the calls.  -> ``(buffer[:total], offsets on the host)``."""
        n, px = int(tiles.shape[0]), int(tiles.shape[1])
        scratch = self._scratch(entry, int(scratch_bytes), scratch)
        off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        setattr(self, counter_attr, 0)
        while True:
            out = torch.empty(max(int(cap), 1), dtype=torch.uint8, device=self.device)
            self._check(getattr(self._lib, 'bq_' + entry)(self._ctx, _ptr(tiles), n, px, *mid_args, _ptr(out), int(cap), _ptr(off),
                                                          _ptr(status), _ptr(scratch), scratch.numel(), self._stream()))
            setattr(self, counter_attr, getattr(self, counter_attr) + 1)
            offsets = off.cpu()
            total = int(offsets[-1])
            if n == 0 or total <= int(cap):
                return out[:total], offsets
            assert getattr(self, counter_attr) == 1 and bool((status & 1).any()), f'bq_{entry}: the exact total did not fit'
            cap = total

    def _ws_for(self, n, mc_n):
        """Caller-owned device workspace (a torch uint8 tensor), grown on demand."""
        need = self._lib.bq_workspace_bytes(self._ctx, int(n), int(mc_n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        return self._ws

    def _mean_std(self, n, out):
        """The (mean, std) pair of a call, float32 [n, 2] each on the device: ``out`` when the caller gave one."""
        if out is not None:
            return out
        return tuple(torch.empty((n, 2), dtype=torch.float32, device=self.device) for _ in range(2))

    def set_num_cus(self, n):
        """Size the persistent kernels' grids for ``n`` compute units (``bq_set_num_cus``; 0: the whole device): what a context
        whose launches go to a CU-masked stream wants.  Results do not depend on it."""
        self._check(self._lib.bq_set_num_cus(self._ctx, int(n)))

    def set_option(self, name, value):
        """A tuning knob of the library that changes no result (``bq_set_option``), e.g. ``('inflate_variant', 1)``."""
        self._check(self._lib.bq_set_option(self._ctx, name.encode(), int(value)))

    # ------------------------------------------------------------------ stages
    def stage(self, tiles_u8):
        """uint8 NHWC [n,299,299,3] (device) -> standardised planar NCHW tensor."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        out = torch.empty((n, 3, TILE_PX, TILE_PX), dtype=self._elt, device=self.device)
        self._check(self._lib.bq_stage(self._ctx, _ptr(tiles_u8), n, _ptr(out), self._stream()))
        return out

    def png_unfilter(self, rows_u8):
        """PNG scanline filters reversed on the device (kernels_png.hip): uint8 [n,px,1+3*px] -- per row the filter-type byte
        and the filtered RGB bytes, as `tfrecord_native.NativeReader.decode(rows=True)` delivers them -- -> uint8 NHWC
        [n,px,px,3].  Bit-exact with a host PNG decoder."""
        assert rows_u8.dtype == torch.uint8 and rows_u8.is_cuda and rows_u8.is_contiguous() and rows_u8.dim() == 3
        n, px, rs = rows_u8.shape
        assert rs == 1 + 3 * px, rows_u8.shape
        out = torch.empty((n, px, px, 3), dtype=torch.uint8, device=self.device)
        self._check(self._lib.bq_png_unfilter(self._ctx, _ptr(rows_u8), n, px, _ptr(out), self._stream()))
        return out

    def png_inflate(self, z, off, length, px=TILE_PX, scratch=None):
        """The zlib streams of n PNG tiles, inflated on the device (``bq_png_inflate``, kernels_inflate.hip: one stream per lane):
        ``z`` uint8 [bytes] -- the packed streams of ``NativeReader.extract_z`` --, ``off`` / ``length`` int32 / uint32 [n], all on
        this device.  Returns ``(rows, status)``: rows uint8 [n, stride] (a tile's px rows of 1 + 3 px bytes, then padding to a
        multiple of 4) and status int32 [n], 0 where the stream inflated to exactly that many bytes with a matching Adler-32 --
        what zlib's ``uncompress`` accepts."""
        assert z.dtype == torch.uint8 and z.is_cuda and z.is_contiguous()
        n = int(off.shape[0])
        assert off.is_cuda and length.is_cuda and off.element_size() == 4 and length.element_size() == 4 and length.shape[0] == n
        row_bytes = px * (1 + 3 * px)
        stride = (row_bytes + 4 + 3) // 4 * 4
        rows = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        need = int(self._lib.bq_png_inflate_scratch_bytes(n))
        scratch = self._scratch('inflate', need, scratch)         # (a caller's own: ``inflate_scratch(n)``)
        assert scratch.numel() >= need
        self._check(self._lib.bq_png_inflate(self._ctx, _ptr(z), _ptr(off), _ptr(length), n, px, _ptr(rows), stride,
                                             _ptr(scratch), scratch.numel(), _ptr(status), self._stream()))
        return rows, status

    def inflate_scratch(self, n):
        """Table space for ``png_inflate`` over up to ``n`` streams (one buffer per launch that may be in flight)."""
        return self._bytes(self._lib.bq_png_inflate_scratch_bytes(int(n)))

    def png_unfilter_strided(self, rows, px=TILE_PX):
        """``png_inflate``'s rows [n, stride] -> uint8 NHWC [n,px,px,3] (``bq_png_unfilter_strided``)."""
        n = rows.shape[0]
        out = torch.empty((n, px, px, 3), dtype=torch.uint8, device=self.device)
        self._check(self._lib.bq_png_unfilter_strided(self._ctx, _ptr(rows), rows.shape[1], n, px, _ptr(out), self._stream()))
        return out

    def png_decode_z(self, z, off, length, px=TILE_PX):
        """Compressed PNG tiles -> uint8 NHWC [n,px,px,3] entirely on the device: ``png_inflate``, then the scanline filters
        reversed (``bq_png_unfilter_strided``).  Returns ``(tiles, status)``; a tile whose status is not 0 is undefined."""
        rows, status = self.png_inflate(z, off, length, px)
        return self.png_unfilter_strided(rows, px), status

    def jpeg_decode(self, scan, desc, tables, px=TILE_PX, scratch=None):
        """n baseline-JPEG tiles decoded on the device (``bq_jpeg_decode``, kernels_jpeg.hip: entropy decode one tile per lane,
        then IDCT, upsampling and colour conversion): ``scan`` uint8 [bytes], ``desc`` int32 / uint32 [n, 4] and ``tables`` uint8
        [k, table bytes] as ``NativeReader.extract_jpeg`` wrote them, all on this device.  Returns ``(tiles, status)``: tiles uint8
        NHWC [n,px,px,3] -- the bytes the host decoder and Pillow give -- and status int32 [n], 0 where the tile decoded (a tile
        whose status is not 0 was refused: its bytes are no image).  ``scratch``: ``jpeg_scratch(n, px)`` or larger; launches that
        may overlap on different streams bring their own."""
        assert scan.dtype == torch.uint8 and scan.is_cuda and scan.is_contiguous()
        n = int(desc.shape[0])
        assert desc.is_cuda and desc.is_contiguous() and desc.element_size() == 4 and tuple(desc.shape) == (n, 4)
        assert tables.dtype == torch.uint8 and tables.is_cuda and tables.is_contiguous() and tables.dim() == 2
        out = torch.empty((n, px, px, 3), dtype=torch.uint8, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        need = int(self._lib.bq_jpeg_scratch_bytes(n, px))
        scratch = self._scratch('jpeg', need, scratch)
        assert scratch.numel() >= need
        self._check(self._lib.bq_jpeg_decode(self._ctx, _ptr(scan), _ptr(desc), _ptr(tables), int(tables.shape[0]), n, px, _ptr(out),
                                             _ptr(status), _ptr(scratch), scratch.numel(), self._stream()))
        return out, status

    def jpeg_scratch(self, n, px=TILE_PX):
        """Coefficient space for ``jpeg_decode`` over ``n`` tiles (``bq_jpeg_scratch_bytes``: 554 KB per 299-px tile, for 2 048
        tiles at most -- 1.14 GB; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_jpeg_scratch_bytes(int(n), int(px)))

    def jpeg_decode_canvas(self, scan, desc, tables, seg_w, seg_h, place, canvas, clip, scratch=None):
        """A slide page's own JPEG tiles decoded on the device INTO a canvas (``bq_jpeg_decode_canvas``, kernels_jpeg.hip: the
        entropy and IDCT kernels of ``jpeg_decode``, then a colour-and-place kernel): ``scan``, ``desc``, ``tables`` as
        ``tfrecord_native.extract_jpeg_segments`` packed the ``seg_w`` x ``seg_h`` segments, ``place`` int32 [n, 2] the canvas
        position (x, y) of each segment's top-left pixel (negative or past the canvas allowed), ``canvas`` uint8 [H, W, 3] and
        ``clip`` = (x0, y0, x1, y1) in canvas coordinates -- all tensors on this device.  Exactly the pixels of a segment inside
        both the canvas and ``clip`` are written; the caller fills the canvas beforehand (255 for a slide).  Returns status int32
        [n] on the device, 0 where the segment decoded.  ``scratch``: coefficient space of at least one segment
        (``jpeg_canvas_scratch(n, seg_w, seg_h)`` holds a whole round); the call works in rounds of as many segments as it holds."""
        assert scan.dtype == torch.uint8 and scan.is_cuda and scan.is_contiguous()
        n, seg_w, seg_h = int(desc.shape[0]), int(seg_w), int(seg_h)
        assert desc.is_cuda and desc.is_contiguous() and desc.element_size() == 4 and tuple(desc.shape) == (n, 4)
        assert tables.dtype == torch.uint8 and tables.is_cuda and tables.is_contiguous() and tables.dim() == 2
        return self._decode_canvas('jpeg', 'jpeg', (_ptr(scan), _ptr(desc), _ptr(tables), int(tables.shape[0]), n, seg_w, seg_h),
                                   n, seg_w, seg_h, place, canvas, clip, scratch)

    def jpeg_canvas_scratch(self, n, seg_w, seg_h):
        """Coefficient space for ``jpeg_decode_canvas`` over ``n`` segments (``bq_jpeg_canvas_scratch_bytes``: 393 KB per 256 x 256
        segment, for 2 048 segments at most; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_jpeg_canvas_scratch_bytes(int(n), int(seg_w), int(seg_h)))

    def j2k_decode_canvas(self, desc, blocks, cw, seg_w, seg_h, place, canvas, clip, ycc=False, scratch=None):
        """A slide page's own JPEG 2000 tiles decoded on the device INTO a canvas (``bq_j2k_decode_canvas``, kernels_j2k.hip: tier
        1 a lane per code block, the inverse wavelet transform a workgroup per segment and component, then a colour-and-place
        kernel): ``desc`` int32 [n, 32], ``blocks`` int32 [k, 12] and ``cw`` uint8 [bytes] as ``tfrecord_native.j2k_extract``
        packed the ``seg_w`` x ``seg_h`` segments; ``place``, ``canvas`` and ``clip`` as ``jpeg_decode_canvas`` takes them;
        ``ycc``: the samples are YCbCr (TIFF compression 33003) -- all tensors on this device.  Returns status int32 [n] on the
        device, 0 where the segment decoded; any other segment wrote nothing.  ``scratch``: at least one segment's
        (``j2k_canvas_scratch(n, seg_w, seg_h)`` holds a whole round); the call works in rounds of as many as it holds."""
        n, seg_w, seg_h = int(desc.shape[0]), int(seg_w), int(seg_h)
        assert desc.dtype == torch.int32 and desc.is_cuda and desc.is_contiguous() and tuple(desc.shape) == (n, 32)
        assert blocks.dtype == torch.int32 and blocks.is_cuda and blocks.is_contiguous() and blocks.dim() == 2 and blocks.shape[1] == 12
        assert cw.dtype == torch.uint8 and cw.is_cuda and cw.is_contiguous()
        return self._decode_canvas('j2k', 'j2k', (_ptr(desc), n, _ptr(blocks), int(blocks.shape[0]), _ptr(cw), cw.numel(), seg_w, seg_h,
                                                  int(bool(ycc))), n, seg_w, seg_h, place, canvas, clip, scratch)

    def j2k_canvas_scratch(self, n, seg_w, seg_h):
        """Plane space for ``j2k_decode_canvas`` over ``n`` segments (``bq_j2k_canvas_scratch_bytes``: 24 bytes a pixel, 1.5 MB per
        256 x 256 segment, for 256 segments at most; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_j2k_canvas_scratch_bytes(int(n), int(seg_w), int(seg_h)))

    def lzw_decode_canvas(self, data, desc, seg_w, seg_h, place, canvas, clip, predictor=1, scratch=None):
        """A slide page's own LZW tiles decoded on the device INTO a canvas (``bq_lzw_decode_canvas``, kernels_lzw.hip: the code
        chain a wave per segment, strings copied out of the segment's earlier output 64 bytes a step, then a kernel that undoes
        the predictor and places the rows): ``data`` uint8 [bytes] and ``desc`` int32 / uint32 [n, 2] of (offset, length) as
        ``tfrecord_native.lzw_pack`` packed the ``seg_w`` x ``seg_h`` segments; ``place``, ``canvas`` and ``clip`` as
        ``jpeg_decode_canvas`` takes them; ``predictor`` the page's (1: none, 2: horizontal differencing) -- all tensors on this
        device.  Returns status int32 [n] on the device, 0 where the segment decoded (``tfrecord_native.LZW_*`` bits otherwise);
        any other segment wrote nothing.  ``scratch``: at least one segment's (``lzw_canvas_scratch(n, seg_w, seg_h)`` holds a
        whole round); the call works in rounds of as many as it holds."""
        n, seg_w, seg_h = int(desc.shape[0]), int(seg_w), int(seg_h)
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        assert desc.is_cuda and desc.is_contiguous() and desc.element_size() == 4 and tuple(desc.shape) == (n, 2)
        if int(predictor) not in (1, 2):
            raise ValueError(f'predictor must be 1 or 2, not {predictor!r}')
        return self._decode_canvas('lzw', 'lzw', (_ptr(data), _ptr(desc), n, seg_w, seg_h, int(predictor)),
                                   n, seg_w, seg_h, place, canvas, clip, scratch)

    def lzw_canvas_scratch(self, n, seg_w, seg_h):
        """Output space for ``lzw_decode_canvas`` over ``n`` segments (``bq_lzw_canvas_scratch_bytes``: 3 bytes a pixel, 196 608
        per 256 x 256 segment, for 1 024 segments at most; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_lzw_canvas_scratch_bytes(int(n), int(seg_w), int(seg_h)))

    def jpeg_encode(self, tiles, quality=95, subsampling='4:2:0', cap=None, scratch=None):
        """n tiles encoded as baseline JPEG on the device (``bq_jpeg_encode``, kernels_jpeg_encode.hip): ``tiles`` uint8 NHWC
        [n, px, px, 3] on this device -> ``(buffer, offsets)``: buffer uint8 [bytes] on the device, offsets int64 [n + 1] on the
        host; file i = ``buffer[offsets[i]:offsets[i + 1]]``, the bytes Pillow's ``save(buf, 'JPEG', quality=quality,
        subsampling=subsampling)`` writes ('4:2:0' or '4:4:4').  ``cap``: bytes of the output buffer to try first (None: a
        guess from the tile size and quality); when the files do not fit (status bit 1) the call is repeated once with the
        exact total, which the first call's offsets state.  Reading the offsets waits for the stream.  ``scratch``:
        ``jpeg_encode_scratch(n, px, subsampling)`` or smaller (more rounds), at least one tile's."""
        from .tfrecord_native import jpeg_subsampling
        assert tiles.dtype == torch.uint8 and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 4
        assert tiles.shape[1] == tiles.shape[2] and tiles.shape[3] == 3, tuple(tiles.shape)
        n, px, sub, quality = int(tiles.shape[0]), int(tiles.shape[1]), jpeg_subsampling(subsampling), int(quality)
        if cap is None:                     # (about 2 bits a sample at quality 95; the retry covers what this misses)
            cap = n * (1024 + px * px * 3 // (4 if quality < 98 else 2))
        return self._encode('jpeg_encode', 'jpeg_encode_calls', tiles, cap, scratch,
                            self._lib.bq_jpeg_encode_scratch_bytes(n, max(px, 1), sub), quality, sub)

    def jpeg_encode_scratch(self, n, px=TILE_PX, subsampling='4:2:0'):
        """Scratch for ``jpeg_encode`` over ``n`` tiles (``bq_jpeg_encode_scratch_bytes``: 889 KB per 299-px tile at 4:2:0, for 256
        tiles at most -- 228 MB; a longer call works in rounds)."""
        from .tfrecord_native import jpeg_subsampling
        return self._bytes(self._lib.bq_jpeg_encode_scratch_bytes(int(n), int(px), jpeg_subsampling(subsampling)))

    def png_encode(self, tiles, cap=None, scratch=None):
        """n tiles encoded as PNG on the device (``bq_png_encode``, kernels_png_encode.hip): ``tiles`` uint8 NHWC [n, px, px, 3]
        on this device -> ``(buffer, offsets)``: buffer uint8 [bytes] on the device, offsets int64 [n + 1] on the host; file i =
        ``buffer[offsets[i]:offsets[i + 1]]``, a complete PNG whose filtered rows are Pillow's and whose deflate stream is
        the library's own (``tfrecord_native.png_encode`` writes the same bytes on the CPU).  Lossless, no settings.  ``cap``:
        bytes of the output buffer to try first (None: half the raw size, which a tissue tile stays under); when the files
        do not fit (status bit 1) the call is repeated once with the exact total, which the first call's offsets state.
        Reading the offsets waits for the stream.  ``scratch``: ``png_encode_scratch(n, px)`` or smaller (more rounds), at least
        one tile's."""
        assert tiles.dtype == torch.uint8 and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 4
        assert tiles.shape[1] == tiles.shape[2] and tiles.shape[3] == 3, tuple(tiles.shape)
        n, px = int(tiles.shape[0]), int(tiles.shape[1])
        if cap is None:
            cap = n * (1024 + px * px * 3 // 2)
        return self._encode('png_encode', 'png_encode_calls', tiles, cap, scratch,
                            self._lib.bq_png_encode_scratch_bytes(n, max(px, 1)))

    def png_encode_scratch(self, n, px=TILE_PX):
        """Scratch for ``png_encode`` over ``n`` tiles (``bq_png_encode_scratch_bytes``: 1.71 MB per 299-px tile, for 128 tiles at
        most -- 218 MB; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_png_encode_scratch_bytes(int(n), int(px)))

    def augment(self, tiles_u8, params, out=None, status=None, scratch=None):
        """Slideflow's training augmentation 'xyrjb' on the device (``bq_augment``, kernels_augment.hip): ``tiles_u8`` uint8 NHWC
        [n, px, px, 3] on this device, 8 <= px <= 4096, and ``params`` uint8 [n, 4] = (k, flips, quality, blur) per tile
        (``augment.draw``) -> ``(tiles, status)``: ``blur(flip_ud(flip_lr(rot90^k(jpeg_quality(tile)))))``, the bytes
        ``augment.apply_host`` gives, and status int32 [n] on the device (0, or 1 where the JPEG round trip left its exact range).
        ``params`` on the host is checked (ValueError for a byte out of range) and uploaded; a device tensor is taken as it is,
        and a row out of range there leaves its tile unchanged with status 2.  ``out`` (must not overlap ``tiles_u8``) and
        ``status``: tensors to write into.  ``scratch``: ``augment_scratch(n, px)`` or smaller (more rounds), at least one
        tile's.  The all-zero row is the identity."""
        from . import augment as A
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous() and tiles_u8.dim() == 4
        assert tiles_u8.shape[1] == tiles_u8.shape[2] and tiles_u8.shape[3] == 3, tuple(tiles_u8.shape)
        n, px = int(tiles_u8.shape[0]), int(tiles_u8.shape[1])
        if not A.MIN_PX <= px <= A.MAX_PX:
            raise ValueError(f'the augmenter takes tiles of {A.MIN_PX} .. {A.MAX_PX} px, not {px}')
        if not torch.is_tensor(params):
            params = torch.from_numpy(A.check_params(params, n)).to(self.device)
        self._on_device('params', params)
        assert params.dtype == torch.uint8 and params.is_contiguous() and tuple(params.shape) == (n, 4)
        if out is None:
            out = torch.empty_like(tiles_u8)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == tuple(tiles_u8.shape)
        assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and tuple(status.shape) == (n,)
        scratch = self._scratch('augment', int(self._lib.bq_augment_scratch_bytes(n, px)), scratch)
        assert scratch.is_cuda and scratch.is_contiguous()
        self._check(self._lib.bq_augment(self._ctx, _ptr(tiles_u8), n, px, _ptr(params), _ptr(out), _ptr(status), _ptr(scratch),
                                         scratch.numel() * scratch.element_size(), self._stream()))
        return out, status

    def augment_scratch(self, n, px=TILE_PX):
        """Scratch for ``augment`` over ``n`` tiles (``bq_augment_scratch_bytes``: 1.09 MB per 299-px tile, for 256 tiles at most --
        279 MB; a longer call works in rounds)."""
        return self._bytes(self._lib.bq_augment_scratch_bytes(int(n), int(px)))

    def tile_resample(self, canvas, origin, src_px, px=TILE_PX, out=None):
        """The heatmap's tile grid cut from a slide canvas and resampled on the device (``bq_tile_resample``,
        kernels_resample.hip): ``canvas`` uint8 [H, W, 3] and ``origin`` int32 [n, 2] -- the (x, y) of every tile's ``src_px``
        window in the canvas; windows may overlap and may leave the canvas (white there) -- on this device -> uint8 NHWC
        [n, px, px, 3], the bytes Pillow's ``resize((px, px), LANCZOS)`` gives for each window (``src_px == px``: the window
        itself).  ``out``: a contiguous [n, px, px, 3] uint8 tensor (or view) to write into.  The tap tables of a ``(src_px,
        px)`` pair are built on the host once (``resample.taps``) and stay on the device."""
        assert canvas.dtype == torch.uint8 and canvas.is_cuda and canvas.is_contiguous() and canvas.dim() == 3 and canvas.shape[2] == 3
        assert origin.dtype == torch.int32 and origin.is_cuda and origin.is_contiguous() and origin.dim() == 2 and origin.shape[1] == 2
        n, src_px, px = int(origin.shape[0]), int(src_px), int(px)
        if out is None:
            out = torch.empty((n, px, px, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, px, px, 3)
        bounds = coef = None
        k = 0
        if src_px != px:
            from . import resample
            bounds, coef = self._table('tile_resample', (src_px, px), lambda: resample.taps(src_px, px))
            k = int(coef.shape[1])
        self._check(self._lib.bq_tile_resample(self._ctx, _ptr(canvas), int(canvas.shape[0]), int(canvas.shape[1]), _ptr(origin), n,
                                               src_px, px, _ptr(bounds), _ptr(coef), k, _ptr(out), self._stream()))
        return out

    def tile_grayspace(self, tiles_u8, threshold=0.05):
        """Grey pixels per tile (``bq_tile_grayspace``): uint8 NHWC [n, px, px, 3] on this device -> int32 [n] on the device,
        the number of pixels whose HSV saturation is below ``threshold`` by the float64 definition (``resample.grayspace_limit``
        turns it into the integer table the kernel compares against)."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous() and tiles_u8.dim() == 4
        assert tiles_u8.shape[1] == tiles_u8.shape[2] and tiles_u8.shape[3] == 3
        from . import resample
        key = float(threshold)
        limit = self._table('tile_grayspace', key, lambda: resample.grayspace_limit(key))
        n = int(tiles_u8.shape[0])
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_tile_grayspace(self._ctx, _ptr(tiles_u8), n, int(tiles_u8.shape[1]), _ptr(limit), _ptr(count),
                                                self._stream()))
        return count

    def heatmap_render(self, values, col_table, row_table, lut, thumb, vmin=0.0, vmax=1.0, alpha=0.6, interpolation='none', out=None):
        """One plane of the heatmap grid drawn over the slide's thumbnail (``bq_heatmap_render``, kernels_render.hip; DESIGN.md
        "Heatmap output"): ``values`` float32 [gh, gw] (a cell that holds -1 or a non-finite value is transparent), ``col_table``
        / ``row_table`` int32 as ``render.render_tables`` builds them for ``interpolation`` ('none': [W] / [H]; 'bicubic': [W, 9]
        / [H, 9]), ``lut`` uint8 [256, 3] and ``thumb`` uint8 [H, W, 3] -- all on this device -> uint8 [H, W, 3], the bytes of
        the numpy restatement.  ``out``: a contiguous [H, W, 3] uint8 tensor to write into; it may be ``thumb`` itself (in place)
        and must not overlap it otherwise.  ValueError for ``vmin >= vmax``, a non-finite bound, ``alpha`` outside [0, 1], a
        table of the wrong shape or an unknown interpolation (``render.check_params``)."""
        from . import render
        lo, inv, a256, mode = render.check_params(vmin, vmax, alpha, interpolation)
        for t in (values, col_table, row_table, lut, thumb):
            assert t.is_cuda and t.is_contiguous()
        if values.dtype != torch.float32 or values.dim() != 2 or values.numel() == 0:
            raise ValueError('values must be float32 [gh, gw]')
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError(f'a colour table is uint8 [256, 3], not {lut.dtype} {list(lut.shape)}')
        if thumb.dtype != torch.uint8 or thumb.dim() != 3 or thumb.shape[2] != 3:
            raise ValueError('thumb must be uint8 [H, W, 3]')
        h, w = int(thumb.shape[0]), int(thumb.shape[1])
        want = ((w,), (h,)) if mode == 0 else ((w, render.RENDER_ENTRY), (h, render.RENDER_ENTRY))
        if col_table.dtype != torch.int32 or row_table.dtype != torch.int32 or (tuple(col_table.shape), tuple(row_table.shape)) != want:
            raise ValueError(f'the tables of a {h} x {w} {interpolation!r} render are int32 {list(want[0])} and {list(want[1])}')
        if out is None:
            out = torch.empty_like(thumb)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.shape == thumb.shape
        self._check(self._lib.bq_heatmap_render(self._ctx, _ptr(values), int(values.shape[0]), int(values.shape[1]), _ptr(col_table),
                                                _ptr(row_table), mode, _ptr(lut), _ptr(thumb), _ptr(out), h, w, float(lo), float(inv),
                                                a256, self._stream()))
        return out

    def tissue_blur(self, thumb_u8):
        """The tissue mask's first stage (``bq_tissue_blur``, kernels_tissue.hip; DESIGN.md "Heatmap input", Tissue mask): the
        slide's thumbnail uint8 [H, W, 3] on this device -> (plane uint8 [H, W], the 7 x 7 median of its 8-bit saturation with a
        replicated border, and hist int32 [256], the plane's histogram), both on the device, the integers of the numpy
        restatement.  ``H * W < 2^31``; H or W below 7 are legal."""
        h, w = self._thumb_hw(thumb_u8)
        from . import tissue
        sdiv = self._table('tissue_blur', None, tissue.sdiv_table)
        plane = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        hist = torch.empty(256, dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_tissue_blur(self._ctx, _ptr(thumb_u8), h, w, _ptr(sdiv), _ptr(plane), _ptr(hist), self._stream()))
        return plane, hist

    def tissue_cells(self, plane, T, col, row):
        """The tissue mask's second stage (``bq_tissue_cells``): ``plane`` uint8 [H, W] on this device (``tissue_blur``'s), the
        threshold ``T`` in 0 .. 255 and the cells' ranges ``col`` int32 [gw, 2] / ``row`` int32 [gh, 2] in plane pixels
        (``tissue.cell_ranges``; host arrays) -> int32 [gh, gw] on the device: the pixels with ``plane <= T`` in every cell.
        ValueError for a range that is empty or leaves the plane."""
        h, w = self._plane_hw('plane', plane)
        col, row = self._cell_tables(col, row)
        self._check_cells(T, col, row, h, w)
        gw, gh = len(col), len(row)
        ranges = torch.empty(2 * (gw + gh), dtype=torch.int32, device=self.device)
        count = torch.empty((gh, gw), dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_tissue_cells(self._ctx, _ptr(plane), h, w, int(T), col.ctypes.data, gw, row.ctypes.data, gh,
                                              _ptr(ranges), _ptr(count), self._stream()))
        self._hold(col, row)
        return count

    def tissue_focus(self, thumb_u8, threshold=0.02, sigma=3.0, value=False):
        """The focus mask's first stage (``bq_tissue_focus``, kernels_focus.hip; DESIGN.md "Heatmap input", Focus mask): a
        thumbnail uint8 [H, W, 3] on this device -> (plane uint8 [H, W], 1 = in focus and 0 = out of focus, and count int32 [1],
        the number of out-of-focus pixels), with ``value=True`` also V int32 [H, W], the Gaussian-blurred |Laplacian| of the
        gray image in units of ``tissue.FOCUS_SCALE`` -- all on the device, the integers of the numpy restatement.  A pixel is
        out of focus iff ``V <= floor(threshold * FOCUS_SCALE)``.  ``H * W < 2^31``; H or W below the radius are legal.
        ValueError as ``tissue.check_focus``."""
        from . import tissue
        h, w = self._thumb_hw(thumb_u8, same_device=True)
        thr = tissue.focus_units(threshold)
        key = float(sigma)
        d_taps = self._table('tissue_focus', key, lambda: tissue.focus_taps(key))
        r = (d_taps.numel() - 1) // 2
        work = torch.empty((h, w), dtype=torch.int32, device=self.device)
        v = torch.empty((h, w), dtype=torch.int32, device=self.device) if value else None
        plane = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_tissue_focus(self._ctx, _ptr(thumb_u8), h, w, _ptr(d_taps), r, thr, _ptr(work),
                                              None if v is None else _ptr(v), _ptr(plane), _ptr(count), self._stream()))
        return (plane, count, v) if value else (plane, count)

    def tissue_cells_union(self, otsu_plane, T, focus_plane, col, row, xmap=None, ymap=None):
        """The union of the two masks per grid cell (``bq_tissue_cells_union``): ``otsu_plane`` uint8 [Ho, Wo] (``tissue_blur``'s)
        with its threshold ``T``, ``focus_plane`` uint8 [Hf, Wf] (``tissue_focus``'s), both on this device, and the cells' ranges
        in pixels of the Otsu plane (``tissue.cell_ranges``; host arrays) -> int32 [gh, gw] on the device: the pixels of every
        cell with ``otsu_plane <= T`` or ``focus_plane[ymap[y], xmap[x]] == 0``.  ``xmap`` int32 [Wo] / ``ymap`` int32 [Ho] lay the
        focus plane over the Otsu plane; None: ``tissue.plane_map``'s nearest-neighbour resize.  ValueError for a range that is
        empty or leaves the plane, and for a map of the wrong length, outside the focus plane or decreasing."""
        from . import tissue
        ho, wo = self._plane_hw('otsu_plane', otsu_plane, same_device=True)
        hf, wf = self._plane_hw('focus_plane', focus_plane, same_device=True)
        col, row = self._cell_tables(col, row)
        gw, gh = len(col), len(row)
        if gw > tissue.MAX_GRID or gh > tissue.MAX_GRID:
            raise ValueError(f'a grid is 1 .. {tissue.MAX_GRID} cells a side, not {gh} x {gw}')
        self._check_cells(T, col, row, ho, wo)
        xmap = tissue.plane_map(wo, wf) if xmap is None else np.ascontiguousarray(xmap, np.int32)
        ymap = tissue.plane_map(ho, hf) if ymap is None else np.ascontiguousarray(ymap, np.int32)
        for name, m, n_to, n_from in (('xmap', xmap, wo, wf), ('ymap', ymap, ho, hf)):
            if m.shape != (n_to,):
                raise ValueError(f'{name} must be int32 [{n_to}], not {list(m.shape)}')
            if (m < 0).any() or (m >= n_from).any() or (np.diff(m) < 0).any():
                raise ValueError(f'{name} leaves the focus plane ({n_from}) or decreases')
        tables = torch.empty(wo + ho + 2 * (gw + gh), dtype=torch.int32, device=self.device)
        count = torch.empty((gh, gw), dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_tissue_cells_union(self._ctx, _ptr(otsu_plane), ho, wo, int(T), _ptr(focus_plane), hf, wf,
                                                    xmap.ctypes.data, ymap.ctypes.data, col.ctypes.data, gw, row.ctypes.data, gh,
                                                    _ptr(tables), _ptr(count), self._stream()))
        self._hold(col, row, xmap, ymap)
        return count

    def roi_plane(self, xs, ys, polygons):
        """The region-of-interest mask's plane (``bq_roi_plane``, kernels_roi.hip; DESIGN.md "Heatmap input", Region-of-interest
        mask): ``xs`` int32 [W] / ``ys`` int32 [H], the doubled level-0 coordinates of the sample points (``roi.center_tables`` /
        ``roi.raster_tables``; host arrays, every entry in [0, 2^29]), and ``polygons``, a list of int [n >= 3, 2] arrays of (x, y)
        vertices in level-0 pixels (``roi.check_polygons``) -> uint8 [H, W] on the device: 1 where (xs[x], ys[y]) lies inside any
        polygon (even-odd per polygon, union across polygons), the integers of the numpy restatement.  ValueError for a polygon
        ``roi.check_polygons`` refuses, a table of another shape or range, and ``H * W >= 2^31``."""
        from . import roi
        edges, starts = roi.edge_table(polygons)
        xs, ys = np.ascontiguousarray(xs, np.int32), np.ascontiguousarray(ys, np.int32)
        if xs.ndim != 1 or ys.ndim != 1 or len(xs) < 1 or len(ys) < 1 or len(xs) * len(ys) >= 1 << 31:
            raise ValueError('xs and ys must be int32 [W] and [H] with 1 <= W, H and H * W < 2^31')
        for name, t in (('xs', xs), ('ys', ys)):
            if (t < 0).any() or (t > roi.SAMPLE_MAX).any():
                raise ValueError(f'{name}: a doubled sample coordinate leaves [0, 2^29]')
        w, h = len(xs), len(ys)
        tables = torch.empty(edges.size + len(starts) + w + h, dtype=torch.int32, device=self.device)     # (the allocator aligns to 16)
        plane = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        self._check(self._lib.bq_roi_plane(self._ctx, edges.ctypes.data, len(edges), starts.ctypes.data, len(starts) - 1, xs.ctypes.data,
                                           w, ys.ctypes.data, h, _ptr(tables), _ptr(plane), self._stream()))
        self._hold(edges, starts, xs, ys)
        return plane

    # ------------------------------------------------------------------ the feature map (DESIGN.md "Feature map (Figure 6)")
    def knn(self, x, k, scratch=None):
        """Exact ``k`` nearest neighbours of the rows of ``x`` fp32 [n, D] on this device (``bq_knn``, kernels_knn.hip; D a multiple
        of 16, 1 <= k <= 64, k <= n) -> ``(idx int32 [n, k], dist fp32 [n, k])``: Euclidean distances, every row sorted by
        (distance, index) ascending, the row itself a candidate like any other: ``umap.knn_host``'s table bit for bit, on every row.
        ``scratch``: ``knn_scratch(n, D, k)`` or larger; ``knn_exhaustive_rows`` reads from it which rows the pruning pass could
        not prove.  ValueError for a shape or a ``k`` the entry refuses, and for an ``x`` that is not finite (one host
        synchronisation to learn it)."""
        if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 2):
            raise ValueError('x must be fp32 [n, D]')
        self._on_device('x', x)
        assert x.is_contiguous()
        n, d, k = int(x.shape[0]), int(x.shape[1]), int(k)
        need = int(self._lib.bq_knn_workspace_bytes(n, d, k))
        if need == 0:
            raise ValueError(f'knn takes 1 <= k <= 64, k <= n and D a multiple of 16, not n = {n}, D = {d}, k = {k}')
        if not bool(torch.isfinite(x).all()):
            raise ValueError('knn takes finite values only: x holds a NaN or an infinity')
        scratch = self._scratch('knn', need, scratch)
        assert scratch.numel() >= need
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        dist = torch.empty((n, k), dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_knn(self._ctx, _ptr(x), n, d, k, _ptr(idx), _ptr(dist), _ptr(scratch), scratch.numel(), self._stream()))
        return idx, dist

    def knn_scratch(self, n, d, k):
        """Candidate lists for ``knn`` over ``n`` rows (one buffer per launch that may be in flight)."""
        return self._bytes(self._lib.bq_knn_workspace_bytes(int(n), int(d), int(k)))

    def knn_exhaustive_rows(self, n, scratch=None):
        """Which of the ``n`` rows of the last ``knn`` on ``scratch`` (None: the engine's own) were ranked again over all rows,
        because the pruning pass's certificate did not cover them: bool [n] on the device, a copy of the flags ``bq_knn`` leaves
        in the first 4 n bytes of its workspace."""
        scratch = self._tool_ws.get('knn') if scratch is None else scratch
        if scratch is None or scratch.numel() < 4 * int(n):
            raise ValueError('no knn of that many rows has run on this scratch')
        return scratch[:4 * int(n)].view(torch.int32) != 0

    def umap_smooth(self, idx, dist, scratch=None):
        """The fuzzy graph's rows from ``knn``'s table (``bq_umap_smooth``, kernels_umap.hip) -> ``(rho [n], sigma [n], w [n, k])``
        fp32 on the device: the membership weight of every (row, neighbour), 0 for the row itself."""
        if not (torch.is_tensor(idx) and torch.is_tensor(dist) and idx.dtype == torch.int32 and dist.dtype == torch.float32 and
                idx.dim() == 2 and idx.shape == dist.shape and idx.shape[0] >= 1 and 1 <= idx.shape[1] <= 64):
            raise ValueError('idx int32 [n, k] and dist fp32 [n, k] with 1 <= n and 1 <= k <= 64')
        self._on_device('idx', idx)
        self._on_device('dist', dist)
        assert idx.is_contiguous() and dist.is_contiguous()
        n, k = int(idx.shape[0]), int(idx.shape[1])
        scratch = self._scratch('umap', int(self._lib.bq_umap_smooth_scratch_bytes(n)), scratch)
        rho = torch.empty(n, dtype=torch.float32, device=self.device)
        sigma = torch.empty(n, dtype=torch.float32, device=self.device)
        w = torch.empty((n, k), dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_umap_smooth(self._ctx, _ptr(idx), _ptr(dist), n, k, _ptr(rho), _ptr(sigma), _ptr(w), _ptr(scratch),
                                             scratch.numel(), self._stream()))
        return rho, sigma, w

    def umap_epoch(self, prev, graph, epoch, alpha, a, b, seed, out=None, block=0):
        """One epoch (1-based) of the layout in gather form (``bq_umap_epoch``, kernels_umap.hip): ``prev`` fp32 [n, 2], ``graph`` the
        symmetric CSR on this device as ``(indptr int64 [n + 1], nbr int32 [nnz], eps fp32 [nnz], next fp32 [nnz])`` --
        ``umap.graph_to_device`` checks and uploads one; ``next`` is advanced in place -- -> the new positions fp32 [n, 2] (``out``,
        another tensor than ``prev``).  ``block``: threads per workgroup (0: 64); the result does not depend on it."""
        indptr, nbr, eps, nxt = graph
        n = int(prev.shape[0])
        assert prev.dtype == torch.float32 and prev.is_cuda and prev.is_contiguous() and tuple(prev.shape) == (n, 2)
        assert indptr.dtype == torch.int64 and indptr.is_cuda and indptr.is_contiguous() and indptr.numel() == n + 1
        assert nbr.dtype == torch.int32 and eps.dtype == torch.float32 and nxt.dtype == torch.float32
        assert nbr.is_cuda and eps.is_cuda and nxt.is_cuda and nbr.is_contiguous() and eps.is_contiguous() and nxt.is_contiguous()
        assert nbr.numel() == eps.numel() == nxt.numel()
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, 2)
        self._check(self._lib.bq_umap_epoch(self._ctx, _ptr(prev), _ptr(out), n, _ptr(indptr), _ptr(nbr), _ptr(eps), _ptr(nxt), int(epoch),
                                            float(alpha), float(a), float(b), int(seed) & (2 ** 64 - 1), int(block), self._stream()))
        return out

    def reinhard_fast(self, tiles_u8, target_means, target_stds, out=None):
        """`reinhard_fast` stain normalisation (hp.py:19; results.py:251-252 `wsi_normalizer.rgb_to_rgb`):
        uint8 NHWC [n,299,299,3] -> uint8 NHWC.  target_means/target_stds: the CIE-LAB `norm_fit` of the
        model's params.json (3 floats each).  `out` may be the input tensor (in place)."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        tm = (C.c_float * 3)(*[float(v) for v in target_means])
        ts = (C.c_float * 3)(*[float(v) for v in target_stds])
        if out is None:
            out = torch.empty_like(tiles_u8)
        self._check(self._lib.bq_stain_reinhard_fast(self._ctx, _ptr(tiles_u8), tiles_u8.shape[0], tm, ts,
                                                     _ptr(out), self._stream()))
        return out

    def lab_stats(self, tiles_u8):
        """Per-tile CIE-LAB statistics [n,6] = mean L,a,b, std L,a,b (what the normaliser's fit() stores)."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        out = torch.empty((tiles_u8.shape[0], 6), dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_stain_lab_stats(self._ctx, _ptr(tiles_u8), tiles_u8.shape[0], _ptr(out),
                                                 self._stream()))
        return out

    @staticmethod
    def _reinhard_args(tiles_u8, flags, mask_threshold):
        """(n, px, flags, mask_L) of a Reinhard-family call: square uint8 NHWC tiles of any size the ABI takes; ``mask_L`` is
        float32(100 * mask_threshold), computed in float64 and rounded once."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        assert tiles_u8.dim() == 4 and tiles_u8.shape[1] == tiles_u8.shape[2] and tiles_u8.shape[3] == 3, tuple(tiles_u8.shape)
        with np.errstate(over='ignore'):
            mask_l = float(np.float32(100.0 * float(mask_threshold)))
        return int(tiles_u8.shape[0]), int(tiles_u8.shape[1]), int(flags), mask_l

    def reinhard(self, tiles_u8, target_means, target_stds, flags, mask_threshold=0.93, out=None, status=None):
        """Slideflow's Reinhard family (``bq_stain_reinhard``; DESIGN.md "Reinhard family"): uint8 NHWC [n,px,px,3] -> uint8 NHWC.
        ``flags``: 1 = brightness standardisation, 2 = tissue mask (``stain.REINHARD_FLAGS`` names the four methods; 0 gives
        ``reinhard_fast``'s bytes).  A pixel is tissue when its L is below ``100 * mask_threshold``.  `out` may be the input tensor
        (in place).  `status` (int32 [n] on the device, optional) receives each tile's status: 0 normalised, 1 no tissue pixel
        (only the brightness stage applied), 2 too dark to standardise (passed through)."""
        n, px, flags, mask_l = self._reinhard_args(tiles_u8, flags, mask_threshold)
        tm = (C.c_float * 3)(*[float(v) for v in target_means])
        ts = (C.c_float * 3)(*[float(v) for v in target_stds])
        if out is None:
            out = torch.empty_like(tiles_u8)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.shape == tiles_u8.shape
        if status is not None:
            assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() >= n
        self._check(self._lib.bq_stain_reinhard(self._ctx, _ptr(tiles_u8), n, px, flags, mask_l, tm, ts, _ptr(out), _ptr(status),
                                                self._stream()))
        return out

    def reinhard_stats(self, tiles_u8, flags, mask_threshold=0.93):
        """Each tile's own Reinhard-family fit (what ``stain.Reinhard.fit`` stores): ``(stats, status)`` device tensors, stats
        float32 [n,8] = mean L, a, b, std L, a, b over the tissue pixels of the brightness-standardised tile (NaN when the status
        is not 0), the 90th percentile of L (100 without flag 1), the tissue fraction; status int32 [n] as ``reinhard``."""
        n, px, flags, mask_l = self._reinhard_args(tiles_u8, flags, mask_threshold)
        stats = torch.empty((n, 8), dtype=torch.float32, device=self.device)
        st = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_stain_reinhard_stats(self._ctx, _ptr(tiles_u8), n, px, flags, mask_l, _ptr(stats), _ptr(st),
                                                      self._stream()))
        return stats, st

    def macenko(self, tiles_u8, he_ref, maxc_ref, out=None, status=None):
        """`macenko` stain normalisation (``bq_stain_macenko``; DESIGN.md "Macenko"): uint8 NHWC [n,299,299,3] -> uint8 NHWC.
        he_ref: the fit's stain matrix (3x2, columns H and E), maxc_ref: its two concentrations (> 0).  `out` may be the input
        tensor (in place).  `status` (int32 [n] on the device, optional) receives each tile's status: 0 normalised, 1 / 2 / 3
        degenerate (too little tissue / singular stain matrix / non-finite or non-positive concentration) and passed through."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        he = np.asarray(he_ref, dtype=np.float32).reshape(6)
        mc = np.asarray(maxc_ref, dtype=np.float32).reshape(2)
        if out is None:
            out = torch.empty_like(tiles_u8)
        if status is not None:
            assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() >= tiles_u8.shape[0]
        self._check(self._lib.bq_stain_macenko(self._ctx, _ptr(tiles_u8), tiles_u8.shape[0], (C.c_float * 6)(*he.tolist()),
                                               (C.c_float * 2)(*mc.tolist()), _ptr(out), _ptr(status), self._stream()))
        return out

    def macenko_stats(self, tiles_u8):
        """Each tile's own Macenko fit (what ``stain.Macenko.fit`` stores): ``(stats, status)`` device tensors, stats float32
        [n,8] = HE row-major (3x2, H first), maxC (2) -- NaN where a degenerate tile stopped before them --, status int32 [n,2] =
        status (as ``macenko``), number of tissue pixels."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        stats = torch.empty((n, 8), dtype=torch.float32, device=self.device)
        st = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        self._check(self._lib.bq_stain_macenko_stats(self._ctx, _ptr(tiles_u8), n, _ptr(stats), _ptr(st), self._stream()))
        return stats, st

    def stage_f32(self, tiles_f32):
        assert tiles_f32.dtype == torch.float32 and tiles_f32.is_cuda and tiles_f32.is_contiguous()
        n = tiles_f32.shape[0]
        out = torch.empty((n, 3, TILE_PX, TILE_PX), dtype=self._elt, device=self.device)
        self._check(self._lib.bq_stage_f32(self._ctx, _ptr(tiles_f32), n, _ptr(out), self._stream()))
        return out

    def backbone(self, staged):
        n = staged.shape[0]
        ws = self._ws_for(n, 1)
        feat = torch.empty((n, 2048), dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_backbone(self._ctx, _ptr(staged), n, _ptr(feat), _ptr(ws), ws.numel(),
                                          self._stream()))
        return feat

    def backbone_u8(self, tiles_u8):
        """uint8 NHWC tiles (device) -> [n,2048] features through the kernels ``mc_infer`` runs (``bq_backbone_u8``: in a
        16-bit context the fused front kernel, not stage + stem + conv2)."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        ws = self._ws_for(n, 1)
        feat = torch.empty((n, 2048), dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_backbone_u8(self._ctx, _ptr(tiles_u8), n, _ptr(feat), _ptr(ws), ws.numel(),
                                             self._stream()))
        return feat

    def mc_head(self, feat, mc_n, seed, tile_idx0=0, out=None, tile_idx=None):
        """GAP features [n,2048] -> (mean[n,2], std[n,2]) over mc_n dropout passes; the Philox tile counter of row i
        is tile_idx0 + i, or tile_idx0 + tile_idx[i] with ``tile_idx`` (int64 [n], device).  ``out``: (mean, std) to write into (contiguous [n,2] fp32 views are fine)."""
        assert feat.dtype == torch.float32 and feat.is_cuda and feat.is_contiguous()
        n = feat.shape[0]
        ws = self._ws_for(n, mc_n)
        state = torch.empty((n, 5), dtype=torch.float32, device=self.device)
        mean, std = self._mean_std(n, out)
        if out is not None:
            assert mean.is_contiguous() and std.is_contiguous() and mean.shape == (n, 2) and std.shape == (n, 2)
        with self._tile_index_array(tile_idx, n):
            self._check(self._lib.bq_mc_head(self._ctx, _ptr(feat), n, int(tile_idx0), int(mc_n), 0,
                                             int(seed), 1, 1, _ptr(state), _ptr(mean), _ptr(std), _ptr(ws),
                                             ws.numel(), self._stream()))
        return mean, std

    def set_tile_index_ptr(self, idx_tensor):
        """Device-side addend to ``tile_idx0`` of the head kernels (``bq_set_tile_index_ptr``): an int64 tensor of one
        element on this device, or None.  Kernels read it when they run, so a captured HIP graph can be replayed with
        another Philox tile counter by writing 8 bytes."""
        if idx_tensor is not None:
            assert idx_tensor.dtype == torch.int64 and idx_tensor.is_cuda and idx_tensor.numel() == 1
        self._check(self._lib.bq_set_tile_index_ptr(self._ctx, _ptr(idx_tensor)))

    def _tile_index_array(self, tile_idx, n):
        """Context manager: per-tile Philox indices (int64 [n] on this device, or None) for the calls made inside
        (``bq_set_tile_index_array``; the kernels take the pointer when they are LAUNCHED, the tensor has to outlive them)."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            if tile_idx is None:
                yield
                return
            assert tile_idx.dtype == torch.int64 and tile_idx.is_cuda and tile_idx.is_contiguous() and tile_idx.numel() == n
            self._check(self._lib.bq_set_tile_index_array(self._ctx, _ptr(tile_idx)))
            try:
                yield
            finally:
                self._lib.bq_set_tile_index_array(self._ctx, None)
        return scope()

    def mc_infer(self, tiles_u8, mc_n, seed, tile_idx0=0, mc_mode='head', out=None, tile_idx=None):
        """uint8 NHWC tiles (device) -> (mean[n,2], std[n,2]) on device.  ``tile_idx``: the tiles' Philox indices (int64 [n], device)
        when they are not ``tile_idx0 + row`` -- a batch across slide boundaries."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        ws = self._ws_for(n, mc_n)
        mean, std = self._mean_std(n, out)
        mode = _lib.BQ_MC_HEAD if mc_mode == 'head' else _lib.BQ_MC_FULL
        with self._tile_index_array(tile_idx, n):
            self._check(self._lib.bq_mc_infer(self._ctx, _ptr(tiles_u8), n, int(tile_idx0), int(mc_n),
                                              int(seed), mode, _ptr(mean), _ptr(std), _ptr(ws), ws.numel(),
                                              self._stream()))
        return mean, std

    def slide_reduce(self, mean2, std2, slide_idx, n_slides, tile_uq=None, acc=None):
        """Accumulate per-slide fixed-point sums; returns the accumulator triple."""
        n = mean2.shape[0]
        if acc is None:
            acc = (torch.zeros(n_slides, dtype=torch.int64, device=self.device),
                   torch.zeros(n_slides, dtype=torch.int64, device=self.device),
                   torch.zeros(n_slides, dtype=torch.int32, device=self.device))
        uq = float('nan') if not tile_uq else float(tile_uq)   # threshold.py:297 `if tile_uq:`
        self._check(self._lib.bq_slide_reduce(self._ctx, _ptr(mean2), _ptr(std2), _ptr(slide_idx), n,
                                              int(n_slides), uq, _ptr(acc[0]), _ptr(acc[1]), _ptr(acc[2]),
                                              self._stream()))
        return acc

    def slide_finish(self, acc):
        n_slides = acc[0].shape[0]
        mp = torch.empty(n_slides, dtype=torch.float64, device=self.device)
        mu = torch.empty(n_slides, dtype=torch.float64, device=self.device)
        self._check(self._lib.bq_slide_finish(self._ctx, _ptr(acc[0]), _ptr(acc[1]), _ptr(acc[2]),
                                              n_slides, _ptr(mp), _ptr(mu), self._stream()))
        return mp, mu, acc[2]

    def youden(self, y_true, y_score):
        """Youden threshold of the ROC curve of (y_true, y_score) on the device: the value the consumer gets
        from ``thresh[argmax(tpr - fpr)]`` over ``sklearn.metrics.roc_curve`` (``threshold.py:145-155,
        417-426``).  Arrays or tensors; labels must be 0/1 (or bool).  Raises ``ValueError`` when only one
        class is present, like the reference's ``max()`` over NaN rates.  Returns ``(threshold, info)``."""
        if torch.is_tensor(y_score):
            score = y_score.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            score = torch.from_numpy(np.ascontiguousarray(y_score, dtype=np.float64)).to(self.device)
        if torch.is_tensor(y_true):
            label = (y_true != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        else:
            yt = np.asarray(y_true)
            if yt.dtype != bool and not np.isin(yt, (0, 1)).all():
                raise ValueError('youden: labels must be 0/1')
            label = torch.from_numpy(np.ascontiguousarray(yt != 0).view(np.uint8)).to(self.device)
        n = int(score.numel())
        if n == 0 or label.numel() != n:
            raise ValueError('youden: empty input or length mismatch')
        ws = torch.empty(int(self._lib.bq_roc_workspace_bytes(n)), dtype=torch.uint8, device=self.device)
        out = torch.empty(6, dtype=torch.float64, device=self.device)
        self._check(self._lib.bq_roc_youden(self._ctx, _ptr(score), _ptr(label), n, _ptr(ws), ws.numel(), _ptr(out),
                                            self._stream()))
        o = out.cpu().numpy()
        if o[4] == 0 or o[5] == 0:
            raise ValueError('ROC undefined: only one class present')
        return float(o[0]), {'j': float(o[1]), 'tpr': float(o[2]), 'fpr': float(o[3]), 'n_pos': int(o[4]), 'n_neg': int(o[5])}

    # ------------------------------------------------------------------ UQ calibration (kernels_calib.hip)
    UQ_MAX_GRID = 1024

    def _uq_inputs(self, tool, x, correct, grid):
        """``(x float64 [n], correct uint8 [n])`` on this device from arrays or tensors, as ``youden`` takes them; ValueError for
        an empty input, a length mismatch, a non-finite ``x`` or a ``grid`` outside 2 .. 1024."""
        if torch.is_tensor(x):
            xd = x.to(device=self.device, dtype=torch.float64).contiguous().reshape(-1)
            finite = bool(torch.isfinite(xd).all())
        else:
            xh = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            finite = bool(np.isfinite(xh).all())
            xd = torch.from_numpy(xh).to(self.device)
        if torch.is_tensor(correct):
            cd = (correct != 0).to(device=self.device, dtype=torch.uint8).contiguous().reshape(-1)
        else:
            cd = torch.from_numpy(np.ascontiguousarray(np.asarray(correct) != 0).reshape(-1).view(np.uint8)).to(self.device)
        n = int(xd.numel())
        if n == 0 or cd.numel() != n or n >= 1 << 31:
            raise ValueError(f'{tool}: empty input, length mismatch or more than 2^31 - 1 rows')
        if not finite:
            raise ValueError(f'{tool}: uncertainty must be finite')
        if not 2 <= int(grid) <= self.UQ_MAX_GRID:
            raise ValueError(f'{tool}: grid must lie in 2 .. {self.UQ_MAX_GRID}, not {grid!r}')
        return xd, cd, n

    def uq_chunk_rows(self, n):
        """Rows of one chunk of the calibration sums over ``n`` rows (``bq_uq_chunk_rows``): the order of summation is fixed by it."""
        return int(self._lib.bq_uq_chunk_rows(int(n)))

    def uq_kde_scratch(self, n, grid=200):
        """Scratch for ``uq_kde`` over ``n`` rows (one buffer per launch that may be in flight)."""
        return self._bytes(self._lib.bq_uq_kde_workspace_bytes(int(n), int(grid)))

    def uq_loess_scratch(self, n, grid=200):
        """Scratch for ``uq_loess`` over ``n`` rows (one buffer per launch that may be in flight)."""
        return self._bytes(self._lib.bq_uq_loess_workspace_bytes(int(n), int(grid)))

    def uq_kde(self, x, correct, grid=200, cut=3.0, scratch=None):
        """Gaussian kernel density of the uncertainty ``x`` per group of ``correct`` over every row (``bq_uq_kde``): Scott's
        bandwidth, ``grid`` support points from ``min - cut bw`` to ``max + cut bw``.  Arrays or tensors.  -> host float64 arrays
        ``{'support' [2, grid], 'density' [2, grid], 'n' [2], 'min', 'max', 'mean', 'std', 'bw' [2], 'valid' bool [2]}``, index 0
        the incorrect and 1 the correct rows; the density integrates to 1 per group (``scipy.stats.gaussian_kde``); a group
        with fewer than two rows or no spread is not ``valid`` and its curve is NaN.  ValueError for a non-finite ``x``."""
        xd, cd, n = self._uq_inputs('uq_kde', x, correct, grid)
        grid, cut = int(grid), float(cut)
        if not 0.0 <= cut <= 1e6:
            raise ValueError(f'uq_kde: cut must lie in 0 .. 1e6, not {cut!r}')
        need = int(self._lib.bq_uq_kde_workspace_bytes(n, grid))
        scratch = self._scratch('uq', need, scratch)
        assert scratch.is_cuda and scratch.numel() >= need
        out = torch.empty(4 * grid + 16, dtype=torch.float64, device=self.device)
        self._check(self._lib.bq_uq_kde(self._ctx, _ptr(xd), _ptr(cd), n, grid, cut, _ptr(out), _ptr(scratch), scratch.numel(), self._stream()))
        o = out.cpu().numpy()
        st = o[4 * grid:].reshape(2, 8)
        return {'support': o[:2 * grid].reshape(2, grid).copy(), 'density': o[2 * grid:4 * grid].reshape(2, grid).copy(),
                'n': st[:, 0].astype(np.int64), 'min': st[:, 1].copy(), 'max': st[:, 2].copy(), 'mean': st[:, 3].copy(),
                'std': st[:, 4].copy(), 'bw': st[:, 5].copy(), 'valid': st[:, 6] != 0}

    def uq_loess(self, x, correct, grid=200, span=0.75, scratch=None):
        """Local quadratic regression of ``correct`` on the uncertainty ``x`` over every row, fitted at ``grid`` vertices from
        ``min x`` to ``max x`` (``bq_uq_loess``): window of ``floor(span n + 1e-5)`` rows, tricube weights.  Arrays or tensors.
        -> host float64 arrays ``{'vertex', 'fit', 'l2', 'lam', 'h'}`` [grid] and the scalars ``'nu'``, ``'rss'``,
        ``'degenerate'``, ``'q'``, ``'n'``; a degenerate vertex has NaN ``fit``, ``l2`` and ``lam``.  ValueError for a non-finite
        ``x`` or a span whose window holds no row or more than all of them."""
        xd, cd, n = self._uq_inputs('uq_loess', x, correct, grid)
        grid, span = int(grid), float(span)
        q = int(np.floor(span * n + 1e-5)) if span > 0 else 0
        if not 1 <= q <= n:
            raise ValueError(f'uq_loess: the window of span {span!r} over {n} rows holds {q} rows; it must hold 1 .. {n}')
        need = int(self._lib.bq_uq_loess_workspace_bytes(n, grid))
        scratch = self._scratch('uq', need, scratch)
        assert scratch.is_cuda and scratch.numel() >= need
        out = torch.empty(5 * grid + 4, dtype=torch.float64, device=self.device)
        self._check(self._lib.bq_uq_loess(self._ctx, _ptr(xd), _ptr(cd), n, grid, span, _ptr(out), _ptr(scratch), scratch.numel(), self._stream()))
        o = out.cpu().numpy()
        res = {k: o[i * grid:(i + 1) * grid].copy() for i, k in enumerate(('vertex', 'fit', 'l2', 'lam', 'h'))}
        res.update(nu=float(o[5 * grid]), rss=float(o[5 * grid + 1]), degenerate=int(o[5 * grid + 2]), q=int(o[5 * grid + 3]), n=n)
        return res

    # ------------------------------------------------------------------ prediction metrics (kernels_delong.hip)
    DELONG_MAX_K, DELONG_MAX_ROWS = 8, 1 << 25

    def delong_scratch(self, k, n):
        """Scratch for ``delong`` over ``k`` classifiers and ``n`` rows (one buffer per launch that may be in flight)."""
        return self._bytes(self._lib.bq_delong_workspace_bytes(int(k), int(n)))

    def delong_chunk_rows(self, n):
        """Rows of one chunk of the covariance sums over ``n`` rows (``bq_delong_chunk_rows``): the order of summation is fixed by it."""
        return int(self._lib.bq_delong_chunk_rows(int(n)))

    def delong(self, y_true, scores, components=False, scratch=None):
        """AUROC and DeLong's covariance of ``k`` classifiers on the same ``n`` rows (``bq_delong``).  ``y_true`` [n]: 0/1 or bool;
        ``scores`` [k, n] or [n] (k = 1), float64; arrays or tensors.  -> host arrays ``{'auc' [k], 'cov' [k, k], 'n_pos', 'n_neg'}``
        and, with ``components``, ``'V' [k, n]``: the structural component of every row, in row order.  ValueError, with nothing
        launched, for a NaN score, labels other than 0/1, one class only, k outside 1 .. 8, n above 2^25 or a shape mismatch."""
        if torch.is_tensor(scores):
            sd = scores.to(device=self.device, dtype=torch.float64).contiguous()
            nan = bool(torch.isnan(sd).any())
        else:
            sh = np.ascontiguousarray(scores, dtype=np.float64)
            nan = bool(np.isnan(sh).any())
            sd = torch.from_numpy(sh).to(self.device)
        if sd.dim() == 1:
            sd = sd.reshape(1, -1)
        if torch.is_tensor(y_true):
            binary = y_true.dtype == torch.bool or bool(((y_true == 0) | (y_true == 1)).all())
            ld = (y_true != 0).to(device=self.device, dtype=torch.uint8).contiguous().reshape(-1)
        else:
            yt = np.asarray(y_true)
            binary = yt.dtype == bool or bool(np.isin(yt, (0, 1)).all())
            ld = torch.from_numpy(np.ascontiguousarray(yt != 0).reshape(-1).view(np.uint8)).to(self.device)
        if sd.dim() != 2 or not 1 <= sd.shape[0] <= self.DELONG_MAX_K:
            raise ValueError(f'delong: scores are [k, n] with 1 <= k <= {self.DELONG_MAX_K}, not {tuple(sd.shape)}')
        k, n = int(sd.shape[0]), int(sd.shape[1])
        if n == 0 or ld.numel() != n or n > self.DELONG_MAX_ROWS:
            raise ValueError(f'delong: empty input, length mismatch or more than 2^25 rows ({n} scores, {ld.numel()} labels)')
        if nan:
            raise ValueError('delong: a score is NaN')
        if not binary:
            raise ValueError('delong: labels must be 0/1')
        m = int(ld.sum())
        if m == 0 or m == n:
            raise ValueError('delong: only one class present')
        need = int(self._lib.bq_delong_workspace_bytes(k, n))
        scratch = self._scratch('delong', need, scratch)
        assert scratch.is_cuda and scratch.numel() >= need
        out = torch.empty(k + k * k + 2, dtype=torch.float64, device=self.device)
        V = torch.empty((k, n), dtype=torch.float64, device=self.device) if components else None
        self._check(self._lib.bq_delong(self._ctx, _ptr(sd), _ptr(ld), k, n, _ptr(scratch), scratch.numel(), _ptr(out),
                                        _ptr(V), self._stream()))
        o = out.cpu().numpy()
        res = {'auc': o[:k].copy(), 'cov': o[k:k + k * k].reshape(k, k).copy(), 'n_pos': int(o[k + k * k]), 'n_neg': int(o[k + k * k + 1])}
        if components:
            res['V'] = V.cpu().numpy()
        return res

    # ------------------------------------------------------------------ head training (kernels_train.hip)
    HEAD_PARAMS, HEAD_TRAIN_MAX_ROWS, HEAD_VALIDATE_MAX_ROWS = 3149826, 1024, 4096          # (train.py holds copies of these three)

    def train_scratch(self, n):
        """A caller's own scratch for ``head_grad`` / ``head_train_steps`` with batches of up to ``n`` rows (``scratch=``): uint8
        [``bq_head_train_workspace_bytes(n)``] on this device.  Calls that may overlap on different streams each bring one; without
        one the calls share the engine's cached ``train`` buffer."""
        return self._bytes(self._lib.bq_head_train_workspace_bytes(int(n)))

    def _train_state(self, *named):
        for name, t in named:
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == self.HEAD_PARAMS and t.is_contiguous()):
                raise ValueError(f'{name} must be contiguous float32 [{self.HEAD_PARAMS}]')
            self._on_device(name, t)

    def _train_batch(self, feats, rows, labels, count):
        """``feats`` float32 [N, 2048], ``rows`` int64 and ``labels`` uint8, ``count`` of each, all on this device; ValueError otherwise."""
        if not (torch.is_tensor(feats) and feats.dtype == torch.float32 and feats.dim() == 2 and feats.shape[1] == 2048 and
                feats.shape[0] >= 1 and feats.is_contiguous()):
            raise ValueError('feats must be contiguous float32 [N, 2048] with N >= 1')
        if not (torch.is_tensor(rows) and rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() == count):
            raise ValueError(f'rows must be contiguous int64 [{count}]')
        if not (torch.is_tensor(labels) and labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() == count):
            raise ValueError(f'labels must be contiguous uint8 [{count}]')
        for name, t in (('feats', feats), ('rows', rows), ('labels', labels)):
            self._on_device(name, t)

    def _head_open(self, family, need, rate, first, count, scratch, refusal, ok=True):
        """Where the preamble of the three head calls ends -> ``(rate, scratch)``: ``rate`` as a float (None: the engine's) and the
        scratch of ``family`` with at least ``need`` bytes (``scratch``: the caller's own); ValueError(``refusal``) unless the rate
        lies in [0, 1), the Philox passes ``first`` .. ``first + count - 1`` in 0 .. 2^32 - 1 and the call's own ``ok`` holds."""
        rate = float(self.hp.dropout if rate is None else rate)
        if not ok or not 0.0 <= rate < 1.0 or not 0 <= int(first) <= (1 << 32) - count:
            raise ValueError(refusal)
        scratch = self._scratch(family, int(need), scratch)
        assert scratch.is_cuda and scratch.is_contiguous()        # (too small: the library refuses, BQ_ERR_WORKSPACE)
        return rate, scratch

    def head_grad(self, params, feats, rows, labels, step, seed, rate=None, grad=None, scratch=None):
        """Gradient of the head's mean cross-entropy over the rows ``feats[rows]`` (``bq_head_grad``): ``params`` float32 [P] in the
        order of ``train.HEAD_TENSORS``, ``feats`` float32 [N, 2048], ``rows`` int64 [n] (also the Philox tile counters), ``labels``
        uint8 [n] in {0, 1}, 1 <= n <= 1024, all on this device; dropout ``rate`` (the engine's when None) with pass = ``step``.
        -> ``(grad [P], loss [1])`` on the device.  The engine's own weights play no part."""
        n = int(rows.numel()) if torch.is_tensor(rows) else -1
        if not 1 <= n <= self.HEAD_TRAIN_MAX_ROWS:
            raise ValueError(f'head_grad: 1 <= n <= {self.HEAD_TRAIN_MAX_ROWS} rows, as an int64 tensor')
        self._train_state(('params', params))
        self._train_batch(feats, rows, labels, n)
        if grad is None:
            grad = torch.empty(self.HEAD_PARAMS, dtype=torch.float32, device=self.device)
        self._train_state(('grad', grad))
        rate, scratch = self._head_open('train', self._lib.bq_head_train_workspace_bytes(n), rate, step, 1, scratch,
                                        'head_grad: the rate lies in [0, 1) and the step in 0 .. 2^32 - 1')
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_head_grad(self._ctx, _ptr(params), _ptr(feats), int(feats.shape[0]), _ptr(rows), _ptr(labels), n, int(step),
                                           int(seed), rate, _ptr(grad), _ptr(loss), _ptr(scratch), scratch.numel(), self._stream()))
        return grad, loss

    def validate_scratch(self, n):
        """A caller's own scratch for ``head_validate`` over up to ``n`` rows (``scratch=``): uint8
        [``bq_head_validate_workspace_bytes(n)``] on this device; without one the calls share the engine's cached ``validate`` buffer."""
        return self._bytes(self._lib.bq_head_validate_workspace_bytes(int(n)))

    def head_validate(self, params, feats, rows, labels, pass_, seed, rate=0.0, rowloss=False, hit=False, scratch=None):
        """The head ``params`` scored on the rows ``feats[rows]`` (``bq_head_validate``): the forward half of ``head_grad`` in the same
        arithmetic, 1 <= n <= 4096 rows.  ``rate`` 0 (the default, unlike ``head_grad``'s) is inference mode and draws no mask; a
        positive rate draws the training masks with pass = ``pass_``.  -> ``(stats, rowloss, hit)`` on the device: ``stats`` float64
        [2], the sum of the rows' losses and the number of rows whose larger logit is their label's (a tie goes to class 0);
        ``rowloss`` float64 [n] and ``hit`` uint8 [n] where asked for, else None.  A row that is not finite, lies outside ``feats``
        or has a label above 1 has a NaN loss and hit 0.  ``params`` is only read; nothing waits for the device."""
        n = int(rows.numel()) if torch.is_tensor(rows) else -1
        if not 1 <= n <= self.HEAD_VALIDATE_MAX_ROWS:
            raise ValueError(f'head_validate: 1 <= n <= {self.HEAD_VALIDATE_MAX_ROWS} rows, as an int64 tensor')
        self._train_state(('params', params))
        self._train_batch(feats, rows, labels, n)
        rate, scratch = self._head_open('validate', self._lib.bq_head_validate_workspace_bytes(n), float(rate), pass_, 1, scratch,
                                        'head_validate: the rate lies in [0, 1) and the pass in 0 .. 2^32 - 1')
        stats = torch.empty(2, dtype=torch.float64, device=self.device)
        loss = torch.empty(n, dtype=torch.float64, device=self.device) if rowloss else None
        hits = torch.empty(n, dtype=torch.uint8, device=self.device) if hit else None
        self._check(self._lib.bq_head_validate(self._ctx, _ptr(params), _ptr(feats), int(feats.shape[0]), _ptr(rows), _ptr(labels), n,
                                               int(pass_), int(seed), rate, _ptr(stats), _ptr(loss), _ptr(hits), _ptr(scratch),
                                               scratch.numel(), self._stream()))
        return stats, loss, hits

    def head_adam(self, params, m, v, grad, step, lr, b1=0.9, b2=0.999, eps=1e-7):
        """One Keras-Adam pass over the head's parameters in place (``bq_head_adam``), t = ``step`` + 1."""
        self._train_state(('params', params), ('m', m), ('v', v), ('grad', grad))
        if not 0 <= int(step) < 1 << 32:
            raise ValueError('head_adam: the step lies in 0 .. 2^32 - 1')
        self._check(self._lib.bq_head_adam(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), int(step), float(lr), float(b1), float(b2),
                                           float(eps), self._stream()))

    def head_train_steps(self, params, m, v, feats, rows, labels, batch, step0, seed, lr, rate=None, b1=0.9, b2=0.999, eps=1e-7,
                         grad=None, scratch=None):
        """``S`` = ceil(len(rows) / batch) steps of ``head_grad`` + ``head_adam`` back to back (``bq_head_train_steps``), step
        ``step0 + i`` over ``rows[i * batch:(i + 1) * batch]`` -- the last batch short when ``len(rows)`` is no multiple of ``batch``
        -- with the learning rate ``lr[i]`` (a sequence of ``S`` floats).  ``params``, ``m``, ``v`` change in place; -> losses
        float32 [S] on the device.  The same bits as the single calls."""
        count = int(rows.numel()) if torch.is_tensor(rows) else 0
        batch = int(batch)
        if not 1 <= batch <= self.HEAD_TRAIN_MAX_ROWS or count < 1:
            raise ValueError(f'head_train_steps: 1 <= batch <= {self.HEAD_TRAIN_MAX_ROWS} and at least one row')
        steps = -(-count // batch)
        last_n = count - (steps - 1) * batch
        self._train_state(('params', params), ('m', m), ('v', v))
        self._train_batch(feats, rows, labels, count)
        if grad is None:
            grad = torch.empty(self.HEAD_PARAMS, dtype=torch.float32, device=self.device)
        self._train_state(('grad', grad))
        lr = np.ascontiguousarray(lr, dtype=np.float64).reshape(-1)
        rate, scratch = self._head_open('train', self._lib.bq_head_train_workspace_bytes(batch), rate, step0, steps, scratch,
                                        f'head_train_steps: {steps} learning rates, a rate in [0, 1) and steps below 2^32', len(lr) == steps)
        losses = torch.empty(steps, dtype=torch.float32, device=self.device)
        self._check(self._lib.bq_head_train_steps(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), _ptr(feats), int(feats.shape[0]),
                                                  _ptr(rows), _ptr(labels), steps, batch, last_n, int(step0), int(seed), rate,
                                                  lr.ctypes.data_as(C.POINTER(C.c_double)), float(b1), float(b2), float(eps), _ptr(losses),
                                                  _ptr(scratch), scratch.numel(), self._stream()))
        return losses

    # ------------------------------------------------------------------ exit-flow fine-tuning (kernels_train.hip)
    EXIT_PARAMS, EXIT_BN_STATS, EXIT_MAX_ROWS, EXIT_ACT_SHAPE = 4748800, 7168, 256, (10, 10, 1024)   # (train.py holds copies)
    ALL_PARAMS = EXIT_PARAMS + HEAD_PARAMS

    def trunk(self, tiles_u8, packed=False):
        """uint8 NHWC tiles (device) -> ``block13_out`` float32 [n, 10, 10, 1024] at true scale (``bq_trunk_u8``): ``backbone_u8``'s
        launches up to the tensor block 14 reads, what ``train.cache_activations`` keeps per tile.  ``packed`` (a 16-bit engine's;
        ValueError on an f32 one): ``(acts16, mul)`` instead (``bq_trunk_u8_packed``) -- the tensor as the engine stores it, in the
        engine's own 16-bit type, and the power of two with ``acts16.float() * mul`` the unpacked result bit for bit."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        if packed and self.dtype == 'f32':
            raise ValueError('trunk(packed=True): an f32 engine stores block13_out in 32 bits, so a 16-bit copy would not be lossless')
        ws = self._ws_for(n, 1)
        out = torch.empty((n,) + self.EXIT_ACT_SHAPE, dtype=self._elt if packed else torch.float32, device=self.device)
        if packed:
            mul = C.c_float(0.0)
            self._check(self._lib.bq_trunk_u8_packed(self._ctx, _ptr(tiles_u8), n, _ptr(out), C.byref(mul), _ptr(ws), ws.numel(), self._stream()))
            return out, float(mul.value)
        self._check(self._lib.bq_trunk_u8(self._ctx, _ptr(tiles_u8), n, _ptr(out), _ptr(ws), ws.numel(), self._stream()))
        return out

    def exit_train_scratch(self, n, staged=None):
        """A caller's own scratch for ``exit_grad`` / ``exit_train_steps`` with batches of up to ``n`` rows (``scratch=``); without one
        the calls share the engine's cached ``exit_train`` buffer.  ``staged``: for a cache in pinned host memory of that torch dtype
        (the staging rows behind the rest; the family ``exit_train_staged``)."""
        return self._bytes(self._exit_need(True, int(n), staged))

    def exit_features_scratch(self, n, staged=None):
        """A caller's own scratch for ``exit_features`` over up to ``n`` rows; without one the calls share the cached ``exit_features``
        buffer (``staged``: as ``exit_train_scratch``'s; the family ``exit_features_staged``)."""
        return self._bytes(self._exit_need(False, int(n), staged))

    def exit_bn_scratch(self, n, staged=None):
        """``exit_train_scratch`` for the calls with ``bn='batch'`` [``bq_exit_bn_workspace_bytes``]; the families ``exit_bn`` and
        ``exit_bn_staged``."""
        return self._bytes(self._exit_bn_need(int(n), staged))

    def _exit_bn_need(self, n, staged):
        return int(self._lib.bq_exit_bn_workspace_bytes(n, self.ACT_TYPES[torch.float32 if staged is None else staged],
                                                        _lib.BQ_ACT_DEVICE if staged is None else _lib.BQ_ACT_HOST))

    def _bn_mode(self, call, bn, acts, cache):
        """``bn`` is 'frozen' or 'batch' -> whether 'batch', and the descriptor its calls take for every cache (a float32 device
        tensor's too).  The workspace of a 16-bit device cache is the float32 one's: the size does not depend on the type there."""
        if bn not in ('frozen', 'batch'):
            raise ValueError(f"{call}: bn is 'frozen' or 'batch', not {bn!r}")
        if bn == 'batch' and cache is None:
            cache = _lib.BqActCache(acts.data_ptr(), int(acts.shape[0]), _lib.BQ_DTYPE_F32, 1.0, _lib.BQ_ACT_DEVICE)
        return bn == 'batch', cache

    ACT_TYPES = {torch.float32: _lib.BQ_DTYPE_F32, torch.bfloat16: _lib.BQ_DTYPE_BF16, torch.float16: _lib.BQ_DTYPE_F16}

    def _exit_need(self, train, n, staged):
        """The bytes of an exit call's workspace over ``n`` rows; ``staged``: None, or the dtype of a cache in host memory."""
        if staged is None:
            return int((self._lib.bq_exit_train_workspace_bytes if train else self._lib.bq_exit_features_workspace_bytes)(n))
        return int((self._lib.bq_exit_staged_workspace_bytes if train else self._lib.bq_exit_features_staged_workspace_bytes)(n, self.ACT_TYPES[staged]))

    def _act_cache(self, call, acts, act_mul):
        """What an exit call reads ``acts`` as -> ``(descriptor, staged)``: ``descriptor`` None for a float32 device tensor -- the
        calls without a descriptor --, else the ``bq_act_cache`` of a 16-bit device tensor or of a pinned host tensor of any of the
        three types; ``staged`` None on the device, the dtype of a cache in host memory.  ValueError, before anything is launched, for
        another shape or type, a tensor that is not contiguous, a device tensor elsewhere, a host tensor that is not mapped pinned
        memory, a 16-bit cache in another type than the engine's own (only its own stored values are the float32 cache's exactly)
        and an ``act_mul`` that is not a positive finite power of two (1 for float32, which is read as it is)."""
        if not (torch.is_tensor(acts) and acts.dtype in self.ACT_TYPES and acts.dim() == 4 and tuple(acts.shape[1:]) == self.EXIT_ACT_SHAPE and
                acts.shape[0] >= 1 and acts.is_contiguous()):
            raise ValueError(f'{call}: acts must be contiguous float32, float16 or bfloat16 [N, 10, 10, 1024] with N >= 1')
        mul = float(act_mul)
        if not (mul > 0.0 and np.isfinite(mul) and np.frexp(mul)[0] == 0.5 and np.float32(mul) == mul and np.isfinite(np.float32(mul))):
            raise ValueError(f'{call}: act_mul must be a positive finite power of two, not {act_mul!r}')
        if acts.dtype == torch.float32 and mul != 1.0:
            raise ValueError(f'{call}: a float32 cache is read as it is: act_mul must be 1, not {act_mul!r}')
        if acts.dtype != torch.float32 and acts.dtype != self._elt:
            raise ValueError(f'{call}: a 16-bit cache must be in the engine\'s own type {self._elt} (only its stored values are the float32 '
                             f'cache\'s exactly), not {acts.dtype}')
        if acts.is_cuda:
            self._on_device('acts', acts)
            if acts.dtype == torch.float32:
                return None, None
            return _lib.BqActCache(acts.data_ptr(), int(acts.shape[0]), self.ACT_TYPES[acts.dtype], mul, _lib.BQ_ACT_DEVICE), None
        dev = C.c_void_p(0)
        if acts.device.type != 'cpu' or not acts.is_pinned() or self._lib.bq_host_device_pointer(C.c_void_p(acts.data_ptr()), C.byref(dev)) < 0 \
                or not dev.value:
            raise ValueError(f'{call}: acts in host memory must be pinned (torch.empty(..., pin_memory=True)): the gather kernel reads them '
                             'through the mapped device pointer')
        return _lib.BqActCache(dev.value, int(acts.shape[0]), self.ACT_TYPES[acts.dtype], mul, _lib.BQ_ACT_HOST), acts.dtype

    def _exit_vec(self, count, *named):
        for name, t in named:
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == count and t.is_contiguous()):
                raise ValueError(f'{name} must be contiguous float32 [{count}]')
            self._on_device(name, t)

    def _exit_batch(self, call, bn_stats, acts, rows, labels, count, act_mul=1.0):
        """``bn_stats`` float32 [7168], ``rows`` int64 and (unless None) ``labels`` uint8, ``count`` of each, all on this device, and
        ``acts`` [N, 10, 10, 1024] in a form ``_act_cache`` takes; ValueError otherwise -> ``_act_cache``'s pair."""
        if bn_stats is not None:                # (None: exit_grad in training mode, which does not read them)
            self._exit_vec(self.EXIT_BN_STATS, ('bn_stats', bn_stats))
        cache = self._act_cache(call, acts, act_mul)
        if not (torch.is_tensor(rows) and rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() == count):
            raise ValueError(f'{call}: rows must be contiguous int64 [{count}]')
        if labels is not None and not (torch.is_tensor(labels) and labels.dtype == torch.uint8 and labels.is_contiguous() and
                                       labels.numel() == count):
            raise ValueError(f'{call}: labels must be contiguous uint8 [{count}]')
        for name, t in (('rows', rows),) + ((('labels', labels),) if labels is not None else ()):
            self._on_device(name, t)
        return cache

    def exit_features(self, exit_params, bn_stats, acts, rows, out=None, scratch=None, act_mul=1.0):
        """Block 14 and the pool over the rows ``acts[rows]`` (``bq_exit_features``): ``exit_params`` float32 [P_EXIT] in the order of
        ``train.EXIT_TENSORS``, ``bn_stats`` float32 [7168] (``train.exit_bn_stats``), ``acts`` [N, 10, 10, 1024], ``rows`` int64
        [n], 1 <= n <= 256 -> float32 [n, 2048] on the device (``out``: written there).  A tile's row depends on the tile and the
        parameters only.  ``acts`` is float32 on this device, the engine's own 16-bit type on this device (``trunk(packed=True)``'s,
        with its ``mul`` as ``act_mul``: the values are ``acts.float() * act_mul`` and the result has the float32 cache's bits), or a
        pinned host tensor of either form (``bq_exit_features_c``: the rows are gathered into the scratch first)."""
        n = int(rows.numel()) if torch.is_tensor(rows) else -1
        if not 1 <= n <= self.EXIT_MAX_ROWS:
            raise ValueError(f'exit_features: 1 <= n <= {self.EXIT_MAX_ROWS} rows, as an int64 tensor')
        self._exit_vec(self.EXIT_PARAMS, ('exit_params', exit_params))
        cache, staged = self._exit_batch('exit_features', bn_stats, acts, rows, None, n, act_mul)
        if out is None:
            out = torch.empty((n, 2048), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, 2048)
        scratch = self._scratch('exit_features' if staged is None else 'exit_features_staged', self._exit_need(False, n, staged), scratch)
        assert scratch.is_cuda and scratch.is_contiguous()
        if cache is None:
            self._check(self._lib.bq_exit_features(self._ctx, _ptr(exit_params), _ptr(bn_stats), _ptr(acts), int(acts.shape[0]), _ptr(rows), n,
                                                   _ptr(out), _ptr(scratch), scratch.numel(), self._stream()))
        else:
            self._check(self._lib.bq_exit_features_c(self._ctx, _ptr(exit_params), _ptr(bn_stats), C.byref(cache), _ptr(rows), n, _ptr(out),
                                                     _ptr(scratch), scratch.numel(), self._stream()))
        return out

    def exit_features_all(self, exit_params, bn_stats, acts, rows, act_mul=1.0):
        """``exit_features`` over any number of rows, in calls of up to 256 -> float32 [len(rows), 2048]."""
        out = torch.empty((int(rows.numel()), 2048), dtype=torch.float32, device=self.device)
        for a in range(0, int(rows.numel()), self.EXIT_MAX_ROWS):
            self.exit_features(exit_params, bn_stats, acts, rows[a:a + self.EXIT_MAX_ROWS].contiguous(), out=out[a:a + self.EXIT_MAX_ROWS],
                               act_mul=act_mul)
        return out

    def exit_grad(self, params, bn_stats, acts, rows, labels, step, seed, rate=None, grad=None, scratch=None, act_mul=1.0, bn='frozen'):
        """Gradient of the mean cross-entropy over the rows ``acts[rows]`` through block 14 and the head (``bq_exit_grad``): ``params``
        float32 [P_ALL] -- the exit vector, then the head's --, ``labels`` uint8 [n] in {0, 1}, 1 <= n <= 256; dropout ``rate`` (the
        engine's when None) with pass = ``step`` and the rows as Philox tile counters.  -> ``(grad [P_ALL], loss [1])`` on the device.
        ``acts``, ``act_mul``: as ``exit_features``'.

        ``bn='batch'`` (``bq_exit_grad_bn``): training-mode batch norm -- each layer normalised by the batch's own mean and biased
        variance over its 100 n rows, the gradient through them -- -> ``(grad, loss, batch_stats [7168])``: mu1 | var1 | mu2 | var2 as
        used.  ``bn_stats`` is then neither read nor written and may be None (``exit_bn_move`` is the moving statistics' update)."""
        n = int(rows.numel()) if torch.is_tensor(rows) else -1
        if not 1 <= n <= self.EXIT_MAX_ROWS:
            raise ValueError(f'exit_grad: 1 <= n <= {self.EXIT_MAX_ROWS} rows, as an int64 tensor')
        self._exit_vec(self.ALL_PARAMS, ('params', params))
        if bn_stats is None and bn != 'batch':
            raise ValueError("exit_grad: bn_stats is None with bn='batch' only")
        cache, staged = self._exit_batch('exit_grad', bn_stats, acts, rows, labels, n, act_mul)
        batch_mode, cache = self._bn_mode('exit_grad', bn, acts, cache)
        if grad is None:
            grad = torch.empty(self.ALL_PARAMS, dtype=torch.float32, device=self.device)
        self._exit_vec(self.ALL_PARAMS, ('grad', grad))
        if batch_mode:
            rate, scratch = self._head_open('exit_bn' if staged is None else 'exit_bn_staged', self._exit_bn_need(n, staged), rate, step, 1,
                                            scratch, 'exit_grad: the rate lies in [0, 1) and the step in 0 .. 2^32 - 1')
            loss = torch.empty(1, dtype=torch.float32, device=self.device)
            batch_stats = torch.empty(self.EXIT_BN_STATS, dtype=torch.float32, device=self.device)
            self._check(self._lib.bq_exit_grad_bn(self._ctx, _ptr(params), C.byref(cache), _ptr(rows), _ptr(labels), n, int(step), int(seed),
                                                  rate, _ptr(grad), _ptr(loss), _ptr(batch_stats), _ptr(scratch), scratch.numel(),
                                                  self._stream()))
            return grad, loss, batch_stats
        rate, scratch = self._head_open('exit_train' if staged is None else 'exit_train_staged', self._exit_need(True, n, staged), rate, step, 1,
                                        scratch, 'exit_grad: the rate lies in [0, 1) and the step in 0 .. 2^32 - 1')
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        if cache is None:
            self._check(self._lib.bq_exit_grad(self._ctx, _ptr(params), _ptr(bn_stats), _ptr(acts), int(acts.shape[0]), _ptr(rows), _ptr(labels),
                                               n, int(step), int(seed), rate, _ptr(grad), _ptr(loss), _ptr(scratch), scratch.numel(),
                                               self._stream()))
        else:
            self._check(self._lib.bq_exit_grad_c(self._ctx, _ptr(params), _ptr(bn_stats), C.byref(cache), _ptr(rows), _ptr(labels), n, int(step),
                                                 int(seed), rate, _ptr(grad), _ptr(loss), _ptr(scratch), scratch.numel(), self._stream()))
        return grad, loss

    def adam_n(self, params, m, v, grad, step, lr, b1=0.9, b2=0.999, eps=1e-7):
        """One Keras-Adam pass in place over float32 vectors of any one length (``bq_adam_n``: ``head_adam``'s kernel), t = ``step`` + 1."""
        count = int(params.numel()) if torch.is_tensor(params) else 0
        if count < 1:
            raise ValueError('adam_n: at least one parameter')
        self._exit_vec(count, ('params', params), ('m', m), ('v', v), ('grad', grad))
        if not 0 <= int(step) < 1 << 32:
            raise ValueError('adam_n: the step lies in 0 .. 2^32 - 1')
        self._check(self._lib.bq_adam_n(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), count, int(step), float(lr), float(b1),
                                        float(b2), float(eps), self._stream()))

    def exit_bn_move(self, bn_stats, batch_stats, n):
        """The moving statistics ``bn_stats`` [7168] in place after a training-mode step over ``n`` tiles whose batch statistics were
        ``batch_stats`` (``bq_exit_bn_move``): 0.99 moving + 0.01 batch, the variances with the batch's unbiased one, M = 100 n."""
        self._exit_vec(self.EXIT_BN_STATS, ('bn_stats', bn_stats), ('batch_stats', batch_stats))
        if not 1 <= int(n) <= self.EXIT_MAX_ROWS:
            raise ValueError(f'exit_bn_move: 1 <= n <= {self.EXIT_MAX_ROWS}')
        self._check(self._lib.bq_exit_bn_move(self._ctx, _ptr(bn_stats), _ptr(batch_stats), int(n), self._stream()))

    def exit_train_steps(self, params, m, v, bn_stats, acts, rows, labels, batch, step0, seed, lr, rate=None, b1=0.9, b2=0.999, eps=1e-7,
                         grad=None, scratch=None, act_mul=1.0, bn='frozen'):
        """``S`` = ceil(len(rows) / batch) steps of ``exit_grad`` + ``adam_n`` over [P_ALL] back to back (``bq_exit_train_steps``), as
        ``head_train_steps``: ``params``, ``m``, ``v`` change in place; -> losses float32 [S].  The same bits as the single calls.
        ``acts``, ``act_mul``: as ``exit_features``'; a cache in host memory is gathered once per step.

        ``bn='batch'`` (``bq_exit_train_steps_bn``): steps of ``exit_grad(..., bn='batch')`` + ``adam_n`` + ``exit_bn_move``;
        ``bn_stats`` changes in place as well."""
        count = int(rows.numel()) if torch.is_tensor(rows) else 0
        batch = int(batch)
        if not 1 <= batch <= self.EXIT_MAX_ROWS or count < 1:
            raise ValueError(f'exit_train_steps: 1 <= batch <= {self.EXIT_MAX_ROWS} and at least one row')
        steps = -(-count // batch)
        last_n = count - (steps - 1) * batch
        self._exit_vec(self.ALL_PARAMS, ('params', params), ('m', m), ('v', v))
        cache, staged = self._exit_batch('exit_train_steps', bn_stats, acts, rows, labels, count, act_mul)
        batch_mode, cache = self._bn_mode('exit_train_steps', bn, acts, cache)
        if grad is None:
            grad = torch.empty(self.ALL_PARAMS, dtype=torch.float32, device=self.device)
        self._exit_vec(self.ALL_PARAMS, ('grad', grad))
        lr = np.ascontiguousarray(lr, dtype=np.float64).reshape(-1)
        family, need = ('exit_bn', self._exit_bn_need(batch, staged)) if batch_mode else ('exit_train', self._exit_need(True, batch, staged))
        rate, scratch = self._head_open(family if staged is None else family + '_staged', need, rate, step0,
                                        steps, scratch, f'exit_train_steps: {steps} learning rates, a rate in [0, 1) and steps below 2^32',
                                        len(lr) == steps)
        losses = torch.empty(steps, dtype=torch.float32, device=self.device)
        tail = (steps, batch, last_n, int(step0), int(seed), rate, lr.ctypes.data_as(C.POINTER(C.c_double)), float(b1), float(b2), float(eps),
                _ptr(losses), _ptr(scratch), scratch.numel(), self._stream())
        if batch_mode:
            self._check(self._lib.bq_exit_train_steps_bn(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), _ptr(bn_stats), C.byref(cache),
                                                         _ptr(rows), _ptr(labels), *tail))
        elif cache is None:
            self._check(self._lib.bq_exit_train_steps(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), _ptr(bn_stats), _ptr(acts),
                                                      int(acts.shape[0]), _ptr(rows), _ptr(labels), *tail))
        else:
            self._check(self._lib.bq_exit_train_steps_c(self._ctx, _ptr(params), _ptr(m), _ptr(v), _ptr(grad), _ptr(bn_stats), C.byref(cache),
                                                        _ptr(rows), _ptr(labels), *tail))
        return losses

    def exit_validate(self, params, bn_stats, acts, rows, labels, pass_, seed, rowloss=False, hit=False, act_mul=1.0):
        """``params`` [P_ALL] scored on the rows ``acts[rows]`` in inference mode: ``exit_features`` into scratch, then ``head_validate``
        at rate 0 on those features with ``rows = arange(n)``, 1 <= n <= 256 -> ``head_validate``'s ``(stats, rowloss, hit)``.
        ``acts``, ``act_mul``: as ``exit_features``'."""
        n = int(rows.numel()) if torch.is_tensor(rows) else -1
        if not 1 <= n <= self.EXIT_MAX_ROWS:
            raise ValueError(f'exit_validate: 1 <= n <= {self.EXIT_MAX_ROWS} rows, as an int64 tensor')
        self._exit_vec(self.ALL_PARAMS, ('params', params))
        feats = self._scratch('exit_validate', n * 2048 * 4).view(torch.float32)[:n * 2048].view(n, 2048)
        self.exit_features(params[:self.EXIT_PARAMS], bn_stats, acts, rows, out=feats, act_mul=act_mul)
        at = self._table('exit_validate', n, lambda: np.arange(n, dtype=np.int64))
        return self.head_validate(params[self.EXIT_PARAMS:], feats, at, labels, pass_, seed, rate=0.0, rowloss=rowloss, hit=hit)

    def debug_activation(self, name, staged, shape_hwc, true_scale=True):
        """The named activation as fp32 [n,H,W,C]; with activation exponents (``act_exp``) the stored tensor times 2^k, i.e. the
        network's values, unless ``true_scale=False``."""
        return self._debug_tap(self._lib.bq_debug_activation, name, staged, shape_hwc, true_scale)

    def debug_activation_u8(self, name, tiles_u8, shape_hwc, true_scale=True):
        """The same tap on the path ``mc_infer`` takes in a 16-bit context: uint8 tiles [n,299,299,3] through the fused front
        kernel (standardise + block1_conv1 + block1_conv2 in one launch), then the network up to ``name``."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        return self._debug_tap(self._lib.bq_debug_activation_u8, name, tiles_u8, shape_hwc, true_scale)

    def _debug_tap(self, entry, name, src, shape_hwc, true_scale):
        n = src.shape[0]
        ws = self._ws_for(n, 1)
        h, w, c = shape_hwc
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=self.device)
        rc = entry(self._ctx, name.encode(), _ptr(src), n, _ptr(ws), ws.numel(), _ptr(out), out.numel(), self._stream())
        self._check(rc)
        assert rc == out.numel(), (rc, out.numel())
        k = self._tap_exp.get(name, 0)
        return out * float(2.0 ** k) if (k and true_scale) else out

    def schedule(self, n, u8=True, tap=None):
        """The launch schedule of a batch of ``n`` tiles as ``[(layer or block output, route)]`` (``bq_describe_schedule``): which
        kernel family runs each matrix layer from uint8 tiles (``mc_infer`` / ``backbone_u8``; ``u8=False``: from staged tiles,
        ``backbone``), up to the debug tap ``tap`` if one is named.  Decided by the code that launches; launches nothing."""
        buf = C.create_string_buffer(8192)
        self._check(self._lib.bq_describe_schedule(self._ctx, int(n), 1 if u8 else 0, tap.encode() if tap else None, buf, len(buf)))
        return [tuple(line.split(' ', 1)) for line in buf.value.decode().splitlines()]

    # layers whose outputs the 16-bit storage can clip: the largest activations of Xception sit behind the un-normalised sums
    # of the residual stream and in front of the pooled features
    HEADROOM_TAPS = (('block1_conv2', (147, 147, 64)), ('block2_out', (74, 74, 128)), ('block4_out', (19, 19, 728)),
                     ('block8_out', (19, 19, 728)), ('block12_out', (19, 19, 728)), ('block13_out', (10, 10, 1024)),
                     ('block14_sepconv1', (10, 10, 1536)), ('block14_sepconv2', (10, 10, 2048)))

    def f16_headroom(self, tiles_u8, limit=65504.0):
        """Saturation indicator for the f16 storage type (round-3 advisory): every f16 kernel runs with MODE.FP16_OVFL, so
        an activation beyond +-65504 is clamped SILENTLY -- harmless on the synthetic weights (peak 10-22), but a trained
        checkpoint with a saturating layer would give plausible, wrong predictions.  Runs up to eight of ``tiles_u8``
        through tapped layers and returns ``{'max_abs': {layer: value}, 'saturated': {layer: count}, 'headroom': min over
        layers of limit / max_abs}``; a caller loading real weights should call it once (the CLI does, on its first tiles)
        and fall back to bf16 or fp32 if anything saturates.  Meaningless (inf headroom) for the other storage types."""
        out = {'max_abs': {}, 'saturated': {}, 'headroom': float('inf'), 'dtype': self.dtype}
        for name, a in self._headroom_taps(tiles_u8):
            m = float(a.max())
            out['max_abs'][name] = m
            out['saturated'][name] = int((a >= limit).sum())
            out['headroom'] = min(out['headroom'], limit / max(m, 1e-30))
        return out

    def _headroom_taps(self, tiles_u8):
        """The tap loop of both monitors: (layer, |activation| as stored -- what the range limit applies to) for every one of
        ``HEADROOM_TAPS`` on up to eight of ``tiles_u8``; nothing for the other storage types or without tiles."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda
        t = tiles_u8[:min(8, tiles_u8.shape[0], self.max_batch)].contiguous()
        if self.dtype == 'f16' and t.shape[0] > 0:
            for name, shp in self.HEADROOM_TAPS:
                yield name, self.debug_activation_u8(name, t, shp, true_scale=False).abs_()

    def f16_headroom_async(self, tiles_u8, limit=65504.0):
        """``f16_headroom`` without a host synchronisation, for a monitor inside a running loop (``inference.evaluate``'s
        ``headroom_every``): the eight taps on up to eight of ``tiles_u8``, everything enqueued on the current stream; returns a
        device tensor float32 [8, 2] -- per tap (max |activation| as stored, number of values at the clamp) -- that the caller
        copies out and looks at later.  None for the other storage types."""
        rows = [torch.stack([a.max(), (a >= limit).sum().to(torch.float32)]) for _, a in self._headroom_taps(tiles_u8)]
        return torch.stack(rows) if rows else None

    def range_key(self, tiles_u8):
        """The range screen's key of every tile (``bq_range_key``): uint8 NHWC [n,299,299,3] (device, any byte offset) -> float32
        [n] on the device, the largest |value| per-image standardisation gives the tile, max(hi - mu, mu - lo) / max(sd, 1/sqrt(N))
        from its exact byte sums in float64."""
        assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_cuda and tiles_u8.is_contiguous()
        n = tiles_u8.shape[0]
        key = torch.empty(n, dtype=torch.float32, device=self.device)
        ws = torch.empty(self._lib.bq_range_ws_bytes(n), dtype=torch.uint8, device=self.device)
        self._check(self._lib.bq_range_key(self._ctx, _ptr(tiles_u8), n, _ptr(key), _ptr(ws), ws.numel(), self._stream()))
        return key

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on=True):
        self._check(self._lib.bq_profile_enable(self._ctx, 1 if on else 0))

    def profile_read(self):
        arr = (_lib.BqProfEntry * _lib.BQ_PROF_MAX)()
        k = self._check(self._lib.bq_profile_read(self._ctx, arr, _lib.BQ_PROF_MAX))
        return [ProfileEntry(arr[i].name.decode(), arr[i].launches, arr[i].ms, arr[i].flops,
                             arr[i].bytes) for i in range(k)]


class RangeScreen:
    """The f16 range screen of one engine (``bq_range_screen``): ``k`` candidate slots on the engine's device
    that keep the tiles with the largest ``Engine.range_key`` seen since the last ``reset()`` -- key, global tile index and the
    tile's bytes -- ranked by (key desc, global index asc).  ``update`` enqueues on the current stream and never synchronises; the
    number of filled slots is known on the host (min(k, tiles since the reset)), so ``tiles`` is a view without a device read.
    ``screened`` counts the tiles that went through the key."""

    MAX_BATCH = 2048

    def __init__(self, engine, k=8, max_batch=None):
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError(f'k must lie in [1, 64], not {k}')
        max_batch = int(engine.max_batch if max_batch is None else max_batch)
        if not 1 <= max_batch <= self.MAX_BATCH:
            raise ValueError(f'max_batch must lie in [1, {self.MAX_BATCH}], not {max_batch}')
        self.engine, self.k, self.max_batch = engine, k, max_batch
        dev = engine.device
        self.key = torch.empty(k, dtype=torch.float32, device=dev)
        self.idx = torch.empty(k, dtype=torch.int64, device=dev)
        self.slots = torch.empty((k, TILE_PX, TILE_PX, 3), dtype=torch.uint8, device=dev)
        self._ws = torch.empty(engine._lib.bq_range_ws_bytes(max_batch), dtype=torch.uint8, device=dev)
        self.filled = 0
        self.screened = 0

    def update(self, tiles, tile_idx0=0, tile_idx=None):
        """Merge a batch (uint8 [n,299,299,3], device) into the slots; its global tile indices are ``tile_idx0 + row``, or
        ``tile_idx`` (int64 [n], device) when given -- ``Engine.mc_infer``'s convention."""
        assert tiles.dtype == torch.uint8 and tiles.is_cuda and tiles.is_contiguous() and tuple(tiles.shape[1:]) == (TILE_PX, TILE_PX, 3)
        n = int(tiles.shape[0])
        if n > self.max_batch:
            raise ValueError(f'batch of {n} tiles exceeds the screen\'s max_batch {self.max_batch}')
        if tile_idx is not None:
            assert tile_idx.dtype == torch.int64 and tile_idx.is_cuda and tile_idx.is_contiguous() and tile_idx.numel() == n
        if n == 0:
            return
        eng = self.engine
        eng._check(eng._lib.bq_range_screen(eng._ctx, _ptr(tiles), n, int(tile_idx0), _ptr(tile_idx), _ptr(self.key), _ptr(self.idx),
                                            _ptr(self.slots), self.k, self.filled, _ptr(self._ws), self._ws.numel(), eng._stream()))
        self.filled = min(self.k, self.filled + n)
        self.screened += n

    def reset(self):
        """Start a new interval: the slots count as empty (nothing is launched; the next update overwrites them in stream order)."""
        self.filled = 0

    @property
    def tiles(self):
        """The filled slots, uint8 [m,299,299,3] (a view)."""
        return self.slots[:self.filled]

    def candidates(self):
        """(key float32 [m], global tile index int64 [m]) of the filled slots: device views, in slot order."""
        return self.key[:self.filled], self.idx[:self.filled]


class EnginePool:
    """Round-robin pool of independent contexts, each on its own HIP stream, so consecutive batches are in
    flight together; by default every stream owns a disjoint group of XCDs (see __init__ and DESIGN.md).
    Every context owns its weights copy and workspace; results are independent of the stream used."""

    def __init__(self, weights, n_streams=2, cu_split='contig', size_grids=False, reserve_cus=0, decode_streams=2, **kw):
        self.engines = [Engine(weights, **kw) for _ in range(max(1, int(n_streams)))]
        self.size_grids = bool(size_grids)      # persistent grids sized for the CUs of each stream's mask (Engine.set_num_cus)
        # reserve_cus: the LAST compute units of the chip are kept out of every inference stream's mask (and the persistent grids
        # are sized for what is left) and handed to `decode_streams` streams of their own: the device inflate's waves run for
        # ~100 ms each and must not sit on CUs the persistent inference kernels want (inference.evaluate, gpu_decode)
        self.reserve_cus = int(reserve_cus)
        self._n_decode_streams = int(decode_streams)
        self.decode_streams = []
        dev = self.engines[0].device
        # Two streams own disjoint halves of the chip (hipExtStreamCreateWithCUMask; mask bits 0..127 and
        # 128..255 = XCDs 0-3 and 4-7, each with its own L2s): two batches in flight then run side by side
        # out of phase -- one's HBM-bound prologues/epilogues under the other's compute -- instead of
        # interleaving workgroups on every CU.  Measured at batch 256: 12.6-12.8 ms per batch vs 13.0 on one
        # stream and a bimodal 12.8 / 15.3 with two unmasked streams.  cu_split: 'contig' (default),
        # 'xcd', 'interleave' (experiments) or None / 'none' for plain streams.
        split = None if cu_split in (None, '', 'none', '0') else cu_split
        self.device = dev
        self.hp = self.engines[0].hp
        self.cu_split = split
        self._sets = {}                 # batches in flight -> list of streams
        self.active = len(self.engines)
        self.streams = self._stream_set(self.active)
        self._apply_grid_size(self.active)

    def _stream_set(self, n):
        """n streams: CU-masked (each owns 1/n of the chip's XCDs) when n >= 2 and masks are available,
        one plain whole-chip stream for n = 1."""
        if n in self._sets:
            return self._sets[n]
        dev = self.device
        streams = None
        if (n >= 2 or self.reserve_cus) and self.cu_split:
            try:
                streams = self._masked_streams(self.cu_split, dev, n)
            except BiscuitHipError as e:       # scheduling aid only: plain streams compute the same results
                import warnings
                warnings.warn(f'CU-masked streams unavailable ({e}); using plain HIP streams')
                self.cu_split = None
        masked = streams is not None
        if streams is None:
            streams = [torch.cuda.Stream(device=dev) for _ in range(n)]
        self._sets[n] = streams
        self._masked = getattr(self, '_masked', {})
        self._masked[n] = masked
        return streams

    def _apply_grid_size(self, n):
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count - self.reserve_cus
        sized = self.size_grids or self.reserve_cus > 0
        for k, eng in enumerate(self.engines):
            eng.set_num_cus(ncu // n if (sized and k < n and self._masked.get(n)) else 0)

    def set_in_flight(self, n):
        """Use the first n contexts, each on its own share of the chip (n = 1: one whole-chip stream).
        Results do not depend on n."""
        n = max(1, min(int(n), len(self.engines)))
        self.synchronize()
        self.active = n
        self.streams = self._stream_set(n)
        self._apply_grid_size(n)

    def _masked_streams(self, split, dev, nst):
        streams = []
        ncu_all = torch.cuda.get_device_properties(dev).multi_processor_count
        ncu = ncu_all - self.reserve_cus
        if self.reserve_cus and not self.decode_streams:
            if not 8 <= self.reserve_cus <= ncu_all // 2:
                raise BiscuitHipError(f'reserve_cus must lie in [8, {ncu_all // 2}]')
            self.decode_streams = [_mask_stream(self.engines[0], range(ncu, ncu_all), ncu_all) for _ in range(max(1, self._n_decode_streams))]
        for k in range(nst):
            if split == 'contig':
                mine = [cu for cu in range(ncu) if cu * nst // ncu == k]
            elif split == 'xcd':              # bit i -> XCD i % 8 (experiment)
                mine = [cu for cu in range(ncu) if (cu % 8) * nst // 8 == k]
            else:
                mine = [cu for cu in range(ncu) if cu % nst == k]
            streams.append(_mask_stream(self.engines[k], mine, ncu_all))
        return streams

    def close(self):
        """Destroy the CU-masked streams this pool created (plain torch streams are torch's)."""
        self.synchronize()
        for n, streams in list(self._sets.items()):
            for k, st in enumerate(streams):
                if isinstance(st, torch.cuda.ExternalStream):
                    self.engines[k]._lib.bq_stream_destroy(self.engines[k]._ctx, C.c_void_p(st.cuda_stream))
            del self._sets[n]
        for st in self.decode_streams:
            st.synchronize()
            self.engines[0]._lib.bq_stream_destroy(self.engines[0]._ctx, C.c_void_p(st.cuda_stream))
        self.decode_streams = []
        self.streams = []

    def __len__(self):
        return self.active

    def run(self, i, fn, wait_for_current=False):
        """Call fn(engine) with stream i % n current.  wait_for_current: first make that stream
        wait for work already enqueued on the caller's stream (inputs prepared there)."""
        k = i % self.active
        if wait_for_current:
            self.streams[k].wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.streams[k]):
            return fn(self.engines[k])

    def synchronize(self):
        for st in self.streams:
            st.synchronize()


def _mask_stream(eng, cus, ncu):
    """A HIP stream restricted to the compute units in ``cus`` (bq_stream_create_masked)."""
    bits = [0] * ((ncu + 31) // 32)
    for cu in cus:
        bits[cu // 32] |= 1 << (cu % 32)
    arr = (C.c_uint32 * len(bits))(*bits)
    h = C.c_void_p()
    eng._check(eng._lib.bq_stream_create_masked(eng._ctx, arr, len(bits), C.byref(h)))
    return torch.cuda.ExternalStream(h.value, device=eng.device)


class UncertaintyInterface:
    """Mirror of ``sf.model.tensorflow.UncertaintyInterface`` as the reference uses it
    (``results.py:234,250-260``): called with a batch of *standardised* float32 NHWC
    tiles, returns ``(mean, uncertainty)`` each ``[B, 2]``; ``uncertainty[0][0]`` is what
    ``results.py:258`` compares with the tile-UQ threshold."""

    def __init__(self, engine: Engine, uq_n=30, seed=0, norm_fit=None, normalizer='reinhard_fast'):
        from .stain import make_normalizer
        self.engine, self.uq_n, self.seed = engine, int(uq_n), int(seed)
        self._calls = 0
        # results.py:251-252: `if interface.wsi_normalizer: norm_image = ...rgb_to_rgb(image)`
        self.wsi_normalizer = make_normalizer(engine, normalizer, norm_fit)

    def enable_graph(self):
        """Capture the one-tile call (stage -> ~60 backbone launches -> MC head) in a HIP graph: the heatmap loop of
        results.py:250-258 calls the interface once per tile, and at B = 1 every kernel is a few microseconds long, so
        the launch sequence itself is what a call costs.  The Philox tile counter stays the call index: it is read from
        device memory by the head kernels (``Engine.set_tile_index_ptr``), results are bit-identical to the eager path."""
        eng = self.engine
        self._gx = torch.zeros((1, TILE_PX, TILE_PX, 3), dtype=torch.float32, device=eng.device)
        self._gidx = torch.zeros(1, dtype=torch.int64, device=eng.device)
        eng._ws_for(1, self.uq_n)                               # the workspace must exist before capture

        def body():
            feat = eng.backbone(eng.stage_f32(self._gx))
            return eng.mc_head(feat, self.uq_n, self.seed, tile_idx0=0)
        side = torch.cuda.Stream(device=eng.device)
        side.wait_stream(torch.cuda.current_stream(eng.device))
        eng.set_tile_index_ptr(self._gidx)
        try:
            with torch.cuda.stream(side):
                for _ in range(2):                              # warm-up: kernel attributes, allocator
                    body()
            torch.cuda.current_stream(eng.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._gmean, self._gstd = body()
        finally:
            eng.set_tile_index_ptr(None)
        self._graph = graph

    def device_call(self, x):
        """The same call with everything left on the device: x float32 [B,299,299,3] on the engine's GPU ->
        (mean, std) device tensors, nothing synchronises."""
        eng = self.engine
        if x.ndim != 4 or tuple(x.shape[1:]) != (TILE_PX, TILE_PX, 3):
            raise ValueError(f'expected [B,{TILE_PX},{TILE_PX},3] standardised tiles, got {tuple(x.shape)}')
        if getattr(self, '_graph', None) is not None and x.shape[0] == 1:
            self._gx.copy_(x)
            self._gidx.fill_(self._calls)
            self._graph.replay()
            self._calls += 1
            return self._gmean.clone(), self._gstd.clone()
        feat = eng.backbone(eng.stage_f32(x))
        mean, std = eng.mc_head(feat, self.uq_n, self.seed, tile_idx0=self._calls)
        self._calls += x.shape[0]
        return mean, std

    def __call__(self, batch):
        eng = self.engine
        x = torch.as_tensor(np.asarray(batch) if not torch.is_tensor(batch) else batch)
        x = x.to(device=eng.device, dtype=torch.float32).contiguous()
        mean, std = self.device_call(x)
        return mean.cpu().numpy(), std.cpu().numpy()
