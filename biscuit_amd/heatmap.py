"""Whole-slide UQ heatmap front-end (reference: results.py:216-265).

The reference builds ``sf.Heatmap(slide, model, stride_div=1)`` and masks it with the tile-level
uncertainty threshold (results.py:217-227), then walks the slide's tile grid through
``UncertaintyInterface`` and sorts the tiles into ``uq_incl`` / ``uq_excl`` (results.py:234-265).
This front-end takes the tiles of a grid -- one slide's TFRecord with its ``loc_x`` / ``loc_y``, a region in memory
(``from_region``), or a pyramidal TIFF / SVS slide file (``from_slide``: this build's own reader, ``biscuit_amd/wsi.py``, behind the
slide input stage, ``biscuit_amd/slide_input.py``) -- and lays the same MC-dropout kernels' outputs out as the two grids the reference uses:

    hm.logits       [gy, gx, 2]   mean class probabilities over the MC passes
    hm.uncertainty  [gy, gx, 2]   their population std

Grid cells without a tile hold -1, the value results.py:225 also writes into masked cells.

The picture of Figure 5a (results.py:216-227: ``hm.save(dir, cmap=truncate_colormap(PRGn, 0.1, 0.9))``, once for the full map and
once after the uncertain cells are set to -1) is ``Heatmap.render`` / ``Heatmap.save``: one plane of a grid drawn over the slide's
thumbnail (``wsi.WSI.thumbnail``) through a 256-entry colour table by ``Engine.heatmap_render`` (csrc/kernels_render.hip), masked
cells transparent, written as PNGs through Pillow.  DESIGN.md "Heatmap output" states what is drawn; ``render.py`` holds the host
side (geometry tables, colour table, checks).
"""
import numpy as np
import torch

from .slide_input import DECODE_STATS, MaskSpec, add_mask_arguments, band_stats, batches, build_masks, mask_keywords, upload

MASKED = -1.0


def tile_grid(region, tile_px=299, stride_div=1):
    """The tile grid ``sf.Heatmap(slide, model, stride_div=...)`` walks (results.py:217), over a slide region that is
    already in memory: tiles of ``tile_px`` at stride ``tile_px // stride_div``, row-major, border remainders dropped.
    region: uint8 [H, W, 3] (numpy or torch, host or device).  Returns (tiles [T, tile_px, tile_px, 3] -- a torch
    tensor on the region's device -- and grid int64 [T, 2] of (gx, gy) cells)."""
    r = region if torch.is_tensor(region) else torch.from_numpy(np.ascontiguousarray(region))
    if r.dim() != 3 or r.shape[2] != 3 or r.dtype != torch.uint8:
        raise ValueError('region must be uint8 [H, W, 3]')
    if stride_div < 1 or tile_px % stride_div:
        raise ValueError('stride_div must divide tile_px')
    stride = tile_px // stride_div
    gy = (r.shape[0] - tile_px) // stride + 1 if r.shape[0] >= tile_px else 0
    gx = (r.shape[1] - tile_px) // stride + 1 if r.shape[1] >= tile_px else 0
    if gy == 0 or gx == 0:
        return r.new_zeros((0, tile_px, tile_px, 3)), np.zeros((0, 2), np.int64)
    # [gy, gx, 3, tile_px, tile_px] view -> NHWC tiles
    t = r.unfold(0, tile_px, stride).unfold(1, tile_px, stride)
    tiles = t.permute(0, 1, 3, 4, 2).reshape(gy * gx, tile_px, tile_px, 3).contiguous()
    ys, xs = np.divmod(np.arange(gy * gx, dtype=np.int64), gx)
    return tiles, np.stack([xs, ys], 1)


class Heatmap:
    # what ``render`` needs to place the grid on the slide; ``from_slide`` records them, the other constructors have no slide
    slide_path = slide_w0 = slide_h0 = stride = extract_px = None
    _slide_kw = None
    # what ``from_slide``'s masks did (``slide_input.Masks``): the bool [gh, gw] keep mask, the ``qc`` and the ``roi`` record; None without
    cell_mask = qc = roi = None

    def __init__(self, engine, tiles, grid, grid_shape=None, mc_n=30, seed=0, batch=256, norm_fit=None, normalizer='reinhard_fast'):
        """tiles: uint8 [T,299,299,3] (host or device); grid: int [T,2] (gx, gy) cell of each tile.  ``norm_fit`` / ``normalizer``:
        the model's stain normaliser (stain.METHODS; ``norm_fit=None``: none)."""
        from . import stain
        stain.check(normalizer, norm_fit)
        grid = np.asarray(grid, dtype=np.int64).reshape(-1, 2)
        n = int(tiles.shape[0])
        if grid.shape[0] != n:
            raise ValueError(f'{n} tiles but {grid.shape[0]} grid positions')
        if n and grid.min() < 0:
            raise ValueError('negative grid position')
        if grid_shape is None:
            grid_shape = (int(grid[:, 1].max()) + 1, int(grid[:, 0].max()) + 1) if n else (0, 0)
        gy, gx = grid_shape
        if n and (grid[:, 0].max() >= gx or grid[:, 1].max() >= gy):
            raise ValueError('grid position outside grid_shape')
        self.grid = grid
        self.dropped = 0                 # tiles a background filter left out (from_slide(grayspace_fraction=...))
        self.decode_stats = dict.fromkeys(DECODE_STATS, 0)                       # (from_slide(resample='gpu') counts its bands)
        self.logits = np.full((gy, gx, 2), MASKED, dtype=np.float32)
        self.uncertainty = np.full((gy, gx, 2), MASKED, dtype=np.float32)
        dev = engine.device
        t = tiles if torch.is_tensor(tiles) else torch.from_numpy(np.ascontiguousarray(tiles))
        for s in range(0, n, batch):
            cur = t[s:s + batch].to(dev).contiguous()
            cur = stain.normalise(engine, cur, normalizer, norm_fit)
            mean, std = engine.mc_infer(cur, mc_n, seed, tile_idx0=s)
            g = grid[s:s + batch]
            self.logits[g[:, 1], g[:, 0]] = mean.cpu().numpy()
            self.uncertainty[g[:, 1], g[:, 0]] = std.cpu().numpy()

    @classmethod
    def from_region(cls, engine, region, tile_px=299, stride_div=1, **kw):
        """Heatmap of a slide region in memory: the stride-``tile_px // stride_div`` grid of ``tile_grid``."""
        tiles, grid = tile_grid(region, tile_px, stride_div)
        if len(grid) == 0:
            raise ValueError(f'region {tuple(region.shape[:2])} holds no {tile_px} x {tile_px} tile')
        shape = (int(grid[:, 1].max()) + 1, int(grid[:, 0].max()) + 1)      # (gy, gx) of tile_grid's clamped grid
        return cls(engine, tiles, grid, grid_shape=shape, **kw)

    @classmethod
    def from_slide(cls, engine, path, tile_px=299, tile_um=302, stride_div=1, mpp=None, resample='gpu', canvas_bytes=256 << 20,
                   grayspace_fraction=None, grayspace_threshold=0.05, decode='host', cell_mask=None, qc=None, qc_width=2048,
                   qc_fraction=0.6, focus_threshold=None, focus_mpp=4.0, focus_sigma=3.0, rois=None, roi_method='auto',
                   roi_filter_method='center', roi_width=2048, **kw):
        """``sf.Heatmap(slide, model, stride_div=1)`` (results.py:217) for a pyramidal TIFF / SVS slide file: the tile grid of
        ``wsi.WSI(path, tile_px, tile_um, stride_div)`` through the MC-dropout kernels.  (The reader is this build's own --
        ``biscuit_amd/wsi.py`` says what it reads and what about it is unpinned.)

        ``resample='gpu'`` (default) streams the slide: the grid is read as bands of one canvas each (``WSI.bands``, at most
        ``canvas_bytes`` a canvas), a band's canvas is uploaded once and its tiles are cut and resampled on the device
        (``Engine.tile_resample``: Pillow's LANCZOS bytes), batch by batch, straight into the stain normaliser and ``mc_infer``;
        no tile is held on the host and the device holds one canvas and one batch.  ``resample='host'`` reads and resamples
        every tile on the host first (``WSI.tiles``); both give the same arrays.  A tile's Philox index is its row-major grid
        index ``gy * grid_w + gx`` either way.

        ``grayspace_fraction`` (``resample='gpu'`` only; default None = off): drop a tile as background when more than this
        fraction of its pixels has an HSV saturation below ``grayspace_threshold`` (Slideflow's extraction filter, restated:
        fraction 0.6 and threshold 0.05 there), before stain normalisation.  Dropped cells hold ``MASKED`` in both grids,
        ``self.grid`` lists the kept tiles only and ``self.dropped`` counts the rest; a kept tile's values do not depend on the
        filter.

        ``decode='gpu'`` (``resample='gpu'`` only; default 'host'): a band whose level is a tiled JPEG page is not decoded by
        ``read_region`` on the host -- its raw tiles are read, packed (``tfrecord_native.extract_jpeg_segments``), uploaded
        and decoded on the device straight into the band's canvas (``Engine.jpeg_decode_canvas``): the same bytes, so the same
        arrays.  A tiled JPEG 2000 page (compression 33003 / 33005 / 34712) goes the same way through
        ``tfrecord_native.j2k_extract`` and ``Engine.j2k_decode_canvas``: the same bytes for reversible tiles; for irreversible
        ones the bytes of the decoder's CPU statement, which tests/test_j2k.py holds within one level of OpenJPEG's.  A tiled LZW
        page (compression 5, tiles up to 1024 pixels a side) is only packed on the host (``tfrecord_native.lzw_pack``) and decoded
        by ``Engine.lzw_decode_canvas``: the host decoder's bytes, which are libtiff's.  A band goes through ``read_region`` as before -- the pixels and any ``SlideError`` are then the host's -- when
        the extractor refuses one of its segments, when a segment's device status is not 0, or when the level is not a tiled
        JPEG, JPEG 2000 or LZW page.  ``self.decode_stats = {'gpu_bands', 'host_bands', 'segments'}`` counts the bands either way took and the
        segments the device decoded.

        ``cell_mask`` / ``qc`` (``resample='gpu'`` only; default None = off): a keep mask over the grid, applied BEFORE anything
        is read at full resolution (DESIGN.md "Heatmap input", Tissue mask).  ``cell_mask`` is the caller's own bool [grid_h,
        grid_w] (True = run the cell).  ``qc='otsu'`` computes one from the slide's ``thumbnail(qc_width)`` on the device
        (``Engine.tissue_blur`` / ``tissue_cells``; ``tissue.py``): one Otsu threshold on the 7 x 7 median of the saturation
        channel, and a cell is dropped when more than ``qc_fraction`` of its thumbnail pixels are background -- Slideflow's
        ``qc='otsu'`` restated from memory, unpinned.  Given both, a cell must pass both.  Only bands that hold a kept cell are
        read (``WSI.bands(keep=...)``) and only kept cells are resampled; ``grayspace_fraction``, if on, then judges what
        remains.  Dropped cells hold ``MASKED``, ``self.dropped`` counts every cell not run, ``self.cell_mask`` is the mask used
        and ``self.qc = {'method', 'threshold', 'cells_dropped', 'bands_read', 'bands_skipped_rows'}`` says what it did (the Otsu
        threshold; cells the mask dropped; bands read; grid rows never read).  A kept cell's values do not depend on the mask.
        A mask that keeps no cell gives an all-``MASKED`` heatmap with an empty ``grid``.

        ``focus_threshold`` (``resample='gpu'`` only; default None = off): the focus mask, Slideflow's Gaussian blur QC restated
        from memory in integers, unpinned (DESIGN.md "Heatmap input", Focus mask).  On the slide's thumbnail at ``focus_mpp``
        microns per pixel (``tissue.focus_width``; separate from ``qc_width``) the device takes the gray image, the absolute
        Laplacian and a Gaussian of ``focus_sigma`` pixels (``Engine.tissue_focus``); a pixel is out of focus when the result is
        at most ``focus_threshold``, and a cell is dropped when more than ``qc_fraction`` of its thumbnail pixels are.  ``qc``
        keeps its strings: Slideflow's ``qc='blur'`` is spelled ``focus_threshold=0.02`` and its ``qc='both'`` is ``qc='otsu',
        focus_threshold=0.02`` -- a pixel of the Otsu plane is then bad when it is background or when the focus plane, resized
        onto it by nearest neighbour, says out of focus (``Engine.tissue_cells_union``), and ``qc_fraction`` judges the union.
        ``cell_mask`` still ANDs on top.  ``self.qc`` then also holds ``focus_threshold``, ``focus_width`` and ``focus_share``
        (out-of-focus pixels / all pixels of the focus thumbnail).

        ``rois`` (``resample='gpu'`` only; default None = off): the pathologist's regions of interest, Slideflow's ROI filter
        restated from memory in integers, unpinned (DESIGN.md "Heatmap input", Region-of-interest mask) -- the path of a
        ``ROI_Name,X_base,Y_base`` CSV file (``roi.read_csv``) or a list of int [n, 2] arrays of (x, y) vertices in level-0
        pixels, one polygon each (even-odd inside a polygon, the union across polygons).  ``roi_method``: 'inside' keeps the
        cells inside the region, 'outside' the others, 'auto' is 'inside' with ``rois`` and 'ignore' without, 'ignore' does
        nothing.  ``roi_filter_method='center'`` judges a cell by its centre; a share f in (0, 1] keeps a cell when at least f
        of its pixels on a ``roi_width``-wide raster of the slide (the thumbnail's geometry; nothing is read) lie inside --
        for 'outside', outside.  The polygons become a plane on the device (``Engine.roi_plane``; ``roi.py``), a share is counted
        by ``Engine.tissue_cells``.  The mask ANDs with ``cell_mask``, ``qc`` and ``focus_threshold`` and acts as they do: only
        bands that hold a kept cell are read, dropped cells hold ``MASKED``, a kept cell's values do not depend on it.
        ``self.roi = {'method', 'filter', 'polygons', 'vertices', 'cells_dropped'}`` says what it did (the method used; 'center'
        or the share; the polygons and their vertices; cells this mask alone drops); ``self.qc`` keeps its keys."""
        from .wsi import WSI
        if resample not in ('gpu', 'host'):
            raise ValueError(f"resample must be 'gpu' or 'host', not {resample!r}")
        if resample == 'host' and grayspace_fraction is not None:
            raise ValueError("the background filter runs on the device: grayspace_fraction needs resample='gpu'")
        if decode not in ('host', 'gpu'):
            raise ValueError(f"decode must be 'host' or 'gpu', not {decode!r}")
        if resample == 'host' and decode == 'gpu':
            raise ValueError("the device decodes into the band's canvas: decode='gpu' needs resample='gpu'")
        spec = MaskSpec(cell_mask=cell_mask, qc=qc, qc_width=qc_width, qc_fraction=qc_fraction, focus_threshold=focus_threshold,
                        focus_mpp=focus_mpp, focus_sigma=focus_sigma, rois=rois, roi_method=roi_method,
                        roi_filter_method=roi_filter_method, roi_width=roi_width).checked()
        if resample == 'host' and (qc is not None or cell_mask is not None):
            raise ValueError("the tissue mask steers the streamed read: qc and cell_mask need resample='gpu'")
        if resample == 'host' and focus_threshold is not None:
            raise ValueError("the focus mask steers the streamed read: focus_threshold needs resample='gpu'")
        if spec.roi_method != 'ignore' and resample == 'host':
            raise ValueError("the region-of-interest mask steers the streamed read: rois needs resample='gpu'")
        w = WSI(path, tile_px=tile_px, tile_um=tile_um, stride_div=stride_div, mpp=mpp)
        try:
            if w.grid_w * w.grid_h == 0:
                raise ValueError(f'{path}: the slide holds no {tile_um} um tile')
            if resample == 'host':
                tiles, grid = w.tiles()
                hm = cls(engine, tiles, grid, grid_shape=(w.grid_h, w.grid_w), **kw)
            else:
                hm = cls._streamed(engine, w, build_masks(engine, w, spec), int(canvas_bytes), grayspace_fraction, grayspace_threshold,
                                   decode=decode, **kw)
            hm.slide_path, (hm.slide_w0, hm.slide_h0), hm.stride, hm.extract_px = path, w.slide.dimensions, w.stride, w.extract_px
            hm._slide_kw = dict(tile_px=tile_px, tile_um=tile_um, stride_div=stride_div, mpp=mpp)
            return hm
        finally:
            w.close()

    @classmethod
    def _streamed(cls, engine, w, masks, canvas_bytes, gray_fraction, gray_threshold, mc_n=30, seed=0, batch=256, norm_fit=None,
                  normalizer='reinhard_fast', decode='host'):
        """``from_slide(resample='gpu')``: bands -> batches of exactly the tiles ``Heatmap(engine, *w.tiles())`` would put in
        each batch (a batch is filled across band boundaries: ``slide_input.batches``), so an unfiltered slide runs the same
        launches on the same bytes.  ``masks`` (``slide_input.Masks``): only its kept cells are read and run; ``hm.qc`` / ``hm.roi``."""
        from . import stain
        stain.check(normalizer, norm_fit)
        hm = cls.__new__(cls)
        gh, gw, dev = w.grid_h, w.grid_w, engine.device
        hm.logits = np.full((gh, gw, 2), MASKED, dtype=np.float32)
        hm.uncertainty = np.full((gh, gw, 2), MASKED, dtype=np.float32)
        hm.cell_mask = masks.keep
        stats, kept = band_stats(), []
        for tiles, ids, _ in batches(engine, w, canvas_bytes, gray_fraction, gray_threshold, batch, decode, masks.keep, stats):
            cur = stain.normalise(engine, tiles, normalizer, norm_fit)
            mean, std = engine.mc_infer(cur, mc_n, seed, tile_idx=torch.from_numpy(ids).to(dev))
            gy, gx = np.divmod(ids, gw)
            hm.logits[gy, gx] = mean.cpu().numpy()
            hm.uncertainty[gy, gx] = std.cpu().numpy()
            kept.append(ids)
        hm.dropped = masks.dropped + stats['gray_dropped']
        hm.qc, hm.roi = masks.qc(stats['bands_read'], cells_dropped=True), masks.roi
        hm.decode_stats = {k: stats[k] for k in DECODE_STATS}
        cells = np.concatenate(kept) if kept else np.zeros(0, np.int64)
        hm.grid = np.stack([cells % gw, cells // gw], 1)
        return hm

    # ---- the picture (results.py:216-227; DESIGN.md "Heatmap output") -----------------------------------------------------------
    def _plane(self, plane, index):
        if isinstance(plane, str):
            if plane not in ('logits', 'uncertainty'):
                raise ValueError(f"plane must be 'logits', 'uncertainty' or a float32 [gh, gw] array, not {plane!r}")
            src = getattr(self, plane)
            if not 0 <= int(index) < src.shape[2]:
                raise ValueError(f'{plane} has planes 0 .. {src.shape[2] - 1}, not {index}')
            return np.ascontiguousarray(src[:, :, int(index)], np.float32)
        v = np.ascontiguousarray(plane, np.float32)
        if v.shape != self.logits.shape[:2]:
            raise ValueError(f'a plane of this heatmap is [{self.logits.shape[0]}, {self.logits.shape[1]}], not {list(v.shape)}')
        return v

    def thumbnail(self, width=2048):
        """The slide's thumbnail (``wsi.WSI.thumbnail``), for a heatmap ``from_slide`` built."""
        from .wsi import WSI
        if self.slide_path is None:
            raise ValueError('this heatmap was not built from a slide file (from_slide): pass thumb=')
        w = WSI(self.slide_path, **self._slide_kw)
        try:
            return w.thumbnail(width)
        finally:
            w.close()

    def render(self, engine, plane='logits', index=0, thumb=None, cmap=None, vmin=0.0, vmax=1.0, alpha=0.6, interpolation='none',
               width=2048, slide_w0=None, slide_h0=None, stride=None, extract_px=None):
        """One plane of the heatmap drawn over the slide's thumbnail -> uint8 [H, W, 3] (DESIGN.md "Heatmap output"):
        ``plane`` / ``index`` name ``hm.logits[:, :, index]`` or ``hm.uncertainty[:, :, index]`` (``plane`` may also be a float32
        [gh, gw] array); ``thumb`` uint8 [H, W, 3] (None: the slide's ``thumbnail(width)`` is read); ``cmap`` a uint8 [256, 3]
        table or a matplotlib colormap (None: ``render.PRGN_TRUNC``, the reference's); values are mapped from [``vmin``,
        ``vmax``]; ``alpha`` is the overlay's weight; ``interpolation`` 'none' or 'bicubic'.  Cells that hold -1 or a non-finite
        value stay transparent.  A heatmap built by ``Heatmap(...)`` or ``from_region`` has no slide: it needs ``thumb`` and
        the four geometry numbers ``slide_w0``, ``slide_h0``, ``stride``, ``extract_px`` (level-0 pixels) as keywords."""
        from . import render as R
        R.check_params(vmin, vmax, alpha, interpolation)
        lut = R.lut_from(cmap)
        values = self._plane(plane, index)
        geom = {'slide_w0': slide_w0, 'slide_h0': slide_h0, 'stride': stride, 'extract_px': extract_px}
        geom = {k: getattr(self, k) if v is None else v for k, v in geom.items()}
        missing = [k for k, v in geom.items() if v is None]
        if missing:
            raise ValueError('this heatmap was not built from a slide file (from_slide): render needs thumb= and the geometry '
                             f'keywords slide_w0, slide_h0, stride, extract_px; missing: {", ".join(missing)}')
        if thumb is None:
            thumb = self.thumbnail(width)
        thumb = np.ascontiguousarray(thumb)
        if thumb.dtype != np.uint8 or thumb.ndim != 3 or thumb.shape[2] != 3:
            raise ValueError('thumb must be uint8 [H, W, 3]')
        gh, gw = values.shape
        col, row = R.render_tables(gw, gh, thumb.shape[1], thumb.shape[0], interpolation=interpolation, **geom)
        d_thumb, d_values, d_col, d_row, d_lut = (upload(a, engine.device) for a in (thumb, values, col, row, lut))
        out = engine.heatmap_render(d_values, d_col, d_row, d_lut, d_thumb, vmin=vmin, vmax=vmax, alpha=alpha,
                                    interpolation=interpolation, out=d_thumb)
        return out.cpu().numpy()

    def save(self, engine, outdir, name=None, tile_uq_thresh=None, uncertainty_vmax=None, **render_kw):
        """``hm.save(dir, cmap=...)`` (results.py:219, 227) as PNGs through Pillow: ``<name>-raw.png`` (the thumbnail),
        ``<name>-0.png`` and ``<name>-1.png`` (the two planes of ``logits``) and ``<name>-uncertainty.png`` (``uncertainty[:, :,
        0]`` over [0, ``uncertainty_vmax``]; default: its largest live value, 1 when no live value is positive); with
        ``tile_uq_thresh`` also ``high_confidence/<name>-0.png`` and ``-1.png`` from a COPY of the logits with the cells whose
        ``uncertainty[:, :, 0]`` exceeds the threshold set to -1 (results.py:222-225) -- ``hm.logits`` is not touched.  ``name``
        defaults to the slide file's name without its extension.  ``render_kw``: ``render``'s keywords.  -> the paths written."""
        import os
        from PIL import Image
        if name is None:
            name = os.path.splitext(os.path.basename(str(self.slide_path)))[0] if self.slide_path is not None else 'heatmap'
        kw = dict(render_kw)
        for k in ('plane', 'index'):
            if k in kw:
                raise ValueError(f'save draws every plane: {k}= is not one of its keywords')
        if kw.get('thumb') is None:
            kw['thumb'] = self.thumbnail(kw.get('width', 2048))
        thumb = np.ascontiguousarray(kw['thumb'])
        paths = []

        def write(sub, suffix, img):
            d = os.path.join(outdir, sub) if sub else outdir
            os.makedirs(d, exist_ok=True)
            paths.append(os.path.join(d, f'{name}-{suffix}.png'))
            Image.fromarray(img).save(paths[-1])

        write('', 'raw', thumb)
        for c in (0, 1):
            write('', str(c), self.render(engine, 'logits', c, **kw))
        unc = self.uncertainty[:, :, 0]
        live = unc[np.isfinite(unc) & (unc != MASKED)]
        if uncertainty_vmax is None:
            uncertainty_vmax = float(live.max()) if live.size and float(live.max()) > 0.0 else 1.0
        write('', 'uncertainty', self.render(engine, 'uncertainty', 0, **dict(kw, vmin=0.0, vmax=uncertainty_vmax)))
        if tile_uq_thresh is not None:
            masked = self.logits.copy()
            masked[unc > tile_uq_thresh, :] = [MASKED, MASKED]
            for c in (0, 1):
                write('high_confidence', str(c), self.render(engine, masked[:, :, c], **kw))
        return paths

    def mask_uncertain(self, tile_uq_thresh):
        """results.py:224-225: ``uq_mask = hm.uncertainty[:, :, 0] > thresh; hm.logits[uq_mask, :] = [-1, -1]``.
        Returns the mask."""
        uq_mask = self.uncertainty[:, :, 0] > tile_uq_thresh
        self.logits[uq_mask, :] = [MASKED, MASKED]
        return uq_mask

    def split_by_uncertainty(self, tile_uq_thresh):
        """results.py:258-265: tiles with ``uncertainty[0][0] > thresh`` go to `uq_excl`, the others to
        `uq_incl`; file names ``f"{u:.4f}-{x}-{y}.png"``.  -> (incl, excl) lists of (tile index, name)."""
        incl, excl = [], []
        for i, (x, y) in enumerate(self.grid):
            u = float(self.uncertainty[y, x, 0])
            (excl if u > tile_uq_thresh else incl).append((i, f'{u:.4f}-{x}-{y}.png'))
        return incl, excl


def main(argv=None):
    """``python -m biscuit_amd.heatmap SLIDE --out DIR``: the UQ heatmap of one slide file (results.py:216-265) on disk --
    ``DIR/heatmap.npz`` (``logits``, ``uncertainty``, ``grid``; with ``--tile-uq`` also ``uq_mask`` and ``masked_logits``, the
    logits with the uncertain cells set to -1 as results.py:222-225 does), ``DIR/summary.json`` and, with ``--save-tiles``, the
    tiles as ``uq_incl/`` / ``uq_excl/`` PNGs named as results.py:259 names them.  Under the mask flags (``--qc otsu``, ``--qc-focus
    [THRESHOLD]``, ``--rois FILE`` and their companions: ``from_slide``'s mask keywords) only the kept cells are read and run:
    ``heatmap.npz`` then also holds ``cell_mask``, and ``summary.json`` a ``qc`` entry (``--qc``, ``--qc-focus``; Slideflow's
    ``qc='both'`` is both) and a ``roi`` entry (``--rois``).  ``--render`` adds the pictures of ``Heatmap.save`` (results.py:217-227):
    ``<slide>-raw.png``, ``-0.png``, ``-1.png``, ``-uncertainty.png`` and, with ``--tile-uq``, the masked pair under
    ``high_confidence/``; ``summary.json`` then lists them as ``rendered``."""
    import argparse
    import json
    import os
    import time
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.heatmap', description=main.__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('slide', metavar='SLIDE', help='pyramidal TIFF / SVS slide file')
    ap.add_argument('--weights', help='as python -m biscuit_amd --weights')
    ap.add_argument('--model', help='as python -m biscuit_amd --model')
    ap.add_argument('--params', help="Slideflow params.json: its normalizer and norm_fit switch the stain normaliser on")
    ap.add_argument('--out', required=True)
    ap.add_argument('--stride-div', type=int, default=1)
    ap.add_argument('--mc', type=int, default=None, help='MC-dropout passes (default: uq_n of the model, 30)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--dtype', default='f16', choices=['f16', 'bf16', 'f32'])
    ap.add_argument('--tile-uq', type=float, default=None, help='tile-level uncertainty threshold: adds uq_mask and masked_logits')
    ap.add_argument('--grayspace-fraction', type=float, default=None,
                    help='drop tiles with more than this fraction of grey pixels (Slideflow extracts with 0.6); default: off')
    ap.add_argument('--grayspace-threshold', type=float, default=0.05)
    add_mask_arguments(ap)
    ap.add_argument('--gpu-decode', action='store_true',
                    help="decode the slide's own JPEG, JPEG 2000 or LZW tiles on the device (from_slide(decode='gpu')); the arrays do not change")
    ap.add_argument('--mpp', type=float, default=None, help='microns per pixel, for a file that does not say')
    ap.add_argument('--save-tiles', action='store_true', help='write the tiles to uq_incl/ and uq_excl/ (needs --tile-uq)')
    ap.add_argument('--render', action='store_true',
                    help='write the heatmap as PNGs over the slide thumbnail (Heatmap.save); with --tile-uq also high_confidence/')
    ap.add_argument('--render-interpolation', default='none', choices=['none', 'bicubic'])
    ap.add_argument('--render-width', type=int, default=2048, help='thumbnail width in pixels')
    ap.add_argument('--render-alpha', type=float, default=0.6, help='weight of the overlay, 0 .. 1')
    args = ap.parse_args(argv)
    if args.save_tiles and args.tile_uq is None:
        ap.error('--save-tiles sorts by --tile-uq')
    masks = mask_keywords(ap, args)
    from .__main__ import load_model_weights, model_hp_from
    from .engine import Engine
    weights, model_params = load_model_weights(args.model, args.weights)
    hp, norm_fit = model_hp_from(model_params, args.params)
    mc = hp.uq_n if args.mc is None else args.mc
    eng = Engine(weights, hp=hp, dtype=args.dtype, max_batch=args.batch, max_mc=mc)
    try:
        t0 = time.perf_counter()
        hm = Heatmap.from_slide(eng, args.slide, stride_div=args.stride_div, mpp=args.mpp, mc_n=mc, seed=args.seed, batch=args.batch,
                                norm_fit=norm_fit, normalizer=hp.normalizer or 'reinhard_fast',
                                grayspace_fraction=args.grayspace_fraction, grayspace_threshold=args.grayspace_threshold,
                                decode='gpu' if args.gpu_decode else 'host', **masks)
        torch.cuda.synchronize(eng.device)
        seconds = time.perf_counter() - t0
        rendered = None
        if args.render:                                                  # (after the clock: the engine stays open for it)
            paths = hm.save(eng, args.out, tile_uq_thresh=args.tile_uq, interpolation=args.render_interpolation,
                            width=args.render_width, alpha=args.render_alpha)
            rendered = [os.path.relpath(p, args.out) for p in paths]
    finally:
        eng.close()
    os.makedirs(args.out, exist_ok=True)
    arrays = {'logits': hm.logits.copy(), 'uncertainty': hm.uncertainty, 'grid': hm.grid}
    if args.tile_uq is not None:
        incl, excl = hm.split_by_uncertainty(args.tile_uq)
        arrays['uq_mask'] = hm.mask_uncertain(args.tile_uq)              # (writes -1 into hm.logits: results.py:225)
        arrays['masked_logits'] = hm.logits
        if args.save_tiles:
            from PIL import Image
            from .wsi import WSI
            w = WSI(args.slide, stride_div=args.stride_div, mpp=args.mpp)
            try:
                for name, items in (('uq_incl', incl), ('uq_excl', excl)):
                    os.makedirs(os.path.join(args.out, name), exist_ok=True)
                    for i, fname in items:
                        gx, gy = hm.grid[i]
                        Image.fromarray(w._tile(int(gx), int(gy))).save(os.path.join(args.out, name, fname))
            finally:
                w.close()
    if args.qc is not None or args.qc_focus is not None or hm.roi is not None:
        arrays['cell_mask'] = hm.cell_mask
    np.savez(os.path.join(args.out, 'heatmap.npz'), **arrays)
    run = int(len(hm.grid))
    summary = {'slide': args.slide, 'grid_shape': list(hm.logits.shape[:2]), 'tiles_run': run, 'tiles_dropped': int(hm.dropped),
               'seconds': seconds, 'tiles_per_s': run / seconds if seconds > 0 else None, 'decode_stats': hm.decode_stats}
    if args.qc is not None or args.qc_focus is not None:
        summary['qc'] = hm.qc
    if hm.roi is not None:
        summary['roi'] = hm.roi
    if rendered is not None:
        summary['rendered'] = rendered
    with open(os.path.join(args.out, 'summary.json'), 'w') as f:
        json.dump(summary, f)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
