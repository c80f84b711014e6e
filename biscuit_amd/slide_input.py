"""A slide's input half, shared by ``Heatmap.from_slide`` and ``extract.extract_slide`` (DESIGN.md "Heatmap input"): which cells of
the tile grid are read (``MaskSpec`` -> ``build_masks`` -> ``Masks``), the band loop that brings them to the device as batches
(``batches``), and the two command lines' mask flags (``add_mask_arguments``).  What a keyword means is ``from_slide``'s docstring."""
import dataclasses
import os

import numpy as np
import torch

from . import tfrecord_native as tn

DECODE_STATS = ('gpu_bands', 'host_bands', 'segments')      # bands the device decoded, bands the host read, segments decoded


def upload(a, device):
    """A numpy array on the device.  A read-only one (a Pillow array is) is copied first: ``torch.from_numpy`` wants to write."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)


@dataclasses.dataclass(frozen=True)
class MaskSpec:
    """The mask keywords of ``Heatmap.from_slide`` and ``extract.extract_slide``."""
    cell_mask: object = None
    qc: object = None
    qc_width: int = 2048
    qc_fraction: float = 0.6
    focus_threshold: object = None
    focus_mpp: float = 4.0
    focus_sigma: float = 3.0
    rois: object = None
    roi_method: str = 'auto'
    roi_filter_method: object = 'center'
    roi_width: int = 2048

    def checked(self):
        """The keywords checked, on or off, without a slide or an engine: ValueError, or the spec resolved -- ``rois`` the
        polygons read, ``roi_method`` with 'auto' decided, ``roi_filter_method`` 'center' or a float, ``roi_width`` an int."""
        from . import roi, tissue
        if self.qc is not None and self.qc not in tissue.QC_METHODS:
            raise ValueError(f"qc must be None or one of {tissue.QC_METHODS}, not {self.qc!r}")
        if self.qc is not None:
            tissue.check_fraction(self.qc_fraction)
            if int(self.qc_width) < 1:
                raise ValueError(f'qc_width must be at least 1, not {self.qc_width!r}')
        tissue.check_focus(0.0 if self.focus_threshold is None else self.focus_threshold, self.focus_mpp, self.focus_sigma)
        if self.focus_threshold is not None:
            tissue.check_fraction(self.qc_fraction)
        roi_filter, roi_width = roi.check_filter(self.roi_filter_method), roi.check_width(self.roi_width)
        polygons = self.rois
        if polygons is not None:
            polygons = roi.read_csv(polygons) if isinstance(polygons, (str, os.PathLike)) else roi.check_polygons(polygons)
        return dataclasses.replace(self, rois=polygons, roi_method=roi.check_method(self.roi_method, polygons is not None),
                                   roi_filter_method=roi_filter, roi_width=roi_width)


class Masks:
    """What ``build_masks`` made of a spec: ``keep`` bool [grid_h, grid_w], the masks ANDed (None without any); ``method`` the spec's
    ``qc``; the Otsu ``threshold``; the ``focus`` entries of the ``qc`` record; the ``roi`` record -- each None without its mask."""
    keep = method = threshold = focus = roi = None
    dropped = 0                                                              # cells ``keep`` leaves out

    def qc(self, bands_read, cells_dropped=False):
        """The ``qc`` record of a run that read ``bands_read`` bands; None without a mask."""
        if self.keep is None:
            return None
        return dict(method=self.method, threshold=self.threshold, **({'cells_dropped': self.dropped} if cells_dropped else {}),
                    bands_read=bands_read, bands_skipped_rows=int((~self.keep.any(1)).sum()), **(self.focus or {}))


def build_masks(engine, w, spec):
    """The masks of the open slide ``w`` under a checked ``spec``: the caller's mask, the tissue / focus QC and the regions of
    interest, in this order, ANDed -> ``Masks``."""
    from . import tissue
    m, keeps = Masks(), []
    m.method = spec.qc
    if spec.cell_mask is not None:
        keeps.append(tissue.check_mask(spec.cell_mask, w.grid_h, w.grid_w).copy())
    if spec.focus_threshold is not None:
        keep, m.threshold, m.focus = focus_mask(engine, w, spec)
        keeps.append(keep)
    elif spec.qc is not None:
        keep, m.threshold = otsu_mask(engine, w, spec)
        keeps.append(keep)
    if spec.roi_method != 'ignore':
        keep = roi_mask(engine, w, spec)
        m.roi = {'method': spec.roi_method, 'filter': spec.roi_filter_method, 'polygons': len(spec.rois),
                 'vertices': int(sum(len(a) for a in spec.rois)), 'cells_dropped': int(keep.size - keep.sum())}
        keeps.append(keep)
    for keep in keeps:
        m.keep = keep if m.keep is None else m.keep & keep
        m.dropped = int(m.keep.size - m.keep.sum())
    return m


def otsu_mask(engine, w, spec, focus_plane=None):
    """``qc='otsu'`` for the open slide ``w``: (keep bool [grid_h, grid_w], the Otsu threshold).  The thumbnail goes up once; 256
    histogram counts and the cells' counts come back -- with ``focus_plane`` (``Engine.tissue_focus``'s) the union's counts."""
    from . import tissue
    thumb = upload(w.thumbnail(int(spec.qc_width)), engine.device)
    plane, hist = engine.tissue_blur(thumb)
    threshold = tissue.otsu_threshold(hist.cpu().numpy())
    sw, sh = w.slide.dimensions
    col, row = tissue.cell_ranges(w.grid_w, w.grid_h, int(thumb.shape[1]), int(thumb.shape[0]), sw, sh, w.stride, w.extract_px)
    counts = (engine.tissue_cells(plane, threshold, col, row) if focus_plane is None else
              engine.tissue_cells_union(plane, threshold, focus_plane, col, row))
    return tissue.keep_from_counts(counts.cpu().numpy(), col, row, spec.qc_fraction), threshold


def focus_mask(engine, w, spec):
    """``focus_threshold=...`` for the open slide ``w``, alone (``qc`` None) or with ``qc='otsu'``: (keep bool [grid_h, grid_w],
    the Otsu threshold or None, the focus entries of the ``qc`` record).  Alone, a cell's out-of-focus pixels are counted over
    its range of the focus plane; with Otsu, ``otsu_mask`` counts the union."""
    from . import tissue
    sw, sh = w.slide.dimensions
    fthumb = upload(w.thumbnail(tissue.focus_width(sw, w.mpp, spec.focus_mpp)), engine.device)
    fh, fw = int(fthumb.shape[0]), int(fthumb.shape[1])
    fplane, fcount = engine.tissue_focus(fthumb, spec.focus_threshold, spec.focus_sigma)
    del fthumb
    if spec.qc is None:
        col, row = tissue.cell_ranges(w.grid_w, w.grid_h, fw, fh, sw, sh, w.stride, w.extract_px)
        counts = engine.tissue_cells(fplane, 0, col, row).cpu().numpy()
        keep, threshold = tissue.keep_from_counts(counts, col, row, spec.qc_fraction), None
    else:
        keep, threshold = otsu_mask(engine, w, spec, focus_plane=fplane)
    info = {'focus_threshold': float(spec.focus_threshold), 'focus_width': fw, 'focus_share': int(fcount.cpu().numpy()[0]) / float(fh * fw)}
    return keep, threshold, info


def roi_mask(engine, w, spec):
    """``rois=...`` for the open slide ``w`` -> keep bool [grid_h, grid_w].  'center': the plane of the cells' centres comes
    back; a share: the plane is made on a ``roi_width``-wide raster and stays on the device, the cells' counts come back."""
    from . import roi, tissue
    if spec.roi_filter_method == 'center':
        xs, ys = roi.center_tables(w.grid_w, w.grid_h, w.stride, w.extract_px)
        return roi.keep_from_plane(engine.roi_plane(xs, ys, spec.rois).cpu().numpy(), spec.roi_method)
    sw, sh = w.slide.dimensions
    xs, ys = roi.raster_tables(sw, sh, spec.roi_width)
    col, row = tissue.cell_ranges(w.grid_w, w.grid_h, len(xs), len(ys), sw, sh, w.stride, w.extract_px)
    outside = engine.tissue_cells(engine.roi_plane(xs, ys, spec.rois), 0, col, row).cpu().numpy()
    return roi.keep_from_share(outside, col, row, spec.roi_filter_method, spec.roi_method)


def band_stats():
    """The counters of ``batches``: ``DECODE_STATS``, 'bands_read' (under a mask) and 'gray_dropped' (by the background filter)."""
    return dict.fromkeys(DECODE_STATS + ('bands_read', 'gray_dropped'), 0)


def _pack_jpeg(sg):
    scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)
    return scan, desc.view(np.int32), tables


def _pack_lzw(sg):
    packed, desc = tn.lzw_pack(sg.data, sg.offsets, sg.lengths)
    return packed, desc.view(np.int32)


# ``BandSegments.codec`` -> how ``decode_band`` decodes such a band: the host's extractor (-> the packed arrays the engine call
# takes first, or ValueError -- UnsupportedImage is one -- for a segment it refuses), the ``Engine`` method, the keywords the
# method takes from the segments beside the common ones, and the longest side of a segment the device decoder takes (None: any).
BAND_CODECS = {
    'jpeg': (_pack_jpeg, 'jpeg_decode_canvas', lambda sg: {}, None),
    'j2k': (lambda sg: tn.j2k_extract(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h), 'j2k_decode_canvas',
            lambda sg: {'ycc': sg.ycc}, tn.J2K_MAX_SIDE),
    'lzw': (_pack_lzw, 'lzw_decode_canvas', lambda sg: {'predictor': sg.predictor}, tn.LZW_MAX_SIDE),
}


def decode_band(engine, sg):
    """A band's canvas decoded on the device from its raw JPEG, JPEG 2000 or LZW tiles (``wsi.BandSegments``, by its row of
    ``BAND_CODECS``): extract on the host, upload what the extractor packed and the places, fill the canvas with 255, decode, read
    the status once.  -> the canvas (uint8 [H, W, 3] on the device), or None when a segment is larger than the device decoder
    takes, the extractor refuses one, or any status is not 0."""
    extract, entry, keywords, max_side = BAND_CODECS[sg.codec]
    if max_side and max(sg.seg_w, sg.seg_h) > max_side:
        return None
    try:
        packed = extract(sg)
    except ValueError:
        return None
    dev = engine.device
    canvas = torch.full(tuple(sg.shape) + (3,), 255, dtype=torch.uint8, device=dev)
    if len(sg) == 0:
        return canvas
    status = getattr(engine, entry)(*(torch.from_numpy(a).to(dev) for a in packed), sg.seg_w, sg.seg_h, torch.from_numpy(sg.place).to(dev),
                                    canvas, sg.clip, **keywords(sg))
    return None if bool(status.any().item()) else canvas


def batches(engine, w, canvas_bytes, gray_fraction, gray_threshold, batch, decode, mask, stats):
    """The band-to-batch loop of a streamed slide: walks ``w.bands``, uploads or device-decodes each band's canvas, fills ONE
    device batch with ``Engine.tile_resample`` across band boundaries and drops background tiles with ``Engine.tile_grayspace``
    if asked.  Yields ``(tiles, ids, gy0)`` for every full batch and the last partial one: a view of the batch buffer (uint8
    [n, px, px, 3] on the device, valid until the next step), the tiles' row-major grid indices (int64 [n], the caller's to keep)
    and the first grid row of the band being read (``WSI.band_rows``, not the rectangle's own: a later column range of the band
    may start higher up) -- every cell of an earlier row has been yielded by then.  ``stats``: ``band_stats()``, counted up."""
    if gray_fraction is not None and not 0.0 <= float(gray_fraction) <= 1.0:
        raise ValueError('grayspace_fraction must lie in [0, 1]')
    gw, px, dev, batch = w.grid_w, w.tile_px, engine.device, int(batch)
    buf = torch.empty((batch, px, px, 3), dtype=torch.uint8, device=dev)      # the one batch the device holds
    idx = np.empty(batch, np.int64)                                          # its tiles' row-major grid indices
    fill = 0
    for gy0, gy1, gx0, gx1, canvas, origin, src_px in w.bands(canvas_bytes, segments=decode == 'gpu', keep=mask):
        d_canvas = None
        if decode == 'gpu' and canvas is not None:
            d_canvas = decode_band(engine, canvas)
            if d_canvas is not None:
                stats['gpu_bands'] += 1
                stats['segments'] += len(canvas)
        if d_canvas is None:
            if decode == 'gpu':
                canvas = w.band(gy0, gy1, gx0, gx1)[0]                       # the host's pixels, or the host's SlideError
            d_canvas = torch.from_numpy(canvas).to(dev)
            stats['host_bands'] += 1
        d_origin = torch.from_numpy(origin).to(dev)
        del canvas, origin                                                   # uploaded: the host holds one canvas at a time
        cell = (np.arange(gy0, gy1, dtype=np.int64)[:, None] * gw + np.arange(gx0, gx1, dtype=np.int64)[None, :]).reshape(-1)
        if mask is not None:
            stats['bands_read'] += 1
            pos = np.flatnonzero(mask[gy0:gy1, gx0:gx1].reshape(-1))       # the rectangle's kept cells, row-major
            if len(pos) < len(cell):
                d_origin, cell = d_origin[torch.from_numpy(pos).to(dev)], cell[pos]
        a = 0
        while a < len(cell):
            m = min(len(cell) - a, batch - fill)
            dst = buf[fill:fill + m]
            engine.tile_resample(d_canvas, d_origin[a:a + m], src_px, px, out=dst)
            ids = cell[a:a + m]
            if gray_fraction is not None:
                grey = engine.tile_grayspace(dst, gray_threshold).cpu().numpy()
                keep = ~(grey / float(px * px) > float(gray_fraction))
                if not keep.all():
                    sel = torch.from_numpy(np.flatnonzero(keep)).to(dev)
                    if len(sel):
                        dst[:len(sel)] = dst[sel]                             # (the right side is a copy: no overlap)
                    stats['gray_dropped'] += m - len(sel)
                    ids = ids[keep]
            idx[fill:fill + len(ids)] = ids
            fill += len(ids)
            a += m
            if fill == batch:
                yield buf[:fill], idx[:fill].copy(), w.band_rows[0]
                fill = 0
        del d_canvas
    if fill:
        yield buf[:fill], idx[:fill].copy(), w.grid_h


def add_mask_arguments(ap):
    """The mask flags of ``python -m biscuit_amd.heatmap`` and ``python -m biscuit_amd.extract``; ``mask_keywords`` reads them."""
    ap.add_argument('--qc', default=None, choices=['otsu'], help="tissue mask from the slide's thumbnail (from_slide(qc=...)); default: off")
    ap.add_argument('--qc-width', type=int, default=2048, help='width of the thumbnail --qc judges')
    ap.add_argument('--qc-fraction', type=float, default=0.6, help='drop a cell with more than this fraction of background pixels')
    ap.add_argument('--qc-focus', type=float, nargs='?', const=0.02, default=None, metavar='THRESHOLD',
                    help="focus mask (from_slide(focus_threshold=...); bare: 0.02), alone or with --qc otsu (Slideflow's 'both'); off")
    ap.add_argument('--qc-focus-mpp', type=float, default=4.0, help='microns per pixel of the thumbnail --qc-focus judges')
    ap.add_argument('--qc-focus-sigma', type=float, default=3.0, help="sigma of --qc-focus's Gaussian, in thumbnail pixels")
    ap.add_argument('--rois', default=None, metavar='FILE', help="regions of interest, Slideflow's ROI_Name,X_base,Y_base CSV; default: off")
    ap.add_argument('--roi-method', default='auto', choices=['auto', 'inside', 'outside', 'ignore'], help="'auto': inside when --rois is given")
    ap.add_argument('--roi-filter', default='center', metavar='center|SHARE',
                    help='judge a cell by its centre, or keep it when at least SHARE (0 < SHARE <= 1) of it lies inside')
    ap.add_argument('--roi-width', type=int, default=2048, help='width of the raster a --roi-filter SHARE is counted on')


def mask_keywords(ap, args):
    """The flags of ``add_mask_arguments`` as ``ap`` parsed them -> the mask keywords; ``ap.error`` for a bad ``--roi-filter``."""
    roi_filter = args.roi_filter
    if roi_filter != 'center':
        try:
            roi_filter = float(roi_filter)
        except ValueError:
            ap.error(f"--roi-filter takes 'center' or a share in (0, 1], not {args.roi_filter!r}")
    return dict(qc=args.qc, qc_width=args.qc_width, qc_fraction=args.qc_fraction, focus_threshold=args.qc_focus,
                focus_mpp=args.qc_focus_mpp, focus_sigma=args.qc_focus_sigma, rois=args.rois, roi_method=args.roi_method,
                roi_filter_method=roi_filter, roi_width=args.roi_width)
