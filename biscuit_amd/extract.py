"""Tile extraction: a slide file -> one Slideflow tile TFRecord, on the device (DESIGN.md "Tile extraction").

The reference starts with ``extract_tiles(tile_px=299, tile_um=302, qc='both')`` over a cohort; ``extract_slide`` is that step for
one pyramidal TIFF / SVS file.  It is the slide input stage (``slide_input.py``) with no network behind it: the masks over the grid
(``MaskSpec`` / ``build_masks``: the caller's mask, Otsu and focus QC, regions of interest), the band-to-batch loop
(``batches``: ``WSI.bands``, canvas upload or device decode, ``Engine.tile_resample``, ``Engine.tile_grayspace``) -- and
then, in place of stain normalisation and ``mc_infer``, ``Engine.jpeg_encode`` or ``Engine.png_encode``: the batch leaves the
device as finished files -- the JPEG files Pillow would have written for its tiles (``img_format='jpg'``, the default), or PNG
files (``'png'``, the reference's own setting: lossless, Pillow's filtered rows in the project's own deflate stream).  The host
frames them as records (``tfrecord.SlideWriter``) and holds no pixels.

    python -m biscuit_amd.extract SLIDE [SLIDE ...] --out DIR [--qc otsu] [--qc-focus] [--rois FILE] [--img-format png] ...

writes ``DIR/SLIDE.tfrecords`` and ``DIR/SLIDE.extract.json`` per slide; ``evaluate()`` reads the TFRecords back, on the host or
with ``gpu_decode``.
"""
import json
import os

import numpy as np

from . import tfrecord
from .slide_input import DECODE_STATS, MaskSpec, add_mask_arguments, band_stats, batches, build_masks, mask_keywords


def tile_loc(cells, grid_w, stride, extract_px):
    """``loc_x`` / ``loc_y`` of row-major grid cells: the tile's centre in level-0 pixels, ``(gx * stride + extract_px // 2, gy *
    stride + extract_px // 2)`` -- Slideflow's convention restated from memory (unpinned).  -> int64 [n, 2]."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    gy, gx = np.divmod(cells, int(grid_w))
    return np.stack([gx * int(stride) + int(extract_px) // 2, gy * int(stride) + int(extract_px) // 2], 1)


class RowMajor:
    """Records that arrive band by band, written in row-major grid order: ``add`` takes a batch's (cell, file) pairs and the first
    grid row that may still receive cells; every pending record of an earlier row is then written, sorted by cell.  Holds the
    encoded records of the bands in flight, never a slide's."""

    def __init__(self, write):
        self.write, self.pending = write, []

    def add(self, cells, files, open_row_cell):
        self.pending.extend(zip((int(c) for c in cells), files))
        self.flush(open_row_cell)

    def flush(self, below=None):
        self.pending.sort(key=lambda r: r[0])
        k = len(self.pending) if below is None else sum(1 for c, _ in self.pending if c < below)
        for c, f in self.pending[:k]:
            self.write(c, f)
        del self.pending[:k]


IMG_FORMATS = ('jpg', 'png')             # Slideflow's spellings of ``extract_tiles(img_format=...)``


def extract_slide(engine, path, out, tile_px=299, tile_um=302, stride_div=1, mpp=None, quality=95, subsampling='4:2:0', decode='host',
                  canvas_bytes=256 << 20, qc=None, focus_threshold=None, rois=None, cell_mask=None, grayspace_fraction=None, batch=256,
                  grayspace_threshold=0.05, qc_width=2048, qc_fraction=0.6, focus_mpp=4.0, focus_sigma=3.0, roi_method='auto',
                  roi_filter_method='center', roi_width=2048, img_format='jpg'):
    """One slide's tiles -> ``out`` (a ``.tfrecords`` path, or a directory: ``SLIDE.tfrecords`` in it) as JPEG records of
    (quality, subsampling) or, with ``img_format='png'``, as PNG records (lossless; ``quality`` and ``subsampling`` do not
    apply and read ``None`` in the summary), plus ``SLIDE.extract.json`` next to it; returns that summary as a dict.

    The grid is ``wsi.WSI(path, tile_px, tile_um, stride_div, mpp)``'s; ``decode``, ``canvas_bytes``, ``cell_mask``, ``qc``,
    ``focus_threshold``, ``rois``, ``grayspace_fraction`` and their companions are ``Heatmap.from_slide``'s keywords with the same
    meaning (Slideflow's ``qc='both'`` is ``qc='otsu', focus_threshold=0.02``).  Every record's ``image_raw`` is the file
    ``tfrecord.encode_image(tile, 'JPEG')`` -- Pillow -- writes for the tile at the default quality 95 / 4:2:0; ``loc_x`` /
    ``loc_y`` are ``tile_loc``'s; records stand in row-major grid order whatever the banding.  A PNG record decodes to the
    resampled tile bit for bit, so ``evaluate()`` over the file equals ``Heatmap.from_slide`` for any slide."""
    import torch
    from .tfrecord_native import jpeg_subsampling
    from .wsi import WSI
    if img_format not in IMG_FORMATS:
        raise ValueError(f"img_format must be 'jpg' or 'png', not {img_format!r}")
    if decode not in ('host', 'gpu'):
        raise ValueError(f"decode must be 'host' or 'gpu', not {decode!r}")
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f'quality must lie in 1..100, not {quality!r}')
    jpeg_subsampling(subsampling)
    spec = MaskSpec(cell_mask=cell_mask, qc=qc, qc_width=qc_width, qc_fraction=qc_fraction, focus_threshold=focus_threshold,
                    focus_mpp=focus_mpp, focus_sigma=focus_sigma, rois=rois, roi_method=roi_method, roi_filter_method=roi_filter_method,
                    roi_width=roi_width).checked()
    name = os.path.splitext(os.path.basename(str(path)))[0]
    if os.path.isdir(out) or not str(out).endswith('.tfrecords'):
        os.makedirs(out, exist_ok=True)
        out = os.path.join(out, name + '.tfrecords')
    w = WSI(path, tile_px=tile_px, tile_um=tile_um, stride_div=stride_div, mpp=mpp)
    try:
        if w.grid_w * w.grid_h == 0:
            raise ValueError(f'{path}: the slide holds no {tile_um} um tile')
        masks, stats, gw = build_masks(engine, w, spec), band_stats(), w.grid_w
        with tfrecord.SlideWriter(out, name) as writer:
            def write(cell, image):
                (lx, ly), = tile_loc([cell], gw, w.stride, w.extract_px)
                writer.write(image, lx, ly)
            order = RowMajor(write)
            for tiles, ids, gy0 in batches(engine, w, int(canvas_bytes), grayspace_fraction, grayspace_threshold, batch, decode, masks.keep, stats):
                buf, off = engine.png_encode(tiles) if img_format == 'png' else engine.jpeg_encode(tiles, quality, subsampling)
                data = buf.cpu().numpy()
                off = off.numpy()
                order.add(ids, [data[off[i]:off[i + 1]].tobytes() for i in range(len(ids))], gy0 * gw)
            order.flush()
            torch.cuda.synchronize(engine.device)
        summary = {
            'slide': str(path), 'tfrecord': out, 'grid_shape': [w.grid_h, w.grid_w], 'tile_px': int(tile_px), 'tile_um': tile_um,
            'stride_div': int(stride_div), 'stride': int(w.stride), 'extract_px': int(w.extract_px),
            'cells': int(w.grid_h * w.grid_w), 'cells_kept_by_masks': int(w.grid_h * w.grid_w - masks.dropped),
            'cells_dropped': {'masks': masks.dropped, 'roi': None if masks.roi is None else masks.roi['cells_dropped'],
                              'grayspace': int(stats['gray_dropped'])},
            'qc': masks.qc(stats['bands_read']), 'roi': masks.roi, 'tiles_written': writer.records, 'bytes_written': writer.nbytes,
            'decode_stats': {k: stats[k] for k in DECODE_STATS},
            'img_format': img_format, 'quality': quality,
            'subsampling': subsampling if isinstance(subsampling, str) else {0: '4:4:4', 2: '4:2:0'}[subsampling],
        }
        if img_format == 'png':
            summary['quality'] = summary['subsampling'] = None
    finally:
        w.close()
    with open(out[:-len('.tfrecords')] + '.extract.json', 'w') as f:
        json.dump(summary, f, indent=1)
    return summary


def main(argv=None):
    """Extract the tiles of slide files to Slideflow TFRecords on the GPU (one ``SLIDE.tfrecords`` + ``SLIDE.extract.json`` per slide)."""
    import argparse
    import time
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.extract', description=main.__doc__)
    ap.add_argument('slides', metavar='SLIDE', nargs='+', help='pyramidal TIFF / SVS slide files')
    ap.add_argument('--out', required=True, metavar='DIR')
    ap.add_argument('--tile-px', type=int, default=299)
    ap.add_argument('--tile-um', type=float, default=302)
    ap.add_argument('--stride-div', type=int, default=1)
    ap.add_argument('--mpp', type=float, default=None, help='microns per pixel, for a file that does not say')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--img-format', default='jpg', choices=list(IMG_FORMATS), help="the records' image format (default jpg; png is lossless)")
    ap.add_argument('--quality', type=int, default=None, help='JPEG quality, 1..100 (default 95: tfrecord.encode_image); jpg only')
    ap.add_argument('--subsampling', default=None, choices=['4:2:0', '4:4:4'], help='JPEG chroma subsampling (default 4:2:0); jpg only')
    ap.add_argument('--gpu-decode', action='store_true', help="decode the slide's own JPEG, JPEG 2000 or LZW tiles on the device; the records do not change")
    ap.add_argument('--grayspace-fraction', type=float, default=None,
                    help='drop tiles with more than this fraction of grey pixels (Slideflow extracts with 0.6); default: off')
    ap.add_argument('--grayspace-threshold', type=float, default=0.05)
    add_mask_arguments(ap)
    args = ap.parse_args(argv)
    if args.img_format == 'png' and (args.quality is not None or args.subsampling is not None):
        ap.error('--quality and --subsampling apply to --img-format jpg only: a PNG record is lossless')
    quality, subsampling = 95 if args.quality is None else args.quality, args.subsampling or '4:2:0'
    masks = mask_keywords(ap, args)
    from .engine import Engine
    from .weights import synthetic_weights
    eng = Engine(synthetic_weights(1), max_batch=8, max_mc=2)          # (no network runs here: the context is what is needed)
    try:
        for slide in args.slides:
            t0 = time.perf_counter()
            s = extract_slide(eng, slide, args.out, tile_px=args.tile_px, tile_um=args.tile_um, stride_div=args.stride_div, mpp=args.mpp,
                              quality=quality, subsampling=subsampling, img_format=args.img_format, decode='gpu' if args.gpu_decode else 'host',
                              grayspace_fraction=args.grayspace_fraction, batch=args.batch, grayspace_threshold=args.grayspace_threshold, **masks)
            dt = time.perf_counter() - t0
            print(json.dumps({'slide': slide, 'tfrecord': s['tfrecord'], 'tiles_written': s['tiles_written'],
                              'bytes_written': s['bytes_written'], 'seconds': round(dt, 3)}))
    finally:
        eng.close()


if __name__ == '__main__':
    main()
