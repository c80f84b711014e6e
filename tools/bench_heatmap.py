"""Time the whole-slide heatmap (``Heatmap.from_slide``) and its input stage on one GPU.

    python tools/bench_heatmap.py --out DIR                      # this tree, the streamed path
    python tools/bench_heatmap.py --out DIR --resample host      # this tree, tiles read and resampled on the host
    python tools/bench_heatmap.py --out DIR --root OTHER_TREE --resample default --no-kernel
                                                                 # another checkout (e.g. the parent commit), its default path

The slide file is generated from ``--seed`` (deflate tiles of 256 px, two pyramid levels, 1 um per pixel: 302 um tiles are 302
level-0 pixels, ``--grid`` cells at stride_div 1) into ``--slide`` once and reused by later calls, so two trees are timed on
the same bytes.  Per ``--stride-div`` value: ``--runs`` timed calls of ``from_slide`` (wall clock around a call that ends with
every result on the host) after one untimed call; the logits / uncertainty arrays are written to ``DIR/arrays_<tag>.npz`` so
that runs of two trees can be compared.  Then (unless ``--no-kernel``) the resample kernel alone at 302 -> 299 and 604 -> 299 and
``Engine.mc_infer`` alone, in tiles a second (device events around 20 launches of one batch).  One JSON object per line on
stdout and in ``DIR/bench_heatmap_<tag>.jsonl``.

    python tools/bench_heatmap.py --out DIR --decode host --grid 72x56       # the decode leg: a slide of JPEG tiles,
    python tools/bench_heatmap.py --out DIR --decode gpu --grid 72x56        # decoded by read_region / on the device

``--decode`` times ``from_slide(decode=...)`` on a slide of the same picture written with JPEG tiles (``JPEGTables`` plus
abbreviated streams, 4:2:0 at level 0, 4:4:4 at level 1; ``OUT/bench_slide_jpeg.svs``) and, walking the same bands stage by stage
with a device synchronisation behind each, the seconds a band spends in read (+ extract, for 'gpu'; + the host's decode, for
'host'), upload, device decode, and the rest (the band's share of ``from_slide`` minus those).  Run the two values in separate,
alternating processes.

    python tools/bench_heatmap.py --out DIR --render                         # the render leg: no slide, no inference

``--render`` times ``Engine.heatmap_render`` alone (device events around 20 launches, out of place) on a 100 x 100 grid with a
tenth of its cells masked under a 2 048 x 1 536 thumbnail, in both interpolation modes, next to the wall time of the numpy
restatement (``tests/_render_ref.py``) on the same inputs, and checks that the two pictures are equal.

    python tools/bench_heatmap.py --out DIR --qc off --stride-div 1          # the tissue-mask leg: the deflate slide (its right
    python tools/bench_heatmap.py --out DIR --qc otsu --stride-div 1         # fifth is glass) without and with the mask

``--qc`` times ``from_slide(qc=...)`` at the first ``--stride-div`` value -- 'off' passes no mask -- and prints the tiles run, the
mask's own report (``hm.qc``) and, for 'otsu', the host seconds of ``WSI.thumbnail`` and the device milliseconds of
``Engine.tissue_blur`` and ``Engine.tissue_cells`` alone (device events around 20 launches) on that thumbnail.  Run the two values
in separate, alternating processes.

    python tools/bench_heatmap.py --out DIR --qc otsu --qc-focus --stride-div 1      # the focus mask on top (Slideflow's 'both')
    python tools/bench_heatmap.py --out DIR --qc off --qc-focus --stride-div 1       # the focus mask alone

``--qc-focus [THRESHOLD]`` (with ``--qc``; bare: 0.02) passes ``focus_threshold`` as well and prints, as ``focus_mask_parts``, the
host seconds of the 4 um / pixel thumbnail and the device milliseconds of ``Engine.tissue_focus`` on it and of
``Engine.tissue_cells`` / ``Engine.tissue_cells_union`` behind it.  The tool's slide has no out-of-focus region: what the mask
skips on a real slide (``qc_report``: ``cells_dropped``, ``bands_skipped_rows``, ``focus_share``) needs ``--slide`` with one.

    python tools/bench_heatmap.py --out DIR --roi --stride-div 1             # the region-of-interest leg

``--roi`` times ``Engine.roi_plane`` alone (device events around 20 calls, each with its table upload and one launch): on the
'center' grid of a 100 000 x 80 000 pixel slide (167 x 133 cells of 598 pixels) under a 3 000-vertex cogwheel, on a 2 048-wide raster of
the same slide under that cogwheel plus 40 small polygons, and on a 2 048 x 2 048 raster under a 10 000-vertex cogwheel (the design's
worst case); the two rasters next to the wall time of the numpy restatement (``tests/_roi_ref.py``) on the same input, with a check
that the planes are equal.  Then ``from_slide(rois=...)`` on the tool's slide (a cogwheel over its middle, a share of 0.5 on a
2 048-wide raster) at the first ``--stride-div`` value next to the seconds of the mask alone (``slide_input.roi_mask``, every result on
the host): the share of the masked run that the mask takes."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_slide(path, gw, gh, seed, tile=256, px=302, jpeg=False):
    """A two-level tiled deflate TIFF with an Aperio description (MPP = 1.0): level 0 of gw x gh tiles' worth of pixels plus
    a ragged border, level 1 at a quarter of it.  Smooth colour gradients plus seeded noise, a white margin on the right.
    ``jpeg``: JPEG tiles instead (compression 7: abbreviated streams + JPEGTables, quality 85, 4:2:0 at level 0, 4:4:4 at level 1)."""
    w, h = gw * px + 57, gh * px + 31
    rng = np.random.default_rng(seed)

    def encoder(li):
        if not jpeg:
            return (lambda t: zlib.compress(t.tobytes(), 1)), None
        import io

        from PIL import Image

        def enc(t, streamtype=2):
            b = io.BytesIO()
            Image.fromarray(t).save(b, format='JPEG', quality=85, subsampling=2 if li == 0 else 0, streamtype=streamtype)
            return b.getvalue()
        return enc, enc(np.zeros((tile, tile, 3), np.uint8), 1)

    def level(lw, lh, f, enc):
        segs = []
        xx = np.arange(-(-lw // tile) * tile, dtype=np.float32)[None, :] * f
        for ty in range(-(-lh // tile)):
            yy = (np.arange(tile, dtype=np.float32)[:, None] + ty * tile) * f
            row = np.stack([150 + 70 * np.sin(xx / 211 + seed) + 0 * yy, 110 + 60 * np.cos(yy / 173) + 0 * xx,
                            160 + 50 * np.sin((xx + yy) / 307)], -1)
            row += rng.normal(0, 4, row.shape).astype(np.float32)
            row = np.clip(row, 0, 255).astype(np.uint8)
            row[:, int(0.8 * lw):] = 255
            for tx in range(-(-lw // tile)):
                segs.append(enc(np.ascontiguousarray(row[:, tx * tile:(tx + 1) * tile])))
        return segs

    with open(path, 'wb') as f:
        f.write(b'II' + struct.pack('<HHHQ', 43, 8, 0, 0))                  # BigTIFF
        ptr_at = 8
        for li, (lw, lh, fac) in enumerate(((w, h, 1.0), (w // 4, h // 4, 4.0))):
            enc, tables = encoder(li)
            segs = level(lw, lh, fac, enc)
            offs = []
            for s in segs:
                offs.append(f.tell())
                f.write(s)
            desc = (b'Aperio synthetic |MPP = 1.0' if li == 0 else b'level') + b'\0'
            blobs = {}
            for tag, data in ((270, desc), (324, struct.pack(f'<{len(offs)}Q', *offs)), (325, struct.pack(f'<{len(segs)}Q', *map(len, segs))),
                              (258, struct.pack('<3H', 8, 8, 8))) + (((347, tables),) if jpeg else ()):
                blobs[tag] = (f.tell(), data)
                f.write(data + b'\0' * (-len(data) % 8))
            ents = [(256, 4, 1, lw), (257, 4, 1, lh), (258, 3, 3, None), (259, 3, 1, 7 if jpeg else 8), (262, 3, 1, 6 if jpeg else 2), (270, 2, len(desc), None),
                    (277, 3, 1, 3), (284, 3, 1, 1), (322, 4, 1, tile), (323, 4, 1, tile), (324, 16, len(offs), None), (325, 16, len(segs), None)]
            if jpeg:
                ents.append((347, 7, len(tables), None))
            ifd = f.tell()
            f.write(struct.pack('<Q', len(ents)))
            for tag, typ, cnt, val in ents:
                size = {2: 1, 3: 2, 4: 4, 7: 1, 16: 8}[typ] * cnt
                f.write(struct.pack('<HHQ', tag, typ, cnt))
                if val is not None:
                    f.write(struct.pack('<Q', val))
                elif size <= 8:
                    f.write(blobs[tag][1] + b'\0' * (8 - size))
                else:
                    f.write(struct.pack('<Q', blobs[tag][0]))
            nxt = f.tell()
            f.write(struct.pack('<Q', 0))
            f.seek(ptr_at)
            f.write(struct.pack('<Q', ifd))
            f.seek(0, 2)
            ptr_at = nxt
    return w, h


def decode_leg(args, eng, slide, tag, emit, kw):
    """``--decode``: from_slide(decode=...) as a whole, then the same bands stage by stage."""
    import torch
    from biscuit_amd import tfrecord_native as tn
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.wsi import WSI
    dev, sd = eng.device, args.stride_div[0]

    def sync():
        torch.cuda.synchronize(dev)
        return time.perf_counter()
    total = []
    for r in range(args.runs + 1):                                          # the first call is the warm-up
        t0 = sync()
        hm = Heatmap.from_slide(eng, slide, stride_div=sd, decode=args.decode, **kw)
        if r:
            total.append(sync() - t0)
    np.savez(os.path.join(args.out, f'arrays_{tag}.npz'), logits=hm.logits, uncertainty=hm.uncertainty)
    stages = []                                                             # per run: [read, upload, decode] summed over the bands
    for r in range(args.runs + 1):
        w = WSI(slide, stride_div=sd)
        acc, bands, segments = [0.0, 0.0, 0.0], 0, 0
        try:
            for b in w.bands(segments=args.decode == 'gpu'):
                gy0, gy1, gx0, gx1 = b[:4]
                t0 = sync()
                if args.decode == 'gpu':
                    sg = w.band_segments(gy0, gy1, gx0, gx1)[0]             # (read again: the generator's read is not timed)
                    scan, desc, tables = tn.extract_jpeg_segments(sg.data, sg.offsets, sg.lengths, sg.seg_w, sg.seg_h, sg.jpeg_tables)
                    t1 = time.perf_counter()
                    up = [torch.from_numpy(a).to(dev) for a in (scan, desc.view(np.int32), tables, sg.place)]
                    t2 = sync()
                    canvas = torch.full(tuple(sg.shape) + (3,), 255, dtype=torch.uint8, device=dev)
                    status = eng.jpeg_decode_canvas(up[0], up[1], up[2], sg.seg_w, sg.seg_h, up[3], canvas, sg.clip)
                    assert not bool(status.any().item())
                    t3 = sync()
                    segments += len(sg)
                else:
                    canvas = w.band(gy0, gy1, gx0, gx1)[0]
                    t1 = time.perf_counter()
                    canvas = torch.from_numpy(canvas).to(dev)
                    t3 = t2 = sync()
                acc = [acc[0] + t1 - t0, acc[1] + t2 - t1, acc[2] + t3 - t2]
                bands += 1
                del canvas
        finally:
            w.close()
        if r:
            stages.append(acc)
    med = lambda v: float(np.median(v))                                      # noqa: E731
    per = [med([s[k] for s in stages]) / bands for k in range(3)]
    tot = med(total) / bands
    emit({'what': 'decode_leg', 'decode': args.decode, 'stride_div': sd, 'cells': int(hm.logits.shape[0] * hm.logits.shape[1]), 'bands': bands,
          'segments': segments, 'decode_stats': hm.decode_stats, 'mc': args.mc, 'from_slide_s': [round(t, 4) for t in total],
          'per_band_s': {'read_extract' if args.decode == 'gpu' else 'read_decode_host': round(per[0], 4), 'upload': round(per[1], 4),
                         'decode_device': round(per[2], 4), 'rest': round(tot - sum(per), 4), 'total': round(tot, 4)},
          'per_band_runs_s': [[round(v / bands, 4) for v in s] for s in stages],
          'spread_total': round((max(total) - min(total)) / med(total), 4)})


def qc_leg(args, eng, slide, tag, emit, kw):
    """``--qc``: from_slide with or without the tissue mask, then the mask's own pieces."""
    import torch
    from biscuit_amd import tissue
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.wsi import WSI
    sd = args.stride_div[0]
    if args.qc != 'off':
        kw = dict(kw, qc=args.qc, qc_width=args.qc_width)
    if args.qc_focus is not None:
        kw = dict(kw, focus_threshold=args.qc_focus)
    times = []
    for r in range(args.runs + 1):                                          # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hm = Heatmap.from_slide(eng, slide, stride_div=sd, **kw)
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    np.savez(os.path.join(args.out, f'arrays_{tag}.npz'), logits=hm.logits, uncertainty=hm.uncertainty)
    cells, med = int(hm.logits.shape[0] * hm.logits.shape[1]), float(np.median(times))
    emit({'what': 'from_slide_qc', 'qc': args.qc, 'qc_focus': args.qc_focus, 'stride_div': sd, 'mc': args.mc, 'cells': cells, 'tiles_run': int(len(hm.grid)),
          'dropped': int(hm.dropped), 'qc_report': hm.qc, 'seconds': [round(t, 4) for t in times], 'median_s': round(med, 4),
          'spread': round((max(times) - min(times)) / med, 4)})
    if args.qc == 'off' and args.qc_focus is None:
        return

    def thumb_of(width_of):
        """-> (the thumbnail, its cells' ranges, the host seconds of three reads)."""
        w = WSI(slide, stride_div=sd)
        try:
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                thumb = np.ascontiguousarray(w.thumbnail(width_of(w)))
                host.append(time.perf_counter() - t0)
            col, row = tissue.cell_ranges(w.grid_w, w.grid_h, thumb.shape[1], thumb.shape[0], *w.slide.dimensions, w.stride, w.extract_px)
        finally:
            w.close()
        return thumb, col, row, host

    def ms(fn, reps=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return round(a.elapsed_time(b) / reps, 4)

    up = lambda t: torch.from_numpy(t if t.flags.writeable else t.copy()).to(eng.device)       # noqa: E731
    plane = thr = None
    if args.qc != 'off':
        thumb, col, row, host = thumb_of(lambda w: args.qc_width)
        d_thumb = up(thumb)
        plane, hist = eng.tissue_blur(d_thumb)
        thr = tissue.otsu_threshold(hist.cpu().numpy())
        emit({'what': 'tissue_mask_parts', 'thumb': list(thumb.shape[:2]), 'grid': [len(row), len(col)], 'threshold': thr,
              'thumbnail_host_s': [round(t, 4) for t in host], 'tissue_blur_ms': ms(lambda: eng.tissue_blur(d_thumb)),
              'tissue_cells_ms': ms(lambda: eng.tissue_cells(plane, thr, col, row))})
    if args.qc_focus is None:
        return
    fthumb, fcol, frow, fhost = thumb_of(lambda w: tissue.focus_width(w.slide.dimensions[0], w.mpp))
    d_fthumb = up(fthumb)
    fplane, fcount = eng.tissue_focus(d_fthumb, args.qc_focus)
    parts = {'what': 'focus_mask_parts', 'thumb': list(fthumb.shape[:2]), 'grid': [len(frow), len(fcol)], 'focus_threshold': args.qc_focus,
             'focus_share': int(fcount.cpu().numpy()[0]) / float(fthumb.shape[0] * fthumb.shape[1]),
             'thumbnail_host_s': [round(t, 4) for t in fhost], 'tissue_focus_ms': ms(lambda: eng.tissue_focus(d_fthumb, args.qc_focus))}
    if plane is None:
        parts['tissue_cells_ms'] = ms(lambda: eng.tissue_cells(fplane, 0, fcol, frow))
    else:
        parts['tissue_cells_union_ms'] = ms(lambda: eng.tissue_cells_union(plane, thr, fplane, col, row))
    emit(parts)


def roi_leg(args, eng, slide, tag, emit, kw):
    """``--roi``: the rasteriser alone on three inputs, next to the numpy restatement, then the mask's share of a masked from_slide."""
    import torch
    sys.path.insert(0, HERE)
    from biscuit_amd import roi
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.slide_input import MaskSpec, roi_mask
    from biscuit_amd.wsi import WSI
    from tests import _roi_ref as ref

    def cog(cx, cy, r_out, r_in, n):
        k = np.arange(n)
        t = 2.0 * np.pi * k / n
        r = np.where((k // 25) % 2 == 0, float(r_out), float(r_in))
        return np.stack([np.rint(cx + r * np.cos(t)), np.rint(cy + r * np.sin(t))], 1).astype(np.int32)

    def ms(fn, reps=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return round(a.elapsed_time(b) / reps, 4)

    rng = np.random.default_rng(args.seed)
    w0, h0 = 100_000, 80_000
    ring = cog(w0 // 2, h0 // 2, 0.45 * h0, 0.3 * h0, 3000)
    small = [np.stack([cx + rng.integers(-3000, 3001, 5), cy + rng.integers(-3000, 3001, 5)], 1).astype(np.int32)
             for cx, cy in zip(rng.integers(0, w0, 40), rng.integers(0, h0, 40))]
    gw, gh = (w0 - 598) // 598 + 1, (h0 - 598) // 598 + 1
    inputs = [('center_grid', roi.center_tables(gw, gh, 598, 598), [ring], False),
              ('raster_2048', roi.raster_tables(w0, h0, 2048), [ring] + small, True),
              ('raster_2048x2048_10k_edges', roi.raster_tables(w0, w0, 2048), [cog(w0 // 2, w0 // 2, 0.45 * w0, 0.3 * w0, 10000)], True)]
    for name, (xs, ys), polys, with_numpy in inputs:
        d = {'what': 'roi_plane', 'input': name, 'plane': [len(ys), len(xs)], 'polygons': len(polys), 'edges': int(sum(len(a) for a in polys)),
             'device_ms': ms(lambda: eng.roi_plane(xs, ys, polys))}
        got = eng.roi_plane(xs, ys, polys).cpu().numpy()
        d['inside_share'] = round(float(got.mean()), 4)
        if with_numpy:
            t0 = time.perf_counter()
            want = ref.plane(xs, ys, polys)
            d['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            d['equal'] = bool(np.array_equal(got, want))
        emit(d)
    # the mask's share of a masked run, on the tool's slide
    sd = args.stride_div[0]
    w = WSI(slide, stride_div=sd)
    sw, sh = w.slide.dimensions
    polys = [cog(sw // 2, sh // 2, 0.45 * min(sw, sh), 0.3 * min(sw, sh), 3000)]
    rkw = dict(rois=polys, roi_filter_method=0.5, roi_width=2048)
    spec = MaskSpec(**rkw).checked()                                        # ('auto' is 'inside' with polygons)
    try:
        alone = []
        for r in range(args.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = roi_mask(eng, w, spec)
            torch.cuda.synchronize()
            if r:
                alone.append(time.perf_counter() - t0)
    finally:
        w.close()
    times = []
    for r in range(args.runs + 1):                                          # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hm = Heatmap.from_slide(eng, slide, stride_div=sd, **rkw, **kw)
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    assert np.array_equal(hm.cell_mask, keep)
    np.savez(os.path.join(args.out, f'arrays_{tag}.npz'), logits=hm.logits, uncertainty=hm.uncertainty, cell_mask=hm.cell_mask)
    med, med_mask = float(np.median(times)), float(np.median(alone))
    emit({'what': 'from_slide_roi', 'stride_div': sd, 'mc': args.mc, 'cells': int(keep.size), 'tiles_run': int(len(hm.grid)), 'roi_report': hm.roi,
          'qc_report': hm.qc, 'seconds': [round(t, 4) for t in times], 'median_s': round(med, 4), 'mask_alone_s': [round(t, 5) for t in alone],
          'mask_share_of_run': round(med_mask / med, 5), 'spread': round((max(times) - min(times)) / med, 4)})


def render_leg(args, eng, emit):
    """``--render``: the kernel's milliseconds per picture and the numpy restatement's, same inputs, same bytes."""
    import torch
    sys.path.insert(0, HERE)
    from biscuit_amd import render as R
    from tests import _render_ref as ref
    rng = np.random.default_rng(args.seed)
    gw = gh = 100
    W, H = 2048, 1536
    geom = dict(slide_w0=gw * 302 + 57, slide_h0=gh * 302 + 31, stride=302, extract_px=302)
    values = rng.uniform(0, 1, (gh, gw)).astype(np.float32)
    values[rng.uniform(0, 1, (gh, gw)) < 0.1] = R.MASKED
    thumb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)                    # noqa: E731
    d_values, d_lut, d_thumb, out = up(values), up(R.PRGN_TRUNC), up(thumb), torch.empty((H, W, 3), dtype=torch.uint8, device=eng.device)
    for mode in R.INTERPOLATIONS:
        col, row = (up(t) for t in R.render_tables(gw, gh, W, H, interpolation=mode, **geom))
        fn = lambda: eng.heatmap_render(d_values, col, row, d_lut, d_thumb, interpolation=mode, out=out)   # noqa: E731
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        t0 = time.perf_counter()
        want = ref.render(values, thumb, R.PRGN_TRUNC, interpolation=mode, **geom)
        numpy_s = time.perf_counter() - t0
        emit({'what': 'heatmap_render', 'interpolation': mode, 'grid': [gh, gw], 'thumb': [H, W], 'masked_cells': int((values == R.MASKED).sum()),
              'device_ms': round(a.elapsed_time(b) / reps, 4), 'numpy_ms': round(numpy_s * 1e3, 1),
              'equal': bool(np.array_equal(out.cpu().numpy(), want))})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', required=True)
    ap.add_argument('--root', default=HERE, help='the checkout whose biscuit_amd is timed (default: this one)')
    ap.add_argument('--tag', default=None)
    ap.add_argument('--slide', default=None, help='slide file to generate / reuse (default: OUT/bench_slide.svs)')
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--grid', default='36x28', help='grid cells at stride_div 1 (columns x rows; at least 1 000 cells by default)')
    ap.add_argument('--resample', default='gpu', choices=['gpu', 'host', 'default'], help="'default': pass no resample argument")
    ap.add_argument('--stride-div', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--mc', type=int, default=30)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--no-kernel', action='store_true')
    ap.add_argument('--decode', default=None, choices=['host', 'gpu'],
                    help='the decode leg only: from_slide(decode=...) on a slide of JPEG tiles, and seconds per band by stage')
    ap.add_argument('--render', action='store_true', help='the render leg only: Engine.heatmap_render next to its numpy restatement')
    ap.add_argument('--qc', default=None, choices=['off', 'otsu'],
                    help="the tissue-mask leg only: from_slide without ('off') or with the mask, and the mask's own pieces")
    ap.add_argument('--qc-width', type=int, default=2048)
    ap.add_argument('--qc-focus', type=float, nargs='?', const=0.02, default=None, metavar='THRESHOLD',
                    help="with --qc: pass focus_threshold too (bare: 0.02) and time the focus mask's own pieces")
    ap.add_argument('--roi', action='store_true',
                    help="the region-of-interest leg only: Engine.roi_plane next to its numpy restatement, and the mask's share of from_slide(rois=...)")
    args = ap.parse_args()
    if args.qc_focus is not None and args.qc is None:
        ap.error("--qc-focus belongs to the tissue-mask leg: give --qc off (the focus mask alone) or --qc otsu")
    os.makedirs(args.out, exist_ok=True)
    tag = args.tag or ('render' if args.render else 'roi' if args.roi else 'qc_' + args.qc + ('_focus' if args.qc_focus is not None else '') if args.qc is not None else
                       args.resample if args.decode is None else 'decode_' + args.decode)
    slide = args.slide or os.path.join(args.out, 'bench_slide.svs' if args.decode is None else 'bench_slide_jpeg.svs')
    gw, gh = (int(v) for v in args.grid.lower().split('x'))
    if not os.path.exists(slide) and not args.render:
        t0 = time.perf_counter()
        write_slide(slide, gw, gh, args.seed, jpeg=args.decode is not None)
        print(json.dumps({'slide': slide, 'bytes': os.path.getsize(slide), 'written_in_s': round(time.perf_counter() - t0, 2)}), flush=True)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from biscuit_amd.engine import Engine
    from biscuit_amd.heatmap import Heatmap
    from biscuit_amd.weights import synthetic_weights
    log = open(os.path.join(args.out, f'bench_heatmap_{tag}.jsonl'), 'a')

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=args.batch, max_mc=args.mc)
    kw = dict(mc_n=args.mc, seed=0, batch=args.batch)
    if args.render:
        render_leg(args, eng, emit)
        eng.close()
        return
    if args.decode is not None:
        decode_leg(args, eng, slide, tag, emit, kw)
        eng.close()
        return
    if args.roi:
        roi_leg(args, eng, slide, tag, emit, kw)
        eng.close()
        return
    if args.qc is not None:
        qc_leg(args, eng, slide, tag, emit, kw)
        eng.close()
        return
    if args.resample != 'default':
        kw['resample'] = args.resample
    arrays = {}
    for sd in args.stride_div:
        times = []
        for r in range(args.runs + 1):                                      # the first call is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hm = Heatmap.from_slide(eng, slide, stride_div=sd, **kw)
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        cells = int(hm.logits.shape[0] * hm.logits.shape[1])
        arrays[f'logits_{sd}'], arrays[f'uncertainty_{sd}'] = hm.logits, hm.uncertainty
        emit({'what': 'from_slide', 'tag': tag, 'root': os.path.abspath(args.root), 'stride_div': sd, 'cells': cells,
              'seconds': [round(t, 4) for t in times], 'median_s': round(float(np.median(times)), 4),
              'spread': round((max(times) - min(times)) / float(np.median(times)), 4), 'tiles_per_s': round(cells / float(np.median(times)), 1)})
    np.savez(os.path.join(args.out, f'arrays_{tag}.npz'), **arrays)
    if not args.no_kernel:
        rng = np.random.default_rng(args.seed)
        n = args.batch

        def rate(fn, reps=20):
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            return n * reps / (a.elapsed_time(b) * 1e-3)

        for src in (302, 604):
            for sdiv in (1, 2):                                             # a band of the grid: sdiv = 2 overlaps the windows
                step, cols = src // sdiv, 16 * sdiv
                rows = -(-n // cols)
                canvas = torch.from_numpy(rng.integers(0, 256, ((rows - 1) * step + src, (cols - 1) * step + src, 3), dtype=np.uint8)).to(eng.device)
                org = np.array([[x * step, y * step] for y in range(rows) for x in range(cols)][:n], np.int32)
                origin = torch.from_numpy(org).to(eng.device)
                out = torch.empty((n, 299, 299, 3), dtype=torch.uint8, device=eng.device)
                emit({'what': 'tile_resample', 'src_px': src, 'stride_div': sdiv, 'batch': n,
                      'tiles_per_s': round(rate(lambda: eng.tile_resample(canvas, origin, src, out=out)), 1)})
        tiles = torch.from_numpy(rng.integers(0, 256, (n, 299, 299, 3), dtype=np.uint8)).to(eng.device)
        emit({'what': 'tile_grayspace', 'batch': n, 'tiles_per_s': round(rate(lambda: eng.tile_grayspace(tiles)), 1)})
        emit({'what': 'mc_infer', 'batch': n, 'mc': args.mc, 'tiles_per_s': round(rate(lambda: eng.mc_infer(tiles, args.mc, 0), reps=10), 1)})
    eng.close()


if __name__ == '__main__':
    main()
