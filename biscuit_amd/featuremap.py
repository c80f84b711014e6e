"""The cohort's feature map -- Figure 6 of the paper (results.py:270-306: ``generate_features(model, max_tiles=10)``, then
``generate_mosaic`` and UMAPs labelled by prediction, uncertainty, confidence and slide label): the post-pooling activations of a
few tiles per slide, their prediction and uncertainty, a 2-D UMAP of the activations and a mosaic of the tiles laid out on it.

    python -m biscuit_amd.featuremap SLIDE.tfrecords ... --out DIR

writes ``umap.csv`` and ``mosaic.png``.  The scatter plots themselves are out of scope, like the rest of the plotting.

Unpinned against Slideflow (restated from memory, DESIGN.md "Feature map (Figure 6)"): which tiles of a slide are kept (here the
first ``max_tiles`` records), the defaults ``n_neighbors = 50`` and ``min_dist = 0.1``, the mosaic's assignment, and UMAP itself
(biscuit_amd/umap.py).  Pinned: a kept tile's features, prediction and uncertainty are exactly ``evaluate()``'s for that tile --
``backbone_u8``, then ``mc_head`` with the tile's index in the whole, unclipped slide list.
"""
import argparse
import json
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import umap


@dataclass
class FeatureMap:
    """Per kept tile, in slide order: ``slide`` names, ``index`` (the record's index in its slide), ``loc`` int64 [N, 2],
    ``features`` fp32 [N, 2048] at true scale, ``y_pred`` / ``uncertainty`` fp32 [N, 2], ``tiles`` uint8 [N, 299, 299, 3] as read
    (before any stain normaliser; None when not kept), ``xy`` float32 [N, 2] once ``embed`` has run."""
    slide: list
    index: np.ndarray
    loc: np.ndarray
    features: np.ndarray
    y_pred: np.ndarray
    uncertainty: np.ndarray
    tiles: Optional[np.ndarray] = None
    xy: Optional[np.ndarray] = None
    labels: dict = field(default_factory=dict)          # slide name -> label (optional column of umap.csv)
    mosaic_image: Optional[np.ndarray] = None
    mosaic_cells: list = field(default_factory=list)    # (cell x, cell y, row of the table) of every used cell

    def __len__(self):
        return len(self.slide)

    def frame(self, outcome='cohort', tile_uq=None):
        """The table ``save`` writes: slide, loc_x, loc_y, x, y, ``{outcome}-y_pred1``, ``{outcome}-uncertainty1``, confident
        (uncertainty < ``tile_uq``; all True without a threshold) and, with ``labels``, label."""
        import pandas as pd
        if self.xy is None:
            raise ValueError('embed the features first')
        unc = self.uncertainty[:, 1].astype(np.float64)
        cols = {'slide': pd.Series(list(self.slide), dtype=str), 'loc_x': self.loc[:, 0], 'loc_y': self.loc[:, 1],
                'x': self.xy[:, 0].astype(np.float64), 'y': self.xy[:, 1].astype(np.float64),
                f'{outcome}-y_pred1': self.y_pred[:, 1].astype(np.float64), f'{outcome}-uncertainty1': unc,
                'confident': unc < float(tile_uq) if tile_uq else np.ones(len(unc), bool)}
        if self.labels:
            cols['label'] = [self.labels.get(s, '') for s in self.slide]
        return pd.DataFrame(cols)

    def save(self, directory, outcome='cohort', tile_uq=None):
        """``umap.csv`` and -- when ``mosaic`` has run -- ``mosaic.png`` into ``directory``.  -> the paths written."""
        os.makedirs(directory, exist_ok=True)
        paths = [os.path.join(directory, 'umap.csv')]
        self.frame(outcome, tile_uq).to_csv(paths[0], index=False)
        if self.mosaic_image is not None:
            from PIL import Image
            paths.append(os.path.join(directory, 'mosaic.png'))
            Image.fromarray(self.mosaic_image).save(paths[1])
        return paths


def _first_records(slide, count, px):
    """The first ``count`` tiles of a slide and their locations, reading no more than those from a TFRecord."""
    src = getattr(slide, 'source', None)
    if src is not None and hasattr(src, 'path'):
        from . import tfrecord
        from . import tfrecord_native as tn
        if tn.available():
            try:
                with tn.NativeReader(src.path) as r:
                    tiles, loc = r.decode(0, count, px)
                    return np.ascontiguousarray(tiles), np.asarray(loc, np.int64).reshape(-1, 2)
            except tn.UnsupportedImage:
                pass
        _, tiles, loc = tfrecord.read_slide(src.path, px)
        return np.ascontiguousarray(tiles[:count]), np.asarray(loc[:count], np.int64).reshape(-1, 2)
    t = slide.load()
    if hasattr(t, 'rows'):
        raise ValueError(f'slide {slide.name!r}: filtered PNG scanlines without a chunk source are not tiles')
    t = t[:count]
    t = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, 'cpu') else t)
    loc = np.asarray(slide.loc)[:count] if slide.loc is not None else np.stack([np.arange(count), np.zeros(count, np.int64)], 1)
    return t, np.asarray(loc, np.int64).reshape(-1, 2)


def walk_features(eng, slides, max_tiles, on_batch, norm_fit=None, normalizer='reinhard_fast', keep_tiles=False, batch=None, prepare=None,
                  stage=None):
    """``evaluate()``'s input stage over the first ``max_tiles`` tiles of every slide (0 / None: all): decode, stain normaliser,
    ``backbone_u8`` in batches of at most ``batch`` (the engine's ``max_batch`` when None or larger).  ``on_batch(f, g)`` gets each
    batch's features fp32 [b, 2048] and global tile indices int64 [b], both on the device, in slide order: a tile's index is its
    index in the UNCLIPPED slide list (``distributed.global_tile_offsets`` of the slides' tile counts), its Philox tile counter in
    ``evaluate()``.  ``prepare(tiles_u8, g)``, when given, gets each step's uint8 batch and its global indices on the device before
    the stain normaliser and returns the tiles to go on with (``train.cache_features`` augments there).  ``stage``, when given, is
    called in the place of ``backbone_u8`` and ``on_batch`` gets what it returns (``train.cache_activations``: ``Engine.trunk``).
    -> ``(names, index, loc, tiles)``: per kept tile its slide's name, its record's index in the slide, its location int64 [N, 2], and
    the tiles as read uint8 [N, px, px, 3] (None unless ``keep_tiles``)."""
    import torch
    from . import distributed as D, stain
    stain.check(normalizer, norm_fit)
    px = int(eng.hp.tile_px)
    step = int(eng.max_batch if not batch else min(int(batch), eng.max_batch))
    offsets = D.global_tile_offsets([s.n_tiles for s in slides])
    names, index, locs, tiles = [], [], [], []

    def flush(batch_tiles, batch_gidx):
        t = torch.from_numpy(np.concatenate(batch_tiles)).to(eng.device)
        g = torch.from_numpy(np.concatenate(batch_gidx)).to(eng.device)
        for a in range(0, len(t), step):
            cur, gi = t[a:a + step].contiguous(), g[a:a + step].contiguous()
            if prepare is not None:
                cur = prepare(cur, gi)
            cur = stain.normalise(eng, cur, normalizer, norm_fit)
            on_batch((stage or eng.backbone_u8)(cur), gi)

    pend_t, pend_g, pending = [], [], 0
    for si, s in enumerate(slides):
        count = s.n_tiles if not max_tiles else min(int(max_tiles), s.n_tiles)
        if count == 0:
            continue
        t, loc = _first_records(s, count, px)
        names += [s.name] * count
        index.append(np.arange(count, dtype=np.int64))
        locs.append(loc)
        if keep_tiles:
            tiles.append(t)
        pend_t.append(t); pend_g.append(int(offsets[si]) + np.arange(count, dtype=np.int64)); pending += count
        if pending >= 4 * step:
            flush(pend_t, pend_g)
            pend_t, pend_g, pending = [], [], 0
    if pending:
        flush(pend_t, pend_g)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    return names, cat(index, (0,), np.int64), cat(locs, (0, 2), np.int64), cat(tiles, (0, px, px, 3), np.uint8) if keep_tiles else None


def generate_features(engine_or_pool, slides, max_tiles=10, mc_n=None, seed=None, norm_fit=None, normalizer='reinhard_fast', keep_tiles=True):
    """The first ``max_tiles`` tiles of every slide (0 / None: all) through ``backbone_u8`` and ``mc_head`` -> ``FeatureMap``.  The
    Philox index of a tile is its index in the UNCLIPPED slide list (``walk_features``), so its numbers are exactly the ones
    ``evaluate()`` over the same slides gives it."""
    eng = engine_or_pool.engines[0] if hasattr(engine_or_pool, 'engines') else engine_or_pool
    mc_n = int(mc_n or eng.hp.uq_n)
    seed = int(eng.hp.seed if seed is None else seed)
    feats, means, stds = [], [], []

    def head(f, g):
        m, s = eng.mc_head(f, mc_n, seed, tile_idx0=0, tile_idx=g)
        feats.append(f.cpu().numpy()); means.append(m.cpu().numpy()); stds.append(s.cpu().numpy())

    names, index, loc, tiles = walk_features(eng, slides, max_tiles, head, norm_fit, normalizer, keep_tiles)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    return FeatureMap(names, index, loc, cat(feats, (0, 2048), np.float32), cat(means, (0, 2), np.float32), cat(stds, (0, 2), np.float32),
                      tiles)


def embed(engine, features, n_neighbors=50, min_dist=0.1, seed=0, n_epochs=None):
    """``features`` fp32 [N, D] -> the UMAP float32 [N, 2] (``umap.embed``: neighbours, weights and epochs on the device, graph
    and PCA start on the host).  A ``FeatureMap`` is embedded in place (its ``xy``) and returned."""
    eng = engine.engines[0] if hasattr(engine, 'engines') else engine
    if isinstance(features, FeatureMap):
        features.xy = umap.embed(eng, features.features, n_neighbors, min_dist, seed, n_epochs)
        return features
    return umap.embed(eng, features, n_neighbors, min_dist, seed, n_epochs)


def mosaic_cells(xy, num_tiles_x):
    """The mosaic's assignment, on the host: a grid of ``num_tiles_x`` square cells spans the map's extent in x (as many rows as
    its extent in y needs, row 0 at the TOP: the largest y); every cell takes the point nearest its centre among the points inside
    it (the lower row of the table on a tie).  -> ``(cells, (rows, cols))``, cells = [(cell x, cell y, point)] in row-major
    order."""
    xy = np.asarray(xy, np.float64)
    nx = int(num_tiles_x)
    if nx < 1 or xy.ndim != 2 or xy.shape[1] != 2 or len(xy) < 1 or not np.isfinite(xy).all():
        raise ValueError('mosaic: num_tiles_x >= 1 and a finite [N >= 1, 2] map')
    lo, hi = xy.min(0), xy.max(0)
    cell = max(hi[0] - lo[0], 1e-12) / nx
    ny = max(1, int(np.ceil((hi[1] - lo[1]) / cell - 1e-9)))
    cx = np.minimum(((xy[:, 0] - lo[0]) / cell).astype(np.int64), nx - 1)
    cy = np.minimum(((hi[1] - xy[:, 1]) / cell).astype(np.int64), ny - 1)
    centre = np.stack([lo[0] + (cx + 0.5) * cell, hi[1] - (cy + 0.5) * cell], 1)
    d2 = ((xy - centre) ** 2).sum(1)
    best = {}
    for p in np.lexsort((np.arange(len(xy)), d2)):
        best.setdefault((int(cy[p]), int(cx[p])), int(p))
    return [(x, y, p) for (y, x), p in sorted(best.items())], (ny, nx)


def mosaic(engine, fmap, num_tiles_x=20, cell_px=64):
    """The tiles laid out on the map: ``mosaic_cells`` chooses, ``Engine.tile_resample`` shrinks the chosen tiles to ``cell_px``
    (stacked as one canvas, a 299-px window each; the kernel shrinks by up to 8, so ``cell_px`` >= 38), the host pastes them into one white uint8 [rows * cell_px, num_tiles_x *
    cell_px, 3] image -> ``fmap.mosaic_image`` / ``fmap.mosaic_cells``.  Returns the image."""
    import torch
    eng = engine.engines[0] if hasattr(engine, 'engines') else engine
    if fmap.xy is None or fmap.tiles is None:
        raise ValueError('mosaic needs an embedded FeatureMap that kept its tiles')
    cells, (ny, nx) = mosaic_cells(fmap.xy, num_tiles_x)
    px, cell_px = int(fmap.tiles.shape[1]), int(cell_px)
    image = np.full((ny * cell_px, nx * cell_px, 3), 255, np.uint8)
    chunk = max(1, min(len(cells), 256))
    for a in range(0, len(cells), chunk):
        part = cells[a:a + chunk]
        canvas = torch.from_numpy(np.ascontiguousarray(fmap.tiles[[p for _, _, p in part]]).reshape(len(part) * px, px, 3)).to(eng.device)
        origin = torch.tensor([[0, i * px] for i in range(len(part))], dtype=torch.int32, device=eng.device)
        small = eng.tile_resample(canvas, origin, px, cell_px).cpu().numpy()
        for (x, y, _), t in zip(part, small):
            image[y * cell_px:(y + 1) * cell_px, x * cell_px:(x + 1) * cell_px] = t
    fmap.mosaic_image, fmap.mosaic_cells = image, cells
    return image


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.featuremap', description=__doc__.split('\n\n')[0])
    ap.add_argument('tfrecords', nargs='+', help='Slideflow *.tfrecords, one per slide')
    ap.add_argument('--out', required=True)
    ap.add_argument('--weights', help='weights file (see python -m biscuit_amd --help)')
    ap.add_argument('--model', help='Slideflow model directory: weights plus params.json')
    ap.add_argument('--params', help='params.json whose normaliser and fit to use')
    ap.add_argument('--labels', help='CSV with slide,label: the optional label column of umap.csv')
    ap.add_argument('--outcome', default='cohort')
    ap.add_argument('--dtype', default='f16', choices=['f16', 'bf16', 'f32'])
    ap.add_argument('--mc', type=int, default=None, help='MC-dropout passes (default: uq_n of the model, 30)')
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--max-tiles', type=int, default=10, help='tiles kept per slide, from its first record on (0: all)')
    ap.add_argument('--n-neighbors', type=int, default=50)
    ap.add_argument('--min-dist', type=float, default=0.1)
    ap.add_argument('--tile-uq', type=float, default=0.0, help='tile-level uncertainty threshold of the confident column (0 = off)')
    ap.add_argument('--mosaic', type=int, default=20, metavar='N', help='cells across the mosaic (0: no mosaic)')
    ap.add_argument('--cell-px', type=int, default=64)
    args = ap.parse_args(argv)
    from .__main__ import load_model_weights, model_hp_from
    from .engine import Engine
    from .inference import slides_from_tfrecords
    w, model_params = load_model_weights(args.model, args.weights)
    hp, norm_fit = model_hp_from(model_params, args.params)
    labels = {}
    if args.labels:
        import pandas as pd
        lab = pd.read_csv(args.labels, dtype={'slide': str})
        labels = dict(zip(lab['slide'], lab['label']))
    slides = slides_from_tfrecords(list(args.tfrecords), {}, gpu_unfilter=False)
    act_exp = None
    if args.dtype == 'f16' and (args.model or args.weights) and any(s.n_tiles for s in slides):
        first = next(s for s in slides if s.n_tiles)
        probe, _ = _first_records(first, min(16, first.n_tiles), hp.tile_px)
        act_exp, _ = Engine.calibrate(w, probe, hp=hp, norm_fit=norm_fit, normalizer=hp.normalizer)
    eng = Engine(w, hp=hp, dtype=args.dtype, max_batch=64, max_mc=int(args.mc or hp.uq_n), act_exp=act_exp)
    try:
        fmap = generate_features(eng, slides, max_tiles=args.max_tiles, mc_n=args.mc, seed=args.seed, norm_fit=norm_fit,
                                 normalizer=hp.normalizer)
        if len(fmap) < 2:
            raise SystemExit('a map needs at least two tiles')
        fmap.labels = labels
        embed(eng, fmap, n_neighbors=args.n_neighbors, min_dist=args.min_dist)
        if args.mosaic > 0:
            mosaic(eng, fmap, num_tiles_x=args.mosaic, cell_px=args.cell_px)
        paths = fmap.save(args.out, args.outcome, args.tile_uq)
    finally:
        eng.close()
    print(json.dumps({'tiles': len(fmap), 'slides': len(set(fmap.slide)), 'files': paths}))


if __name__ == '__main__':
    main()
