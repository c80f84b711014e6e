"""Host side of the heatmap's output stage (DESIGN.md "Heatmap output"; reference: results.py:216-227, ``sf.Heatmap(...).save(dir,
cmap=truncate_colormap(PRGn, 0.1, 0.9))``): the constants of the contract by name, the geometry tables the kernel reads
(``render_tables``), the default colour table (``PRGN_TRUNC``) and the argument checks.  The device side is
``Engine.heatmap_render`` (csrc/kernels_render.hip); ``heatmap.Heatmap.render`` / ``save`` put the two together.  Nothing here
imports matplotlib unless ``lut_from`` is handed one of its colormaps."""
import numpy as np

MASKED = -1.0                            # heatmap.MASKED: a cell with this value (or a non-finite one) is transparent
RENDER_MAX_PX = 16384                    # 1 <= W, H <= this
RENDER_ALPHA = 0.6                       # default alpha; used as A = round(alpha * 256) = 154
RENDER_ALPHA_ONE = 256
RENDER_Q_BITS = 16                       # q = clamp(floor(t * 2^16), 0, 2^16 - 1); the colour is lut[q >> 8]
RENDER_WEIGHT_BITS = 12                  # Catmull-Rom weights: 12 fractional bits, each group of four sums to 4096
RENDER_WEIGHT_ONE = 1 << RENDER_WEIGHT_BITS
RENDER_CUBIC_A = -0.5                    # Catmull-Rom
RENDER_ENTRY = 9                         # 'bicubic' table entry: cell, four tap cells, four weights
INTERPOLATIONS = ('none', 'bicubic')     # the C entry's interpolation argument is the index

# truncate_colormap(PRGn, 0.1, 0.9) as results.py:216 calls it, at indices 0..255 (tools/make_colormap.py regenerates this)
# --- PRGN_TRUNC begin (tools/make_colormap.py) ---
PRGN_TRUNC = np.array([
    (116,  41, 129), (118,  43, 131), (119,  45, 132), (120,  47, 133), (121,  49, 135), (122,  51, 136),
    (123,  53, 137), (124,  55, 138), (125,  57, 139), (126,  59, 141), (127,  61, 142), (129,  64, 143),
    (130,  66, 144), (131,  68, 146), (132,  71, 147), (134,  74, 149), (135,  77, 151), (136,  79, 152),
    (137,  81, 153), (138,  83, 154), (140,  86, 156), (141,  88, 157), (142,  90, 158), (143,  92, 159),
    (144,  94, 161), (145,  96, 162), (146,  98, 163), (147, 100, 164), (148, 103, 165), (149, 105, 167),
    (150, 107, 168), (151, 109, 169), (152, 111, 170), (154, 113, 171), (155, 114, 172), (156, 116, 174),
    (157, 118, 175), (158, 119, 176), (160, 121, 177), (161, 122, 178), (162, 124, 179), (163, 126, 180),
    (165, 127, 181), (166, 129, 182), (167, 131, 183), (168, 132, 185), (170, 134, 186), (171, 135, 187),
    (172, 137, 188), (173, 139, 189), (175, 140, 190), (176, 142, 191), (178, 144, 192), (179, 146, 194),
    (181, 149, 196), (183, 150, 197), (184, 152, 198), (185, 154, 199), (186, 155, 200), (188, 157, 201),
    (189, 158, 202), (190, 160, 203), (191, 162, 205), (193, 163, 206), (194, 165, 207), (195, 166, 207),
    (196, 168, 208), (197, 169, 209), (198, 171, 210), (199, 172, 210), (201, 173, 211), (202, 175, 212),
    (203, 176, 213), (204, 178, 214), (205, 179, 214), (206, 181, 215), (207, 182, 216), (208, 183, 217),
    (210, 185, 217), (211, 186, 218), (212, 188, 219), (213, 189, 220), (214, 191, 220), (215, 192, 221),
    (216, 193, 222), (217, 195, 223), (219, 196, 223), (220, 198, 224), (221, 200, 225), (223, 202, 226),
    (224, 204, 227), (226, 205, 228), (227, 207, 229), (228, 208, 230), (229, 210, 231), (230, 211, 231),
    (231, 212, 232), (231, 213, 232), (232, 214, 233), (232, 215, 233), (233, 217, 234), (233, 218, 234),
    (234, 219, 235), (234, 220, 235), (235, 221, 235), (235, 222, 236), (236, 223, 236), (236, 224, 237),
    (237, 225, 237), (237, 226, 238), (238, 227, 238), (238, 228, 239), (239, 229, 239), (239, 230, 240),
    (240, 231, 240), (240, 232, 240), (241, 234, 241), (241, 235, 241), (242, 236, 242), (242, 237, 242),
    (243, 238, 243), (243, 239, 243), (244, 240, 244), (244, 241, 244), (244, 242, 245), (245, 243, 245),
    (245, 244, 246), (245, 245, 245), (245, 246, 245), (245, 246, 244), (244, 246, 243), (243, 246, 242),
    (242, 245, 241), (241, 245, 240), (240, 245, 239), (239, 245, 238), (238, 245, 236), (237, 244, 235),
    (236, 244, 234), (235, 244, 233), (234, 244, 232), (234, 243, 231), (233, 243, 230), (232, 243, 229),
    (231, 243, 228), (230, 243, 227), (229, 242, 226), (228, 242, 224), (227, 242, 223), (226, 242, 222),
    (225, 242, 221), (224, 241, 220), (224, 241, 219), (223, 241, 218), (222, 241, 217), (221, 241, 216),
    (220, 240, 215), (219, 240, 213), (218, 240, 212), (217, 240, 211), (216, 239, 210), (214, 239, 208),
    (213, 238, 207), (211, 237, 205), (210, 237, 204), (208, 236, 202), (206, 235, 200), (203, 234, 197),
    (202, 233, 196), (200, 233, 194), (199, 232, 193), (197, 231, 191), (195, 231, 189), (194, 230, 188),
    (192, 230, 186), (191, 229, 185), (189, 228, 183), (188, 228, 182), (186, 227, 180), (185, 226, 179),
    (183, 226, 177), (181, 225, 175), (180, 224, 174), (178, 224, 172), (177, 223, 171), (175, 222, 169),
    (174, 222, 168), (172, 221, 166), (171, 221, 165), (169, 220, 163), (167, 219, 161), (166, 218, 160),
    (164, 217, 158), (161, 216, 156), (159, 215, 154), (157, 213, 152), (155, 212, 150), (152, 211, 148),
    (150, 209, 147), (148, 208, 145), (145, 207, 143), (143, 205, 141), (139, 203, 138), (136, 201, 135),
    (133, 199, 133), (131, 198, 131), (128, 197, 129), (126, 195, 127), (124, 194, 125), (121, 192, 123),
    (119, 191, 121), (117, 190, 119), (115, 188, 117), (112, 187, 115), (110, 186, 113), (108, 184, 111),
    (105, 183, 110), (103, 181, 108), (101, 180, 106), ( 98, 179, 104), ( 96, 177, 102), ( 94, 176, 100),
    ( 91, 175,  98), ( 89, 173,  97), ( 87, 172,  95), ( 85, 170,  94), ( 83, 168,  92), ( 81, 167,  91),
    ( 80, 165,  90), ( 78, 163,  89), ( 76, 162,  87), ( 74, 160,  86), ( 72, 158,  85), ( 70, 157,  83),
    ( 68, 155,  82), ( 66, 153,  81), ( 64, 152,  80), ( 62, 150,  78), ( 60, 149,  77), ( 58, 147,  76),
    ( 56, 145,  74), ( 53, 142,  72), ( 50, 140,  70), ( 48, 138,  69), ( 46, 137,  68), ( 44, 135,  66),
    ( 43, 133,  65), ( 41, 132,  64), ( 39, 130,  63), ( 37, 128,  61), ( 35, 127,  60), ( 33, 125,  59),
    ( 31, 123,  58), ( 29, 122,  56), ( 28, 120,  55), ( 26, 118,  54),
], np.uint8)
# --- PRGN_TRUNC end ---


def check_params(vmin=0.0, vmax=1.0, alpha=RENDER_ALPHA, interpolation='none'):
    """The scalars of one render, checked: -> (vmin float32, inv float32 = 1 / (vmax - vmin) computed in float32, A =
    round(alpha * 256), mode = index of ``interpolation``).  ValueError for vmin >= vmax, a non-finite bound, a span whose
    float32 reciprocal is not a normal number, alpha outside [0, 1], an unknown interpolation."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f'interpolation must be one of {INTERPOLATIONS}, not {interpolation!r}')
    try:
        with np.errstate(over='ignore'):
            lo, hi, al = np.float32(vmin), np.float32(vmax), float(alpha)
    except (TypeError, ValueError):
        raise ValueError('vmin, vmax and alpha must be numbers') from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f'vmin and vmax must be finite float32 numbers, not {vmin!r}, {vmax!r}')
    if not lo < hi:
        raise ValueError(f'need vmin < vmax, not {vmin!r} >= {vmax!r}')
    with np.errstate(over='ignore', divide='ignore'):
        span = np.float32(hi - lo)
        inv = np.float32(1.0) / span
    if not (np.isfinite(span) and np.isfinite(inv) and inv >= np.finfo(np.float32).tiny):
        raise ValueError(f'the span vmax - vmin = {span!r} has no normal float32 reciprocal')
    if not (np.isfinite(al) and 0.0 <= al <= 1.0):
        raise ValueError(f'alpha must lie in [0, 1], not {alpha!r}')
    return lo, np.float32(inv), int(np.floor(al * RENDER_ALPHA_ONE + 0.5)), INTERPOLATIONS.index(interpolation)


def lut_from(cmap=None):
    """A colour table: None -> ``PRGN_TRUNC``; a uint8 [256, 3] array -> itself; a matplotlib colormap -> ``cmap(np.arange(256),
    bytes=True)[:, :3]`` (a colormap with another number of entries is sampled at ``np.linspace(0, 1, 256)``).  ValueError for anything else."""
    if cmap is None:
        return PRGN_TRUNC
    if callable(cmap) and hasattr(cmap, 'N'):                               # a matplotlib colormap (matplotlib is the caller's)
        rgba = np.asarray(cmap(np.arange(256) if cmap.N == 256 else np.linspace(0.0, 1.0, 256), bytes=True))
        return np.ascontiguousarray(rgba[:, :3], np.uint8)
    a = np.asarray(cmap)
    if a.dtype != np.uint8 or a.shape != (256, 3):
        raise ValueError(f'a colour table is uint8 [256, 3], not {a.dtype} {list(a.shape)}')
    return np.ascontiguousarray(a)


def _axis_u(n_out, extent0, stride, extract_px):
    """Grid coordinate of every output pixel centre along one axis, float64: ((x + 0.5) * extent0 / n_out - extract_px / 2) /
    stride + 0.5, evaluated left to right."""
    x = np.arange(n_out, dtype=np.float64)
    return ((x + 0.5) * float(extent0) / float(n_out) - float(extract_px) / 2.0) / float(stride) + 0.5


def _axis_table(n_cells, n_out, extent0, stride, extract_px, bicubic):
    u = _axis_u(n_out, extent0, stride, extract_px)
    fl = np.floor(u)
    inside = (u >= 0.0) & (u < float(n_cells))
    cell = np.where(inside, fl, -1.0).astype(np.int32)
    if not bicubic:
        return cell
    s = u - 0.5
    i0 = np.floor(s)
    f = s - i0
    # Catmull-Rom (a = -0.5), Horner form as DESIGN.md states it
    w = np.stack([((-0.5 * f + 1.0) * f - 0.5) * f,
                  (1.5 * f - 2.5) * f * f + 1.0,
                  ((-1.5 * f + 2.0) * f + 0.5) * f,
                  (0.5 * f - 0.5) * f * f], 1)
    wi = np.floor(w * RENDER_WEIGHT_ONE + 0.5).astype(np.int64)
    # the rounding's deficit goes to the largest weight (the first of equals)
    k = np.argmax(wi, 1)
    wi[np.arange(n_out), k] += RENDER_WEIGHT_ONE - wi.sum(1)
    taps = np.clip(i0[:, None] + np.arange(-1, 3, dtype=np.float64)[None, :], 0, n_cells - 1)
    out = np.empty((n_out, RENDER_ENTRY), np.int32)
    out[:, 0] = cell
    out[:, 1:5] = taps.astype(np.int32)
    out[:, 5:9] = wi
    return out


def render_tables(gw, gh, W, H, slide_w0, slide_h0, stride, extract_px, interpolation='none'):
    """The geometry of one render as the two tables ``Engine.heatmap_render`` takes (DESIGN.md "Heatmap output", Geometry):
    cell (gx, gy) of the ``gh`` x ``gw`` grid is the ``stride`` x ``stride`` level-0 square centred on its tile's centre ``gx *
    stride + extract_px / 2``; output pixel x of a ``W`` x ``H`` picture of the ``slide_w0`` x ``slide_h0`` slide has grid
    coordinate ``u = ((x + 0.5) * slide_w0 / W - extract_px / 2) / stride + 0.5``.  -> (col, row): 'none' int32 [W] / [H], the
    cell ``floor(u)`` or -1 outside [0, gw); 'bicubic' int32 [W, 9] / [H, 9] = that cell, the four cells ``floor(u - 0.5) - 1
    .. + 2`` clamped to the grid and their Catmull-Rom weights with 12 fractional bits, each group summing to 4096."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f'interpolation must be one of {INTERPOLATIONS}, not {interpolation!r}')
    gw, gh, W, H = int(gw), int(gh), int(W), int(H)
    if not (1 <= W <= RENDER_MAX_PX and 1 <= H <= RENDER_MAX_PX):
        raise ValueError(f'a render is 1 .. {RENDER_MAX_PX} pixels a side, not {W} x {H}')
    if gw < 1 or gh < 1:
        raise ValueError(f'empty grid {gh} x {gw}')
    if not (float(slide_w0) > 0 and float(slide_h0) > 0 and float(stride) > 0 and float(extract_px) > 0):
        raise ValueError('slide_w0, slide_h0, stride and extract_px must be positive')
    bicubic = interpolation == 'bicubic'
    return (_axis_table(gw, W, slide_w0, stride, extract_px, bicubic), _axis_table(gh, H, slide_h0, stride, extract_px, bicubic))
