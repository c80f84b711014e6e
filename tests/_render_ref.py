"""The heatmap's output stage restated in numpy from DESIGN.md "Heatmap output": geometry tables, the value-to-q step, both
interpolation modes and the blend.  Written from the contract; shares no code with ``biscuit_amd/render.py`` or the kernel
(tables in plain Python floats -- IEEE double, the contract's expressions in its order --, pixels in plain loops over integers)."""
import math

import numpy as np

MASKED = -1.0


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def axis_u(x, n_out, extent0, stride, extract_px):
    return ((x + 0.5) * float(extent0) / float(n_out) - float(extract_px) / 2.0) / float(stride) + 0.5


def axis_cells(n_cells, n_out, extent0, stride, extract_px):
    """'none': floor(u), or -1 outside [0, n_cells)."""
    out = []
    for x in range(n_out):
        u = axis_u(float(x), n_out, extent0, stride, extract_px)
        out.append(int(math.floor(u)) if 0.0 <= u < float(n_cells) else -1)
    return np.array(out, np.int32)


def axis_taps(n_cells, n_out, extent0, stride, extract_px):
    """'bicubic': (cells int [n, 4] clamped to the grid, weights int [n, 4] summing to 4096)."""
    cells, weights = [], []
    for x in range(n_out):
        s = axis_u(float(x), n_out, extent0, stride, extract_px) - 0.5
        i0 = math.floor(s)
        f = s - i0
        w = [((-0.5 * f + 1.0) * f - 0.5) * f,
             (1.5 * f - 2.5) * f * f + 1.0,
             ((-1.5 * f + 2.0) * f + 0.5) * f,
             (0.5 * f - 0.5) * f * f]
        wi = [int(math.floor(v * 4096.0 + 0.5)) for v in w]
        wi[wi.index(max(wi))] += 4096 - sum(wi)
        cells.append([min(max(int(i0) + k, 0), n_cells - 1) for k in (-1, 0, 1, 2)])
        weights.append(wi)
    return np.array(cells, np.int64), np.array(weights, np.int64)


def tables(gw, gh, W, H, slide_w0, slide_h0, stride, extract_px, interpolation):
    """The two tables in the layout ``render.render_tables`` documents."""
    col, row = axis_cells(gw, W, slide_w0, stride, extract_px), axis_cells(gh, H, slide_h0, stride, extract_px)
    if interpolation == 'none':
        return col, row
    out = []
    for cell, (c, w) in ((col, axis_taps(gw, W, slide_w0, stride, extract_px)), (row, axis_taps(gh, H, slide_h0, stride, extract_px))):
        out.append(np.concatenate([cell[:, None], c, w], 1).astype(np.int32))
    return tuple(out)


# ---- value -> q ----------------------------------------------------------------------------------------------------------------
def cell_q(values, vmin, vmax):
    """int64 [gh, gw]: q of every live cell, -1 for a cell that is MASKED or not finite."""
    v = np.asarray(values, np.float32)
    lo = np.float32(vmin)
    inv = np.float32(1.0) / np.float32(np.float32(vmax) - lo)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (v - lo).astype(np.float32) * inv                               # two float32 roundings
        s = np.floor(t.astype(np.float32) * np.float32(65536.0))
    live = np.isfinite(v) & (v != np.float32(MASKED))
    q = np.clip(np.where(live, s, 0.0), 0.0, 65535.0).astype(np.int64)
    return np.where(live, q, -1)


# ---- the picture ---------------------------------------------------------------------------------------------------------------
def render(values, thumb, lut, slide_w0, slide_h0, stride, extract_px, vmin=0.0, vmax=1.0, alpha=0.6, interpolation='none'):
    values = np.asarray(values, np.float32)
    gh, gw = values.shape
    H, W = thumb.shape[:2]
    A = int(math.floor(alpha * 256 + 0.5))
    q = cell_q(values, vmin, vmax)
    cx, cy = axis_cells(gw, W, slide_w0, stride, extract_px), axis_cells(gh, H, slide_h0, stride, extract_px)
    own = np.where((cy[:, None] >= 0) & (cx[None, :] >= 0), q[np.maximum(cy, 0)[:, None], np.maximum(cx, 0)[None, :]], -1)   # [H, W]
    drawn = own >= 0
    if interpolation == 'none':
        Q = own
    else:
        assert interpolation == 'bicubic'
        tx, wx = axis_taps(gw, W, slide_w0, stride, extract_px)
        ty, wy = axis_taps(gh, H, slide_h0, stride, extract_px)
        num = np.zeros((H, W), np.int64)
        S = np.zeros((H, W), np.int64)
        for j in range(4):
            for i in range(4):
                qq = q[ty[:, j][:, None], tx[:, i][None, :]]
                w = wy[:, j][:, None] * wx[:, i][None, :]
                livetap = qq >= 0
                num += np.where(livetap, w * qq, 0)
                S += np.where(livetap, w, 0)
        pos = S > 0
        Sd = np.where(pos, S, 1)
        Q = np.where(pos, np.clip((num + Sd // 2) // Sd, 0, 65535), own)
    colour = np.asarray(lut, np.uint8)[np.clip(Q, 0, 65535) >> 8].astype(np.int64)              # [H, W, 3]
    blend = (A * colour + (256 - A) * thumb.astype(np.int64) + 128) >> 8
    return np.where(drawn[:, :, None], blend, thumb).astype(np.uint8)
