"""float64 numpy restatement of the f16 range screen (kernels_screen.hip): the key of a tile and the
candidate slots' update rule.  Used by tests/test_range_screen.py and tests/test_gpu_range_screen.py."""
import numpy as np

PX = 299
N = PX * PX * 3


def range_key(tiles):
    """uint8 [n,299,299,3] -> float32 [n]: max(hi - mu, mu - lo) / max(sd, 1/sqrt(N)), mu / sd from the exact integer sums in
    float64, one rounding to float32 at the end (no fused operations: numpy has none)."""
    t = np.asarray(tiles, np.uint8).reshape(len(tiles), -1)
    out = np.empty(len(t), np.float32)
    n = np.float64(t.shape[1])
    for i, x in enumerate(t):
        s1 = int(x.sum(dtype=np.int64))
        s2 = int((x.astype(np.int64) ** 2).sum())
        mu = np.float64(s1) / n
        var = np.float64(s2) / n - mu * mu
        if var < 0:
            var = np.float64(0)
        sd, floor_sd = np.sqrt(var), np.float64(1.0) / np.sqrt(n)
        den = sd if sd > floor_sd else floor_sd
        a, b = np.float64(int(x.max())) - mu, mu - np.float64(int(x.min()))
        out[i] = np.float32((a if a > b else b) / den)
    return out


def standardised_peak(tiles):
    """The same number the long way: per_image_standardization of every value in float64, then max |value|."""
    t = np.asarray(tiles, np.float64).reshape(len(tiles), -1)
    mu = t.mean(axis=1, keepdims=True)
    sd = np.maximum(t.std(axis=1, keepdims=True), 1.0 / np.sqrt(t.shape[1]))
    return np.abs((t - mu) / sd).max(axis=1)


def screen_update(slots, batch, k):
    """One update of the k candidate slots.  slots: list of the filled slots' entries (key, global index, payload), a prefix of the
    slot array; batch: the batch's entries in row order.  Keeps the top k of (slots + batch) by key descending, global index
    ascending, earlier position first (a total order); survivors keep their slot, the admitted batch entries take the freed slots
    in rank order, lowest first.  Returns the new list of filled slots."""
    union = list(slots) + list(batch)
    order = sorted(range(len(union)), key=lambda e: (-float(union[e][0]), int(union[e][1]), e))[:k]
    m = len(slots)
    out = [None] * k
    for e in order:
        if e < m:
            out[e] = union[e]
    free = iter([s for s in range(k) if out[s] is None])
    for e in order:
        if e >= m:
            out[next(free)] = union[e]
    filled = min(k, len(union))
    assert all(x is not None for x in out[:filled]) and all(x is None for x in out[filled:])
    return out[:filled]


def top_k(entries, k):
    """The k best entries of a whole interval by (key desc, global index asc)."""
    return sorted(entries, key=lambda x: (-float(x[0]), int(x[1])))[:k]
