"""numpy restatements of what csrc/vis3d.hip and utils/vis3d.py compute (test infrastructure only; float64 throughout):
the colour sampler, the volume chain of visualize_3dhm, the disc painter and the 8-bit Gaussian - and scipy's own filter,
the oracle the Gaussian restatement is pinned to."""
import numpy as np

SIGMA, RADIUS = 0.8, 3


def default_colormap():
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([i, j, 255 - (i + j) // 2], -1).astype(np.uint8)


def sample_colours(y01, table):
    """table[clamp(round(x (W - 1)), 0, W - 1), clamp(round(y (H - 1)), 0, H - 1)] per row of y01 (fp32 -> float64 first);
    np.rint is Python's round on a float64: half to even."""
    y = np.asarray(y01, np.float32).astype(np.float64)
    w, h = table.shape[:2]
    ix = np.clip(np.rint(y[:, 0] * (w - 1)), 0, w - 1).astype(np.int64)
    iy = np.clip(np.rint(y[:, 1] * (h - 1)), 0, h - 1).astype(np.int64)
    return table[ix, iy]


def sample_colours_direct(y01, table):
    """The sampling rule written out pick by pick with Python's own round / min / max on Python floats."""
    w, h = table.shape[:2]
    out = np.zeros((len(y01), 3), np.uint8)
    for n, (x, y) in enumerate(np.asarray(y01, np.float32)):
        sx = (float(x) - 0.0) * (float(w - 1) - 0.0) / (1.0 - 0.0) + 0.0
        sy = (float(y) - 0.0) * (float(h - 1) - 0.0) / (1.0 - 0.0) + 0.0
        out[n] = table[int(min(w - 1, max(0, round(sx)))), int(min(h - 1, max(0, round(sy))))]
    return out


def reorder(rec, order, compress):
    """(Z, R, C) float64 of an MRC data block: the axis order, then the max of every two slices (even z only)."""
    rec = np.asarray(rec, np.float64)
    if order == "xzy":
        rec = np.swapaxes(rec, 2, 1)
    if order == "yxz":
        rec = np.swapaxes(rec, 1, 0)
    vol = rec if order == "zxy" else np.moveaxis(rec, 2, 0)
    if compress:
        assert vol.shape[0] % 2 == 0
        vol = np.maximum(vol[0::2], vol[1::2])
    return np.ascontiguousarray(vol)


def _quantize_level(x, mi=-2.5, ma=3.0):
    return np.clip(255.0 * (x - mi) / (ma - mi), 0, 255)


def volume_chain(vol):
    """(bytes (Z, R, C) uint8, pre-round levels (Z, R, C) float64) of a reordered float64 volume: per slice z-score,
    quantize(-2.5, 3), min-max to [0, 1]; global min-max, global z-score; per slice z-score, quantize(-2.5, 3).  A slice of
    zero variance (one value; its computed deviation is rounding noise, not 0) gives 0 at every step."""
    vol = np.asarray(vol, np.float64)
    unit = np.zeros_like(vol)
    for s, sl in enumerate(vol):
        if sl.max() > sl.min():
            q = np.round(_quantize_level((sl - sl.mean()) / sl.std()))
            unit[s] = (q - q.min()) / (q.max() - q.min()) if q.max() > q.min() else 0.0
    if unit.max() > unit.min():
        unit = (unit - unit.min()) / (unit.max() - unit.min())
        unit = (unit - unit.mean()) / unit.std()
    level = np.zeros_like(vol)
    for s, sl in enumerate(unit):
        if sl.max() > sl.min():
            level[s] = _quantize_level((sl - sl.mean()) / sl.std())
    return np.round(level).astype(np.uint8), level


def tomogram_picks(coords, names, use_name):
    rows = np.flatnonzero(np.asarray(names) == use_name)
    c = np.asarray(coords, np.float64)[rows]
    return rows, np.concatenate([np.trunc(c[:, :2]), c[:, 2:3]], 1).astype(np.int64)


def paint(picks, colours, shape):
    """(Z, R, C, 3) uint8.  picks (n, 3) integers (column, row, slice) in input order.  A slice that holds a pick takes, pick by
    pick in input order (so the last one stays on top), the disc of radius 12 - |dz| of every pick within 2 slices."""
    z, r, c = shape
    out = np.zeros((z, r, c, 3), np.uint8)
    picks = np.asarray(picks, np.int64)
    for s in np.unique(picks[:, 2]):
        near = np.flatnonzero(np.abs(picks[:, 2] - s) <= 2)
        for (x, y, pz), colour in zip(picks[near], colours[near]):
            r0, r1, c0, c1 = max(y - 12, 0), min(y + 13, r), max(x - 12, 0), min(x + 13, c)     # the disc's box, clipped
            if r0 < r1 and c0 < c1:
                rows, cols = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing="ij")
                out[s, r0:r1, c0:c1][(cols - x) ** 2 + (rows - y) ** 2 <= (12 - abs(pz - s)) ** 2] = colour
    return out


def gaussian_weights(sigma=SIGMA, radius=RADIUS):
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def _pass(a, axis, w):
    """One 1-D pass over uint8 `a`: `reflect` borders, the float64 sum in scipy's order, floor to uint8."""
    n = a.shape[axis]
    idx = np.arange(-RADIUS, n + RADIUS) % (2 * n)
    idx = np.where(idx < n, idx, 2 * n - 1 - idx)
    p = np.take(a, idx, axis=axis).astype(np.float64)
    tap = lambda k: np.take(p, np.arange(n) + RADIUS + k, axis=axis)
    t = tap(0) * w[RADIUS]
    for k in range(RADIUS):
        t = t + (tap(-(RADIUS - k)) + tap(RADIUS - k)) * w[k]
    return np.floor(t).astype(np.uint8)


def gaussian_u8(vol):
    """(Z, R, C, 3) uint8 of a (Z, R, C) uint8 volume: the three equal channels, then the passes along z, rows, columns and
    the channel axis, each floored to uint8."""
    a = np.stack([np.asarray(vol, np.uint8)] * 3, -1)
    w = gaussian_weights()
    for axis in range(4):
        a = _pass(a, axis, w)
    return a


def gaussian_scipy(vol):
    """scipy.ndimage.gaussian_filter itself on the stacked bytes, as the reference calls it."""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.stack([np.asarray(vol, np.uint8)] * 3, -1), sigma=SIGMA)
