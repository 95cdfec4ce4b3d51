"""Plain float64 numpy restatements of the operations of csrc/preproc.hip (MRC reorder, per-slice statistics, z-score, 8-bit
quantise + min-max) and csrc/crop_norm.hip (raw, sum-z / min-max, z-normalised and chain crops with clamped reads, the table
form, the 8-bit round trip).  No torch, no library call: tests/test_data_path_ref_cpu.py proves every function here against
the oracle (oracle/preproc_ref.py, oracle/infer_ref.py) and the committed fixtures, tests/test_data_path_gpu.py measures the
kernels against them.  What the oracle already states is taken from it (`u8_roundtrip_normalize`).

The seeded inputs both test modules use are made here too, so that what the CPU module proves about them (the share of
voxels next to a rounding tie) is a property of the very arrays the GPU module feeds the kernels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.infer_ref import u8_roundtrip_normalize       # noqa: E402,F401

ORDERS = ("xyz", "xzy", "yxz", "zxy")
MRC_DTYPES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}
RAW, SUMZ_MINMAX, ZNORM, CHAIN = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------
# loader
# ------------------------------------------------------------------------------------------------
def reorder(rec, order, compress=False):
    """out[j][a][b] of loader.py `load_rec` in front of its z-score, as float32: the file's (d0, d1, d2) block with the
    slice axis first, then (compress) the maximum of slices (2j, 2j + 1), the last one alone when the count is odd.
    zxy + compress with an odd count overruns in the reference: IndexError."""
    axes = {"xyz": (2, 0, 1), "xzy": (1, 0, 2), "yxz": (2, 1, 0), "zxy": (0, 1, 2)}[order]
    r = np.transpose(np.asarray(rec), axes)
    if compress:
        if order == "zxy" and r.shape[0] % 2:
            raise IndexError("zxy + compress with an odd slice count")
        r = np.stack([r[i:i + 2].max(0) for i in range(0, r.shape[0], 2)])
    return np.ascontiguousarray(r).astype(np.float32)


def slice_stats(x):
    """(n, e) -> (n, 4) float64 {mean, population std, min, max}; a NaN in a slice makes all four of its values NaN"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([x.mean(1), x.std(1), x.min(1), x.max(1)], 1)


def zscore(x):
    """(n, e) -> float64 (x - mean) / std of each slice (a constant slice: 0 / 0 = NaN)"""
    x = np.asarray(x, np.float64)
    st = slice_stats(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - st[:, :1]) / st[:, 1:2]


def quantize_levels(x, mi=-2.5, ma=2.0):
    """(n, e) -> (q, t): t = clip(255 (z - mi) / (ma - mi), 0, 255) of the z-score z, q = round-half-even(t)"""
    t = np.clip(255.0 * (zscore(x) - mi) / (ma - mi), 0.0, 255.0)
    return np.round(t), t


def preprocess(x, mi=-2.5, ma=2.0, flat_zero=False):
    """(n, e) -> float64 (q - qmin) / (qmax - qmin) per slice; a slice whose levels are all equal (or NaN) gives NaN, or
    0 with flat_zero"""
    q, _ = quantize_levels(x, mi, ma)
    with np.errstate(invalid="ignore", divide="ignore"):
        lo, hi = q.min(1, keepdims=True), q.max(1, keepdims=True)
        out = (q - lo) / (hi - lo)
    if flat_zero:
        out = np.where(hi - lo > 0, out, 0.0)
    return out


def tie_adjacent(t, margin=1e-9):
    """True where the pre-rounding value lies within `margin` of a half-integer (NaN: False)"""
    with np.errstate(invalid="ignore"):
        return np.abs(t - np.floor(t) - 0.5) <= margin


# ------------------------------------------------------------------------------------------------
# crops
# ------------------------------------------------------------------------------------------------
def crop_indices(c, s, n):
    """the window [c - s // 2, c - s // 2 + s) along an axis of extent n, every index clamped into the axis"""
    return np.clip(np.arange(c - s // 2, c - s // 2 + s), 0, n - 1)


def crop_raw(vol, centre, size, flip_x=False):
    """centre = (x, y, z), size = (cz, cy, cx) -> float64 (cz, cy, cx)"""
    vol = np.asarray(vol)
    x, y, z = (int(v) for v in centre)
    cz, cy, cx = size
    iz, iy, ix = crop_indices(z, cz, vol.shape[0]), crop_indices(y, cy, vol.shape[1]), crop_indices(x, cx, vol.shape[2])
    sub = vol[np.ix_(iz, iy, ix)].astype(np.float64)
    return sub[:, :, ::-1] if flip_x else sub


def minmax01(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a - a.min()) / (a.max() - a.min())


def znorm(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a - a.mean()) / a.std(ddof=1)


def crop(vol, centre, size, mode, flip_x=False):
    """one crop of mi_crop_normalize in float64: (cy, cx) for SUMZ_MINMAX, else (cz, cy, cx)"""
    sub = crop_raw(vol, centre, size, flip_x)
    if mode == RAW:
        return sub
    if mode == SUMZ_MINMAX:
        return minmax01(sub.sum(0))
    if mode == ZNORM:
        return znorm(sub)
    return znorm(minmax01(znorm(sub)) * 6.0 - 3.0)


def crops(vol, centres, size, mode, flip_x=False):
    return np.stack([crop(vol, c, size, mode, flip_x) for c in centres])


def sumz_minmax_f32(vol, centre, size, flip_x=False):
    """SUMZ_MINMAX with every operation rounded to float32, slices added in ascending z"""
    sub = crop_raw(vol, centre, size, flip_x).astype(np.float32)
    s = np.zeros(sub.shape[1:], np.float32)
    for z in range(sub.shape[0]):
        s = s + sub[z]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s - s.min()) / (s.max() - s.min())


def table_crops(vols, owner, centres, shift, order, first, n, size, mode, flip_x=False):
    """mi_crop_normalize_table: crop k is sample i = order[first + k] (order None: first + k) - gather the sample's volume
    (owner None: volume 0), centre + shift (shift None: the centre), then crop"""
    out = []
    for k in range(n):
        i = int(order[first + k]) if order is not None else first + k
        c = np.asarray(centres[i], np.int64) + (np.asarray(shift[i], np.int64) if shift is not None else 0)
        out.append(crop(vols[int(owner[i]) if owner is not None else 0], c, size, mode, flip_x))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and the GPU module
# ------------------------------------------------------------------------------------------------
STAT_SHAPES = [(1, 1), (1, 255), (3, 257), (2, 65536), (2, 65537), (3, 131077), (1, 1048876)]


def slices(n, e, mean=100.0, sigma=7.0):
    """(n, e) float32 N(mean, sigma), the loader tests' own distribution"""
    rng = np.random.default_rng(1000 * n + e)
    return (rng.standard_normal((n, e)) * sigma + mean).astype(np.float32)


def quantiser_slices(n, e):
    """the quantiser cases: `slices`, and at (3, 257) slice 1 constant"""
    x = slices(n, e)
    if (n, e) == (3, 257):
        x[1] = 97.25
    return x


def hot_pixel_cases():
    """{name: (n, e) float32}: the shifted-sum variance takes K = element 0 of the slice; here that element is an outlier"""
    a = slices(3, 131077)
    a[1, 0] = 32767.0
    rng = np.random.default_rng(16)
    b = np.round(rng.standard_normal((2, 65537)) * 50.0 + 100.0).astype(np.int16)
    b[:, 0] = 32767
    return {"N(100, 7), slice 1 voxel 0 = 32767": a, "int16 sigma 50, voxel 0 = 32767": b.astype(np.float32)}


def volume(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 7.0 + 100.0).astype(np.float32)


def centres16(shape, size, seed, keep_y=False):
    """16 centres (x, y, z) int32 for crops of `size` from a (D, H, W) volume: four outside the volume by up to a full
    window on each axis (one of them on all three: that window is constant), four on faces and corners, eight inside.
    keep_y: y stays where at least two different rows of the volume are read, so that no window is constant."""
    D, H, W = shape
    cz, cy, cx = size
    rng = np.random.default_rng(seed)
    c = [(-cx, H // 2, D // 2), (W - 1 + cx, -cy, D - 1 + cz), (W // 2, H - 1 + cy, -cz), (-1, -1, D),
         (0, 0, 0), (W - 1, H - 1, D - 1), (0, H // 3, D - 1), (W // 2, H - 1, 0)]
    c += [(int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, D))) for _ in range(8)]
    c = np.asarray(c, np.int32)
    if keep_y:          # the window's last row >= 1 and its first row <= H - 2
        c[:, 1] = np.clip(c[:, 1], 2 - cy + cy // 2, H - 2 + cy // 2)
    return c
