"""The colour of every pick on the 2-D map and the two volumes of the reference's visualize_3dhm.py, on the MI355X
(csrc/vis3d.hip):

    colours = sample_colours(y01, table)                 # (N, 3) uint8: plot_2d's all_colors.npy
    vol = load_volume(path, order="xzy", compress=False) # (Z, R, C) fp32 on the device
    rec = rec3d(vol)                                     # (Z, R, C, 3) uint8: {name}_rec3d.npy
    picks = tomogram_picks(coords, names, name, Z)       # host: this tomogram's rows, (column, row, slice) int32
    hm = paint(picks, colours_of_them, (Z, R, C))        # (Z, R, C, 3) uint8: {name}_hm3d_simsiam.npy

The default colour table is NOT one of the reference's (those are its data files): it is generated arithmetically,
table[i, j] = (i, j, 255 - (i + j) // 2).  `load_colormap` takes any (W, H, 3) uint8 .npy, the Ziegler table of a reference
installation for instance.  Differences from the reference in the volumes: fp32 storage between the steps as utils/loader.py
has it, a slice of zero variance gives bytes 0 (the reference casts NaN), and the disc is dx^2 + dy^2 <= r^2, whose rim
pixels may differ from cv2.circle's.  There is no CPU path.
"""
import numpy as np
import torch

from .. import _lib as L
from . import loader as Ld
from . import mrc as _mrc

SIGMA, RADIUS = 0.8, 3                    # gaussian_filter(sigma=0.8): truncate 4.0 -> radius int(4 * 0.8 + 0.5) = 3
QUANT_MI, QUANT_MA = -2.5, 3.0            # visualize_3dhm.py's own quantize defaults
DISC_RADIUS, DISC_REACH = 12, 2
INDEX_BUDGET_BYTES = 1 << 30              # the painter's index image is made slab by slab above this


def default_colormap():
    """(256, 256, 3) uint8, table[i, j] = (i, j, 255 - (i + j) // 2): not a colour table of the reference."""
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([i, j, 255 - (i + j) // 2], -1).astype(np.uint8)


def load_colormap(path=None):
    """The (W, H, 3) uint8 table of a .npy file; the default table without a path."""
    if path is None:
        return default_colormap()
    table = np.load(path)
    if table.ndim != 3 or table.shape[2] != 3 or table.dtype != np.uint8 or 0 in table.shape:
        raise ValueError("%s: a colour table is a (W, H, 3) uint8 array, got %s %s" % (path, table.shape, table.dtype))
    return np.ascontiguousarray(table)


def sample_colours(y01, table):
    """(N, 3) uint8 device tensor: table[clamp(round(x (W - 1))), clamp(round(y (H - 1)))] of every row (x, y) of y01."""
    y01 = L.require_cuda(y01, "y01").contiguous()
    if y01.ndim != 2 or y01.shape[1] != 2:
        raise ValueError("y01 must be (N, 2), got %s" % (tuple(y01.shape),))
    if isinstance(table, np.ndarray):
        table = torch.from_numpy(np.ascontiguousarray(table)).to(y01.device)
    table = L.require_cuda(table, "table", torch.uint8).contiguous()
    if table.ndim != 3 or table.shape[2] != 3:
        raise ValueError("table must be (W, H, 3) uint8, got %s" % (tuple(table.shape),))
    out = torch.empty((y01.shape[0], 3), dtype=torch.uint8, device=y01.device)
    L.call("mi_vis_sample_colours", y01, y01.shape[0], table, table.shape[0], table.shape[1], out)
    return out


def gaussian_weights(sigma=SIGMA, radius=RADIUS):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius): (2 radius + 1,) float64."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gaussian_u8(vol):
    """(Z, R, C, 3) uint8 = scipy.ndimage.gaussian_filter(np.stack([vol] * 3, -1), sigma=0.8) of a (Z, R, C) uint8 device tensor."""
    vol = L.require_cuda(vol, "vol", torch.uint8).contiguous()
    if vol.ndim != 3 or 0 in vol.shape:
        raise ValueError("vol must be a non-empty (Z, R, C) volume, got %s" % (tuple(vol.shape),))
    z, r, c = vol.shape
    lib = L.lib()
    out = torch.empty((z, r, c, 3), dtype=torch.uint8, device=vol.device)
    ws = L.workspace(lib.mi_vis_gauss_workspace_bytes(z, r, c), vol.device, "vis3d")
    w = (L._c.c_double * 7)(*gaussian_weights())
    L.call("mi_vis_gauss_u8", vol, z, r, c, L._c.cast(w, L._c.c_void_p), out, ws, ws.numel())
    return out


def reordered_slices(shape, order, compress):
    """Z of load_volume for an MRC data block of `shape`, from the shape alone.  visualize_3dhm.py allocates int(z // 2)
    slices for every order and walks range(0, z, 2), so an odd z with --compress overruns there: ValueError here."""
    if order not in Ld.ORDERS:
        raise ValueError("order must be one of %s" % sorted(Ld.ORDERS))
    d0, d1, d2 = (int(s) for s in shape)
    z = {"xyz": d2, "xzy": d1, "yxz": d2, "zxy": d0}[order]
    if compress and z % 2:
        raise ValueError("--compress needs an even number of slices: this tomogram has %d along z (order %s), and the "
                         "reference's visualize_3dhm allocates z // 2 slices for every order" % (z, order))
    return z // 2 if compress else z


def load_volume(path, order="xzy", compress=False):
    """visualize_3dhm.py:30-47 up to the first per-slice step: the axis reorder (+ z-pair max) -> (Z, R, C) fp32 on the device.
    `path` may also be an already-read (nz, ny, nx) array."""
    rec = _mrc.open_data(path) if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__") else np.asarray(path)
    if rec.ndim != 3:
        raise ValueError("a 3-D MRC data block is required, got shape %s" % (rec.shape,))
    reordered_slices(rec.shape, order, compress)
    return Ld.rec_to_device(rec, order, compress)


def volume_bytes(vol):
    """The reference's chain from the reordered volume to the bytes it smooths (visualize_3dhm.py:48-64,:126-130): per slice
    z-score, quantize(-2.5, 3), min-max to [0, 1]; then, per slice again, z-score and quantize(-2.5, 3) to a byte.  The global
    min-max and z-score in between (:63-64) are one increasing affine map of the whole volume, which the per-slice z-score
    behind them takes out again, so they are not run.  (Z, R, C) fp32 -> (Z, R, C) uint8."""
    v = L.require_cuda(vol, "vol").contiguous()
    if v.ndim != 3 or 0 in v.shape:
        raise ValueError("vol must be a non-empty (Z, R, C) volume, got %s" % (tuple(v.shape),))
    z, e = v.shape[0], v[0].numel()
    unit = torch.empty_like(v)
    L.call("mi_zscore_quantize_minmax", v, unit, z, e, Ld._stats(v, z, e), QUANT_MI, QUANT_MA, 1)
    out = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
    L.call("mi_vis_slice_bytes", unit, z, e, Ld._stats(unit, z, e), QUANT_MI, QUANT_MA, out)
    return out


def rec3d(vol):
    """{name}_rec3d.npy of a reordered (Z, R, C) fp32 volume: (Z, R, C, 3) uint8 on the device."""
    return gaussian_u8(volume_bytes(vol))


def tomogram_picks(coords, names, use_name, n_slices):
    """Host step of get_3d_hm (:116-122): (rows of the input that belong to `use_name`, their (column, row, slice) as int32
    with int() truncation of x and y).  ValueError (before anything is launched) for a slice outside [0, n_slices) - the
    reference would index out of range - or a slice that is not a whole number."""
    rows = np.flatnonzero(np.asarray(names) == use_name)
    c = np.asarray(coords, dtype=np.float64).reshape(len(names), -1)[rows]
    if len(rows) == 0:
        return rows, np.zeros((0, 3), np.int32)
    z = c[:, -1]
    if not np.all(np.isfinite(c)) or np.any(z != np.floor(z)):
        raise ValueError("%s: the picks need finite coordinates and whole-numbered slices" % use_name)
    bad = np.flatnonzero((z < 0) | (z >= n_slices))
    if len(bad):
        raise ValueError("%s: pick %d has z = %g outside the volume's %d slices [0, %d)"
                         % (use_name, int(rows[bad[0]]), z[bad[0]], n_slices, n_slices))
    xy = np.clip(np.trunc(c[:, :2]), -2.0 ** 30, 2.0 ** 30)           # (a centre that far out paints nothing either way)
    return rows, np.concatenate([xy, z[:, None]], 1).astype(np.int32)


def paint(picks, colours, shape, device=None, index_budget_bytes=INDEX_BUDGET_BYTES):
    """{name}_hm3d_simsiam.npy: (Z, R, C, 3) uint8 on the device.  picks (n, 3) int32 numpy (column, row, slice) in input order
    as `tomogram_picks` returns them, colours (n, 3) uint8.  Slices that hold a pick are painted, every other stays zero; the
    int32 index image covers those slices only and is made slab by slab when it would exceed `index_budget_bytes`."""
    z, r, c = (int(s) for s in shape)
    picks = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1, 3)
    colours = np.ascontiguousarray(colours, dtype=np.uint8).reshape(-1, 3)
    if len(picks) != len(colours):
        raise ValueError("%d picks but %d colours" % (len(picks), len(colours)))
    if len(picks) and (picks[:, 2].min() < 0 or picks[:, 2].max() >= z):
        raise ValueError("a pick lies outside the volume's %d slices" % z)
    dev = torch.device(device) if device is not None else Ld._dev()
    with torch.cuda.device(dev):
        out = torch.empty((z, r, c, 3), dtype=torch.uint8, device=dev)
        d_picks, d_col = torch.from_numpy(picks).to(dev), torch.from_numpy(colours).to(dev)
        used = np.zeros(z, bool)
        used[picks[:, 2]] = True
        per_slab = max(1, int(index_budget_bytes // (4 * r * c)))
        z0 = 0
        while z0 < z:                                      # a slab ends before its (per_slab + 1)-th painted slice
            over = np.flatnonzero(np.cumsum(used[z0:]) > per_slab)
            nz = int(over[0]) if len(over) else z - z0
            slot = np.full(z, -1, np.int32)
            mine = z0 + np.flatnonzero(used[z0:z0 + nz])
            slot[mine] = np.arange(len(mine), dtype=np.int32)
            d_slot = torch.from_numpy(slot).to(dev)
            index = torch.empty((max(len(mine), 1), r, c), dtype=torch.int32, device=dev)
            L.call("mi_vis_paint", d_picks, d_col, len(picks), d_slot, len(mine), z, r, c, z0, nz, index, out)
            z0 += nz
    return out
