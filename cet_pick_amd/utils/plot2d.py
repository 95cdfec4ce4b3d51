"""The pictures of the 2-D map and the thumbnails of the picks, on the MI355X (csrc/plot2d.hip): the
reference's plot_2d.py:96-103 and :121-218.

    idx = select(y01, thr)                               # (n_shown,) int32 on the device: the picks that get a thumbnail
    thumbs = thumbnails(patches, idx, T=32)              # (n_shown, T, T) uint8
    grey = patch_bytes(patches)                          # (N, b, b) uint8 numpy: the bytes of imgs/{i}.png
    out = draw_out(y01, idx, thumbs, colours, P)         # (P, P, 3) uint8: 2d_visualization_out
    lab = draw_labels(y01, idx, thumbs, labels, P)       # (P, P, 3) uint8: 2d_visualization_labels
    write_png(path, array)                               # host: 8-bit grey, RGB or RGBA
    g = class_gallery(patches, emb, centroids, assign, labels, k)   # per class: mean, std, count, exemplars, and their picture
                                                         # (csrc/class_gallery.hip, DESIGN.md 4.24: this project's own)

What is drawn, in which order and at which data-unit sizes is the reference's; the layout of the canvas (below) is this
project's own: no axes, ticks or tight bounding box.  There is no CPU path.
"""
import struct
import zlib

import numpy as np
import torch

from .. import _lib as L

THUMB = 32                                # the reference's int(rcParams['figure.figsize'][0] * 5) with matplotlib's 6.4
PLOT_SIZE = 1500                          # its figsize 15 in at 100 dpi
MIN_PLOT_SIZE = 128
MARGIN = 48
DISC_RADIUS_UNITS = 0.03                  # Circle(xy, 0.03)
LABEL_DX_UNITS, LABEL_DY_UNITS = 0.025, 0.020             # ax.text(x - 0.025, y + 0.020, ...)
GLYPH_PX, GLYPH_GAP, BOX_PAD, BOX_BORDER = 2, 2, 3, 2
PATCH_BUDGET_BYTES = 1 << 28              # patch_bytes uploads at most this many bytes of patches at a time
GRAY_LUT = (np.linspace(0, 1, 256) * 255).astype(np.uint8)                  # matplotlib's `gray` table as bytes: not the identity
DIGITS_5X7 = np.array([                   # 7 rows of 5 bits per digit, bit 4 the left pixel
    [0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E],
    [0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E],
    [0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F],
    [0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E],
    [0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02],
    [0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E],
    [0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E],
    [0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08],
    [0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E],
    [0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C]], np.uint8)


def layout(P=PLOT_SIZE, T=THUMB):
    """The canvas of a P x P picture with T x T thumbnails, as the dictionary the kernel's mi_plot_layout takes: span
    S = P - 1 - 2 M; disc radius and label offsets are the reference's data units times S, rounded half to even."""
    P, T = int(P), int(T)
    if P < MIN_PLOT_SIZE:
        raise ValueError("a picture is at least %d pixels wide, got %d" % (MIN_PLOT_SIZE, P))
    if P > 16384 or not 1 <= T <= 1024:
        raise ValueError("a picture is at most 16384 pixels wide and a thumbnail 1..1024, got %d and %d" % (P, T))
    S = P - 1 - 2 * MARGIN
    return dict(P=P, M=MARGIN, R=int(round(DISC_RADIUS_UNITS * S)), T=T, label_dx=int(round(LABEL_DX_UNITS * S)),
                label_dy=int(round(LABEL_DY_UNITS * S)), glyph_px=GLYPH_PX, glyph_gap=GLYPH_GAP, box_pad=BOX_PAD,
                box_border=BOX_BORDER)


def _map(y01):
    y01 = L.require_cuda(y01, "y01").contiguous()
    if y01.ndim != 2 or y01.shape[1] != 2:
        raise ValueError("y01 must be (N, 2), got %s" % (tuple(y01.shape),))
    return y01


def _patches(patches):
    shape = tuple(np.shape(patches))
    if len(shape) != 4 or 0 in shape:
        raise ValueError("patches must be a non-empty (N, C, b, b) array, got %s" % (shape,))
    if shape[2] != shape[3]:
        raise ValueError("patches must be square, got %d x %d" % (shape[2], shape[3]))
    return L.require_cuda(patches, "patches").contiguous()


def _index(idx, n, device):
    if isinstance(idx, np.ndarray):
        idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(device)
    idx = L.require_cuda(idx, "idx", torch.int32).contiguous()
    if idx.ndim != 1:
        raise ValueError("idx must be (n_shown,), got %s" % (tuple(idx.shape),))
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError("idx names a pick outside [0, %d)" % n)
    return idx


def select(y01, thr):
    """(n_shown,) int32 device tensor, ascending: the reference's filter.  Pick i is shown unless a pick shown before it (or
    pick 0, which starts the list) lies at a float32 squared distance below thr = float32(--min_dist_vis)."""
    y01 = _map(y01)
    n = y01.shape[0]
    thr = float(np.float32(thr))
    if n and not bool(torch.isfinite(y01).all()):
        raise ValueError("y01 must be finite")
    lib = L.lib()
    shown = torch.empty((max(n, 1),), dtype=torch.int32, device=y01.device)
    count = torch.zeros((1,), dtype=torch.int32, device=y01.device)
    nbytes = lib.mi_plot_select_workspace_bytes(n, thr)
    if n and nbytes == 0:
        raise L.HipExtensionError("mi_plot_select failed: unsupported (%d picks)" % n)
    ws = L.workspace(nbytes, y01.device, "plot2d_select")
    L.call("mi_plot_select", y01, n, thr, shown, count, ws, ws.numel())
    c = int(count.item())
    if c < 0:
        raise L.HipExtensionError("mi_plot_select failed: the cell lists of the selection were corrupted")
    return shown[:c].clone()


def thumbnails(patches, idx, T=THUMB, return_pre=False):
    """(n_shown, T, T) uint8 device tensor: z-score over the whole (C, b, b) patch, quantize(-3, 3), channel 0 resized as
    torchvision 0.12's functional.resize(tensor, T) does.  return_pre: also the (n_shown, C, b, b) bytes before the resize."""
    patches = _patches(patches)
    n, c, b, _ = patches.shape
    idx = _index(idx, n, patches.device)
    m = idx.numel()
    out = torch.empty((m, int(T), int(T)), dtype=torch.uint8, device=patches.device)
    pre = torch.empty((m, c, b, b), dtype=torch.uint8, device=patches.device) if return_pre else None
    L.call("mi_plot_thumbs", patches, n, c, b, idx, m, int(T), out, pre)
    return (out, pre) if return_pre else out


def patch_bytes(patches, lut=GRAY_LUT, device=None, budget_bytes=PATCH_BUDGET_BYTES):
    """(N, b, b) uint8 numpy: the red (= green = blue) channel of plt.imsave(patch[0], cmap='gray') for every pick.  patches
    (N, C, b, b) fp32, numpy or a device tensor; a numpy array goes to the device at most `budget_bytes` at a time."""
    if isinstance(patches, np.ndarray):
        if patches.ndim != 4 or 0 in patches.shape:
            raise ValueError("patches must be a non-empty (N, C, b, b) array, got %s" % (patches.shape,))
        if patches.shape[2] != patches.shape[3]:
            raise ValueError("patches must be square, got %d x %d" % (patches.shape[2], patches.shape[3]))
        if not torch.cuda.is_available():
            raise L.HipExtensionError("patches must go to the MI355X (cuda) device; there is no CPU path")
        from . import loader as Ld
        dev = torch.device(device) if device is not None else Ld._dev()
        per = max(1, int(budget_bytes // (4 * patches[0].size)))
        slabs = (torch.from_numpy(np.ascontiguousarray(patches[i:i + per], dtype=np.float32)).to(dev)
                 for i in range(0, len(patches), per))
    else:
        slabs = (patches,)
    outs = []
    for slab in slabs:
        slab = _patches(slab)
        n, c, b, _ = slab.shape
        with torch.cuda.device(slab.device):
            table = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint8).reshape(256)).to(slab.device)
            out = torch.empty((n, b, b), dtype=torch.uint8, device=slab.device)
            L.call("mi_plot_patch_bytes", slab, n, c, b, table, out)
            outs.append(out.cpu().numpy())
    return np.concatenate(outs, 0)


def _draw(y01, idx, thumbs, P, mode, colours=None, labels=None, glyphs=None):
    y01 = _map(y01)
    dev, n = y01.device, y01.shape[0]
    idx = _index(idx, n, dev)
    thumbs = L.require_cuda(thumbs, "thumbs", torch.uint8).contiguous()
    if thumbs.ndim != 3 or thumbs.shape[0] != idx.numel() or thumbs.shape[1] != thumbs.shape[2]:
        raise ValueError("thumbs must be (%d, T, T), got %s" % (idx.numel(), tuple(thumbs.shape)))
    lay = layout(P, thumbs.shape[1] if idx.numel() else THUMB)
    if mode == 0:
        side = torch.as_tensor(np.ascontiguousarray(colours.cpu().numpy() if isinstance(colours, torch.Tensor) else colours,
                                                    dtype=np.uint8)).to(dev)
        if tuple(side.shape) != (n, 3):
            raise ValueError("colours must be (%d, 3) uint8, got %s" % (n, tuple(side.shape)))
        args = (side, None, None)
    else:
        lab = np.ascontiguousarray(labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
        if lab.shape != (n,) or (n and lab.min() < 0) or (n and lab.max() > 0x7fffffff):
            raise ValueError("labels must be (%d,) class numbers >= 0" % n)
        side = torch.from_numpy(lab.astype(np.int32)).to(dev)
        g = np.ascontiguousarray(DIGITS_5X7 if glyphs is None else glyphs, dtype=np.uint8)
        if g.shape != (10, 7):
            raise ValueError("glyphs must be (10, 7) uint8, got %s" % (g.shape,))
        g = torch.from_numpy(g).to(dev)
        args = (None, side, g)
    out = torch.empty((lay["P"], lay["P"], 3), dtype=torch.uint8, device=dev)
    ws = L.workspace(L.lib().mi_plot_raster_workspace_bytes(lay["P"]), dev, "plot2d_raster")
    L.call("mi_plot_raster", y01, n, idx, idx.numel(), thumbs, *args, L._c.byref(L.PlotLayout(**lay)), mode, out, ws, ws.numel())
    return out


def draw_out(y01, idx, thumbs, colours, P=PLOT_SIZE):
    """2d_visualization_out as a (P, P, 3) uint8 device tensor: the disc of every shown pick in its colour of `colours` (N, 3),
    in shown order, then the framed thumbnails in shown order (matplotlib draws patches under annotation boxes)."""
    return _draw(y01, idx, thumbs, P, 0, colours=colours)


def draw_labels(y01, idx, thumbs, labels, P=PLOT_SIZE, glyphs=None):
    """2d_visualization_labels as a (P, P, 3) uint8 device tensor: per shown pick, in order, its framed thumbnail and then
    the box with its class number `labels[idx[k]]`, digits from `glyphs` (10, 7) uint8 (DIGITS_5X7 by default)."""
    return _draw(y01, idx, thumbs, P, 1, labels=labels, glyphs=glyphs)


def class_gallery(patches, emb, centroids, assign, labels, k_classes, m=8, scale=2, device=None):
    """The class gallery (csrc/class_gallery.hip) of the picks: per class of `labels` (N,) in [0, k_classes) the
    mean and the population deviation of the patches (N, h, w), the member count, and the m members whose embedding emb (N, d) is
    nearest to the centroid `assign` (N,) gives them among `centroids` (k, d); numpy in, numpy out.  Returns a dictionary with
    mean, std (k_classes, h, w) fp32, count (k_classes,) int32, exemplar_index (k_classes, m) int32 (-1 where a class has fewer
    members), exemplar_d2 (k_classes, m) float64 (+inf there), order (k_classes,) int32 - the class of every row of the picture,
    by descending count, then ascending class - and picture (H, W, 3) uint8: per row the class number over its count, the mean
    (min-max scaled), the deviation (scaled by the largest deviation of all classes) and the m exemplars (min-max scaled each),
    every patch enlarged `scale` times.  There is no CPU path."""
    from .. import hipops as H
    if not torch.cuda.is_available():
        raise L.HipExtensionError("the class gallery is made on the MI355X (cuda) device; there is no CPU path")
    if device is None:
        from . import loader as Ld
        device = Ld._dev()
    dev = torch.device(device)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    with torch.cuda.device(dev):
        x, lab = up(patches, np.float32), up(labels, np.int32)
        mean, std, count = H.gallery_moments(x, lab, k_classes)
        idx, d2 = H.gallery_exemplars(up(emb, np.float32), up(centroids, np.float32), up(assign, np.int32), lab, k_classes, m)
        pic, order = H.gallery_raster(mean, std, count, idx, x, up(DIGITS_5X7, np.uint8), scale=scale)
        return dict(mean=mean.cpu().numpy(), std=std.cpu().numpy(), count=count.cpu().numpy(), exemplar_index=idx.cpu().numpy(),
                    exemplar_d2=d2.cpu().numpy(), order=order.cpu().numpy(), picture=pic.cpu().numpy())


def write_png(path, array):
    """An 8-bit PNG of a (H, W) grey, (H, W, 3) RGB or (H, W, 4) RGBA uint8 array: filter type 0, zlib, nothing else."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or 0 in a.shape or (a.ndim == 3 and a.shape[2] not in (3, 4)):
        raise ValueError("write_png takes (H, W), (H, W, 3) or (H, W, 4) uint8, got %s %s" % (a.shape, a.dtype))
    h, w = a.shape[:2]
    colour_type = 0 if a.ndim == 2 else (2 if a.shape[2] == 3 else 6)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], 1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))
