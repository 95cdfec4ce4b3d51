"""NumPy / torch-CPU restatements of csrc/plot2d.hip (the arbiters of tests/test_plot2d_cpu.py and tests/test_plot2d_gpu.py):
the thumbnail filter, the thumbnail of a pick, the grey bytes of a patch, the two pictures, and a PNG reader."""
import struct
import zlib

import numpy as np

GRAY_LUT = (np.linspace(0, 1, 256) * 255).astype(np.uint8)
MARGIN = 48


def select_literal(y01, thr):
    """plot_2d.py:123-137 of the reference, transcribed: quadratic, the arbiter of `select`."""
    y = np.asarray(y01, np.float32)
    shown, idx = np.expand_dims(y[0], 0), []
    for i in range(len(y)):
        d = np.sum((y[i] - shown) ** 2, 1)
        if np.min(d) < thr:
            continue
        shown = np.r_[shown, [y[i]]]
        idx.append(i)
    return np.asarray(idx, np.int32)


def select(y01, thr):
    """The same list with the distances spelled out in float32 and the shown picks in a preallocated array."""
    y = np.asarray(y01, np.float32)
    thr = np.float32(thr)
    sx, sy = np.empty(len(y) + 1, np.float32), np.empty(len(y) + 1, np.float32)
    sx[0], sy[0], m, idx = y[0, 0], y[0, 1], 1, []
    for i in range(len(y)):
        dx, dy = y[i, 0] - sx[:m], y[i, 1] - sy[:m]
        d = dx * dx + dy * dy
        assert d.dtype == np.float32
        if d.min() < thr:
            continue
        sx[m], sy[m] = y[i]
        m += 1
        idx.append(i)
    return np.asarray(idx, np.int32)


def thumb_q64(patch):
    """255 ((x - mean) / std + 3) / 6 clipped to [0, 255], in float64, of a whole (C, b, b) patch; zeros where std is 0."""
    x = np.asarray(patch, np.float64)
    std = x.std()
    if not std > 0:
        return np.zeros(x.shape)
    return np.clip(255 * ((x - x.mean()) / std + 3) / 6, 0, 255)


def thumb_bytes64(patch):
    q = thumb_q64(patch)
    return np.rint(q).astype(np.uint8), np.abs(q - np.floor(q) - 0.5) <= 2.0 ** -10      # bytes, excused pixels


def thumb_bytes32(patch):
    """The reference's own float32 chain (plot_2d.py:147-148 with its quantize(-3, 3)); a constant patch gives NaN there."""
    img = np.asarray(patch, np.float32)
    img = (img - img.mean()) / img.std()
    x = 255 * (img - (-3)) / 6
    return np.round(np.clip(x, 0, 255)).astype(np.uint8)


def thumb_cases():
    """name -> (n, C, b, b) float32 patches of the thumbnail and patch-byte tests.  The seeds are fixed;
    tests/test_plot2d_cpu.py asserts that with them the reference's own float32 chain disagrees with `thumb_bytes64` on at most
    1 % of a case's pixels, the share the GPU test excuses."""
    rs = np.random.RandomState(20240611)
    cases = {"b%d" % b: rs.standard_normal((3, 1, b, b)).astype(np.float32) * rs.uniform(0.5, 20) + rs.uniform(-5, 5)
             for b in (9, 36, 40)}
    cases["two_channels"] = rs.standard_normal((3, 2, 12, 12)).astype(np.float32)
    cases["two_channels"][:, 1] += 4.0                                 # statistics over both channels, picture from channel 0
    cases["constant"] = np.full((1, 1, 12, 12), 2.5, np.float32)
    cases["outlier"] = rs.standard_normal((1, 1, 36, 36)).astype(np.float32)
    cases["outlier"][0, 0, 5, 7] = 1e6
    return cases


def resize(bytes2d, T=32):
    """torchvision 0.12's functional.resize of a uint8 tensor, written out: float32 bilinear weights of align_corners=False,
    source index clamped at 0, no antialias, round half to even."""
    a = np.asarray(bytes2d, np.uint8).astype(np.float32)
    b = a.shape[0]
    scale = np.float32(b) / np.float32(T)
    src = np.maximum(scale * (np.arange(T, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), b - 1)
    i1 = np.minimum(i0 + 1, b - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = np.float32(1) - l1
    top = l0[None, :] * a[i0][:, i0] + l1[None, :] * a[i0][:, i1]
    bot = l0[None, :] * a[i1][:, i0] + l1[None, :] * a[i1][:, i1]
    out = l0[:, None] * top + l1[:, None] * bot
    assert out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def resize_torch(bytes2d, T=32):
    import torch
    t = torch.from_numpy(np.asarray(bytes2d, np.uint8)).float()[None, None]
    r = torch.nn.functional.interpolate(t, size=(T, T), mode="bilinear", align_corners=False)
    return torch.round(r)[0, 0].to(torch.uint8).numpy()


def patch_bytes(patch0, lut=GRAY_LUT):
    """plt.imsave(patch0, cmap='gray'): float32 min-max, index floor(256 t) capped at 255, the colour table's byte."""
    x = np.asarray(patch0, np.float32)
    mn, mx = x.min(), x.max()
    if not mx > mn:
        return np.full(x.shape, lut[0], np.uint8)
    t = (x - mn) / np.float32(mx - mn)
    assert t.dtype == np.float32
    return lut[np.minimum(np.floor(t * np.float32(256)).astype(np.int64), 255)]


def layout(P, T):
    S = P - 1 - 2 * MARGIN
    return dict(P=P, M=MARGIN, S=S, R=int(round(0.03 * S)), T=T, dx=int(round(0.025 * S)), dy=int(round(0.020 * S)))


def centre(y01, i, lay):
    u, v = float(y01[i][0]), float(y01[i][1])
    return lay["M"] + int(np.rint(u * lay["S"])), lay["M"] + int(np.rint((1.0 - v) * lay["S"]))


def _put(canvas, col, row, colour):
    if 0 <= col < canvas.shape[1] and 0 <= row < canvas.shape[0]:
        canvas[row, col] = colour


def _disc(canvas, col, row, R, colour):
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx * dx + dy * dy <= R * R:
                _put(canvas, col + dx, row + dy, colour)


def _thumb(canvas, col, row, thumb):
    T = thumb.shape[0]
    x0, y0 = col - T // 2, row - T // 2
    for dy in range(-1, T + 1):
        for dx in range(-1, T + 1):
            inside = 0 <= dx < T and 0 <= dy < T
            _put(canvas, x0 + dx, y0 + dy, (thumb[dy, dx],) * 3 if inside else (0, 0, 0))


def _box(canvas, col, row, label, glyphs, lay, px=2, gap=2, pad=3, border=2):
    digits = [int(c) for c in "%d" % label]
    w = len(digits) * 5 * px + (len(digits) - 1) * gap + 2 * (pad + border)
    h = 7 * px + 2 * (pad + border)
    x0, y0 = col - lay["dx"], row - lay["dy"] - h + 1                # its bottom-left pixel is (x0, row - dy)
    for by in range(h):
        for bx in range(w):
            edge = bx < border or by < border or bx >= w - border or by >= h - border
            _put(canvas, x0 + bx, y0 + by, (0, 0, 255) if edge else (255, 255, 255))
    for d, digit in enumerate(digits):
        for gy in range(7):
            for gx in range(5):
                if (int(glyphs[digit][gy]) >> (4 - gx)) & 1:
                    for sy in range(px):
                        for sx in range(px):
                            _put(canvas, x0 + border + pad + d * (5 * px + gap) + gx * px + sx,
                                 y0 + border + pad + gy * px + sy, (0, 0, 255))


def draw_out(y01, idx, thumbs, colours, P):
    """Painter's algorithm: every disc in shown order, then every framed thumbnail in shown order."""
    lay = layout(P, thumbs.shape[1] if len(idx) else 32)
    canvas = np.full((P, P, 3), 255, np.uint8)
    for i in idx:
        _disc(canvas, *centre(y01, i, lay), lay["R"], tuple(colours[i]))
    for k, i in enumerate(idx):
        _thumb(canvas, *centre(y01, i, lay), thumbs[k])
    return canvas


def draw_labels(y01, idx, thumbs, labels, glyphs, P):
    lay = layout(P, thumbs.shape[1] if len(idx) else 32)
    canvas = np.full((P, P, 3), 255, np.uint8)
    for k, i in enumerate(idx):
        _thumb(canvas, *centre(y01, i, lay), thumbs[k])
        _box(canvas, *centre(y01, i, lay), int(labels[i]), glyphs, lay)
    return canvas


def read_png(path):
    """8-bit grey / RGB / RGBA PNGs with filter type 0 on every row (what write_png writes): (H, W[, 3 | 4]) uint8."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype, comp, filt, lace = head
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2, 6)
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    out = rows[:, 1:].reshape(h, w, ch)
    return out[:, :, 0].copy() if ch == 1 else out.copy()
