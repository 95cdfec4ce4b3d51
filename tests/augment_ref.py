"""CPU restatement of the view augmentation (cet_pick_amd/csrc/augment2d.hip) for the tests: the chain on 8-bit grey
levels in plain numpy (single-pass float32 bilinear, truncating float32 blends), and Philox-4x32-10 with the record
derivation of `mi_aug2d_params`.  tests/golden/augment2d.npz holds what PIL makes of the same records
(tests/golden/gen_golden_augment.py); test_augment_cpu.py checks this restatement against it."""
import numpy as np

F32 = np.float32


def blend(d, g, f):
    """(uint8)(d + f * (g - d)) of an 8-bit image blend: float32 product and sum, clip to [0, 255], truncation."""
    t = F32(d) + F32(f) * (g.astype(np.int32) - int(d)).astype(F32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int32)


def mean_level(g):
    """int(mean grey level + 0.5)"""
    return int((2 * int(g.sum()) + g.size) // (2 * g.size))


def resize_bilinear(win, bbox):
    """(s, s) grey levels -> (bbox, bbox): half-pixel centres, taps clamped to the window, rounded to a level."""
    s = win.shape[0]
    scale = F32(s) / F32(bbox)
    c = (np.arange(bbox, dtype=F32) + F32(0.5)) * scale - F32(0.5)
    c0 = np.floor(c)
    w = (c - c0).astype(F32)
    a = np.clip(c0.astype(np.int64), 0, s - 1)
    b = np.clip(c0.astype(np.int64) + 1, 0, s - 1)
    v = win.astype(F32)
    top = v[a][:, a] + w[None, :] * (v[a][:, b] - v[a][:, a])
    bot = v[b][:, a] + w[None, :] * (v[b][:, b] - v[b][:, a])
    out = top + w[:, None] * (bot - top)
    return np.clip(np.floor(out + F32(0.5)), 0, 255).astype(np.int32)


def chain_levels(g0, hflip, vflip, bright_first, brightness, contrast, s, i, j, k):
    """The chain up to the grey levels of the rotated view (`round(255 y)` of the kernel's output at mean 0, std 1).
    g0: (bbox, bbox) uint8 = floor(255 x)."""
    g = g0.astype(np.int32)
    if hflip:
        g = g[:, ::-1]
    if vflip:
        g = g[::-1, :]
    if bright_first:
        g = blend(0, g, brightness)
        g = blend(mean_level(g), g, contrast)
    else:
        g = blend(mean_level(g), g, contrast)
        g = blend(0, g, brightness)
    g = resize_bilinear(g[i:i + s, j:j + s], g0.shape[0])
    return np.rot90(g, k).astype(np.uint8)                       # = torch.rot90(img, k, dims=[1, 2]) of the (1, H, W) image


# ---- Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) ------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 arrays holding 32-bit words -> four arrays of 32-bit words"""
    c0, c1, c2, c3, k0, k1 = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def unit_float(r):
    return (r >> np.uint64(8)).astype(F32) * F32(1.0 / 16777216.0)


def draw_records(sample_ids, seed, epoch, view, bbox, flip_p=0.5, brightness=(0.5, 1.5), contrast=(0.8, 1.2), area=(0.8, 1.0)):
    """`mi_aug2d_params` on the host: {field: array}.  The integer fields are exact restatements; the float32 fields may
    differ from the device's in the last bit (the device may fuse `lo + (hi - lo) * u`), and with them an `s` whose
    `bbox * sqrt(u)` falls on a rounding boundary."""
    sid = np.asarray(sample_ids, dtype=np.int64).astype(np.uint64)
    c0, c1 = sid & MASK, sid >> np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    a = philox4x32_10(c0, c1, np.uint64(epoch & 0xFFFFFFFF), np.uint64(view), k0, k1)
    b = philox4x32_10(c0, c1, np.uint64(epoch & 0xFFFFFFFF), np.uint64(view | (1 << 8)), k0, k1)
    lin = lambda lo, hi, u: F32(lo) + (F32(hi) - F32(lo)) * u
    u = lin(area[0], area[1], unit_float(a[3]))
    s = np.clip(np.rint(F32(bbox) * np.sqrt(u)).astype(np.int64), 1, bbox)
    span = (bbox - s + 1).astype(np.uint64)
    return {"hflip": (unit_float(a[0]) < F32(flip_p)).astype(np.int32), "vflip": (unit_float(b[2]) < F32(flip_p)).astype(np.int32),
            "bright_first": (b[3] >> np.uint64(31)).astype(np.int32), "k": ((b[3] >> np.uint64(16)) & np.uint64(3)).astype(np.int32),
            "neighbour": ((b[3] >> np.uint64(8)) & np.uint64(3)).astype(np.int32),
            "brightness": lin(brightness[0], brightness[1], unit_float(a[1])),
            "contrast": lin(contrast[0], contrast[1], unit_float(a[2])), "s": s.astype(np.int32),
            "i": ((b[0] * span) >> np.uint64(32)).astype(np.int32), "j": ((b[1] * span) >> np.uint64(32)).astype(np.int32)}


def side_probabilities(bbox, lo, hi):
    """{s: P(round(bbox sqrt(u)) == s)} for u ~ U(lo, hi)"""
    out = {}
    for s in range(1, bbox + 1):
        a, b = max(lo, ((s - 0.5) / bbox) ** 2), min(hi, ((s + 0.5) / bbox) ** 2)
        if b > a:
            out[s] = (b - a) / (hi - lo)
    return out


# ---- the record table (layout: include/cetpick_hip.h) --------------------------------------------------------------------
def pack_params(hflip, vflip, bright_first, brightness, contrast, s, i, j, k, neighbour=None):
    """Explicit records (arrays of one length) -> (n, 8) int32 array, the layout `mi_aug2d_params` writes."""
    t = np.zeros((len(s), 8), dtype=np.int32)
    as_i = lambda a: np.asarray(a).astype(np.int32)
    t[:, 0] = as_i(hflip) | (as_i(vflip) << 1) | (as_i(bright_first) << 2)
    t[:, 1] = np.asarray(brightness, dtype=np.float32).view(np.int32)
    t[:, 2] = np.asarray(contrast, dtype=np.float32).view(np.int32)
    t[:, 3], t[:, 4], t[:, 5], t[:, 6] = as_i(s), as_i(i), as_i(j), as_i(k)
    if neighbour is not None:
        t[:, 7] = as_i(neighbour)
    return t


def unpack_params(t):
    """(n, 8) int32 array -> {field: array}"""
    t = np.asarray(t)
    f32 = lambda w: np.ascontiguousarray(t[:, w]).view(np.float32)
    return {"hflip": t[:, 0] & 1, "vflip": (t[:, 0] >> 1) & 1, "bright_first": (t[:, 0] >> 2) & 1, "brightness": f32(1),
            "contrast": f32(2), "s": t[:, 3], "i": t[:, 4], "j": t[:, 5], "k": t[:, 6], "neighbour": t[:, 7]}
