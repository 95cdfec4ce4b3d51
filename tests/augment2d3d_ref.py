"""CPU restatement of the 2d3d view augmentation (cet_pick_amd/csrc/augment2d3d.hip) for the tests: the chain on 8-bit
grey levels of a two-channel image in plain numpy (flips, the imaging library's nearest-neighbour rotation as its 16.16
fixed-point affine map, the clipped erase rectangle, the quarter turn) and the record derivation of `mi_aug2d3d_params`.
tests/golden/augment2d3d.npz holds what PIL makes of the same records (tests/golden/gen_golden_augment2d3d.py);
test_augment2d3d_cpu.py checks this restatement against it."""
import math

import numpy as np

from augment_ref import MASK, philox4x32_10, unit_float

F32 = np.float32
WORDS = 16
STREAM_TAG = 0x2D3D0000
IDENTITY = (65536, 0, 32768, 0, 65536, 32768)
STRONG = dict(flip_p=0.5, angle=(-30.0, 30.0), erase_p=0.5, scale=(0.01, 0.02), ratio=(0.5, 1.5))
WEAK = dict(STRONG, angle=(0.0, 0.0))
FIELDS = ("hflip", "vflip", "erase", "k", "i", "j", "h", "w", "angle", "coef")


# ---- the rotation ----------------------------------------------------------------------------------------------------------
def fix_arguments(angle, bbox):
    """The six values v whose FIX(v) = floor(65536 v + 0.5) are the coefficients a0..a5 of `rotate(angle, NEAREST,
    expand=False, center=None)` on a bbox x bbox image (Python floats: the library computes them in Python)."""
    t = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    c = bbox / 2.0
    m[2] = m[0] * -c + m[1] * -c + m[2] + c
    m[5] = m[3] * -c + m[4] * -c + m[5] + c
    return [m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5]


def rotation_coefficients(angle, bbox):
    return [int(math.floor(v * 65536.0 + 0.5)) for v in fix_arguments(angle, bbox)]


def affine_nearest(img, a):
    """img (..., b, b) -> output pixel (y, x) = input pixel ((a5 + a4 y + a3 x) >> 16, (a2 + a1 y + a0 x) >> 16), 0 outside"""
    b = img.shape[-1]
    y, x = np.mgrid[0:b, 0:b].astype(np.int64)
    sy, sx = (int(a[5]) + int(a[4]) * y + int(a[3]) * x) >> 16, (int(a[2]) + int(a[1]) * y + int(a[0]) * x) >> 16
    inside = (sy >= 0) & (sy < b) & (sx >= 0) & (sx < b)
    return np.where(inside, img[..., np.clip(sy, 0, b - 1), np.clip(sx, 0, b - 1)], 0)


# ---- the chain -------------------------------------------------------------------------------------------------------------
def clip_rect(i, j, h, w, bbox):
    """The erased rectangle [i, i + h) x [j, j + w) clipped to the image -> (i0, i1, j0, j1); empty when i1 <= i0 or j1 <= j0"""
    cl = lambda v: min(max(int(v), 0), bbox)
    return cl(i), max(cl(i), cl(int(i) + max(int(h), 0))), cl(j), max(cl(j), cl(int(j) + max(int(w), 0)))


def chain_levels(g, hflip, vflip, erase, k, i, j, h, w, coef):
    """The chain up to the grey levels of the turned view (`round(255 y)` of the kernel's output at mean 0, std 1).
    g: (2, bbox, bbox) uint8 = floor(255 x) of the two channels."""
    g = g.astype(np.int32)
    if hflip:
        g = g[:, :, ::-1]
    if vflip:
        g = g[:, ::-1, :]
    g = affine_nearest(g, coef)
    if erase:
        i0, i1, j0, j1 = clip_rect(i, j, h, w, g.shape[-1])
        g[:, i0:i1, j0:j1] = 255
    return np.rot90(g, int(k), axes=(1, 2)).astype(np.uint8)     # = torch.rot90(img, k, dims=[1, 2]) of the (2, H, W) image


# ---- the record draw ---------------------------------------------------------------------------------------------------------
def extent_bounds(bbox, ranges):
    """(h_min, h_max, w_min, w_max) of CornerErasing for the ranges, in exact arithmetic"""
    a = bbox * bbox
    (s0, s1), (r0, r1) = ranges["scale"], ranges["ratio"]
    return (int(round(math.sqrt(a * s0 * r0))), int(round(math.sqrt(a * s1 * r1))),
            int(round(math.sqrt(a * s0 / r1))), int(round(math.sqrt(a * s1 / r0))))


def corner_range(near, e, bbox):
    """[lo, hi) of CornerErasing's row (column) for an extent e, on the near side of the centre or the far one"""
    mid = bbox // 2
    return (0, max(1, mid - e - 6)) if near else (mid + 6, max(mid + 7, bbox - e + 6))


def draw_records(sample_ids, seed, epoch, view, bbox, ranges=None):
    """`mi_aug2d3d_params` on the host: {field: array} (+ "near_i", "near_j": the sides the coins chose).  The flags, k and
    the angle are exact restatements (the kernel does not contract `lo + (hi - lo) u`); h and w go through single-precision
    exp / sqrt and may differ where they fall on a rounding boundary, and i, j with them."""
    rg = ranges if ranges is not None else (WEAK if view else STRONG)
    sid = np.asarray(sample_ids, dtype=np.int64).astype(np.uint64)
    c0, c1, c2 = sid & MASK, sid >> np.uint64(32), np.uint64(epoch & 0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    a, b, c = (philox4x32_10(c0, c1, c2, np.uint64(view | (d << 8) | STREAM_TAG), k0, k1) for d in range(3))
    lin = lambda lo, hi, u: F32(lo) + (F32(hi) - F32(lo)) * u
    angle = lin(rg["angle"][0], rg["angle"][1], unit_float(a[2]))
    share = lin(rg["scale"][0], rg["scale"][1], unit_float(b[0]))
    l_lo, l_hi = (F32(math.log(float(F32(r)))) for r in rg["ratio"])
    aspect = np.exp(lin(l_lo, l_hi, unit_float(b[1]))).astype(F32)
    area = F32(bbox * bbox) * share
    mid = bbox // 2
    h = np.clip(np.rint(np.sqrt(area * aspect)).astype(np.int64), 0, mid - 1)
    w = np.clip(np.rint(np.sqrt(area / aspect)).astype(np.int64), 0, mid - 1)
    near_i, near_j = unit_float(b[2]) > F32(0.5), unit_float(b[3]) > F32(0.5)

    def start(near, r, e):
        lo = np.where(near, 0, mid + 6)
        hi = np.where(near, np.maximum(1, mid - e - 6), np.maximum(mid + 7, bbox - e + 6))
        return lo + ((r * (hi - lo).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    return {"hflip": (unit_float(a[0]) < F32(rg["flip_p"])).astype(np.int32),
            "vflip": (unit_float(a[1]) < F32(rg["flip_p"])).astype(np.int32),
            "erase": (unit_float(a[3]) < F32(rg["erase_p"])).astype(np.int32), "k": (c[2] >> np.uint64(30)).astype(np.int32),
            "i": start(near_i, c[0], h).astype(np.int32), "j": start(near_j, c[1], w).astype(np.int32),
            "h": h.astype(np.int32), "w": w.astype(np.int32), "angle": angle.astype(F32),
            "coef": np.array([rotation_coefficients(v, bbox) for v in angle], dtype=np.int32).reshape(-1, 6),
            "near_i": near_i, "near_j": near_j}


# ---- the record table (layout: include/cetpick_hip.h) ------------------------------------------------------------------------
def pack_params(hflip, vflip, erase, k, i, j, h, w, angle, coef, **_):
    """Explicit records (arrays of one length) -> (n, 16) int32 array, the layout `mi_aug2d3d_params` writes."""
    as_i = lambda v: np.asarray(v).astype(np.int32)
    t = np.zeros((len(as_i(k)), WORDS), dtype=np.int32)
    t[:, 0] = as_i(hflip) | (as_i(vflip) << 1) | (as_i(erase) << 2)
    t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 5] = as_i(k), as_i(i), as_i(j), as_i(h), as_i(w)
    t[:, 6] = np.asarray(angle, dtype=np.float32).view(np.int32)
    t[:, 8:14] = as_i(coef)
    return t


def unpack_params(t):
    """(n, 16) int32 array -> {field: array}"""
    t = np.asarray(t)
    return {"hflip": t[:, 0] & 1, "vflip": (t[:, 0] >> 1) & 1, "erase": (t[:, 0] >> 2) & 1, "k": t[:, 1], "i": t[:, 2],
            "j": t[:, 3], "h": t[:, 4], "w": t[:, 5], "angle": np.ascontiguousarray(t[:, 6]).view(np.float32),
            "coef": t[:, 8:14], "reserved": t[:, [7, 14, 15]], "flag_rest": t[:, 0] >> 3}
