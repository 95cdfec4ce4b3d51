"""CPU restatement of the random 3-D views (cet_pick_amd/csrc/augment3d.hip) for the tests, in plain numpy: the chain on one
S^3 box for one record, in float64 (the reference of the GPU tests) or with every operation in float32 (`dtype`: the yardstick
of their tolerance), and the record derivation of `mi_aug3d_params` (bit-level Philox from augment_ref.py).  Written from
the chain's description in include/cetpick_hip.h and DESIGN.md §4.17."""
import numpy as np

from augment_ref import MASK, philox4x32_10, unit_float

F32, F64 = np.float32, np.float64
PARAM_TAG, NOISE_TAG = 0x3D3D0000, 0x3D3E0000
BLUR, NOISE, ROT = 1, 2, 4
FLIP_NONE, FLIP_Z, FLIP_Y = 0, 1, 2
ERASE_NONE, DROP, CENTRE, SWAP = 0, 1, 2, 3
RANGES = dict(blur_p=0.15, sigma=(0.0, 1.0), noise_p=0.5, noise=(0.0, 0.25), rot_p=0.75, angle=(0.0, 60.0),
              flip=(0.33, 0.66), erase=(0.25, 0.5, 0.75))
BAND = 1e-3                      # a rotated voxel whose source coordinate is this close to the box boundary may be excluded


def geometry(c):
    """-> (m, S, e, q): margin, box edge, erased-box edge, half the edge of center_out's window"""
    m = c // 6
    S = c + 2 * m
    return m, S, S // 8, S // 4


def corner_set(c):
    _, _, e, _ = geometry(c)
    return list(range(0, c // 2 - 2 * e)) + list(range(c // 2 + e, c - e))


# ---- the steps ------------------------------------------------------------------------------------------------------------
def taps(sigma, dtype=F64):
    """gaussian_filter's normalised weights for one axis: radius int(4 sigma + 0.5)"""
    r = int(4.0 * float(sigma) + 0.5)
    if r == 0:
        return np.ones(1, dtype)
    k = np.arange(-r, r + 1).astype(dtype)
    w = np.exp(dtype(-0.5) * k * k / (dtype(sigma) * dtype(sigma))).astype(dtype)
    return (w / w.sum(dtype=dtype)).astype(dtype)


def blur(box, sigmas, dtype=F64):
    """separable Gaussian, axes z, y, x in turn, edge mode reflect (d c b a | a b c d)"""
    out = box.astype(dtype)
    for ax, sg in enumerate(sigmas):
        w = taps(sg, dtype)
        r = (len(w) - 1) // 2
        if r == 0:
            continue
        n = out.shape[ax]
        acc = np.zeros_like(out)
        for k in range(-r, r + 1):
            i = np.arange(n) + k
            i = np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
            acc = (acc + w[k + r] * np.take(out, i, axis=ax)).astype(dtype)
        out = acc
    return out


def normals(n, k0, k1, dtype=F64):
    """N(0, 1) of voxels 0 .. n - 1: Box-Muller on words 0, 1 of Philox(counter (i, 0, 0, NOISE_TAG), key (k0, k1)); the
    logarithm's argument is ((w0 >> 8) + 1) / 2^24 in (0, 1]"""
    w0, w1, _, _ = philox4x32_10(np.arange(n, dtype=np.uint64), 0, 0, NOISE_TAG, k0, k1)
    u1 = ((w0 >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dtype(1.0 / 16777216.0)
    u2 = (w1 >> np.uint64(8)).astype(dtype) * dtype(1.0 / 16777216.0)
    return (np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(dtype(2.0 * np.pi) * u2)).astype(dtype)


def source_coords(S, cos, sin, dtype=F64):
    """(fy, fx) of every (y, x) of a plane: rotation about the plane's centre"""
    a = dtype((S - 1) / 2.0)
    d = np.arange(S).astype(dtype) - a
    dy, dx = d[:, None], d[None, :]
    cos, sin = dtype(cos), dtype(sin)
    return (a + (cos * dy - sin * dx)).astype(dtype), (a + (sin * dy + cos * dx)).astype(dtype)


def rotate(box, cos, sin, dtype=F64):
    """every plane of `box` rotated in (y, x), bilinear, the box minimum outside [0, S - 1].  -> (rotated box, band mask
    (S, S): True where a source coordinate is within BAND of the boundary)"""
    S = box.shape[-1]
    box = box.astype(dtype)
    fy, fx = source_coords(S, cos, sin, dtype)
    hi = dtype(S - 1)
    inside = (fy >= 0) & (fy <= hi) & (fx >= 0) & (fx <= hi)
    cy, cx = np.clip(fy, 0, hi), np.clip(fx, 0, hi)
    ya, xa = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
    yb, xb = np.minimum(ya + 1, S - 1), np.minimum(xa + 1, S - 1)
    wy, wx = (cy - ya.astype(dtype)).astype(dtype), (cx - xa.astype(dtype)).astype(dtype)
    v00, v01, v10, v11 = box[:, ya, xa], box[:, ya, xb], box[:, yb, xa], box[:, yb, xb]
    top, bot = v00 + wx * (v01 - v00), v10 + wx * (v11 - v10)
    out = np.where(inside[None], top + wy * (bot - top), box.min()).astype(dtype)
    f64y, f64x = source_coords(S, cos, sin, F64)
    band = np.zeros((S, S), bool)
    for f in (f64y, f64x):
        band |= (np.abs(f) < BAND) | (np.abs(f - (S - 1)) < BAND)
    return out, band


def znorm_rescale_znorm(x, dtype=F64):
    """ZNormalization (unbiased std), RescaleIntensity(-3, 3), ZNormalization"""
    x = x.astype(dtype)
    x = (x - x.mean(dtype=dtype)) / x.std(ddof=1, dtype=dtype)
    x = (x - x.min()) / (x.max() - x.min()) * dtype(6.0) - dtype(3.0)
    return ((x - x.mean(dtype=dtype)) / x.std(ddof=1, dtype=dtype)).astype(dtype)


def flip_erase(x, c, flip, erase, box0, box1):
    """the flip, then the erasure, on a (c, c, c) array (a copy)"""
    _, _, e, q = geometry(c)
    x = x[::-1].copy() if flip == FLIP_Z else (x[:, ::-1].copy() if flip == FLIP_Y else x.copy())
    sl = lambda b: tuple(slice(int(v), int(v) + e) for v in b)
    if erase == DROP:
        x[sl(box0)] = 0
    elif erase == CENTRE:
        keep = np.zeros(c, bool)
        keep[c // 2 - q:c // 2 + q] = True
        x[:, ~(keep[:, None] & keep[None, :])] = 0
    elif erase == SWAP:
        a, b = x[sl(box0)].copy(), x[sl(box1)].copy()
        x[sl(box0)] = b
        x[sl(box1)] = a
    return x


# ---- records -----------------------------------------------------------------------------------------------------------------
def record(c, blur=None, noise=None, angle=None, flip=FLIP_NONE, erase=ERASE_NONE, box0=(0, 0, 0), box1=None, key=(1, 2)):
    """a hand-made record: blur = (sz, sy, sx) or None, noise = sigma or None, angle = degrees or None"""
    cs = corner_set(c)
    box1 = (cs[1],) * 3 if box1 is None else box1
    deg = F32(0.0 if angle is None else angle)
    th = F64(deg) * (np.pi / 180.0)
    return dict(flags=(BLUR if blur is not None else 0) | (NOISE if noise is not None else 0) | (ROT if angle is not None else 0),
                flip=flip, erase=erase, sigma=tuple(F32(v) for v in (blur if blur is not None else (0, 0, 0))),
                sigma_n=F32(0.0 if noise is None else noise), angle=deg, cos=F32(np.cos(th)), sin=F32(np.sin(th)),
                box0=tuple(box0), box1=tuple(box1), key=tuple(key))


def pack(records):
    """records -> (n, 16) int32 table (layout: include/cetpick_hip.h)"""
    t = np.zeros((len(records), 16), np.uint32)
    for i, r in enumerate(records):
        t[i, 0] = r["flags"] | (r["flip"] << 4) | (r["erase"] << 8)
        t[i, 1:8] = np.array(list(r["sigma"]) + [r["sigma_n"], r["angle"], r["cos"], r["sin"]], F32).view(np.uint32)
        t[i, 8:11], t[i, 11:14], t[i, 14:16] = r["box0"], r["box1"], r["key"]
    return t.view(np.int32)


def unpack(table):
    """(n, 16) int32 table -> list of records"""
    t = np.ascontiguousarray(table).view(np.uint32)
    f = t.view(F32)
    return [dict(flags=int(t[i, 0] & 7), flip=int((t[i, 0] >> 4) & 3), erase=int((t[i, 0] >> 8) & 3), sigma=tuple(f[i, 1:4]),
                 sigma_n=f[i, 4], angle=f[i, 5], cos=f[i, 6], sin=f[i, 7], box0=tuple(int(v) for v in t[i, 8:11]),
                 box1=tuple(int(v) for v in t[i, 11:14]), key=(int(t[i, 14]), int(t[i, 15]))) for i in range(len(t))]


def chain(box, c, r, dtype=F64):
    """the whole chain on one S^3 box for record r -> ((c, c, c) view, (c, c) mask of voxels that may be excluded)"""
    m, S, _, _ = geometry(c)
    assert box.shape == (S, S, S)
    x = box.astype(dtype)
    if r["flags"] & BLUR:
        x = blur(x, r["sigma"], dtype)
    if r["flags"] & NOISE:
        x = (x + dtype(r["sigma_n"]) * normals(S ** 3, r["key"][0], r["key"][1], dtype).reshape(S, S, S)).astype(dtype)
    band = np.zeros((S, S), bool)
    if r["flags"] & ROT:
        x, band = rotate(x, r["cos"], r["sin"], dtype)
    x = znorm_rescale_znorm(x[m:m + c, m:m + c, m:m + c], dtype)
    x = flip_erase(x, c, r["flip"], r["erase"], r["box0"], r["box1"])
    # the mask travels with the values: through the flip and the swap
    mask = np.broadcast_to(band[m:m + c, m:m + c][None], (c, c, c))
    mask = flip_erase(mask, c, r["flip"], ERASE_NONE, None, None)
    if r["erase"] == SWAP and mask.any():
        mask = flip_erase(mask.astype(F64), c, FLIP_NONE, SWAP, r["box0"], r["box1"]) > 0
    return x, mask


def draw_records(sample_ids, seed, epoch, view, c, ranges=RANGES):
    """`mi_aug3d_params` on the host -> list of records (float fields: float32 operations, not contracted)"""
    sid = np.asarray(sample_ids, dtype=np.int64).astype(np.uint64)
    c0, c1 = sid & MASK, sid >> np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    w = [philox4x32_10(c0, c1, np.uint64(epoch & 0xFFFFFFFF), np.uint64(view | (j << 8) | PARAM_TAG), k0, k1) for j in range(5)]
    lin = lambda lo_hi, r: F32(lo_hi[0]) + (F32(lo_hi[1]) - F32(lo_hi[0])) * unit_float(r)
    _, _, e, _ = geometry(c)
    cs = np.array(corner_set(c))
    n_set = np.uint64(len(cs))
    below = lambda r, n: ((r * n) >> np.uint64(32)).astype(np.int64)
    flags = ((unit_float(w[0][0]) < F32(ranges["blur_p"])) * BLUR | (unit_float(w[1][0]) < F32(ranges["noise_p"])) * NOISE |
             (unit_float(w[1][2]) < F32(ranges["rot_p"])) * ROT)
    uf, ue = unit_float(w[2][0]), unit_float(w[2][1])
    flip = np.where(uf < F32(ranges["flip"][0]), FLIP_Z, np.where(uf > F32(ranges["flip"][1]), FLIP_Y, FLIP_NONE))
    er = [F32(v) for v in ranges["erase"]]
    erase = np.where(ue < er[0], DROP, np.where(ue < er[1], CENTRE, np.where(ue < er[2], SWAP, ERASE_NONE)))
    sig = [lin(ranges["sigma"], w[0][a]) for a in (1, 2, 3)]
    sn, deg = lin(ranges["noise"], w[1][1]), lin(ranges["angle"], w[1][3])
    th = deg.astype(F64) * (np.pi / 180.0)
    i0 = [below(w[3][a], n_set) for a in range(3)]
    i1 = [below(w[4][a], n_set - np.uint64(1)) for a in range(3)]
    i1 = [i1[a] + (i1[a] >= i0[a]) for a in range(3)]
    return [dict(flags=int(flags[t]), flip=int(flip[t]), erase=int(erase[t]), sigma=(sig[0][t], sig[1][t], sig[2][t]),
                 sigma_n=sn[t], angle=deg[t], cos=F32(np.cos(th[t])), sin=F32(np.sin(th[t])),
                 box0=tuple(int(cs[i0[a][t]]) for a in range(3)), box1=tuple(int(cs[i1[a][t]]) for a in range(3)),
                 key=(int(w[2][2][t]), int(w[2][3][t]))) for t in range(len(sid))]
