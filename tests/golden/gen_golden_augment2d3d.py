"""Golden vectors of the 2d3d view augmentation -> augment2d3d.npz, made with PIL (the calls torchvision's PIL back end
makes for ToPILImage on a two-channel image ("LA"), RandomHorizontalFlip / RandomVerticalFlip, RandomRotation: `transpose`
and `rotate(angle, NEAREST, fillcolor=(0, 0))`); CornerErasing's rectangle and FixedRotation's rot90 are numpy.  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_augment2d3d.py

Per bbox (36, 12): 32 seeded two-channel crops (different content per channel) with explicit records:
    every (hflip, vflip, k) combination, twice;
    angles -30, 30, 0, 1e-9, -1e-9, 19 random ones in [-30, 30], and 8 weak records (no rotation: the identity matrix);
    erase kinds 0 off, 1 inside the top-left corner, 2 sticking out of the bottom / right edge, 3 wholly outside,
    4 the extreme h, w of the reference ranges (scale (0.01, 0.02), ratio (0.5, 1.5)).
Stored: the crops as uint8 grey levels (the kernel's input is (g + 0.5) / 255), the records with the coefficients of the
host formula (tests/augment2d3d_ref.py), the expected views as uint8 grey levels, `weak` and `kind` per record.
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import augment2d3d_ref as R  # noqa: E402

BBOXES = (36, 12)
N = 32


def make_crop(rng, b):
    """A min-max'ed patch like the dataset's: a few blobs on noise, levels 0 and 255 both present."""
    yy, xx = np.mgrid[0:b, 0:b]
    img = rng.standard_normal((b, b)) * 0.6
    for _ in range(int(rng.integers(1, 4))):
        cy, cx, r = rng.uniform(2, b - 2), rng.uniform(2, b - 2), rng.uniform(1.5, b / 6.0)
        img -= rng.uniform(1.5, 3.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    img = (img - img.min()) / (img.max() - img.min())
    return np.floor(np.float32(img) * np.float32(255)).astype(np.uint8)


def records(rng, b):
    idx = np.arange(N)
    mid = b // 2
    h_min, h_max, w_min, w_max = R.extent_bounds(b, R.STRONG)
    weak = idx >= 24
    angle = rng.uniform(-30, 30, N).astype(np.float32)
    angle[:5] = (-30, 30, 0, 1e-9, -1e-9)
    angle[weak] = 0
    kind = rng.permutation(N) % 5
    h, w = rng.integers(h_min, h_max + 1, N), rng.integers(w_min, w_max + 1, N)
    i, j = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for n in range(N):
        if kind[n] == 1:
            i[n], j[n] = (rng.integers(*R.corner_range(True, e, b)) for e in (h[n], w[n]))
        elif kind[n] == 2:                                                  # one or two rows / columns past the edge
            h[n], w[n] = max(h[n], 2), max(w[n], 2)
            i[n], j[n] = b - h[n] + 1, b - w[n] + (2 if w[n] > 2 else 1)
        elif kind[n] == 3:                                                  # the far side's last row, outside for a small h
            h[n] = h_min
            i[n], j[n] = b - h[n] + 5, min(mid + 6, b - 1)
        elif kind[n] == 4:
            if n & 1:
                h[n], w[n], i[n], j[n] = h_max, w_max, 0, 0
            else:
                h[n], w[n], i[n], j[n] = h_min, w_min, mid + 6, R.corner_range(False, w_min, b)[1] - 1
    rec = {"hflip": idx & 1, "vflip": (idx >> 1) & 1, "k": (idx >> 2) & 3, "erase": (kind > 0).astype(np.int64), "i": i, "j": j,
           "h": h, "w": w, "angle": angle, "weak": weak.astype(np.int64), "kind": kind}
    rec["coef"] = np.array([R.IDENTITY if weak[n] else R.rotation_coefficients(angle[n], b) for n in range(N)])
    return rec


def pil_chain(g, r, n):
    """g (2, b, b) uint8 -> (2, b, b) uint8"""
    b = g.shape[-1]
    img = Image.merge("LA", [Image.fromarray(g[0]), Image.fromarray(g[1])])
    if r["hflip"][n]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if r["vflip"][n]:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    if not r["weak"][n]:
        img = img.rotate(float(r["angle"][n]), resample=Image.NEAREST, expand=False, center=None, fillcolor=(0, 0))
    x = np.asarray(img).transpose(2, 0, 1).copy()                           # ToTensor (levels kept as integers)
    if r["erase"][n]:
        i, j, h, w = (int(r[f][n]) for f in "ijhw")
        x[:, i:i + h, j:j + w] = 255                                        # F.erase: the slice clips to the image
    return np.rot90(x, int(r["k"][n]), axes=(1, 2)).copy()


def gen():
    out = {}
    for b in BBOXES:
        rng = np.random.default_rng(2330 + b)
        r = records(rng, b)
        crops = np.stack([np.stack([make_crop(rng, b), make_crop(rng, b)]) for _ in range(N)])
        out["crops_%d" % b] = crops
        out["views_%d" % b] = np.stack([pil_chain(crops[n], r, n) for n in range(N)]).astype(np.uint8)
        for k, v in r.items():
            out["%s_%d" % (k, b)] = v.astype(np.float32 if k == "angle" else np.int32)
    path = os.path.join(HERE, "augment2d3d.npz")
    np.savez_compressed(path, **out)
    print("wrote augment2d3d.npz (%d bytes):" % os.path.getsize(path), {k: v.shape for k, v in out.items() if k[:5] in ("crops", "views")})


if __name__ == "__main__":
    gen()
