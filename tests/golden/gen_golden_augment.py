"""Golden vectors of the view augmentation -> augment2d.npz, made with PIL (the calls torchvision's PIL back end makes
for ToPILImage, RandomHorizontalFlip / RandomVerticalFlip, ColorJitter on a one-channel image, RandomResizedCrop, and
numpy's rot90 for FixedRotation).  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_augment.py

Per bbox (36, 32): 32 seeded crops with explicit parameter records - every (hflip, vflip, bright_first) combination with
every k, and four classes of eight records each:
    0  factors exactly 1, s == bbox   (flips and rotation only)        2  factors exactly 1, s < bbox
    1  jitter, s == bbox                                               3  jitter, s < bbox
with the ends of the jitter and area ranges among them.  Stored: the crops as uint8 grey levels (the kernel's input is
(g + 0.5) / 255), the records, the expected views as uint8 grey levels.
"""
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
BBOXES = (36, 32)


def make_crop(rng, b):
    """A min-max'ed crop like the dataset's: a few blobs on noise, levels 0 and 255 both present."""
    yy, xx = np.mgrid[0:b, 0:b]
    img = rng.standard_normal((b, b)) * 0.6
    for _ in range(int(rng.integers(1, 4))):
        cy, cx, r = rng.uniform(4, b - 4), rng.uniform(4, b - 4), rng.uniform(2.0, 6.0)
        img -= rng.uniform(1.5, 3.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    img = (img - img.min()) / (img.max() - img.min())
    return np.floor(np.float32(img) * np.float32(255)).astype(np.uint8)


def records(rng, b):
    n = 32
    idx = np.arange(n)
    rec = {"hflip": idx & 1, "vflip": (idx >> 1) & 1, "bright_first": (idx >> 2) & 1, "k": (idx >> 3) & 3}
    cls = rng.permutation(n) % 4
    jitter, small = (cls & 1) == 1, cls >= 2
    fb = rng.uniform(0.5, 1.5, n).astype(np.float32)
    fc = rng.uniform(0.8, 1.2, n).astype(np.float32)
    j_idx = np.nonzero(jitter)[0]
    fb[j_idx[:2]], fc[j_idx[2:4]] = (0.5, 1.5), (0.8, 1.2)                     # the ends of the ranges
    s_min = int(round(b * np.sqrt(0.8)))
    s = rng.integers(s_min, b, n)                                              # s < bbox
    s[np.nonzero(small)[0][:2]] = (s_min, b - 1)
    rec["brightness"] = np.where(jitter, fb, np.float32(1)).astype(np.float32)
    rec["contrast"] = np.where(jitter, fc, np.float32(1)).astype(np.float32)
    rec["s"] = np.where(small, s, b)
    rec["i"] = rng.integers(0, b - rec["s"] + 1)
    rec["j"] = rng.integers(0, b - rec["s"] + 1)
    rec["cls"] = cls
    return {k: np.asarray(v) for k, v in rec.items()}


def pil_chain(g0, r, n):
    b = g0.shape[0]
    img = Image.fromarray(g0, mode="L")
    if r["hflip"][n]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if r["vflip"][n]:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    fb, fc = float(r["brightness"][n]), float(r["contrast"][n])
    if r["bright_first"][n]:
        img = ImageEnhance.Contrast(ImageEnhance.Brightness(img).enhance(fb)).enhance(fc)
    else:
        img = ImageEnhance.Brightness(ImageEnhance.Contrast(img).enhance(fc)).enhance(fb)
    s, i, j = int(r["s"][n]), int(r["i"][n]), int(r["j"][n])
    img = img.crop((j, i, j + s, i + s)).resize((b, b), Image.BILINEAR)
    return np.rot90(np.asarray(img), int(r["k"][n])).copy()


def gen():
    out = {}
    for b in BBOXES:
        rng = np.random.default_rng(3170 + b)
        r = records(rng, b)
        crops = np.stack([make_crop(rng, b) for _ in range(32)])
        out["crops_%d" % b] = crops
        out["views_%d" % b] = np.stack([pil_chain(crops[n], r, n) for n in range(32)]).astype(np.uint8)
        for k, v in r.items():
            out["%s_%d" % (k, b)] = v.astype(np.float32 if k in ("brightness", "contrast") else np.int32)
    np.savez_compressed(os.path.join(HERE, "augment2d.npz"), **out)
    print("wrote augment2d.npz:", {k: v.shape for k, v in out.items() if k.startswith(("crops", "views"))})


if __name__ == "__main__":
    gen()
