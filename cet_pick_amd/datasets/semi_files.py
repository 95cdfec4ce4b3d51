"""File-backed dataset of the refinement (detector) training, task 'semi' with `--dataset semi`: the reference's `TOMOMoco`
(datasets/tomo_moco.py) + `ParticleMocoDataset` (datasets/particle_moco.py) on the device.

    image list (`read_image_list`) -> utils.loader.load_tomos_from_list (order, compress, gauss)
    coordinate table (`read_coord_list`: image_name, x_coord, y_coord, z_coord) -> particles downscaled to (x//2, y//2, z)
        (z//2 under --compress) -> one label volume (D, H//2, W//2) per tomogram (`mi_semi_labels`: the reference's
        stencil max-combined at every particle; train: every exact 0 becomes -1, "unlabeled")
    train: every annotation is one sample; the epoch's own / partner centres are drawn on the host (`draw_pairs`) and copied
        to the device once per epoch; a batch is one `mi_semi_pairs` launch: input (2B, 6, 64, 64), input_aug (the same
        mirrored along x, or y when flip_prob > 0.5) and hm (2B, 1, 6, 32, 32), crops ordered own_0, partner_0, own_1, ...
    val: one sample per listed image (images without particles included): the whole tomogram and its label volume, or
        tomo[:110, 200:700, 200:700] / hm[:110, 100:350, 100:350] when D >= 100 and H > 512 (particle_moco.py:164-177)

         meta['gt_det']: the tomogram's downscaled (x, y, z) centres shifted into that window and filtered to it (`window_gt_det`;
         the reference leaves them unshifted)

    --pn (fully annotated tomograms) is `TomoFileSupervisedDataset`: the training labels keep their zeros (no -1) and the partner
        crop is a random place of the partner's tomogram or a wider neighbourhood of its annotation (`draw_pairs(pn=True)`); the
        kernels are the same.  Each class refuses the other's option set.

Out of scope: the unused batch keys (hm_aug, ind, pair_*), a CPU path.  (--ge changes the loss alone,
trains/tomo_cr_semi_trainer.py: the batches are these.)
"""
import math
import os

import numpy as np
import torch

from .. import _lib as L
from ..utils import loader as Ld
from .tomo_files import read_image_list

CROP_Z, CROP, CROP_HM = 6, 64, 32           # (6, 64, 64) input crops, (6, 32, 32) label crops: down_ratio 2 only
EDGE_XY, EDGE_Z = 17, 3                     # the clip window of a downscaled centre: [17, W//2 - 17] x [17, H//2 - 17] x [3, D - 3]
COORD_COLUMNS = ("image_name", "x_coord", "y_coord", "z_coord")


# ---- labels -------------------------------------------------------------------------------------------------------------

def gaussian_radius(height, width, min_overlap=0.7):
    """CenterNet's radius rule (utils/image.py:538-558): the smallest of the three quadratic roots, in float64."""
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * 1 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + np.sqrt(b2 ** 2 - 4 * 4 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def label_radius(bbox, down_ratio=2):
    """tomo_moco.py:103-107: int(gaussian_radius((ceil(h), ceil(h)))) with h = bbox // down_ratio."""
    h = math.ceil(int(bbox) // int(down_ratio))
    return max(0, int(gaussian_radius(h, h)))


def label_stencil(radius, fiber=False):
    """The (2r+1)^3 stamp of `draw_umich_gaussian_3d` in float64, cast once to float32: `gaussian3D` (sigma = (2r+1)/6,
    values below eps * max -> 0, above 0.9 -> 1) or, with --fiber, `gaussian3D_discrete(label1=1, label2=0, thresh=0.2)`."""
    d = 2 * int(radius) + 1
    sigma = d / 6
    a = np.arange(-radius, radius + 1, dtype=np.float64)
    y, x, z = a[:, None, None], a[None, :, None], a[None, None, :]
    h = np.exp(-(x * x + y * y + z * z) / (2 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    if fiber:
        h[h >= 0.2] = 1
        h[h < 0.2] = 0
    else:
        h[h > 0.9] = 1
    return h.astype(np.float32)


def downscale(coords, compress=False):
    """tomo_moco.py:58-64 on (n, 3) int coordinates: (x // 2, y // 2, z), z // 2 under --compress (floor division)."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    return np.stack([c[:, 0] // 2, c[:, 1] // 2, c[:, 2] // 2 if compress else c[:, 2]], 1).astype(np.int32)


def render_labels(shape, centres, stencil, fill_unlabeled, device="cuda"):
    """The label volume (D, H, W) of `centres` (n, 3) downscaled (x, y, z): one `mi_semi_labels` call."""
    D, H, W = (int(s) for s in shape)
    st = np.ascontiguousarray(stencil, dtype=np.float32)
    r = (st.shape[0] - 1) // 2
    if st.shape != (2 * r + 1,) * 3 or (st < 0).any():
        raise ValueError("the label stencil must be a (2r+1)^3 array of values >= 0, got %s" % (st.shape,))
    c = np.ascontiguousarray(np.asarray(centres, dtype=np.int32).reshape(-1, 3))
    hm = torch.empty((D, H, W), dtype=torch.float32, device=device)
    L.require_cuda(hm, "hm")
    st_d = torch.as_tensor(st).to(device)
    c_d = torch.as_tensor(c).to(device)
    L.call("mi_semi_labels", hm, D, H, W, c_d, len(c), st_d, r, int(bool(fill_unlabeled)))
    return hm


# ---- coordinate files ---------------------------------------------------------------------------------------------------

def read_coord_list(path, names):
    """The reference's tab-separated coordinate table (utils/coordinates.py:14-24): columns found by their header name,
    others ignored; values parsed as float and truncated toward zero (`astype(np.int32)`).  -> {name: (n, 3) int32 (x, y, z)}
    for every name of `names` (no row: zero particles); rows of other images are dropped and counted in one line."""
    if not os.path.isfile(path):
        raise FileNotFoundError("coordinate file %s not found (--train_coord_txt / --val_coord_txt under --data_dir)" % path)
    with open(path) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f if ln.strip()]
    header = lines[0].split("\t") if lines else []
    if "source" in header:
        raise ValueError("%s: a `source` column is not supported (the reference then matches no coordinate to any image)"
                         % path)
    missing = [c for c in COORD_COLUMNS if c not in header]
    if missing:
        raise ValueError("%s: the coordinate table needs the tab-separated columns %s; missing %s (header %s)"
                         % (path, " ".join(COORD_COLUMNS), " ".join(missing), header))
    idx = [header.index(c) for c in COORD_COLUMNS]
    listed = set(names)
    rows = {n: [] for n in names}
    dropped = 0
    for k, ln in enumerate(lines[1:], start=2):
        cols = ln.split("\t")
        if len(cols) <= max(idx):
            raise ValueError("%s line %d: %d columns, the header names %d" % (path, k, len(cols), len(header)))
        name = cols[idx[0]]
        if name not in listed:
            dropped += 1
            continue
        try:
            rows[name].append([float(cols[i]) for i in idx[1:]])
        except ValueError:
            raise ValueError("%s line %d: coordinates %s are not numbers" % (path, k, [cols[i] for i in idx[1:]])) from None
    if dropped:
        print("[cet_pick_amd] %s: %d coordinate rows name images that are not listed, dropped" % (path, dropped))
    return {n: np.asarray(v, dtype=np.float64).reshape(-1, 3).astype(np.int32) for n, v in rows.items()}


# ---- the epoch sampler --------------------------------------------------------------------------------------------------

def clip_centres(c, shapes):
    """particle_moco.py:124-131: downscaled (x, y, z) into [17, W//2 - 17] x [17, H//2 - 17] x [3, D - 3] of each centre's own
    tomogram; shapes (n, 3) = (D, H, W) per centre."""
    c = np.asarray(c, dtype=np.int64)
    s = np.asarray(shapes, dtype=np.int64)
    return np.stack([np.clip(c[:, 0], EDGE_XY, s[:, 2] // 2 - EDGE_XY), np.clip(c[:, 1], EDGE_XY, s[:, 1] // 2 - EDGE_XY),
                     np.clip(c[:, 2], EDGE_Z, s[:, 0] - EDGE_Z)], 1)


def draw_pairs(anns, shapes, bbox, translation_ratio, seed, epoch, rank=0, world=1, batch_size=1, return_index=False, pn=False):
    """One epoch of training pairs for one rank (particle_moco.py:34-131).

    anns: (n, 4) downscaled (x, y, z, tomogram); shapes: (T, 3) tomogram extents (D, H, W).  With a Generator seeded from
    (seed, epoch), for every annotation a: own offsets x, y uniform in [-4, 4] (a z offset is drawn and, as in the reference,
    not applied), a partner b != a uniform over the others and, with p = random(): p <= 0.8 -> x, y in [-5, 5), z in [-2, 2);
    otherwise x, y in [-tp, tp), tp = int(bbox * translation_ratio), z in [-2, 2).  Both centres are clipped (`clip_centres`).
    The permutation of the annotations is split over the ranks as DistributedSampler does with drop_last, and cut to whole
    batches.  -> owner (2m,) int32, centres (2m, 3) int32 ordered [own_0, partner_0, own_1, ...], flip_prob (m // batch_size,)
    (+ the own and partner annotation indices (m,) with return_index)

    pn (--pn, :55-86): the partner's centre is instead, with q = random(): q <= 0.5 -> a random place of the partner's tomogram, x
    uniform in [0, W), y in [0, H), z in [0, D) - the FULL-resolution extents against the downscaled clip window, as in the
    reference, so about half of these draws end on the upper clip; otherwise the partner's annotation + x, y in [-tp, tp), z in
    [-5, 5).  Its numbers are drawn after all of the above: the own crops, the partners and the permutation are those of pn=False.
    (return_index then also gives, per pair, whether the partner took the random-place branch)"""
    anns = np.asarray(anns, dtype=np.int64).reshape(-1, 4)
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    n = len(anns)
    if n < 2:
        raise ValueError("the detector training needs at least 2 annotations (a partner is drawn among the others), got %d" % n)
    tp = int(bbox * translation_ratio)
    if tp < 1:
        raise ValueError("--bbox %s x --translation_ratio %s gives a partner translation range of 0 pixels" % (bbox, translation_ratio))
    rng = np.random.default_rng([int(seed), int(epoch)])
    perm = rng.permutation(n)
    own_xy = rng.integers(-4, 5, size=(n, 2))
    rng.integers(-1, 2, size=n)                                       # off_z: drawn, never applied (:47-50)
    partner = rng.integers(0, n - 1, size=n)
    partner += partner >= np.arange(n)
    p = rng.random(n)
    near_xy = rng.integers(-5, 5, size=(n, 2))
    far_xy = rng.integers(-tp, tp, size=(n, 2))
    part_z = rng.integers(-2, 2, size=n)
    part_off = np.concatenate([np.where((p <= 0.8)[:, None], near_xy, far_xy), part_z[:, None]], 1)
    own_off = np.concatenate([own_xy, np.zeros((n, 1), np.int64)], 1)
    part_pos = anns[partner, :3] + part_off                           # unclipped partner centre of every annotation
    if pn:
        q = rng.random(n)
        ext = shapes[anns[partner, 3]]                                # (D, H, W) of every annotation's partner tomogram
        anywhere = np.stack([rng.integers(0, ext[:, 2]), rng.integers(0, ext[:, 1]), rng.integers(0, ext[:, 0])], 1)
        near = np.concatenate([rng.integers(-tp, tp, size=(n, 2)), rng.integers(-5, 5, size=(n, 1))], 1)
        part_pos = np.where((q <= 0.5)[:, None], anywhere, anns[partner, :3] + near)

    per = n // world
    count = (per // batch_size) * batch_size
    a = perm[:per * world][rank::world][:count]
    b = partner[a]
    own = clip_centres(anns[a, :3] + own_off[a], shapes[anns[a, 3]])
    par = clip_centres(part_pos[a], shapes[anns[b, 3]])
    owner = np.empty(2 * count, np.int32)
    centres = np.empty((2 * count, 3), np.int32)
    owner[0::2], owner[1::2] = anns[a, 3], anns[b, 3]
    centres[0::2], centres[1::2] = own, par
    flip = np.random.default_rng([int(seed), int(epoch), int(rank), 1]).random(count // batch_size)
    if return_index and pn:                                           # + which partners took the random-place branch
        return owner, centres, flip, a, b, (q <= 0.5)[a]
    return (owner, centres, flip, a, b) if return_index else (owner, centres, flip)


def check_windows(owner, centres, shapes):
    """Every crop window of a drawn table lies inside its tomogram (input) and its label volume (hm)."""
    s = np.asarray(shapes, dtype=np.int64)[np.asarray(owner, dtype=np.int64)]
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 3)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    ok = ((z - CROP_Z // 2 >= 0) & (z + CROP_Z // 2 <= s[:, 0]) & (2 * y - CROP // 2 >= 0) & (2 * y + CROP // 2 <= s[:, 1]) &
          (2 * x - CROP // 2 >= 0) & (2 * x + CROP // 2 <= s[:, 2]) & (y - CROP_HM // 2 >= 0) &
          (y + CROP_HM // 2 <= s[:, 1] // 2) & (x - CROP_HM // 2 >= 0) & (x + CROP_HM // 2 <= s[:, 2] // 2))
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise ValueError("crop %d: centre %s leaves tomogram extents %s" % (i, c[i].tolist(), s[i].tolist()))


def _descriptors(vols, device):
    """struct mi_vol_desc {const float* vol; int32 D, H, W, reserved} per volume, as a device array"""
    desc = np.zeros((len(vols), 3), dtype=np.int64)
    for i, v in enumerate(vols):
        d, h, w = (int(a) for a in v.shape)
        desc[i] = (v.data_ptr(), d | (h << 32), w)
    return torch.as_tensor(desc).to(device)


def semi_pairs(tomo_desc, label_desc, n_tomos, owner, centres, first, n, flip_y, out=None):
    """One `mi_semi_pairs` launch: crops [first, first + n) of a device table -> (input, input_aug, hm)."""
    dev = owner.device
    if out is None:
        out = (torch.empty((n, CROP_Z, CROP, CROP), dtype=torch.float32, device=dev),
               torch.empty((n, CROP_Z, CROP, CROP), dtype=torch.float32, device=dev),
               torch.empty((n, 1, CROP_Z, CROP_HM, CROP_HM), dtype=torch.float32, device=dev))
    if first < 0 or n < 0 or first + n > int(owner.numel()) or int(centres.numel()) != 3 * int(owner.numel()):
        raise L.HipExtensionError("semi_pairs: crops [%d, %d) outside a table of %d" % (first, first + n, int(owner.numel())))
    inp, aug, hm = out
    L.call("mi_semi_pairs", tomo_desc, label_desc, int(n_tomos), owner, centres, int(first), int(n), int(bool(flip_y)), inp, aug, hm)
    return inp, aug, hm


# ---- the dataset --------------------------------------------------------------------------------------------------------

def val_window(shape):
    """particle_moco.py:168-171: the (input, label) slices of a val tomogram of extents (D, H, W)."""
    D, H, W = shape
    if D >= 100 and H > 512:
        return (slice(0, 110), slice(200, 700), slice(200, 700)), (slice(0, 110), slice(100, 350), slice(100, 350))
    return (slice(None),) * 3, (slice(None),) * 3


def window_gt_det(centres, shape):
    """The ground-truth centres of a val sample: `centres` (n, 3) downscaled (x, y, z) of a tomogram of extents `shape`
    (D, H, W), shifted by the origin of `val_window`'s label window and filtered to it.  -> (m, 3) float32.  Host only."""
    D, H, W = (int(s) for s in shape)
    _, wl = val_window((D, H, W))
    z0, z1, _ = wl[0].indices(D)
    y0, y1, _ = wl[1].indices(H // 2)
    x0, x1, _ = wl[2].indices(W // 2)
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 3)
    keep = ((c[:, 0] >= x0) & (c[:, 0] < x1) & (c[:, 1] >= y0) & (c[:, 1] < y1) & (c[:, 2] >= z0) & (c[:, 2] < z1))
    return (c[keep] - np.array([x0, y0, z0], dtype=np.int64)).astype(np.float32)


def net_hm_extent(h):
    """height / width of the detector's heat-map for an input extent h: the stride-2 7x7 stem with padding 3"""
    return (h - 1) // 2 + 1


class TomoFileDetectorDataset:
    """Listed tomograms + a coordinate table -> training crop pairs ('train') or whole-tomogram validation samples ('val').
    Tomograms and label volumes stay on the device."""
    num_classes = 1
    default_resolution = [64, 64]
    pn = False                                  # positive-unlabeled labels and pairs; `TomoFileSupervisedDataset` is the --pn form

    def __init__(self, opt, split, device="cuda", rank=0, world=1):
        self._check_opt(opt, split)
        if split == "train":
            img_txt, coord_txt = opt.train_img_txt, opt.train_coord_txt
        else:
            img_txt, coord_txt = opt.val_img_txt, opt.val_coord_txt
        items = read_image_list(os.path.join(opt.data_dir, img_txt))
        coords = read_coord_list(os.path.join(opt.data_dir, coord_txt), [n for n, _ in items])
        tomos = Ld.load_tomos_from_list([n for n, _ in items], [p for _, p in items], order=opt.order, compress=opt.compress,
                                        denoise=opt.gauss)
        self._setup(opt, split, tomos, coords, device, rank, world)

    @classmethod
    def from_arrays(cls, opt, split, tomos, coords, device="cuda", rank=0, world=1):
        """The dataset of in-memory tomograms {name: (D, H, W) device tensor} and coordinates {name: (n, 3) (x, y, z)} at full
        resolution (names without coordinates have no particle)."""
        cls._check_opt(opt, split)
        self = cls.__new__(cls)
        self._setup(opt, split, dict(tomos), {k: np.asarray(v, dtype=np.int32).reshape(-1, 3) for k, v in coords.items()},
                    device, rank, world)
        return self

    @classmethod
    def _check_opt(cls, opt, split):
        if bool(getattr(opt, "pn", False)) != cls.pn:
            raise NotImplementedError("--pn %s: %s holds the %s labels and pairs; `detector_dataset(opt)` names the class for an "
                                      "option set" % ("set" if not cls.pn else "not set", cls.__name__,
                                                      "fully annotated" if cls.pn else "positive-unlabeled"))
        if split not in ("train", "val"):
            raise ValueError("TomoFileDetectorDataset splits are 'train' and 'val', got %r" % (split,))
        if int(opt.down_ratio) != 2:
            raise ValueError("--down_ratio %d: the detector's crops (6 x 64 x 64 in, 6 x 32 x 32 labels) need --down_ratio 2"
                             % int(opt.down_ratio))

    def _setup(self, opt, split, tomos, coords, device, rank, world):
        self.opt, self.split, self.device = opt, split, torch.device(device)
        self.batch_size = max(1, int(getattr(opt, "batch_size", 1)))
        self.rank, self.world, self.epoch, self.seed = rank, world, 0, int(getattr(opt, "seed", 317))
        self.bbox, self.translation_ratio = int(opt.bbox), float(opt.translation_ratio)
        self.names = list(tomos)
        self.tomos = [L.require_cuda(torch.as_tensor(tomos[n]).to(self.device, torch.float32).contiguous(), "tomogram")
                      for n in self.names]
        for n, t in zip(self.names, self.tomos):
            if t.dim() != 3:
                raise ValueError("tomogram %s: (D, H, W) expected, got %s" % (n, tuple(t.shape)))
        self.radius = label_radius(self.bbox, 2)
        self.stencil = label_stencil(self.radius, bool(getattr(opt, "fiber", False)))
        self.shapes = np.array([tuple(t.shape) for t in self.tomos], dtype=np.int64).reshape(-1, 3)
        self.labels, anns = [], []
        for i, (n, t) in enumerate(zip(self.names, self.tomos)):
            D, H, W = self.shapes[i]
            c = downscale(coords.get(n, np.zeros((0, 3), np.int32)), compress=bool(getattr(opt, "compress", False)))
            # (--pn: fully annotated, the training labels keep their zeros, tomo_moco.py:122-124)
            self.labels.append(render_labels((D, H // 2, W // 2), c, self.stencil, split == "train" and not self.pn, self.device))
            anns.append(np.concatenate([c.astype(np.int64), np.full((len(c), 1), i, np.int64)], 1))
        self.anns = np.concatenate(anns, 0) if anns else np.zeros((0, 4), np.int64)
        self._table_epoch = None
        if split == "train":
            for n, (D, H, W) in zip(self.names, self.shapes):
                if D < CROP_Z or H < 4 * EDGE_XY or W < 4 * EDGE_XY:
                    raise ValueError("tomogram %s is %d x %d x %d: training crops need D >= %d and H, W >= %d"
                                     % (n, D, H, W, CROP_Z, 4 * EDGE_XY))
            if len(self.anns) < 2:
                raise ValueError("the detector training needs at least 2 annotations (a partner is drawn among the others); "
                                 "the coordinate table gives %d for the listed images" % len(self.anns))
            if int(self.bbox * self.translation_ratio) < 1:
                raise ValueError("--bbox %d x --translation_ratio %g gives a partner translation range of 0 pixels"
                                 % (self.bbox, self.translation_ratio))
            self.tomo_desc = _descriptors(self.tomos, self.device)
            self.label_desc = _descriptors(self.labels, self.device)
            self.num_samples = len(self.anns)
        else:
            for n, t, hm in zip(self.names, self.tomos, self.labels):
                wi, wl = val_window(tuple(t.shape))
                xi, xl = t[wi], hm[wl]
                want = (xi.shape[0], net_hm_extent(xi.shape[1]), net_hm_extent(xi.shape[2]))
                if tuple(xl.shape) != want:
                    raise ValueError("val tomogram %s: input %s gives a %s heat-map, the label is %s (odd extents?)"
                                     % (n, tuple(xi.shape), want, tuple(xl.shape)))
            self.gt_dets = [window_gt_det(self.anns[self.anns[:, 3] == i, :3], self.shapes[i]) for i in range(len(self.names))]
            self.num_samples = len(self.names)
        print("Loaded {} {} samples".format(split, self.num_samples))

    def set_epoch(self, epoch):
        """Draw the epoch's pairs and copy its table to the device (once per epoch)."""
        self.epoch = epoch
        if self.split != "train":
            return
        owner, centres, flip = draw_pairs(self.anns, self.shapes, self.bbox, self.translation_ratio, self.seed, epoch,
                                          self.rank, self.world, self.batch_size, pn=self.pn)
        check_windows(owner, centres, self.shapes)
        self.owner = torch.as_tensor(owner).to(self.device)
        self.centres = torch.as_tensor(centres).to(self.device)
        self.flip_prob = flip
        self._table_epoch = epoch

    def __len__(self):
        if self.split != "train":
            return self.num_samples
        return (len(self.anns) // self.world) // self.batch_size

    def __iter__(self):
        if self.split != "train":
            for n, t, hm, gt in zip(self.names, self.tomos, self.labels, self.gt_dets):
                wi, wl = val_window(tuple(t.shape))
                yield {"input": t[wi].contiguous()[None], "hm": hm[wl].contiguous()[None, None],
                       "meta": {"name": [n], "gt_det": gt}}
            return
        if self._table_epoch != self.epoch:
            self.set_epoch(self.epoch)
        B = self.batch_size
        for k in range(len(self)):
            flip = float(self.flip_prob[k])
            inp, aug, hm = semi_pairs(self.tomo_desc, self.label_desc, len(self.tomos), self.owner, self.centres, 2 * k * B,
                                      2 * B, flip > 0.5)
            yield {"input": inp, "input_aug": aug, "hm": hm, "flip_prob": flip, "meta": {}}


class TomoFileSupervisedDataset(TomoFileDetectorDataset):
    """The same for fully annotated tomograms (--pn): the training labels keep their exact zeros (tomo_moco.py:122-124, no -1) and
    the partner crops are drawn by `draw_pairs(pn=True)` (particle_moco.py:55-86).  Validation samples are the parent's."""
    pn = True


def detector_dataset(opt):
    """the file-backed dataset class of an option set"""
    return TomoFileSupervisedDataset if getattr(opt, "pn", False) else TomoFileDetectorDataset
