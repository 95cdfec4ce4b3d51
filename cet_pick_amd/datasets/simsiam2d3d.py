"""Datasets of the 2d3d exploration mode (task 'simsiam2d3d', arch simsiam2d3d_18): tilt-series patches paired with tomogram
patches.  `TOMOPreProjAngleSelect2D3D.load_data` (datasets/tomo_pre_proj_angle_select_new2d3d.py:153-233) on the device:

    tilts with angle in [low, up] -> DoG picks on the tomogram (`--dog`) -> the pick border rule (:189) -> centre variants
    (test: the pick; train: the pick, (x, y, z+1), (x, y, z-1), (x-1, y, z-1), (x, y+1, z-1); z at full resolution, 2z under
    --compress) -> tilt patches of every variant in ONE launch (`mi_tilt_patches`) + tomogram patches of slice z_full // 2
    (--compress) or z (`mi_crop_normalize_table`, one launch) -> device-side compaction of the valid masks -> dataset mean /
    std of the kept unshifted patches (:227-230, unbiased std).

Batches are {'input', 'input_3d', 'input_aug', 'input_aug_3d'} and nothing else (the step engine captures every tensor of a
batch): view 1 is the pick's patch pair, view 2 one of its valid shifted variants drawn with the epoch-seeded RNG
(datasets/particle_pre_2d_proj_new2d3d.py:81 `np.random.randint(1, n)`), both through the per-channel 8-bit round trip and
`Normalize((mean_subvols, mean_subvols3d), (std_subvols, std_subvols3d))` of the reference transforms.  With `--augment
reference` the train split serves the reference's random views instead (:49-82): the strong chain (flips, RandomRotation(30),
CornerErasing, quarter turn) on the pick's pair, the weak chain (the same without the rotation) on the drawn variant's, both
channels of a view through one set of parameters, drawn and applied on the device (datasets/augment.py, two launches a batch).

  TomoFileSimSiam2D3DDataset     the 4-column image list (image_name, rec_path, tilt_path, angle_path) of --train_img_txt /
                                 --test_img_txt under --data_dir
  SyntheticSimSiam2D3DDataset    synthetic tomograms (make_tomo) and tilt series projected from them (make_tilt_series)
"""
import os

import numpy as np
import torch

from ..synthetic import make_tilt_series, make_tomo
from ..utils import image as Im
from ..utils import loader as Ld
from . import subvols as S

# (dx, dy, dz) of the training variants, in the reference's order (:192-196); variant 0 is the pick itself
TRAIN_SHIFTS = ((0, 0, 0), (0, 0, 1), (0, 0, -1), (-1, 0, -1), (0, 1, -1))
TEST_SHIFTS = ((0, 0, 0),)


def require_even_bbox(bbox):
    if int(bbox) % 2:
        raise ValueError("the 2d3d mode needs an even --bbox (got %d): the reference's tilt windows `t -/+ c//2` are c - 1 "
                         "pixels wide for an odd c" % int(bbox))


def pick_centres(coords, h, w, crop_x, crop_y, compress, shifts):
    """The border rule of :189 and the centre variants of :190-196 for the DoG picks `coords` (n, 3) of one tomogram.
    -> (kept picks (m, 3), tilt centres (m, V, 3) as (x, y, z_full), tomogram centres (m, V, 3) as (x, y, slice))."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    bx, by = S.tilt_border(crop_x), S.tilt_border(crop_y)
    keep = (c[:, 0] > bx) & (c[:, 0] < w - bx) & (c[:, 1] >= by) & (c[:, 1] <= h - by)
    c = c[keep]
    full = c.copy()
    if compress:
        full[:, 2] *= 2
    tilt = full[:, None, :] + np.asarray(shifts, dtype=np.int64)[None]
    rec = tilt.copy()
    if compress:
        rec[..., 2] //= 2                                   # extract_3d_tomo :101-102 `int(z // 2)`
    return c, tilt, rec


def keep_mask(valid):
    """Which picks a split keeps, from the (n, V) validity of their variants' tilt patches (variant 0 = the pick): test
    (V == 1) keeps a pick whose own patch is valid (:214-218); train also needs a valid shifted copy (:205
    `len(patch_sets) > 1`).  Works on bool tensors of any device."""
    return valid[:, 0] if valid.shape[1] == 1 else valid[:, 0] & valid[:, 1:].any(1)


class SimSiam2D3DDataset:
    """The common part of both 2d3d datasets: `_build(items)` with items = [(name, tilt series (T, H, W), tomogram (Z', H, W),
    angles (T,) degrees)], device tensors in [0, 1].  Attributes as the reference's (`tomos` = the selected tilts, `angles`,
    `names`, `names_all`, `coords`, `subvols`, `sub_vols_3d`, `mean_subvols(3d)`, `std_subvols(3d)`), plus the training sets
    `patches_2d` / `patches_3d` (n, V, 1, bbox, bbox) with their validity `set_valid` (n, V)."""
    num_classes = 256
    default_resolution = [24, 24]
    low, up = -20, 20

    def _setup(self, opt, split, size, sigma1, rank, world):
        self.opt, self.split, self.size = opt, split, tuple(int(s) for s in size)
        require_even_bbox(self.size[1])
        require_even_bbox(self.size[2])
        self.sigma1 = list(sigma1)
        self.compress = bool(getattr(opt, "compress", False))
        self.batch_size = max(1, int(getattr(opt, "batch_size", 8)))
        self.rank, self.world, self.epoch, self.seed = rank, world, 0, int(getattr(opt, "seed", 317))

    def _build(self, items, border_z=10):
        cx, cy = self.size[1], self.size[2]
        shifts = TRAIN_SHIFTS if self.split == "train" else TEST_SHIFTS
        V = len(shifts)
        self.tomos, self.angles, self.names = {}, {}, []
        stacks, recs, picks, tilt_c, rec_c, owner, name_of = [], [], [], [], [], [], []
        for name, tilts, rec, angles in items:
            d, h, w = (int(s) for s in rec.shape)
            if tuple(tilts.shape[1:]) != (h, w):
                raise ValueError("%s: tilt images %s differ from the tomogram's (H, W) %s" % (name, tuple(tilts.shape[1:]), (h, w)))
            S.check_tilt_crop(cx, cy, h, w)
            a = np.asarray(angles, dtype=np.float64).ravel()
            used = np.nonzero((a >= self.low) & (a <= self.up))[0]
            used_v = tilts.index_select(0, torch.as_tensor(used, device=tilts.device)).contiguous()
            self.tomos[name], self.angles[name] = used_v, a[used]
            self.names.append(name)
            _, c = Im.get_potential_coords_pyramid(rec, sigmas=self.sigma1, border_z=border_z)
            c, tc, rc = pick_centres(c, h, w, cx, cy, self.compress, shifts)
            stacks.append((used_v, a[used], 2 * d if self.compress else d))
            recs.append(rec.contiguous())
            picks.append(c)
            tilt_c.append(tc.reshape(-1, 3))
            rec_c.append(rc.reshape(-1, 3))
            owner.append(np.full(len(c) * V, len(stacks) - 1, dtype=np.int32))
            name_of += [name] * len(c)
        picks = np.concatenate(picks, 0)
        n = len(picks)
        if n == 0:
            raise RuntimeError("the DoG picker found no particle inside the 2d3d border rule (sigma %s)" % (self.sigma1,))
        owner = np.concatenate(owner)
        # every variant of every pick of every tomogram: one launch for the tilt patches, one for the tomogram patches
        p2, valid = S.TiltStacks(stacks).patches(np.concatenate(tilt_c, 0), cx, cy, owner=owner)
        p3 = S.CropTable(recs, owner, np.concatenate(rec_c, 0)).cut(None, 0, n * V, (1, cy, cx), mode=S.SUMZ_MINMAX)
        valid = valid.view(n, V)
        keep = keep_mask(valid)
        kept = torch.nonzero(keep).view(-1)
        self.patches_2d = p2.view(n, V, 1, cy, cx).index_select(0, kept)
        self.patches_3d = p3.view(n, V, 1, cy, cx).index_select(0, kept)
        self.set_valid = valid.index_select(0, kept)
        self._set_valid_host = self.set_valid.cpu().numpy()
        k_host = kept.cpu().numpy()
        if len(k_host) == 0:
            raise RuntimeError("no 2d3d pick keeps a valid tilt patch%s" % (" and a valid shifted copy" if V > 1 else ""))
        self.coords = [row for row in picks[k_host]]
        self.names_all = [name_of[i] for i in k_host]
        self.subvols = self.patches_2d[:, 0]
        self.sub_vols_3d = self.patches_3d[:, 0]
        self.mean_subvols, self.std_subvols = S.subvol_mean_std(self.subvols)
        self.mean_subvols3d, self.std_subvols3d = S.subvol_mean_std(self.sub_vols_3d)
        # both channels through ToPILImage -> ToTensor -> Normalize, once (the transform is deterministic)
        self.normed_2d = S.to_uint8_normalize(self.patches_2d, self.mean_subvols, self.std_subvols)
        self.normed_3d = S.to_uint8_normalize(self.patches_3d, self.mean_subvols3d, self.std_subvols3d)
        self.num_samples = len(k_host)
        self._build_augmenter()
        print("Loaded {} {} samples".format(self.split, self.num_samples))

    def _build_augmenter(self):
        """--augment reference, train split: the device-side augmenter over the two patch banks (datasets/augment.py)."""
        self.augmenter = None
        if getattr(self.opt, "augment", "mirror") != "reference" or self.split != "train":
            return
        from .augment import PairViewAugmenter
        self.augmenter = PairViewAugmenter(self.patches_2d, self.patches_3d, (self.mean_subvols, self.mean_subvols3d),
                                           (self.std_subvols, self.std_subvols3d), self.seed)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):                      # batches per epoch and rank (drop_last, like the reference's loaders)
        return (self.num_samples // self.world) // self.batch_size

    def epoch_views(self):
        """(this rank's sample order, the second view's variant of every sample) of the epoch: one seeded permutation,
        rank-strided, and per sample a uniform draw among its valid shifted variants."""
        rng = np.random.default_rng(self.seed + 1000 * self.epoch)
        order = rng.permutation(self.num_samples)
        sv = self._set_valid_host
        if sv.shape[1] == 1:
            var = np.zeros(self.num_samples, dtype=np.int64)
        else:
            aug = sv[:, 1:]
            r = rng.integers(0, aug.sum(1))                                     # r-th valid shifted variant
            var = 1 + np.argmax(np.cumsum(aug, 1) > r[:, None], 1)
        return order[self.rank::self.world], var

    def __iter__(self):
        order, var = self.epoch_views()
        dev = self.normed_2d.device
        var = torch.as_tensor(var, device=dev)
        for i in range(len(self)):
            idx = torch.as_tensor(order[i * self.batch_size:(i + 1) * self.batch_size], device=dev)
            v = var[idx]
            if self.augmenter is not None:
                x, x3, a, a3 = self.augmenter.views(idx, v, self.epoch)
                yield {"input": x, "input_3d": x3, "input_aug": a, "input_aug_3d": a3}
                continue
            yield {"input": self.normed_2d[idx, 0], "input_3d": self.normed_3d[idx, 0],
                   "input_aug": self.normed_2d[idx, v], "input_aug_3d": self.normed_3d[idx, v]}


def load_listed_2d3d(opt, split="train"):
    """[(name, tilt series, tomogram, angles)] of the split's 4-column list (loader.py:139-152, orders fixed)."""
    from .tomo_files import read_image_list_2d3d
    txt = opt.train_img_txt if split == "train" else opt.test_img_txt
    rows = read_image_list_2d3d(os.path.join(opt.data_dir, txt))
    names, recs, tilts, angs = zip(*rows)
    t, r, a = Ld.load_tomo_all_and_angles_from_list(names, tilts, recs, angs, compress=bool(getattr(opt, "compress", False)),
                                                    denoise=getattr(opt, "gauss", 0))
    return [(n, t[n], r[n], a[n]) for n in names]


def on_device(device):
    """Context that makes `device` (an MI355X device, e.g. 'cuda' or 'cuda:1') current while a dataset loads and builds: the
    loader and the kernels allocate on the current device."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the 2d3d datasets run on the MI355X (cuda) device; there is no CPU path (device %s)" % dev)
    return torch.cuda.device(dev)


class TomoFileSimSiam2D3DDataset(SimSiam2D3DDataset):
    """`TOMOPreProjAngleSelect2D3D` (:25-233) on listed tilt series and tomograms."""

    def __init__(self, opt, split, size, low=-20, up=20, sigma1=(2.5, 5), device="cuda", rank=0, world=1):
        self.low, self.up = low, up
        self._setup(opt, split, size, sigma1, rank, world)
        with on_device(device):
            self._build(load_listed_2d3d(opt, split))


class SyntheticSimSiam2D3DDataset(SimSiam2D3DDataset):
    """The same dataset on synthetic tomograms and tilt series projected from them (angles -60..60 in steps of 3, so the
    [-20, 20] selection matters), preprocessed by the device loader as listed files are."""

    def __init__(self, opt, split, size, sigma1=(2.5, 5), shape=(32, 192, 192), n_tomos=2, angles=tuple(range(-60, 61, 3)),
                 device="cuda", rank=0, world=1):
        self._setup(opt, split, size, sigma1, rank, world)
        with on_device(device):
            items = []
            for t in range(n_tomos):
                vol, _ = make_tomo(shape, seed=self.seed + t, margin_xy=min(40, shape[1] // 4), margin_z=min(12, shape[0] // 4))
                tilts = Ld.load_rec(make_tilt_series(vol, angles), "zxy", False, is_tilt=True)
                rec = Ld.load_rec(vol, "zxy", self.compress)                    # (the arrays are (Z, H, W) already)
                items.append(("synthetic_%d" % t, Ld.preprocess(tilts, is_tilt=True), Ld.preprocess(rec, is_tilt=False),
                              np.asarray(angles, np.float64)))
            # (a short synthetic tomogram has few slices: the reference's 10-slice z border is a parameter here)
            self._build(items, border_z=min(10, shape[0] // 4))


class ArraySimSiam2D3DDataset(SimSiam2D3DDataset):
    """The dataset on tilt series and tomograms already in memory: items = [(name, tilts (T, H, W), tomogram (Z', H, W),
    angles (T,) degrees)], arrays or device tensors, used as given (no preprocessing)."""

    def __init__(self, opt, split, size, items, sigma1=(2.5, 5), border_z=10, device="cuda", rank=0, world=1):
        self._setup(opt, split, size, sigma1, rank, world)
        dev = torch.device(device)
        with on_device(dev):
            self._build([(n, torch.as_tensor(t, dtype=torch.float32).to(dev), torch.as_tensor(r, dtype=torch.float32).to(dev), a)
                         for n, t, r, a in items], border_z=border_z)
