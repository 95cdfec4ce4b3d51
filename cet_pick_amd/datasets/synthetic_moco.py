"""A dataset with the reference's batch contract ({'input', 'input_aug'}) over a synthetic tomogram:
sub-tomograms are cut and z-normalised on the GPU (datasets/subvols.py), the second view is the
crop shifted by <= 1 voxel and mirrored along x.  With `augment="reference"` both views are the
reference's random 3-D views (datasets/tomo_pre.py:53-62, datasets/particle_pre.py:48-87: blur, noise, in-plane rotation,
margin crop, ZNorm / Rescale / ZNorm, flip, erasure), drawn and applied on the device (datasets/augment.py,
csrc/augment3d.hip).  The reference's MRC I/O is datasets/tomo_files.py."""
import numpy as np
import torch

from ..synthetic import make_tomo
from . import subvols as S

AUGMENTS = ("mirror", "reference")


def centre_border(crop, augment):
    """Voxels a crop centre keeps from every face of its tomogram: crop // 2 + 1 (the shifted second view), plus the margin
    crop // 6 of the random views' source box under `reference`."""
    if augment not in AUGMENTS:
        raise ValueError("augment must be one of %s, got %r" % (AUGMENTS, augment))
    return crop // 2 + 1 + (crop // 6 if augment == "reference" else 0)


class SyntheticMocoLoader:
    """Iterable of batches resident in HBM; `len()` = batches per epoch; `set_epoch` reshuffles
    like DistributedSampler.set_epoch (moco_main.py:155-156)."""

    def __init__(self, shape=(64, 256, 256), crop=32, n_crops=1024, batch_size=64, seed=317, device="cuda",
                 rank=0, world=1, augment="mirror"):
        vol, _ = make_tomo(shape, seed=seed + rank)
        self.vol = torch.as_tensor(vol).to(device)
        g = np.random.default_rng(seed + rank)
        z, h, w = shape
        b = centre_border(crop, augment)
        self.centres = np.stack([g.integers(b, w - b, n_crops), g.integers(b, h - b, n_crops),
                                 g.integers(b, z - b, n_crops)], 1).astype(np.int32)
        self.shift = g.integers(-1, 2, (n_crops, 3)).astype(np.int32)
        self.crop, self.batch_size, self.seed, self.epoch = crop, batch_size, seed, 0
        self.table = S.CropTable([self.vol], np.zeros(n_crops, dtype=np.int32), self.centres, self.shift)
        self._set_augment(augment)

    def _set_augment(self, augment):
        self.augment, self.augmenter = augment, None
        if augment == "reference":
            from .augment import VolumeAugmenter
            self.augmenter = VolumeAugmenter(self.table, self.crop, self.seed)

    def _batch(self, order, b):
        """batch b of the epoch whose device-side order is `order`, on the current stream"""
        c, B = (self.crop,) * 3, self.batch_size
        if self.augmenter is not None:
            x, x_aug = self.augmenter.views(order[b * B:(b + 1) * B], self.epoch)
            return {"input": x, "input_aug": x_aug}
        return {"input": self.table.cut(order, b * B, B, c),
                "input_aug": self.table.cut(order, b * B, B, c, shifted=True, flip_x=True)}

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.centres) // self.batch_size

    def __iter__(self):
        # (the epoch's order goes to the device once; a batch is two launches of mi_crop_normalize_table, or three of the
        # random views)
        order = self.table.epoch_order(np.random.default_rng(self.seed + 1000 * self.epoch).permutation(len(self.centres)))
        for b in range(len(self)):
            yield self._batch(order, b)
