"""Random view augmentation of the SimSiam exploration training on the GPU (csrc/augment2d.hip): the reference's two
torchvision chains (datasets/tomo_pre_proj_angle_select_new3d_vol.py:49-89) and its choice of a neighbouring crop for
the second view (datasets/particle_pre_3d_vol.py:70-85), for a whole batch in two launches per view.

    table = draw_params(sample_ids, seed, epoch, view, bbox)        # mi_aug2d_params: one record per (sample, view)
    views = apply(bank, sample_ids, table, mean, std)               # mi_aug2d_apply:  (B, 1, bbox, bbox)

The 2d3d mode's chains (datasets/tomo_pre_proj_angle_select_new2d3d.py:49-82: flips, RandomRotation(30) in the strong
chain, CornerErasing, FixedRotation, Normalize per channel) act on the tilt patch and the tomogram patch with one set of
parameters (csrc/augment2d3d.hip); both views and both channels of a batch are two launches:

    table = draw_params_2d3d(sample_ids, seed, epoch, bbox)         # mi_aug2d3d_params: (2 views, B, 16)
    four = apply_2d3d(patches_2d, patches_3d, sample_ids, variants, table, means, stds)     # mi_aug2d3d_apply: (4, B, 1, bbox, bbox)

A record is a pure function of (seed, epoch, sample id, view) - counter-based Philox-4x32-10 - so a sample is augmented
the same way whatever batch, rank or world size it is served in, and nothing carries over between launches.
"""
import torch

from .. import _lib as L

STRONG, WEAK = 0, 1
RECORD_WORDS = 8

# the ranges of a chain: RandomHorizontalFlip / RandomVerticalFlip(p), ColorJitter(brightness 0.5, contrast 0.2) as factor
# ranges, RandomResizedCrop's area share (aspect ratio 1)
STRONG_RANGES = dict(flip_p=0.5, brightness=(0.5, 1.5), contrast=(0.8, 1.2), area=(0.8, 1.0))
WEAK_RANGES = dict(flip_p=0.5, brightness=(0.5, 1.5), contrast=(0.8, 1.2), area=(0.9, 1.0))

# the 2d3d chains: flips(p), RandomRotation's angle range in degrees (the weak chain has no rotation), CornerErasing(p,
# scale = share of the area, ratio = aspect h / w)
RECORD_WORDS_2D3D = 16
STRONG_RANGES_2D3D = dict(flip_p=0.5, angle=(-30.0, 30.0), erase_p=0.5, scale=(0.01, 0.02), ratio=(0.5, 1.5))
WEAK_RANGES_2D3D = dict(flip_p=0.5, angle=(0.0, 0.0), erase_p=0.5, scale=(0.01, 0.02), ratio=(0.5, 1.5))


def _ids(sample_ids):
    L.require_cuda(sample_ids, "sample_ids", torch.int64)
    if sample_ids.dim() != 1 or not sample_ids.is_contiguous():
        raise L.HipExtensionError("sample_ids must be a contiguous 1-d int64 device tensor")
    return sample_ids


def draw_params(sample_ids, seed, epoch, view, bbox, ranges=None):
    """The parameter records of `sample_ids` (int64, on the device) for `view` (0 strong, 1 weak) -> (n, 8) int32 table
    (layout: include/cetpick_hip.h)."""
    ids = _ids(sample_ids)
    rg = ranges if ranges is not None else {STRONG: STRONG_RANGES, WEAK: WEAK_RANGES}[view]
    table = torch.empty((ids.numel(), RECORD_WORDS), dtype=torch.int32, device=ids.device)
    L.check(L.lib().mi_aug2d_params(L.ptr(ids), ids.numel(), int(seed) & (2 ** 64 - 1), int(epoch), int(view), int(bbox),
                                    float(rg["flip_p"]), float(rg["brightness"][0]), float(rg["brightness"][1]),
                                    float(rg["contrast"][0]), float(rg["contrast"][1]), float(rg["area"][0]),
                                    float(rg["area"][1]), L.ptr(table), L.stream()), "mi_aug2d_params")
    return table


def apply(bank, sample_ids, table, mean, std, neighbours=False):
    """The chain on crops `sample_ids` of `bank` with the records of `table` -> (B, 1, bbox, bbox) float32.
    bank: (n, bbox, bbox) or (n, 1, bbox, bbox) crops in [0, 1]; with `neighbours` a stack (m, n, [1,] bbox, bbox) of m
    such banks, of which each record's neighbour id picks one."""
    L.require_cuda(bank, "bank")
    ids = _ids(sample_ids)
    L.require_cuda(table, "table", torch.int32)
    if not bank.is_contiguous() or not table.is_contiguous() or table.data_ptr() % 16:
        raise L.HipExtensionError("bank and table must be contiguous, the table 16-byte aligned (the kernel loads whole records)")
    lead = 2 if neighbours else 1
    if bank.dim() == lead + 3 and bank.shape[lead] == 1:                 # the crops' channel axis
        bank = bank.squeeze(lead)
    if bank.dim() != lead + 2 or bank.shape[-1] != bank.shape[-2]:
        raise L.HipExtensionError("bank must be %s(n, [1,] bbox, bbox), got %s" % ("(m, " if neighbours else "", tuple(bank.shape)))
    n_banks, n_samples, bbox = (int(bank.shape[0]) if neighbours else 1), int(bank.shape[lead - 1]), int(bank.shape[-1])
    B = ids.numel()
    if tuple(table.shape) != (B, RECORD_WORDS):
        raise L.HipExtensionError("table must be (%d, %d), got %s" % (B, RECORD_WORDS, tuple(table.shape)))
    out = torch.empty((B, 1, bbox, bbox), dtype=torch.float32, device=bank.device)
    L.check(L.lib().mi_aug2d_apply(L.ptr(bank), n_samples, n_banks, L.ptr(ids), L.ptr(table), B, bbox, float(mean), float(std),
                                   L.ptr(out), L.stream()), "mi_aug2d_apply")
    return out


class ViewAugmenter:
    """The two views of the `simsiam3d` dataset: `strong(anchor crop)` and `weak(crop of a random neighbouring centre)`,
    both normalised with the anchor bank's mean / std (:238-239).  Holds the chains' ranges and the banks; a batch is four
    launches on the current stream."""

    def __init__(self, anchors, neighbours, mean, std, seed, strong=STRONG_RANGES, weak=WEAK_RANGES):
        self.anchors = L.require_cuda(anchors, "anchors").contiguous()                 # (n, 1, bbox, bbox) in [0, 1]
        self.neighbours = L.require_cuda(neighbours, "neighbours").contiguous()        # (4, n, 1, bbox, bbox)
        if tuple(self.neighbours.shape[1:]) != tuple(self.anchors.shape):
            raise L.HipExtensionError("neighbour banks %s do not match the anchor bank %s"
                                      % (tuple(self.neighbours.shape), tuple(self.anchors.shape)))
        self.bbox = int(self.anchors.shape[-1])
        self.mean, self.std, self.seed = float(mean), float(std), int(seed)
        self.strong, self.weak = dict(strong), dict(weak)

    def views(self, sample_ids, epoch):
        """-> (input, input_aug) of the dataset samples `sample_ids` (int64, on the device) in epoch `epoch`"""
        t0 = draw_params(sample_ids, self.seed, epoch, STRONG, self.bbox, self.strong)
        t1 = draw_params(sample_ids, self.seed, epoch, WEAK, self.bbox, self.weak)
        return (apply(self.anchors, sample_ids, t0, self.mean, self.std),
                apply(self.neighbours, sample_ids, t1, self.mean, self.std, neighbours=True))


# ---- the 2d3d mode: two channels, one record ---------------------------------------------------------------------------------
def _ranges_2d3d(rg):
    return L.Aug2d3dRanges(float(rg["flip_p"]), float(rg["angle"][0]), float(rg["angle"][1]), float(rg["erase_p"]),
                           float(rg["scale"][0]), float(rg["scale"][1]), float(rg["ratio"][0]), float(rg["ratio"][1]))


def draw_params_2d3d(sample_ids, seed, epoch, bbox, strong=None, weak=None):
    """The records of `sample_ids` (int64, on the device) for both views -> (2, n, 16) int32 table: [0] drawn with the
    `strong` ranges, [1] with the `weak` ones (layout: include/cetpick_hip.h)."""
    ids = _ids(sample_ids)
    rs = _ranges_2d3d(STRONG_RANGES_2D3D if strong is None else strong)
    rw = _ranges_2d3d(WEAK_RANGES_2D3D if weak is None else weak)
    table = torch.empty((2, ids.numel(), RECORD_WORDS_2D3D), dtype=torch.int32, device=ids.device)
    L.check(L.lib().mi_aug2d3d_params(L.ptr(ids), ids.numel(), int(seed) & (2 ** 64 - 1), int(epoch), int(bbox), rs, rw,
                                      L.ptr(table), L.stream()), "mi_aug2d3d_params")
    return table


def _bank_2d3d(bank, name):
    L.require_cuda(bank, name)
    if bank.dim() == 5 and bank.shape[2] == 1:                           # the patches' channel axis
        bank = bank.squeeze(2)
    if bank.dim() != 4 or bank.shape[-1] != bank.shape[-2] or not bank.is_contiguous():
        raise L.HipExtensionError("%s must be contiguous (n, V, [1,] bbox, bbox), got %s" % (name, tuple(bank.shape)))
    return bank


def apply_2d3d(patches_2d, patches_3d, sample_ids, variants, table, means, stds):
    """Both chains on both channels -> (4, B, 1, bbox, bbox) float32: input, input_3d (variant 0 of `sample_ids` with
    table[0]), input_aug, input_aug_3d (variant `variants` with table[1]).  patches_*: (n, V, [1,] bbox, bbox) in [0, 1];
    means / stds: (tilt channel, tomogram channel)."""
    p2, p3 = _bank_2d3d(patches_2d, "patches_2d"), _bank_2d3d(patches_3d, "patches_3d")
    if p2.shape != p3.shape or p2.device != p3.device:
        raise L.HipExtensionError("patches_2d %s and patches_3d %s differ" % (tuple(p2.shape), tuple(p3.shape)))
    ids = _ids(sample_ids)
    L.require_cuda(variants, "variants", torch.int64)
    L.require_cuda(table, "table", torch.int32)
    B = ids.numel()
    if variants.dim() != 1 or variants.numel() != B or not variants.is_contiguous():
        raise L.HipExtensionError("variants must be a contiguous int64 tensor of %d entries" % B)
    if tuple(table.shape) != (2, B, RECORD_WORDS_2D3D) or not table.is_contiguous() or table.data_ptr() % 16:
        raise L.HipExtensionError("table must be a contiguous (2, %d, %d) tensor, 16-byte aligned (the kernel loads whole "
                                  "records), got %s" % (B, RECORD_WORDS_2D3D, tuple(table.shape)))
    n_samples, n_variants, bbox = int(p2.shape[0]), int(p2.shape[1]), int(p2.shape[-1])
    out = torch.empty((4, B, 1, bbox, bbox), dtype=torch.float32, device=p2.device)
    L.check(L.lib().mi_aug2d3d_apply(L.ptr(p2), L.ptr(p3), n_samples, n_variants, L.ptr(ids), L.ptr(variants), L.ptr(table[0]),
                                     L.ptr(table[1]), B, bbox, float(means[0]), float(stds[0]), float(means[1]), float(stds[1]),
                                     L.ptr(out), L.stream()), "mi_aug2d3d_apply")
    return out


class PairViewAugmenter:
    """The two views of the `simsiam2d3d` dataset: `strong(the pick's patch pair)` and `weak(a shifted variant's pair)`, each
    channel normalised with its own dataset mean / std.  Holds the chains' ranges and the two patch banks; a batch is two
    launches on the current stream."""

    def __init__(self, patches_2d, patches_3d, means, stds, seed, strong=STRONG_RANGES_2D3D, weak=WEAK_RANGES_2D3D):
        self.patches_2d = _bank_2d3d(L.require_cuda(patches_2d, "patches_2d").contiguous(), "patches_2d")
        self.patches_3d = _bank_2d3d(L.require_cuda(patches_3d, "patches_3d").contiguous(), "patches_3d")
        if self.patches_2d.shape != self.patches_3d.shape:
            raise L.HipExtensionError("patches_2d %s and patches_3d %s differ"
                                      % (tuple(self.patches_2d.shape), tuple(self.patches_3d.shape)))
        self.bbox = int(self.patches_2d.shape[-1])
        self.means, self.stds = (float(means[0]), float(means[1])), (float(stds[0]), float(stds[1]))
        self.seed, self.strong, self.weak = int(seed), dict(strong), dict(weak)

    def views(self, sample_ids, variants, epoch):
        """-> (input, input_3d, input_aug, input_aug_3d) of the dataset samples `sample_ids` in epoch `epoch`; the second
        view is made of variant `variants[t]` (both int64, on the device)"""
        table = draw_params_2d3d(sample_ids, self.seed, epoch, self.bbox, self.strong, self.weak)
        return apply_2d3d(self.patches_2d, self.patches_3d, sample_ids, variants, table, self.means, self.stds).unbind(0)
