"""Random view augmentation of the SimSiam exploration training on the GPU (csrc/augment2d.hip): the reference's two
torchvision chains (datasets/tomo_pre_proj_angle_select_new3d_vol.py:49-89) and its choice of a neighbouring crop for
the second view (datasets/particle_pre_3d_vol.py:70-85), for a whole batch in two launches per view.

    table = draw_params(sample_ids, seed, epoch, view, bbox)        # mi_aug2d_params: one record per (sample, view)
    views = apply(bank, sample_ids, table, mean, std)               # mi_aug2d_apply:  (B, 1, bbox, bbox)

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
