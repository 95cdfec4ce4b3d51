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

The 3-D views of the MoCo training (datasets/tomo_pre.py:53-62, datasets/particle_pre.py:48-87: blur, noise, in-plane
rotation, margin crop, ZNorm / Rescale(-3, 3) / ZNorm, a flip, one of three erasures) are made from the tomograms of a
`CropTable` (csrc/augment3d.hip); both views of a batch are three launches:

    table = draw_params_3d(sample_ids, seed, epoch, view, crop)     # mi_aug3d_params: (B, 16)
    views = apply_3d(crop_table, sample_ids, table, crop)           # mi_aug3d_apply:  (B, 1, crop, crop, crop)

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
    L.call("mi_aug2d_params", ids, ids.numel(), int(seed) & (2 ** 64 - 1), int(epoch), int(view), int(bbox), float(rg["flip_p"]),
           float(rg["brightness"][0]), float(rg["brightness"][1]), float(rg["contrast"][0]), float(rg["contrast"][1]), float(rg["area"][0]),
           float(rg["area"][1]), table)
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
    L.call("mi_aug2d_apply", bank, n_samples, n_banks, ids, table, B, bbox, float(mean), float(std), out)
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
    L.call("mi_aug2d3d_params", ids, ids.numel(), int(seed) & (2 ** 64 - 1), int(epoch), int(bbox), rs, rw, table)
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
    L.call("mi_aug2d3d_apply", p2, p3, n_samples, n_variants, ids, variants, table[0], table[1], B, bbox, float(means[0]), float(stds[0]),
           float(means[1]), float(stds[1]), out)
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


# ---- the 3-D views of the MoCo training --------------------------------------------------------------------------------------
RECORD_WORDS_3D = 16
# RandomBlur(p 0.15, std (0, 1)), RandomNoise(p 0.5, std (0, 0.25)), RandomAffine(p 0.75, degrees (0, 60) about the depth
# axis); flip: u < 0.33 reverses z, u > 0.66 reverses y; erase: u < 0.25 drop_out, < 0.5 center_out, < 0.75 swap_out
RANGES_3D = dict(blur_p=0.15, sigma=(0.0, 1.0), noise_p=0.5, noise=(0.0, 0.25), rot_p=0.75, angle=(0.0, 60.0),
                 flip=(0.33, 0.66), erase=(0.25, 0.5, 0.75))
MIN_CROP_3D, MAX_CROP_3D = 6, 32


def geometry_3d(crop):
    """-> (m, S, e, q) of a served edge `crop`: the margin the chain's Crop removes per side, the edge of the source box,
    the edge of an erased box, half the edge of center_out's window.  ValueError for a crop the chain cannot serve."""
    c = int(crop)
    if c < MIN_CROP_3D or c > MAX_CROP_3D or c % 2:
        raise ValueError("the 3-D views need an even crop in %d..%d (the crop sits in LDS), got %d" % (MIN_CROP_3D, MAX_CROP_3D, c))
    m = c // 6
    S = c + 2 * m
    assert S // 8 == m
    return m, S, S // 8, S // 4


def erase_corners_3d(crop):
    """The corners an erased box may take along an axis: [0, c/2 - 2e) U [c/2 + e, c - e), ascending (utils/image.py:484-486).
    ValueError when fewer than two are left (swap_out draws two of them) or the box is empty."""
    _, _, e, _ = geometry_3d(crop)
    c = int(crop)
    corners = list(range(0, c // 2 - 2 * e)) + list(range(c // 2 + e, c - e))
    if e < 1 or len(corners) < 2:
        raise ValueError("a crop of %d leaves %d erasure corners per axis; swap_out needs two" % (c, len(corners)))
    return corners


def _ranges_3d(rg):
    return L.Aug3dRanges(float(rg["blur_p"]), float(rg["sigma"][0]), float(rg["sigma"][1]), float(rg["noise_p"]),
                         float(rg["noise"][0]), float(rg["noise"][1]), float(rg["rot_p"]), float(rg["angle"][0]),
                         float(rg["angle"][1]), float(rg["flip"][0]), float(rg["flip"][1]), float(rg["erase"][0]),
                         float(rg["erase"][1]), float(rg["erase"][2]))


def _draw_3d(sample_ids, seed, epoch, view, n_views, crop, ranges):
    ids = _ids(sample_ids)
    erase_corners_3d(crop)
    table = torch.empty((n_views, ids.numel(), RECORD_WORDS_3D), dtype=torch.int32, device=ids.device)
    L.call("mi_aug3d_params", ids, ids.numel(), int(seed) & (2 ** 64 - 1), int(epoch), int(view), int(n_views), int(crop),
           _ranges_3d(RANGES_3D if ranges is None else ranges), table)
    return table


def draw_params_3d(sample_ids, seed, epoch, view, crop, ranges=None):
    """The records of `sample_ids` (int64, on the device) for `view` -> (n, 16) int32 table (layout: include/cetpick_hip.h)."""
    return _draw_3d(sample_ids, seed, epoch, view, 1, crop, ranges)[0]


def apply_3d(crop_table, sample_ids, table, crop):
    """The chain on the boxes around the centres `sample_ids` of `crop_table` (datasets/subvols.py CropTable) with the records
    of `table` -> (B, 1, crop, crop, crop) float32; a table (V, B, 16) of V views gives (V, B, 1, crop, crop, crop).  ValueError
    when a source box (edge crop + 2 (crop // 6)) would leave its tomogram."""
    _, S, _, _ = geometry_3d(crop)
    erase_corners_3d(crop)
    c = int(crop)
    ids = _ids(sample_ids)
    L.require_cuda(table, "table", torch.int32)
    B = ids.numel()
    stacked = table.dim() == 3
    V = int(table.shape[0]) if stacked else 1
    if tuple(table.shape[-2:]) != (B, RECORD_WORDS_3D) or table.dim() not in (2, 3) or not table.is_contiguous() or table.data_ptr() % 16:
        raise L.HipExtensionError("table must be a contiguous ([V,] %d, %d) tensor, 16-byte aligned (the kernel loads whole "
                                  "records), got %s" % (B, RECORD_WORDS_3D, tuple(table.shape)))
    if not crop_table.boxes_inside(S):
        raise ValueError("a %d^3 source box (crop %d + 2 x %d) leaves its tomogram: keep the centres %d voxels from the edges"
                         % (S, c, c // 6, S // 2))
    dev = crop_table.desc.device
    out = torch.empty((V, B, 1, c, c, c), dtype=torch.float32, device=dev)
    lib = L.lib()
    # (scratch of this call alone, from the allocator of the current stream: a loader cuts on a stream of its own)
    ws = torch.empty(max(int(lib.mi_aug3d_workspace_bytes(B, V, c)), 16), dtype=torch.uint8, device=dev)
    L.call("mi_aug3d_apply", crop_table.desc, crop_table.owner, crop_table.centres, crop_table.n, ids, table, B, V, c, out, ws, ws.numel())
    return out if stacked else out[0]


class VolumeAugmenter:
    """The two views of the reference's 3-D contrastive dataset: two independent draws of the chain on the same box
    (datasets/particle_pre.py:55-87).  Holds the crop table, the ranges and the seed; a batch is three launches on the
    current stream."""

    def __init__(self, crop_table, crop, seed, ranges=RANGES_3D):
        _, S, _, _ = geometry_3d(crop)
        erase_corners_3d(crop)
        if not crop_table.boxes_inside(S):
            raise ValueError("a %d^3 source box (crop %d + 2 x %d) leaves its tomogram" % (S, int(crop), int(crop) // 6))
        self.table, self.crop, self.seed, self.ranges = crop_table, int(crop), int(seed), dict(ranges)

    def views(self, sample_ids, epoch):
        """-> (input, input_aug) of the samples `sample_ids` (int64, on the device) in epoch `epoch`"""
        records = _draw_3d(sample_ids, self.seed, epoch, 0, 2, self.crop, self.ranges)
        return apply_3d(self.table, sample_ids, records, self.crop).unbind(0)
