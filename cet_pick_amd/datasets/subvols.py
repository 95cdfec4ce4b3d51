"""Sub-tomogram extraction on the GPU: the crop + normalise arithmetic of
the reference datasets, without their per-pick Python loops.

`extract_subvols` / `extract_subvols_3d` follow datasets/tomo_pre_proj_angle_select_new3d_vol.py:117-138
for a whole list of picks at once; `crop_znorm` makes the z-normalised 3-D crops the MoCo-3D encoder
consumes.  The volume stays resident on the device; centres are (x, y, z) like the picker returns.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib as L

RAW, SUMZ_MINMAX, ZNORM, ZNORM_RESCALE_ZNORM = 0, 1, 2, 3


def _centres(c, device):
    if isinstance(c, torch.Tensor):
        return c.to(device=device, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(c, dtype=np.int32)).to(device)


def _crop(vol, centres, size, mode, flip_x=False):
    L.require_cuda(vol, "vol")
    vol = vol.contiguous()
    d, h, w = vol.shape
    cz, cy, cx = [int(v) for v in size]
    c = _centres(centres, vol.device)
    n = c.shape[0]
    shape = (n, cy, cx) if mode == SUMZ_MINMAX else (n, cz, cy, cx)
    out = torch.empty(shape, dtype=torch.float32, device=vol.device)
    L.call("mi_crop_normalize", vol, d, h, w, c, n, cz, cy, cx, mode, int(bool(flip_x)), out)
    return out


class CropTable:
    """Everything `mi_crop_normalize_table` needs to cut any batch of a dataset, resident on the device: one descriptor
    per tomogram (pointer + extents), and per sample its tomogram, its centre (x, y, z) and the second view's shift.
    Built once per dataset; a batch is then `cut(order, first, n, ...)` - one launch per view, no host arithmetic, no
    host-to-device copy (the per-batch work of the reference's DataLoader workers, datasets/particle_pre_3d_vol.py:70-85)."""

    def __init__(self, vols, owner, centres, shift=None):
        dev = vols[0].device
        self.vols = [L.require_cuda(v, "vol").contiguous() for v in vols]          # (kept alive: the table holds raw pointers)
        for v in self.vols:
            if v.dtype != torch.float32 or v.dim() != 3:
                raise L.HipExtensionError("CropTable: tomograms must be (D, H, W) float32 device tensors")
        desc = np.zeros((len(self.vols), 3), dtype=np.int64)                          # struct mi_vol_desc {ptr; D, H; W, 0}
        for i, v in enumerate(self.vols):
            d, h, w = (int(a) for a in v.shape)
            desc[i] = (v.data_ptr(), d | (h << 32), w)
        self.desc = torch.as_tensor(desc).to(dev)
        self.owner = torch.as_tensor(np.ascontiguousarray(owner, dtype=np.int32)).to(dev)
        self.centres = _centres(centres, dev)
        self.shift = _centres(shift, dev) if shift is not None else None
        self.n = int(self.centres.shape[0])
        if int(self.owner.numel()) != self.n or (self.shift is not None and tuple(self.shift.shape) != tuple(self.centres.shape)):
            raise L.HipExtensionError("CropTable: owner / centres / shift disagree in length")

        self._inside = {}

    def boxes_inside(self, size):
        """True when the even size^3 box around every centre (placed as `cut` places an even crop: it starts at centre -
        size // 2) lies inside its tomogram.  One read-back per size, then remembered."""
        size = int(size)
        if size not in self._inside:
            ext = torch.tensor([[v.shape[2], v.shape[1], v.shape[0]] for v in self.vols], dtype=torch.int32,
                               device=self.desc.device)[self.owner.long()]                # (n, 3) extents along x, y, z
            lo = self.centres - size // 2
            self._inside[size] = bool(((lo >= 0) & (lo + size <= ext)).all())
        return self._inside[size]

    def epoch_order(self, order):
        """the epoch's sample order (any int array) as the device array `cut` indexes"""
        return torch.as_tensor(np.ascontiguousarray(order, dtype=np.int64)).to(self.desc.device)

    def cut(self, order, first, n, size, mode=ZNORM, shifted=False, flip_x=False, out=None):
        """crops of samples order[first : first + n] (order None: samples first .. first + n - 1) -> (n, 1, cz, cy, cx)
        ((n, 1, cy, cx) for mode SUMZ_MINMAX)"""
        cz, cy, cx = [int(v) for v in size]
        if first < 0 or n < 0 or first + n > (self.n if order is None else int(order.numel())):
            raise L.HipExtensionError("CropTable.cut: samples [%d, %d) outside the epoch's order" % (first, first + n))
        shape = (n, 1, cy, cx) if mode == SUMZ_MINMAX else (n, 1, cz, cy, cx)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.desc.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise L.HipExtensionError("CropTable.cut: `out` must be a contiguous float32 %s tensor" % (shape,))
        L.call("mi_crop_normalize_table", self.desc, self.owner, self.centres, self.shift if shifted else None, order, int(first), int(n),
               cz, cy, cx, int(mode), int(bool(flip_x)), out)
        return out

    def cut_poses(self, first, n, size, poses, out=None):
        """the z-normalised crops of samples first .. first + n - 1 in every pose of `poses` -> (n, P, 1, cz, cy, cx): pose p is
        the crop turned `p & 3` quarter turns (torch.rot90 over (y, x)) and then, with `p & 4`, mirrored along x.  One launch;
        the library refuses cy != cx, a pose outside 0..7, a repeated pose and a list of none or more than eight."""
        cz, cy, cx = [int(v) for v in size]
        poses = [int(p) for p in poses]
        if first < 0 or n < 0 or first + n > self.n:
            raise L.HipExtensionError("CropTable.cut_poses: samples [%d, %d) outside the table's %d" % (first, first + n, self.n))
        shape = (n, len(poses), 1, cz, cy, cx)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.desc.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise L.HipExtensionError("CropTable.cut_poses: `out` must be a contiguous float32 %s tensor" % (shape,))
        L.call("mi_crop_znorm_poses", self.desc, self.owner, self.centres, int(first), int(n), cz, cy, cx,
               L.host_array(poses, ctypes.c_int32), len(poses), out)
        return out


def extract_subvols(v, tomo_coords, subvol_size):
    """:117-128 for every pick: (n, 1, sy, sx) float32 = min-max(sum_z v[z-sz//2 : z+sz//2+1, ...]).
    subvol_size = (sz, sy, sx); an odd sz gives the z-1..z+1 slab of the reference."""
    sz, sy, sx = subvol_size
    return _crop(v, tomo_coords, (2 * (int(sz) // 2) + 1, sy, sx), SUMZ_MINMAX).unsqueeze(1)


def extract_subvols_3d(v, tomo_coords, subvol_size):
    """:130-138 for every pick: raw (n, 2*(sz//2)+1, sy, sx) crops."""
    sz, sy, sx = subvol_size
    return _crop(v, tomo_coords, (2 * (int(sz) // 2) + 1, sy, sx), RAW)


def crop_znorm(v, tomo_coords, size, flip_x=False):
    """(n, 1, cz, cy, cx) z-normalised crops (mean 0, unbiased std 1), optionally mirrored along x."""
    return _crop(v, tomo_coords, size, ZNORM, flip_x).unsqueeze(1)


def crop_znorm_poses(table_or_vol, centres, size, poses):
    """`crop_znorm` in the in-plane lattice poses `poses` (CropTable.cut_poses) -> (n, P, 1, cz, cy, cx).  With a CropTable,
    `centres` is the sample range (first, n) or None for every sample; with a (D, H, W) volume, the (n, 3) centres (x, y, z)."""
    if isinstance(table_or_vol, CropTable):
        first, n = (0, table_or_vol.n) if centres is None else (int(centres[0]), int(centres[1]))
        return table_or_vol.cut_poses(first, n, size, poses)
    L.require_cuda(table_or_vol, "vol")
    n = len(centres)
    return CropTable([table_or_vol], np.zeros(n, np.int32), centres).cut_poses(0, n, size, poses)


def extract_3d_tomo(rec, tomo_coords, crop_size_x, crop_size_y):
    """datasets/tomo_pre_proj_angle_select_new3d_vol.py:109-115 for every pick: the min-max'ed patch of slice z,
    (n, 1, crop_y, crop_x)."""
    return _crop(rec, tomo_coords, (1, crop_size_y, crop_size_x), SUMZ_MINMAX).unsqueeze(1)


def subvol_mean_std(subvols):
    """...:238-239 `torch.mean(torch.stack(sub_vols_3d))`, `torch.std(...)` (unbiased) over all crops, on the device:
    returns two Python floats (one read-back per dataset, like the reference's two scalars)."""
    L.require_cuda(subvols, "subvols")
    x = subvols.contiguous().view(-1)
    n = x.numel()
    lib = L.lib()
    ws = L.workspace(lib.mi_vol_stats_workspace_bytes(1, n), x.device, "stats")
    st = torch.empty(4, dtype=torch.float64, device=x.device)
    L.call("mi_vol_stats", x, 1, n, st, ws, ws.numel())
    mean, std0 = float(st[0]), float(st[1])
    return mean, std0 * (n / (n - 1.0)) ** 0.5


def to_uint8_normalize(subvols, mean, std):
    """simsiam_test_hm_3d.py:45-51 `T.ToPILImage() -> T.ToTensor() -> T.Normalize(mean, std)` for a batch of min-max'ed
    crops (the 8-bit round trip truncates: floor(255 x) / 255)."""
    L.require_cuda(subvols, "subvols")
    x = subvols.contiguous()
    y = torch.empty_like(x)
    L.call("mi_u8_roundtrip_normalize", x, y, x.numel(), float(mean), float(std))
    return y


def cutup_centres(shape, size, stride, margin=(0, 0, 0)):
    """Centres (x, y, z) of the inner crop of every `cutup(v, size, stride)` window (utils/loader.py:124-132 as used at
    datasets/tomo_pre.py:104), window order (i, j, k) row-major; `margin` = voxels the chain's Crop removes per side.
    Returns (centres (n,3) int32, inner size)."""
    nb = [(int(shape[a]) - int(size[a])) // int(stride[a]) + 1 for a in range(3)]
    inner = [int(size[a]) - 2 * int(margin[a]) for a in range(3)]
    iz, iy, ix = np.meshgrid(np.arange(nb[0]), np.arange(nb[1]), np.arange(nb[2]), indexing="ij")
    o = [iz.ravel() * stride[0] + margin[0], iy.ravel() * stride[1] + margin[1], ix.ravel() * stride[2] + margin[2]]
    c = np.stack([o[2] + inner[2] // 2, o[1] + inner[1] // 2, o[0] + inner[0] // 2], 1).astype(np.int32)
    return c, tuple(inner)


def crop_znorm_rescale_znorm(v, tomo_coords, size, flip_x=False):
    """datasets/tomo_pre.py:57-60 (deterministic tail of the torchio chain) for every window: (n, 1, cz, cy, cx) =
    ZNormalization(RescaleIntensity(-3, 3)(ZNormalization(crop)))."""
    return _crop(v, tomo_coords, size, ZNORM_RESCALE_ZNORM, flip_x).unsqueeze(1)


def tilt_border(crop):
    """datasets/tomo_pre_proj_angle_select_new2d3d.py:117,:189 `crop // 1.8`: Python float floor division (36 -> 19.0)."""
    return int(crop) // 1.8


def check_tilt_crop(crop_x, crop_y, H, W):
    """The 2d3d tilt windows need an even crop (the reference's `t -/+ c//2` slice has c - 1 pixels for an odd c and its
    CenterCrop pads them back); with an even crop the skip rule keeps every window inside the (H, W) image - checked here,
    not trusted.  Raises ValueError before any device work."""
    cx, cy = int(crop_x), int(crop_y)
    if cx <= 0 or cy <= 0 or cx % 2 or cy % 2:
        raise ValueError("the 2d3d mode needs an even --bbox (got %d x %d): the reference's tilt windows are c - 1 pixels "
                         "wide for an odd c" % (cx, cy))
    if cx * cy * 4 > 48 * 1024:
        raise ValueError("2d3d tilt patches of %d x %d exceed the kernel's 48 KiB window" % (cx, cy))
    for c, n in ((cx, W), (cy, H)):
        b = tilt_border(c)
        lo, hi = math.floor(b) + 1, math.ceil(n - b) - 1          # first / last centre the skip rule lets through
        if lo <= hi:
            assert lo - c // 2 >= 0 and hi + c // 2 <= n, (c, n, b)


class TiltStacks:
    """The tilt series of a dataset resident on the device, with their descriptors (struct mi_tilt_desc: stack pointer,
    cos / sin of the tilt angles, T, H, W, the full-resolution tomogram depth).  `stacks`: [(tilts (T, H, W) fp32 cuda,
    angles in degrees (T,), Zfull)]."""

    def __init__(self, stacks):
        if not stacks:
            raise L.HipExtensionError("TiltStacks: no tilt series")
        dev = L.require_cuda(stacks[0][0], "tilts").device
        self.tilts, self.cos_sin, self.shapes = [], [], []
        desc = np.zeros((len(stacks), 4), dtype=np.int64)
        for i, (tilts, angles, zfull) in enumerate(stacks):
            t = L.require_cuda(tilts, "tilts").contiguous()
            if t.dim() != 3:
                raise L.HipExtensionError("TiltStacks: tilt series must be (T, H, W), got %s" % (tuple(t.shape),))
            a = [float(v) for v in np.asarray(angles, dtype=np.float64).ravel()]
            if len(a) != t.shape[0]:
                raise L.HipExtensionError("TiltStacks: %d angles for %d tilts" % (len(a), t.shape[0]))
            # the reference's `angle*np.pi/180` through math.cos / math.sin, on the host: a device cos may differ in the
            # last ulp and flip an int() at a window boundary
            cs = [math.cos(v * math.pi / 180) for v in a] + [math.sin(v * math.pi / 180) for v in a]
            cs = torch.tensor(cs, dtype=torch.float64).to(dev)
            T, H, W = (int(s) for s in t.shape)
            desc[i] = (t.data_ptr(), cs.data_ptr(), T | (H << 32), W | (int(zfull) << 32))
            self.tilts.append(t)                                    # (kept alive: the table holds raw pointers)
            self.cos_sin.append(cs)
            self.shapes.append((T, H, W))
        self.desc = torch.as_tensor(desc).to(dev)

    def patches(self, centres, crop_x, crop_y, owner=None):
        """`extract_patches` (:110-133) for every centre (x, y, z_full) of stack owner[i] (owner None: stack 0), one launch.
        -> (patches (n, 1, crop_y, crop_x) fp32 in [0, 1], valid (n,) bool): valid False where the reference returns None."""
        cx, cy = int(crop_x), int(crop_y)
        for _, h, w in self.shapes:
            check_tilt_crop(cx, cy, h, w)
        dev = self.desc.device
        c = _centres(centres, dev).reshape(-1, 3)
        n = int(c.shape[0])
        own = None
        if owner is not None:
            own = _centres(owner, dev).reshape(-1)
            if int(own.numel()) != n:
                raise L.HipExtensionError("TiltStacks.patches: %d owners for %d centres" % (int(own.numel()), n))
        out = torch.empty((n, 1, cy, cx), dtype=torch.float32, device=dev)
        valid = torch.empty((n,), dtype=torch.uint8, device=dev)
        L.call("mi_tilt_patches", self.desc, len(self.shapes), own, c, n, cy, cx, float(tilt_border(cx)), float(tilt_border(cy)), out,
               valid)
        return out, valid.bool()


def tilt_patches(tilts, angles, zfull, centres, crop_x, crop_y):
    """One tilt series: `TiltStacks([(tilts, angles, zfull)]).patches(centres, crop_x, crop_y)`."""
    return TiltStacks([(tilts, angles, zfull)]).patches(centres, crop_x, crop_y)
