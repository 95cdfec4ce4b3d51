"""mi_crop_znorm_poses (csrc/crop_pose.hip) through datasets/subvols.py: the z-normalised crop in the eight in-plane lattice
poses, against a float64 numpy restatement (crop, (x - mean) / unbiased std, np.rot90 over (y, x), np.flip along x).

The bound is the one tests/test_data_path_gpu.py::test_crop_znorm holds `crop_znorm` to: conftest.f32_equivalent with its
defaults - the GPU result may sit 2 x as far from float64 as a float32 evaluation does (norm-relative), + 2e-6.  The float32
evaluation is torch's two-pass (c - c.mean()) / c.std() on the CPU, as there.

Measured on the MI355X (printed again with -s), norm-relative from float64, the same in every pose: box (4, 6, 6) 2.690e-07
against the CPU's 8.239e-07, box (5, 5, 5) 3.203e-07 against 9.436e-07."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((12, 14, 15), (9, 16, 13))
BOXES = [(4, 6, 6), (5, 5, 5)]
POSE_LISTS = [list(range(8)), [0, 5], [3]]
SENTINEL = -7.25


def _window_centres(shape, size):
    """(lowest, highest) legal centre (x, y, z): the window [c - s // 2, c - s // 2 + s) touches the volume's first / last voxel"""
    lo = [s // 2 for s in size[::-1]]
    hi = [e - s + s // 2 for e, s in zip(shape[::-1], size[::-1])]
    return lo, hi


@pytest.fixture(scope="module")
def tomos():
    rng = np.random.default_rng(2610)
    host = [(rng.standard_normal(s) * 7 + 100).astype(np.float32) for s in SHAPES]
    return host, [torch.as_tensor(v).cuda() for v in host]


def _samples(size):
    """five samples over the two tomograms; windows at the lowest and at the highest legal position of every axis"""
    owner = np.array([0, 1, 0, 1, 0], np.int32)
    cen = []
    for k, o in enumerate(owner):
        lo, hi = _window_centres(SHAPES[o], size)
        cen.append([lo, hi, [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]], [(a + b) // 2 for a, b in zip(lo, hi)]][k])
    return owner, np.asarray(cen, np.int32)


def _raw(vol, c, size):
    cz, cy, cx = size
    x0, y0, z0 = int(c[0]) - cx // 2, int(c[1]) - cy // 2, int(c[2]) - cz // 2
    assert x0 >= 0 and y0 >= 0 and z0 >= 0 and z0 + cz <= vol.shape[0] and y0 + cy <= vol.shape[1] and x0 + cx <= vol.shape[2]
    return vol[z0:z0 + cz, y0:y0 + cy, x0:x0 + cx]


def _pose_np(a, p):
    a = np.rot90(a, p & 3, axes=(-2, -1))
    return np.flip(a, -1) if p & 4 else a


def _pose_t(a, p):
    a = torch.rot90(a, p & 3, dims=(-2, -1))
    return torch.flip(a, dims=(-1,)) if p & 4 else a


def _ref64(vol, c, size, p):
    a = _raw(vol, c, size).astype(np.float64)
    return _pose_np((a - a.mean()) / a.std(ddof=1), p)


def _ref32(vol, c, size, p):
    a = torch.from_numpy(np.ascontiguousarray(_raw(vol, c, size)))
    return _pose_t((a - a.mean()) / a.std(), p).numpy()


@pytest.mark.parametrize("poses", POSE_LISTS, ids=lambda p: "poses" + "".join(map(str, p)))
@pytest.mark.parametrize("size", BOXES, ids=lambda s: "x".join(map(str, s)))
def test_poses_match_float64_and_each_other(tomos, size, poses):
    from conftest import f32_equivalent
    from cet_pick_amd.datasets import subvols as S
    host, dev = tomos
    owner, cen = _samples(size)
    table = S.CropTable(dev, owner, cen)
    got = S.crop_znorm_poses(table, None, size, poses)
    assert tuple(got.shape) == (5, len(poses), 1) + tuple(size) and got.dtype == torch.float32
    g = got.cpu().numpy()
    for k, p in enumerate(poses):
        ref64 = np.stack([_ref64(host[o], c, size, p) for o, c in zip(owner, cen)])
        ref32 = np.stack([_ref32(host[o], c, size, p) for o, c in zip(owner, cen)])
        e_g, e_c = f32_equivalent(g[:, k, 0], ref32, ref64, what="box %s pose %d" % (size, p))
        print("box %s pose %d: GPU %.3e from float64, CPU fp32 %.3e" % (size, p, e_g, e_c))
    # pose q is a permuted write of the values pose 0 holds
    zero = got[:, 0] if poses[0] == 0 else S.crop_znorm_poses(table, None, size, [0])[:, 0]
    for k, p in enumerate(poses):
        assert torch.equal(got[:, k], _pose_t(zero, p)), "box %s pose %d is not the image of pose 0" % (size, p)
    # pose 0 against crop_znorm of the same centres, held to the same bound with crop_znorm as the float32 evaluation
    for o in (0, 1):
        sel = np.nonzero(owner == o)[0]
        plain = S.crop_znorm(dev[o], cen[sel], size)
        ref64 = np.stack([_ref64(host[o], c, size, 0) for c in cen[sel]])
        f32_equivalent(zero[sel, 0].cpu().numpy(), plain[:, 0].cpu().numpy(), ref64, what="box %s pose 0 against crop_znorm" % (size,))
    # a sample range that does not start at 0, and the one-volume form of the wrapper
    part = S.crop_znorm_poses(table, (2, 3), size, poses)
    assert torch.equal(part, got[2:5])
    sel = np.nonzero(owner == 1)[0]
    assert torch.equal(S.crop_znorm_poses(dev[1], cen[sel], size, poses), got[sel])


def _direct(table, n, size, poses, out):
    from cet_pick_amd import _lib as L
    cz, cy, cx = size
    L.call("mi_crop_znorm_poses", table.desc, table.owner, table.centres, 0, n, cz, cy, cx, L.host_array(list(poses), ctypes.c_int32),
           len(poses), out)


def test_refusals_leave_the_output_untouched(tomos):
    from cet_pick_amd import _lib as L
    from cet_pick_amd.datasets import subvols as S
    _, dev = tomos
    owner, cen = _samples((4, 6, 6))
    table = S.CropTable(dev, owner, cen)
    out = torch.full((5 * 8 * 4 * 6 * 6 + 64,), SENTINEL, device="cuda")
    for size, poses, what in (((4, 6, 5), [0], "cy != cx"), ((4, 6, 6), [0, 8], "pose 8"), ((4, 6, 6), [-1], "pose -1"),
                              ((4, 6, 6), [1, 2, 1], "a repeated pose"), ((4, 6, 6), [], "P = 0"),
                              ((4, 6, 6), [0, 1, 2, 3, 4, 5, 6, 7, 0], "P = 9")):
        with pytest.raises(L.HipExtensionError, match="bad argument"):
            _direct(table, 5, size, poses, out)
        torch.cuda.synchronize()
        assert bool(torch.all(out == SENTINEL)), what
    # a box the workgroup cannot hold is refused as such, not cropped wrongly (no 64^3 volume is needed: nothing is launched)
    for size in ((64, 64, 64), (2, 65, 65)):
        with pytest.raises(L.HipExtensionError, match="unsupported"):
            _direct(table, 5, size, [0], out)
        torch.cuda.synchronize()
        assert bool(torch.all(out == SENTINEL)), size
    # the wrapper's own checks
    with pytest.raises(L.HipExtensionError):
        table.cut_poses(3, 3, (4, 6, 6), [0])                       # samples 3..5 of 5
    with pytest.raises(L.HipExtensionError, match="bad argument"):
        S.crop_znorm_poses(table, None, (4, 6, 6), [2, 2])
    # ... and the accepted call still writes exactly its floats
    _direct(table, 5, (4, 6, 6), range(8), out)
    torch.cuda.synchronize()
    assert bool(torch.all(out[5 * 8 * 144:] == SENTINEL)) and bool(torch.all(out[:5 * 8 * 144] != SENTINEL))


@pytest.mark.parametrize("size", BOXES, ids=lambda s: "x".join(map(str, s)))
def test_constant_window_is_crop_znorms(tomos, size):
    """zero variance: whatever `crop_znorm` makes of the window (it divides by the zero), in every pose - compared bit for bit,
    every NaN as one pattern.  0.1 is no short binary fraction: the sums of its squares are rounded ones."""
    from cet_pick_amd.datasets import subvols as S
    vol = torch.full((10, 12, 12), 0.1, device="cuda")
    vol[0, 0, 0] = 3.0                                                # (outside both windows)
    cen = np.array([[6, 6, 5], [5, 7, 6]], np.int32)
    want = S.crop_znorm(vol, cen, size)
    got = S.crop_znorm_poses(vol, cen, size, list(range(8)))
    assert not bool(torch.isfinite(want).all()) or float(want.abs().max()) == 0.0          # nothing but 0, inf or NaN comes of it
    for p in range(8):
        a, b = got[:, p], _pose_t(want, p)
        nan = torch.isnan(b)
        assert torch.equal(torch.isnan(a), nan) and torch.equal(a[~nan], b[~nan]), "pose %d" % p
