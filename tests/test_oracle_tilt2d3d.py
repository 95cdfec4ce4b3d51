"""The 2d3d exploration mode on the CPU: a numpy restatement of the reference's tilt-patch methods
(datasets/tomo_pre_proj_angle_select_new2d3d.py:91-133) against tests/golden/tilt2d3d.npz (a), the 4-column image list,
and the checks that run before any device work (odd --bbox, tilt series / tomogram size mismatch)."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CONST_ROWS = 28                 # fixture (a): tilt rows [0, 28) hold 0.5


def ref_tilt_xy(coord, angle, tomo_size):
    """:91-96 `convert_tomo_to_tilt`; tomo_size = [W, H, Zfull]."""
    a = angle * np.pi / 180
    x, y, z = coord[0], coord[1], tomo_size[-1] - coord[2]
    tx = (x - tomo_size[0] // 2) * math.cos(a) + (z - tomo_size[-1] // 2) * math.sin(a) + tomo_size[0] // 2
    return int(tx), int(y)


def ref_extract_patches(v, coord, angles, tomo_size, crop):
    """:110-133 `extract_patches` on the selected tilts v (T, H, W) fp32 -> (crop, crop) fp32 or None."""
    b = crop // 1.8
    W, H = v.shape[2], v.shape[1]
    p = None
    for i, an in enumerate(angles):
        tx, ty = ref_tilt_xy(coord, an, tomo_size)
        if tx <= b or tx >= W - b or ty <= b or ty >= H - b:
            continue
        w = v[i, ty - crop // 2:ty + crop // 2, tx - crop // 2:tx + crop // 2].copy()
        p = w if p is None else p + w
    if p is None or p.min() == p.max():
        return None
    return (p - p.min()) / (p.max() - p.min())


def ref_extract_3d_tomo(rec, coord, crop, compress=False):
    """:98-108 `extract_3d_tomo` (float64 tomogram) -> (crop, crop) fp32."""
    x, y, z = coord
    if compress:
        z = int(z // 2)
    p = rec[z, y - crop // 2:y + crop // 2, x - crop // 2:x + crop // 2].copy()
    return ((p - p.min()) / (p.max() - p.min())).astype(np.float32)


def fixture_a_stack():
    from cet_pick_amd.synthetic import tilt2d3d_inputs
    vol, _, tilts, angles = tilt2d3d_inputs()
    t = tilts.copy()
    t[:, :CONST_ROWS] = 0.5
    sel = np.nonzero((angles >= -20) & (angles <= 20))[0]
    return vol, t[sel], angles[sel]


def test_numpy_restatement_equals_reference_fixture():
    g = np.load(os.path.join(HERE, "golden", "tilt2d3d.npz"))
    vol, used, ang = fixture_a_stack()
    assert np.array_equal(g["a_sel"], np.nonzero((np.arange(-60, 61, 3) >= -20) & (np.arange(-60, 61, 3) <= 20))[0])
    Z, H, W = vol.shape
    for b in (16, 36):
        n_none = 0
        for i, c in enumerate(g["a_centres"]):
            p = ref_extract_patches(used, [int(v) for v in c], ang, [W, H, Z], b)
            assert (p is not None) == bool(g["a_valid_%d" % b][i]), (b, c)
            if p is None:
                n_none += 1
            else:
                assert np.array_equal(p, g["a_patch_%d" % b][i, 0]), (b, c)
            if g["a_tomo_ok_%d" % b][i]:
                np.testing.assert_array_equal(ref_extract_3d_tomo(vol.astype(np.float64), c, b), g["a_tomo_%d" % b][i, 0])
        assert n_none >= 2                            # the fixture covers the `None` cases


FIXTURE_B = ["c0_16", "c0_36", "c1_16", "c1_36", "s10_|c0_52", "s10_|c0_60"]      # (prefix|)config of the (b) / (b2) runs


def b_tags(cfg):
    pre, _, rest = cfg.rpartition("|")
    return pre + "test_" + rest, pre + "train_" + rest


def test_fixture_b_shapes_and_counts():
    g = np.load(os.path.join(HERE, "golden", "tilt2d3d.npz"))
    for cfg in FIXTURE_B:
        te, tr = b_tags(cfg)
        n = len(g["b_coords_" + te])
        assert n > 0 and len(g["b_names_" + te]) == n and (g["b_len_" + te] == 1).all()
        lens = g["b_len_" + tr]
        assert len(lens) == len(g["b_coords_" + tr]) and lens.min() >= 2 and lens.max() <= 5
        assert len(g["b_means_" + tr]) == lens.sum() and len(g["b_sets_" + tr]) == lens[g["b_store_" + tr]].sum()
    # the (b2) runs exercise what the dataset adds: picks dropped by the border rule (a larger box keeps fewer), a pick
    # dropped for an invalid tilt patch (same box, one pick fewer than with 13 tilts), and a partial training set
    assert len(g["b_coords_s10_test_c0_60"]) < len(g["b_coords_s10_test_c0_52"]) < len(g["b_coords_test_c0_16"])
    assert (g["b_len_s10_train_c0_60"] < 5).any()


def test_keep_rule_is_the_references():
    """:205-218: test keeps a pick with a valid own patch; train needs `len(patch_sets) > 1` (a valid own patch and at least
    one valid shifted copy)."""
    import torch
    from cet_pick_amd.datasets.simsiam2d3d import keep_mask
    rng = np.random.default_rng(3)
    valid = rng.random((400, 5)) < 0.4
    want_train = [bool(v[0]) and 1 + int(v[1:].sum()) > 1 for v in valid]
    assert keep_mask(torch.as_tensor(valid)).tolist() == want_train
    assert keep_mask(torch.as_tensor(valid[:, :1])).tolist() == valid[:, 0].tolist()
    assert sum(want_train) < valid[:, 0].sum()                      # the sample has picks that only the test split keeps


def _write_list(tmp_path, header, rows):
    p = tmp_path / "sub" / "list.txt"
    p.parent.mkdir(exist_ok=True)
    p.write_text("\t".join(header) + "\n" + "".join("\t".join(r) + "\n" for r in rows))
    return str(p)


def test_four_column_list_relative_paths_and_column_order(tmp_path):
    from cet_pick_amd.datasets.tomo_files import read_image_list_2d3d
    path = _write_list(tmp_path, ["tilt_path", "image_name", "angle_path", "rec_path"],
                       [["t1.mrc", "tomo1", "a1.tlt", "r1.mrc"], ["/abs/t2.mrc", "tomo2", "a2.tlt", "/abs/r2.mrc"]])
    rows = read_image_list_2d3d(path)
    base = str(tmp_path / "sub")
    assert rows == [("tomo1", os.path.join(base, "r1.mrc"), os.path.join(base, "t1.mrc"), os.path.join(base, "a1.tlt")),
                    ("tomo2", "/abs/r2.mrc", "/abs/t2.mrc", os.path.join(base, "a2.tlt"))]


def test_four_column_list_missing_column_is_named(tmp_path):
    from cet_pick_amd.datasets.tomo_files import read_image_list, read_image_list_2d3d
    path = _write_list(tmp_path, ["image_name", "rec_path", "tilt_path"], [["tomo1", "r1.mrc", "t1.mrc"]])
    with pytest.raises(ValueError, match="missing angle_path"):
        read_image_list_2d3d(path)
    assert read_image_list(path) == [("tomo1", os.path.join(str(tmp_path / "sub"), "r1.mrc"))]   # the 2-column reader is unchanged
    short = _write_list(tmp_path, ["image_name", "rec_path", "tilt_path", "angle_path"], [["tomo1", "r1.mrc"]])
    with pytest.raises(ValueError, match="columns"):
        read_image_list_2d3d(short)


@pytest.mark.parametrize("bbox", [35, 17])
def test_odd_bbox_is_rejected_before_device_work(tmp_path, bbox):
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.datasets.simsiam2d3d import SyntheticSimSiam2D3DDataset, TomoFileSimSiam2D3DDataset
    opt = SimpleNamespace(data_dir=str(tmp_path), train_img_txt="none.txt", compress=False, gauss=0, batch_size=8, seed=1)
    for cls in (TomoFileSimSiam2D3DDataset, SyntheticSimSiam2D3DDataset):
        with pytest.raises(ValueError, match="even --bbox"):
            cls(opt, "train", (3, bbox, bbox))
    with pytest.raises(ValueError, match="even --bbox"):
        S.check_tilt_crop(bbox, bbox, 96, 96)


def test_tilt_border_is_python_floor_division():
    from cet_pick_amd.datasets import subvols as S
    assert S.tilt_border(36) == 19.0 and S.tilt_border(16) == 8.0
    for c in range(2, 112, 2):                         # the skip rule keeps every even window inside the image
        S.check_tilt_crop(c, c, 4 * c, 4 * c)


def test_tilt_and_tomogram_size_mismatch_is_rejected(tmp_path):
    from cet_pick_amd.utils import loader as Ld
    from cet_pick_amd.utils import mrc
    rec = np.zeros((30, 16, 40), np.float32)           # (nz, ny, nx) on disk; order 'xzy' -> (Z' = ny, H = nz, W = nx)
    good = np.zeros((5, 30, 40), np.float32)           # order 'zxy' -> (T, 30, 40)
    bad = np.zeros((5, 30, 41), np.float32)
    for name, a in (("r.mrc", rec), ("good.mrc", good), ("bad.mrc", bad)):
        mrc.write(str(tmp_path / name), a)
    np.savetxt(str(tmp_path / "a.tlt"), np.arange(-6, 9, 3.0))
    np.savetxt(str(tmp_path / "a4.tlt"), np.arange(4.0))
    p = lambda n: str(tmp_path / n)  # noqa: E731
    Ld.check_tilt_rec_sizes(["t"], [p("good.mrc")], [p("r.mrc")], [p("a.tlt")])
    with pytest.raises(ValueError, match="tomogram's size"):
        Ld.load_tomo_all_and_angles_from_list(["t"], [p("bad.mrc")], [p("r.mrc")], [p("a.tlt")])
    with pytest.raises(ValueError, match="4 angles for the 5 tilts"):
        Ld.load_tomo_all_and_angles_from_list(["t"], [p("good.mrc")], [p("r.mrc")], [p("a4.tlt")])
