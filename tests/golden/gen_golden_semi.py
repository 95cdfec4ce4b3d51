"""Golden vectors of the detector's label volumes -> semi_labels.npz, by IMPORTING the reference (utils/image.py
`gaussian_radius`, `gaussian3D`, `gaussian3D_discrete`, `draw_umich_gaussian_3d`; datasets/tomo_moco.py
`TOMOMoco.load_data` with `load_tomos_from_list` fed in-memory volumes).  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_semi.py
Importing gen_golden brings its package stubs.  The fixture holds the coordinate table, the tomogram extents and the outputs.

  (a) the radius and the stencil (gaussian3D, and gaussian3D_discrete(label1=1, label2=0, thresh=0.2) of --fiber) at bbox 12,
      16 and 36
  (b) `load_data` for the train and val splits, --fiber off and on, --compress off and on, bbox 16 and 36: the label volume of
      each listed tomogram and `all_anns`.  The table has float coordinates, centres on, beyond and negative past every face,
      overlapping blobs, a row of an image that is not listed and a listed image without rows.
"""
import math
import os
import sys
import tempfile
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs + sys.path)
import numpy as np  # noqa: E402

SHAPES = {"ta": (14, 40, 48), "tb": (10, 36, 36)}        # (D, H, W) of the listed tomograms (after --compress: as given)
BBOXES = (12, 16, 36)


def coord_rows():
    """(image_name, x, y, z) rows at full resolution; the labels are (D, H//2, W//2) = (14, 20, 24) for 'ta'."""
    rows = [("ta", 20, 16, 7), ("ta", 22.9, 18.2, 7.6), ("ta", 0, 0, 0), ("ta", 47, 39, 13), ("ta", -3.7, 10, 5),
            ("ta", -9, 20, 4), ("ta", 52, 12, 6), ("ta", 20, -5, 3), ("ta", 30, 44, 9), ("ta", 10, 30, -2),
            ("ta", 18, 24, 15), ("ta", 8, 8, 27), ("ta", 60, 60, 40), ("ta", -20, -20, -20), ("ta", 46, 2, 1),
            ("zz", 10, 10, 2)]
    return rows


def _reference_module():
    sys.path.insert(0, "/root/reference/cet_pick")
    from cet_pick.datasets import tomo_moco as RT
    from cet_pick.utils import image as RI
    return RT, RI


def gen():
    RT, RI = _reference_module()
    out = {}
    for b in BBOXES:
        h = b // 2
        r = max(0, int(RI.gaussian_radius((math.ceil(h), math.ceil(h)))))
        d = 2 * r + 1
        out["radius_%d" % b] = np.int32(r)
        out["stencil_%d_f0" % b] = RI.gaussian3D((d, d, d), sigma=d / 6)
        out["stencil_%d_f1" % b] = RI.gaussian3D_discrete((d, d, d), sigma=d / 6, label1=1, label2=0, thresh=0.2)
    rows = coord_rows()
    out["coord_names"] = np.array([r[0] for r in rows])
    out["coord_xyz"] = np.array([r[1:] for r in rows], dtype=np.float64)
    out["tomo_names"] = np.array(list(SHAPES))
    out["tomo_shapes"] = np.array(list(SHAPES.values()), dtype=np.int32)
    rng = np.random.default_rng(5)
    vols = {n: rng.random(s).astype(np.float32) for n, s in SHAPES.items()}
    RT.load_tomos_from_list = lambda names, paths, order="xzy", compress=False, denoise=0: {n: vols[n] for n in names}
    with tempfile.TemporaryDirectory() as td:
        lst, crd = os.path.join(td, "list.txt"), os.path.join(td, "coords.txt")
        with open(lst, "w") as f:
            f.write("image_name\trec_path\n" + "".join("%s\t%s.mrc\n" % (n, n) for n in SHAPES))
        with open(crd, "w") as f:
            f.write("image_name\tx_coord\ty_coord\tz_coord\n" + "".join("%s\t%s\t%s\t%s\n" % r for r in rows))
        for split in ("train", "val"):
            for fiber in (False, True):
                for compress in (False, True):
                    for b in (16, 36):
                        tag = "%s_f%d_c%d_%d" % (split, int(fiber), int(compress), b)
                        me = RT.TOMOMoco.__new__(RT.TOMOMoco)
                        me.__dict__.update(data_dir=lst, coord_dir=crd, split=split, opt=SimpleNamespace(
                            down_ratio=2, bbox=b, compress=compress, fiber=fiber, pn=False, order="xzy", gauss=0))
                        tomos, hms, inds, gt_dets, names, all_anns = RT.TOMOMoco.load_data(me)
                        assert list(names) == list(SHAPES)
                        for n, hm in zip(names, hms):
                            out["hm_%s_%s" % (tag, n)] = hm
                        out["anns_" + tag] = np.array(all_anns, dtype=np.int32).reshape(-1, 4)
                        print(tag, [float((hm > 0).sum()) for hm in hms])
    G.save("semi_labels.npz", **out)


if __name__ == "__main__":
    gen()
