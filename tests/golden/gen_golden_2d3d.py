"""Golden vectors of the 2d3d exploration mode -> tilt2d3d.npz, by IMPORTING the reference's dataset class
(datasets/tomo_pre_proj_angle_select_new2d3d.py `TOMOPreProjAngleSelect2D3D`).  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_2d3d.py
Importing gen_golden brings its package stubs; torchio (absent) is an inert stub: the methods used never reach it.
Inputs are regenerated from seeds (cet_pick_amd.synthetic.tilt2d3d_inputs); the fixture holds coordinates and outputs.

  (a) `extract_patches` / `extract_3d_tomo` (where its window lies inside the tomogram) on explicit centres (skipped
      tilts, every tilt skipped, a constant region: the `None` case), on the selected tilts of a stack whose rows 0..27
      are set to 0.5
  (b) `load_data` for the test and train splits, --compress off and on, bbox 16 and 36: coords, names, set lengths, the
      four mean / std scalars, every kept patch's mean (sets flattened in order) and whole patches (every train set at
      bbox 16, otherwise the first pick's, to keep the file small)
  (b2) the same on a tilt series with ONE tilt inside [-20, 20] (10 degrees), bbox 52 and 60, --compress off: picks that
      the border rule or an invalid tilt patch drop, and partial sets (3 of 5 variants), only those stored whole
"""
import os
import sys
import tempfile
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs + sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CONST_ROWS = 28             # (a): tilt rows [0, 28) hold 0.5
N_BIG = 1                   # (b): picks whose whole patches are stored above bbox 16 (besides partial sets)
ANGLES_B2 = np.array([-30.0, 10.0, 30.0])    # (b2): ONE tilt inside [-20, 20]: picks dropped, partial sets


def _reference_module():
    sys.path.insert(0, "/root/reference/cet_pick")
    G._stub("torchio", Compose=None)
    from cet_pick.datasets import tomo_pre_proj_angle_select_new2d3d as RD
    return RD


def explicit_centres():
    """(x, y, z) centres of (a): inside, near every border (some tilts skipped), skipped everywhere, and constant."""
    return np.array([[48, 48, 20], [30, 60, 5], [70, 40, 40], [22, 50, 30], [75, 70, 12], [48, 77, 22], [88, 48, 22],
                     [24, 40, 2], [60, 14, 20], [40, 18, 35]], dtype=np.int64)


def gen():
    from cet_pick_amd.synthetic import make_tilt_series, tilt2d3d_inputs
    RD = _reference_module()
    C = RD.TOMOPreProjAngleSelect2D3D
    vol, vol_c, tilts, angles = tilt2d3d_inputs()
    sel = np.nonzero((angles >= -20) & (angles <= 20))[0]
    out = {"a_centres": explicit_centres().astype(np.int32), "a_sel": sel.astype(np.int32)}
    # (a)
    t_a = tilts.copy()
    t_a[:, :CONST_ROWS] = 0.5
    used_v = t_a[sel]
    Z, H, W = vol.shape
    for b in (16, 36):
        me = C.__new__(C)
        me.__dict__.update(crop_size_x=b, crop_size_y=b, tomo_size=[W, H, Z], opt=SimpleNamespace(compress=False))
        ps, ok, p3, ok3 = [], [], [], []
        for c in explicit_centres():
            p = C.extract_patches(me, used_v, list(c), angles[sel], tomo_size=[W, H, Z])
            ok.append(p is not None)
            ps.append(p.numpy() if p is not None else np.zeros((1, b, b), np.float32))
            inside = c[0] - b // 2 >= 0 and c[0] + b // 2 <= W and c[1] - b // 2 >= 0 and c[1] + b // 2 <= H
            p3.append(C.extract_3d_tomo(me, vol.astype(np.float64), list(c)).numpy() if inside else np.zeros((1, b, b), np.float32))
            ok3.append(inside)
        out["a_valid_%d" % b] = np.array(ok)
        out["a_tomo_ok_%d" % b] = np.array(ok3)
        out["a_patch_%d" % b] = np.stack(ps)
        out["a_tomo_%d" % b] = np.stack(p3)
    # (b) and (b2)
    tilts1 = make_tilt_series(vol, ANGLES_B2)
    runs = [(False, b, tilts, angles, "") for b in (16, 36)] + [(True, b, tilts, angles, "") for b in (16, 36)]
    runs += [(False, b, tilts1, ANGLES_B2, "s10_") for b in (52, 60)]
    with tempfile.TemporaryDirectory() as td:
        lst = os.path.join(td, "list.txt")
        with open(lst, "w") as f:
            f.write("image_name\trec_path\ttilt_path\tangle_path\nsyn\tr.mrc\tt.mrc\ta.tlt\n")
        for compress, b, tl, an, pre in runs:
            rec = (vol_c if compress else vol).astype(np.float64)

            def fake_loader(names, tilt_paths, rec_paths, angle_paths, compress=False, denoise=0, _rec=rec, _t=tl, _a=an):
                return {"syn": _t.copy()}, {"syn": _rec.copy()}, {"syn": np.asarray(_a, np.float64).reshape(-1, 1).copy()}

            RD.load_tomo_all_and_angles_from_list = fake_loader
            for split in ("test", "train"):
                tag = "%s%s_c%d_%d" % (pre, split, int(compress), b)
                me = C.__new__(C)
                me.__dict__.update(data_dir=lst, opt=SimpleNamespace(compress=compress, gauss=0), size=(3, b, b),
                                   crop_size_x=b, crop_size_y=b, coords=[], names_all=[], low=-20, up=20, split=split,
                                   sigma1=[2.5, 5], K=5000)
                tomos, names, sub_vols, sets, sub3d, sets3d = C.load_data(me)
                out["b_coords_" + tag] = np.asarray(me.coords, dtype=np.int32).reshape(-1, 3)
                out["b_names_" + tag] = np.asarray(me.names_all)
                out["b_stats_" + tag] = np.array([float(me.mean_subvols), float(me.std_subvols),
                                                  float(me.mean_subvols3d), float(me.std_subvols3d)])
                if split == "test":
                    sets, sets3d = [[p] for p in sub_vols], [[p] for p in sub3d]
                lens = np.array([len(s) for s in sets], dtype=np.int32)
                out["b_len_" + tag] = lens
                # every patch's mean, in the flattened order of the sets (cheap, and it pins the order of partial sets)
                out["b_means_" + tag] = np.array([float(p.double().mean()) for s in sets for p in s])
                out["b_means3d_" + tag] = np.array([float(p.double().mean()) for s in sets3d for p in s])
                # whole patches: every train set at bbox 16, the first pick's set (not in b2) and every partial set
                first = N_BIG if not pre else 0
                store = [i for i in range(len(sets)) if (b == 16 and split == "train") or i < first or 1 < lens[i] < 5]
                out["b_store_" + tag] = np.array(store, dtype=np.int32)
                for key, ss in (("b_sets_", sets), ("b_sets3d_", sets3d)):
                    ps = [p.numpy() for i in store for p in ss[i]]
                    out[key + tag] = np.stack(ps) if ps else np.zeros((0, 1, b, b), np.float32)
                print(tag, len(me.coords), "picks, set sizes", sorted(set(lens.tolist())))
    G.save("tilt2d3d.npz", **out)


if __name__ == "__main__":
    gen()
