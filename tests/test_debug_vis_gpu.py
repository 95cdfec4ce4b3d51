"""csrc/debug_vis.hip through the wrappers of utils/debug_vis.py against the restatement of tests/debug_vis_ref.py (every byte
of all four pictures), and the detector's training entry with --debug 4 end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_vis_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

D = 4
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))
THR = np.float32(0.3)
JUST_ABOVE = np.nextafter(THR, np.float32(1))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- min and max ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,z0,nz", [((5, 18, 22), 1, 3), ((3, 66, 140), 1, 2), ((5, 18, 22), 0, 5)])
def test_minmax_equals_numpy(shape, z0, nz):
    from cet_pick_amd.utils import debug_vis as V
    rng = np.random.default_rng(sum(shape))
    vol = rng.normal(size=shape).astype(np.float32)
    vol[z0] = np.float32(-1.25)                                   # a constant slice
    vol[z0 + 1].flat[0], vol[z0 + 1].flat[-1] = np.float32(-50), np.float32(60)       # extremes at the first and last element
    want = np.stack([vol[z0:z0 + nz].min(axis=(1, 2)), vol[z0:z0 + nz].max(axis=(1, 2))], 1)
    got = V.slice_minmax(dev(vol), z0, nz).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (nz, 2) and np.array_equal(got, want)
    assert want[0].tolist() == [-1.25, -1.25] and want[1].tolist() == [-50, 60]


def test_minmax_of_slices_that_start_off_a_16_byte_line():
    import torch
    from cet_pick_amd.utils import debug_vis as V
    rng = np.random.default_rng(5)
    flat = rng.normal(size=1 + 3 * 7 * 9).astype(np.float32)      # 63 values per slice: every slice starts at another offset
    flat[1], flat[-1] = 9, -9
    vol = dev(flat)[1:].view(3, 7, 9)
    assert vol.data_ptr() % 16 == 4
    want = flat[1:].reshape(3, -1)
    got = V.slice_minmax(vol).cpu().numpy()
    assert np.array_equal(got, np.stack([want.min(1), want.max(1)], 1))
    with pytest.raises(Exception, match="bad argument"):
        V.slice_minmax(vol, 2, 2)
    torch.cuda.synchronize()


# ---- the four pictures ----------------------------------------------------------------------------------------------------

def make_case(h, w):
    rng = np.random.default_rng(100 * h + w)
    H, W = 2 * h, 2 * w
    tomo = rng.normal(size=(D, H, W)).astype(np.float32)
    tomo[2] = np.float32(0.75)                                    # a constant slice
    maps = []
    for k in range(2):
        m = rng.random(size=(D, h, w)).astype(np.float32)
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0] = 0.0, 1.0, ONE_BELOW
        m[:, h - 1, w - 1], m[:, h - 1, 0], m[:, 0, w - 1] = 1.0, ONE_BELOW, 0.0
        m[1, 2:5, 3:6] = [[0.0, 1.0, ONE_BELOW]] * 3
        maps.append(m)
    maps[1][3] = 0.0                                              # ground truth without a particle
    cx, cy = W // 2, H // 2
    pred = np.array([
        [0, 0, 1, 0.9, 0.9], [W - 1, 0, 1, 0.9, 0.9], [0, H - 1, 1, 0.9, 0.9], [W - 1, H - 1, 1, 0.9, 0.9],     # every edge clips
        [cx - 2, cy - 1, 2, 0.8, 0.8], [cx + 2, cy + 1, 2, 0.8, 0.8],                     # two overlapping rings
        [cx - 5, cy, 0, 0.5, THR],                                                        # conf == 0.3: absent
        [cx + 5, cy, 0, 0.5, JUST_ABOVE],                                                 # just above: present
        [cx, cy, -2, 0.9, 0.9], [cx, cy, D + 1, 0.9, 0.9],                                # slices outside every range
        [cx + 0.7, cy - 0.8, 3.9, 0.6, 0.6],                                              # fractional: (cx, cy - 1) on slice 3
        [np.nan, 3, 1, 0.9, 0.9]], np.float32)
    gt = np.array([[0, 0, 2], [W - 1, H - 1, 2], [W - 1, 0, 0], [0, H - 1, 0], [cx, cy, 1], [cx + 3, cy, 1],
                   [cx + 0.5, cy + 0.5, 3.5], [cx, cy, D]], np.float32)
    return dict(h=h, w=w, H=H, W=W, tomo=tomo, hm_pred=maps[0], hm_gt=maps[1], pred=pred, gt=gt, cx=cx, cy=cy)


@pytest.fixture(scope="module", params=[(9, 11), (33, 70)], ids=["9x11", "33x70"])
def case(request):
    c = make_case(*request.param)
    c["want"] = R.render(c["tomo"], c["hm_pred"], c["hm_gt"], 0, D, c["pred"], c["gt"], THR, 8)
    c["want"].setflags(write=False)
    return c


def test_the_reference_pictures_hold_what_the_cases_are_about(case):
    want, cx, cy, H, W = case["want"], case["cx"], case["cy"], case["H"], case["W"]
    blue = (want == np.array(R.BLUE, np.uint8)).all(-1)
    assert not blue[:2].any()
    assert blue[2, 0, cy, cx + 5 - 8] and not blue[2, 0, cy, cx - 5 + 8]                 # conf just above / exactly 0.3
    assert blue[2, 1, 8, 0] and blue[2, 1, 0, W - 9] and blue[2, 1, H - 1, 8] and blue[2, 1, H - 9, W - 1]
    assert blue[2, 3, cy - 1, cx + 8] and blue[3, 3, cy, cx - 8]                         # fractional coordinates truncate
    assert blue[3, 1, cy, cx + 8] and blue[3, 1, cy, cx + 3 - 8] and blue[3, 2, 8, 0]
    assert (want[2, 2][~blue[2, 2]] == 0).all()                                          # the constant slice is black
    assert want[0].max() == 255 and want[0].min() == 0 and (want[1, 3] <= 77).all()
    assert {254, 255} <= set(np.unique(R.unit_bytes(case["hm_pred"])))


@pytest.mark.parametrize("z0,nz", [(0, D), (1, 2)])
def test_render_equals_the_restatement_in_every_byte(case, z0, nz):
    from cet_pick_amd.utils import debug_vis as V
    got = V.render(dev(case["tomo"]), dev(case["hm_pred"]), dev(case["hm_gt"]), z0, nz, case["pred"], case["gt"], THR, 8)
    got = got.cpu().numpy()
    want = case["want"][:, z0:z0 + nz]
    assert got.shape == want.shape == (4, nz, case["H"], case["W"], 3) and got.dtype == np.uint8
    for k, name in enumerate(V.PICTURES):
        diff = got[k] != want[k]
        assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def test_render_without_picks_and_without_ground_truth(case):
    from cet_pick_amd.utils import debug_vis as V
    got = V.render(dev(case["tomo"]), dev(case["hm_pred"]), dev(case["hm_gt"]), 0, D, np.zeros((0, 5), np.float32),
                   np.zeros((0, 3), np.float32)).cpu().numpy()
    want = case["want"]
    assert np.array_equal(got[:2], want[:2])
    grey = np.stack([R.grey_slice(case["tomo"][z]) for z in range(D)]).astype(np.uint8)
    assert np.array_equal(got[2], np.repeat(grey[..., None], 3, -1)) and np.array_equal(got[3], got[2])


def test_odd_extents_are_refused_not_rendered():
    import torch
    from cet_pick_amd import _lib as L
    from cet_pick_amd.utils import debug_vis as V
    rng = np.random.default_rng(1)
    hm = dev(rng.random(size=(2, 9, 11)).astype(np.float32))
    none5, none3 = np.zeros((0, 5), np.float32), np.zeros((0, 3), np.float32)
    for shape in ((2, 19, 22), (2, 18, 23), (2, 18, 24)):
        out = torch.full((12 * 2 * shape[1] * shape[2],), 7, dtype=torch.uint8, device="cuda")
        with pytest.raises(L.HipExtensionError, match="mi_dbgvis_render failed: bad argument"):
            V.render(dev(rng.normal(size=shape).astype(np.float32)), hm, hm, 0, 2, none5, none3, out=out)
        assert bool((out == 7).all())
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        V.render(dev(rng.normal(size=(2, 18, 22)).astype(np.float32)), hm, hm, 0, 2, none5, none3, radius=32)


# ---- end to end -----------------------------------------------------------------------------------------------------------

CENTRES = {"tomo0": [(36, 36, 21), (24, 44, 22)], "tomo1": [(40, 30, 20), (30, 42, 23)]}


def run_main(tmp_path, exp_id, debug):
    from cet_pick_amd import main as det_main
    from cet_pick_amd.opts import opts
    args = ["semi", "--arch", "unet_4", "--contrastive", "--dataset", "semi", "--order", "zxy", "--bbox", "16",
            "--batch_size", "2", "--num_epochs", "1", "--num_iters", "2", "--lr", "0.001", "--val_intervals", "1",
            "--exp_id", exp_id, "--debug", str(debug), "--train_img_txt", "train_images.txt", "--train_coord_txt", "coords.txt"]
    det_main.main(opts().parse(args))
    return os.path.join(str(tmp_path), "exp", "semi", exp_id, "debug")


def test_training_with_debug_4_leaves_the_table_and_the_slice_pictures(tmp_path, monkeypatch):
    from PIL import Image
    from cet_pick_amd.utils import mrc
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data"
    data.mkdir()
    lines, rows = ["image_name\trec_path"], ["image_name\tx_coord\ty_coord\tz_coord"]
    for i, (name, cs) in enumerate(CENTRES.items()):
        vol = np.random.default_rng(40 + i).normal(size=(44, 72, 72)).astype(np.float32)
        mrc.write(str(data / (name + ".rec")), vol)
        lines.append("%s\t%s.rec" % (name, name))
        rows += ["%s\t%d\t%d\t%d" % ((name,) + c) for c in cs]
    (data / "train_images.txt").write_text("\n".join(lines) + "\n")
    (data / "coords.txt").write_text("\n".join(rows) + "\n")

    debug_dir = run_main(tmp_path, "dbg", 4)
    files = sorted(os.listdir(debug_dir))
    assert len(files) == 2 * 17, files
    for it, (name, cs) in enumerate(CENTRES.items()):
        mine = [f for f in files if name in f]
        assert [f for f in mine if f.endswith(".txt")] == ["%s_%d.txt" % (name, it)]
        pngs = {"%d_%s%s%d.png" % (it, name, pic, z) for pic in ("pred_hm", "gt_hm", "pred_out", "gt_out") for z in range(20, 24)}
        assert set(mine) - {"%s_%d.txt" % (name, it)} == pngs
        for f in pngs:
            assert np.asarray(Image.open(os.path.join(debug_dir, f))).shape == (72, 72, 3), f
        for line in open(os.path.join(debug_dir, "%s_%d.txt" % (name, it))):
            x, z, y, score = line.rstrip("\n").split("\t")
            assert 0 <= int(x) < 72 and 0 <= int(y) < 72 and 0 <= int(z) < 44 and float(score) > 0.3
        for x, y, z in cs:                                        # the ring of every annotated centre, in blue
            img = np.asarray(Image.open(os.path.join(debug_dir, "%d_%sgt_out%d.png" % (it, name, z))))
            for dx, dy in R.ring_offsets(8):
                assert img[y + dy, x + dx].tolist() == [0, 0, 255], (name, z, dx, dy)
            assert img[y, x, 0] == img[y, x, 1] == img[y, x, 2]   # grey inside
            back = np.asarray(Image.open(os.path.join(debug_dir, "%d_%sgt_hm%d.png" % (it, name, z))))
            assert back[y, x, 0] >= 100                           # the label's peak over the slice: 0.7 (9 x 255 + 8 >> 4) at least

    debug_dir = run_main(tmp_path, "dbg0", 0)
    assert not os.path.isdir(debug_dir) or os.listdir(debug_dir) == []
