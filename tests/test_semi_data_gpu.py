"""The detector's file-backed data path on the GPU: `mi_semi_labels` against the reference fixture tests/golden/semi_labels.npz
and the numpy restatement of tests/test_oracle_semi_data.py, `mi_semi_pairs` against numpy slicing of the same table, the
dataset's train and val samples, and main.py / test.py on MRC files with a coordinate table."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_oracle_semi_data import FIXTURE_TAGS, fixture_labels_inputs, np_labels

pytestmark = pytest.mark.gpu


def _opt(**kw):
    o = dict(down_ratio=2, pn=False, bbox=16, translation_ratio=0.5, fiber=False, compress=False, batch_size=1, seed=11)
    o.update(kw)
    return SimpleNamespace(**o)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


@pytest.mark.parametrize("tag", FIXTURE_TAGS)
def test_label_kernel_equals_reference_fixture(golden, tag, tmp_path):
    from cet_pick_amd.datasets import semi_files as SF
    g = golden("semi_labels.npz")
    for n, shape, c, st, fill in fixture_labels_inputs(g, tag, tmp_path):
        got = SF.render_labels(shape, c, st, fill)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), g["hm_%s_%s" % (tag, n)].view(np.uint32)), (tag, n)


@pytest.mark.parametrize("bbox,fiber", [(16, False), (36, False), (36, True)])
def test_label_kernel_equals_numpy_on_many_random_centres(bbox, fiber):
    from cet_pick_amd.datasets import semi_files as SF
    shape = (64, 256, 256)
    rng = np.random.default_rng(bbox + int(fiber))
    c = np.stack([rng.integers(-8, shape[2] + 8, 3000), rng.integers(-8, shape[1] + 8, 3000), rng.integers(-8, shape[0] + 8, 3000)], 1)
    st = SF.label_stencil(SF.label_radius(bbox), fiber=fiber)
    for fill in (False, True):
        got = SF.render_labels(shape, c, st, fill)
        assert np.array_equal(_bits(got), np_labels(shape, c, st, fill).view(np.uint32)), fill
    # the same call twice: the atomic max does not depend on arrival order
    a, b = SF.render_labels(shape, c, st, True), SF.render_labels(shape, c[::-1].copy(), st, True)
    assert torch.equal(a, b)
    # no centre at all: zeros, or -1 everywhere
    assert float(SF.render_labels((6, 40, 40), np.zeros((0, 3)), st, True).max()) == -1.0


def _np_pairs(tomos, labels, owner, centres, first, n, flip_y):
    inp, hm = [], []
    for s in range(first, first + n):
        t, (x, y, z) = owner[s], centres[s]
        inp.append(tomos[t][z - 3:z + 3, 2 * y - 32:2 * y + 32, 2 * x - 32:2 * x + 32])
        hm.append(labels[t][z - 3:z + 3, y - 16:y + 16, x - 16:x + 16])
    inp = np.stack(inp)
    return inp, np.flip(inp, 2 if flip_y else 3), np.stack(hm)[:, None]


@pytest.mark.parametrize("batch", [1, 16])
def test_pair_kernel_equals_numpy_slicing(batch):
    from cet_pick_amd.datasets import semi_files as SF
    shapes = np.array([(12, 100, 130), (30, 256, 200), (6, 68, 69)], np.int64)
    rng = np.random.default_rng(batch)
    tomos = [rng.standard_normal(tuple(s)).astype(np.float32) for s in shapes]
    labels = [rng.standard_normal((s[0], s[1] // 2, s[2] // 2)).astype(np.float32) for s in shapes]
    anns = np.concatenate([np.stack([rng.integers(0, s[2] // 2, 20), rng.integers(0, s[1] // 2, 20), rng.integers(0, s[0], 20),
                                     np.full(20, t)], 1) for t, s in enumerate(shapes)], 0)
    owner, cen, flip = SF.draw_pairs(anns, shapes, 16, 0.5, seed=1, epoch=0, batch_size=batch)
    assert set(owner.tolist()) == {0, 1, 2}
    td = [torch.as_tensor(t).cuda() for t in tomos]
    ld = [torch.as_tensor(t).cuda() for t in labels]
    tdesc, ldesc = SF._descriptors(td, "cuda"), SF._descriptors(ld, "cuda")
    o_d, c_d = torch.as_tensor(owner).cuda(), torch.as_tensor(cen).cuda()
    for k in range(min(3, len(flip))):
        for flip_y in (False, True):
            got = SF.semi_pairs(tdesc, ldesc, 3, o_d, c_d, 2 * k * batch, 2 * batch, flip_y)
            want = _np_pairs(tomos, labels, owner, cen, 2 * k * batch, 2 * batch, flip_y)
            assert got[0].shape == (2 * batch, 6, 64, 64) and got[2].shape == (2 * batch, 1, 6, 32, 32)
            for g_, w_ in zip(got, want):
                assert np.array_equal(_bits(g_), np.ascontiguousarray(w_).view(np.uint32)), (k, flip_y)


def test_train_batches_hold_a_positive_in_every_own_crop():
    from cet_pick_amd.datasets.semi_files import TomoFileDetectorDataset
    from cet_pick_amd.synthetic import make_tomo
    tomos, coords = {}, {}
    for i, shape in enumerate([(24, 160, 192), (16, 136, 136)]):
        vol, c = make_tomo(shape, seed=40 + i, margin_xy=40, margin_z=6)
        tomos["t%d" % i], coords["t%d" % i] = torch.as_tensor(vol).cuda(), c
    tomos["empty"] = torch.zeros((8, 80, 80), device="cuda")
    n = sum(len(c) for c in coords.values())
    ds = TomoFileDetectorDataset.from_arrays(_opt(batch_size=2), "train", tomos, coords)
    assert len(ds) == n // 2
    for epoch in (1, 2):
        ds.set_epoch(epoch)
        m = 0
        for batch in ds:
            assert batch["input"].shape == batch["input_aug"].shape == (4, 6, 64, 64)
            assert batch["hm"].shape == (4, 1, 6, 32, 32)
            flip = -2 if batch["flip_prob"] > 0.5 else -1
            assert torch.equal(batch["input_aug"], batch["input"].flip(flip))
            hm = batch["hm"].cpu().numpy()
            assert (hm[0::2].reshape(2, -1).max(1) == 1.0).all()
            assert set(np.unique(hm).tolist()) <= set([-1.0]) | set(ds.stencil[ds.stencil > 0].tolist())
            m += 1
        assert m == len(ds)
    with pytest.raises(ValueError, match="at least 2"):
        TomoFileDetectorDataset.from_arrays(_opt(), "train", tomos, {"t0": coords["t0"][:1]})
    with pytest.raises(ValueError, match="68"):
        TomoFileDetectorDataset.from_arrays(_opt(), "train", {"s": torch.zeros((8, 66, 80), device="cuda")},
                                            {"s": np.array([[40, 30, 4], [50, 30, 4]])})
    with pytest.raises(ValueError, match="down_ratio"):
        TomoFileDetectorDataset.from_arrays(_opt(down_ratio=4), "train", tomos, coords)
    with pytest.raises(NotImplementedError):
        TomoFileDetectorDataset.from_arrays(_opt(pn=True), "train", tomos, coords)


def test_val_samples_and_the_subregion_rule():
    from cet_pick_amd.datasets import semi_files as SF
    big = torch.rand((112, 528, 528), device="cuda")
    small = torch.rand((20, 96, 128), device="cuda")
    coords = {"big": np.array([[300, 300, 50], [420, 210, 10]]), "small": np.array([[60, 40, 10]])}
    ds = SF.TomoFileDetectorDataset.from_arrays(_opt(), "val", {"big": big, "small": small, "none": small.clone()}, coords)
    items = list(ds)
    assert len(ds) == len(items) == 3 and [it["meta"]["name"] for it in items] == [["big"], ["small"], ["none"]]
    st = SF.label_stencil(SF.label_radius(16))
    full = np_labels((112, 264, 264), SF.downscale(coords["big"]), st, False)
    assert torch.equal(items[0]["input"], big[:110, 200:700, 200:700][None])
    assert items[0]["input"].shape == (1, 110, 328, 328) and items[0]["hm"].shape == (1, 1, 110, 164, 164)
    assert np.array_equal(_bits(items[0]["hm"][0, 0]), full[:110, 100:350, 100:350].view(np.uint32))
    assert torch.equal(items[1]["input"], small[None]) and items[1]["hm"].shape == (1, 1, 20, 48, 64)
    assert float(items[1]["hm"].max()) == 1.0 and float(items[1]["hm"].min()) == 0.0
    assert float(items[2]["hm"].abs().max()) == 0.0                                       # listed, no particle: all background
    with pytest.raises(ValueError, match="heat-map"):
        SF.TomoFileDetectorDataset.from_arrays(_opt(), "val", {"odd": torch.rand((8, 81, 80), device="cuda")}, {})


def test_detector_main_and_test_on_mrc_files_with_a_coordinate_table(tmp_path, monkeypatch, capsys):
    from cet_pick_amd import main as det_main, test as det_test
    from cet_pick_amd.opts import opts
    from cet_pick_amd.synthetic import make_tomo
    from cet_pick_amd.utils import mrc
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data"
    data.mkdir()
    lines, rows = ["image_name\trec_path"], ["image_name\tx_coord\ty_coord\tz_coord"]
    for i in range(2):
        vol, c = make_tomo((32, 160, 160), seed=600 + i, margin_xy=40, margin_z=8)
        name = "tomo%d" % i
        mrc.write(str(data / (name + ".rec")), vol)
        lines.append("%s\t%s.rec" % (name, name))
        rows += ["%s\t%d\t%d\t%d" % (name, x, y, z) for x, y, z in c]
    (data / "train_images.txt").write_text("\n".join(lines) + "\n")
    # (test.py opens the listed paths as given: absolute ones here; the train list's are relative to the list)
    (data / "test_images.txt").write_text("\n".join(lines[:1] + ["%s\t%s" % (n, data / p) for n, p in
                                                               (ln.split("\t") for ln in lines[1:])]) + "\n")
    (data / "coords.txt").write_text("\n".join(rows) + "\n")
    n_rows = len(rows) - 1
    args = ["semi", "--arch", "unet_4", "--contrastive", "--dataset", "semi", "--order", "zxy", "--bbox", "16",
            "--batch_size", "2", "--num_epochs", "2", "--lr", "0.001", "--lr_step", "1", "--val_intervals", "2", "--exp_id", "f",
            "--debug", "0", "--train_img_txt", "train_images.txt", "--train_coord_txt", "coords.txt"]
    det_main.main(opts().parse(args))
    out = capsys.readouterr().out
    assert "Loaded train %d samples" % n_rows in out and "Loaded val 2 samples" in out
    save_dir = os.path.join(str(tmp_path), "exp", "semi", "f")
    lines = open(os.path.join(save_dir, "log.txt")).read().strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("epoch: 1 |loss ")
    assert lines[1].count("hm_loss") == 2                                               # train + val columns
    vals = [float(v.split()[1]) for v in lines[1].split("|")[1:] if v.strip() and v.split()[0] in ("loss", "hm_loss")]
    assert len(vals) == 4 and np.isfinite(vals).all()
    for f in ("model_last_contrastive.pth", "model_1.pth", "model_last.pth", "model_best_contrastive.pth"):
        assert os.path.exists(os.path.join(save_dir, f)), f
    # a missing coordinate file is an error, not a silent fall-back to synthetic data
    (data / "coords.txt").unlink()
    with pytest.raises(FileNotFoundError, match="coords.txt"):
        det_main.main(opts().parse([a if a != "f" else "g" for a in args]))
    # test.py on the trained detector, on the listed tomograms
    det_test.test(opts().parse(["semi", "--arch", "unet_4", "--exp_id", "f", "--debug", "0", "--with_score", "--K", "100",
                                "--order", "zxy", "--cutoff_z", "1", "--out_thresh", "0.0", "--out_id", "picks",
                                "--load_model", os.path.join(save_dir, "model_last.pth")]))
    for name in ("tomo0", "tomo1"):
        hm, _ = mrc.parse_mrc(os.path.join(save_dir, "picks", name + "_hm.mrc"))
        assert np.isfinite(hm).all() and hm.size == 32 * 80 * 80
        assert os.path.exists(os.path.join(save_dir, "picks", name + ".txt"))
