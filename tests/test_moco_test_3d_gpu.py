"""cet_pick_amd.moco_test_3d end to end on a synthetic tomogram: the file it writes, eval-mode inference on the query encoder of
a checkpoint as moco_main saves it, and the invariance of the pose-pooled embedding under a quarter turn of the tomogram.

--bbox 16 is the smallest box that still holds a voxel per stride of the encoder: the stem (stride 2) and its pool (stride 2) give
16 -> 8 -> 4, layer2 and layer3 (stride 2 each) 4 -> 2 -> 1.

Measured on the MI355X (printed again with -s): one crop at two batch positions gives the same bits, so the invariance tolerance is
the pooling kernel's 1e-5; turned tomogram --tta 8 5.96e-08, --tta 1 1.19e-01; --tta 1 against F.normalize(forward_test(crop_znorm))
2.98e-08; a training-mode copy of the encoder 4.1e-01."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BBOX = 16
SHAPE = (40, 96, 96)
POOL_ATOL = 1e-5                 # tests/test_embed_pool_gpu.py: the pooling kernel's bound on unit-norm rows


def _tomogram():
    rng = np.random.default_rng(77)
    vol = rng.standard_normal(SHAPE).astype(np.float32)
    zz, yy, xx = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
    for (z, y, x), s, sy in (((20, 30, 30), 3.0, 1.0), ((18, 60, 40), 2.5, 2.0), ((22, 40, 66), 3.5, 0.6), ((20, 64, 70), 3.0, 1.5),
                             ((16, 24, 62), 2.0, 2.5), ((24, 70, 24), 3.0, 0.8)):
        vol -= (4.0 * np.exp(-((zz - z) ** 2 + ((yy - y) / sy) ** 2 + (xx - x) ** 2) / (2 * s * s))).astype(np.float32)
    return vol


def _wrapper():
    """a MoCo wrapper with seeded O(1) weights; every BatchNorm's running statistics far from its batch statistics, the key
    encoder and the queue different from the query encoder"""
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.models.moco import MoCo
    from cet_pick_amd.synthetic import seeded_state_dict
    heads = {"proj": 256, "pred": 256}
    q, k = create_model("moco3d_18", heads, -1), create_model("moco3d_18", heads, -1)
    q.load_state_dict(seeded_state_dict(q, seed=11))
    k.load_state_dict(seeded_state_dict(k, seed=12))
    g = torch.Generator().manual_seed(13)
    for m in q.modules():
        if hasattr(m, "running_mean") and m.running_mean is not None:
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.5)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
    model = MoCo(q, k, dim=128)
    with torch.no_grad():
        for pq, pk in zip(q.parameters(), k.parameters()):
            pk.copy_(pq * 0.5 + 0.01)                 # (the constructor copied q into k: a loader that took encoder_k would pass unseen)
    return model


def _opt(extra):
    from cet_pick_amd.opts import opts
    return opts().parse(["moco", "--arch", "moco3d_18", "--order", "zxy", "--bbox", str(BBOX), "--dog", "3,5", "--debug", "0",
                         "--test_img_txt", "list.txt"] + extra)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the files, one `test(opt)` at the default --tta, and the encoder loaded from the checkpoint"""
    from cet_pick_amd import moco_test_3d as M
    from cet_pick_amd.models.model import create_model, save_model
    from cet_pick_amd.utils import mrc
    root = tmp_path_factory.mktemp("moco_test_3d")
    (root / "data").mkdir()
    mrc.write(str(root / "data" / "t0.rec"), _tomogram())
    (root / "data" / "list.txt").write_text("image_name\trec_path\nt0\tt0.rec\n")
    wrapper = _wrapper()
    ckpt = str(root / "model_last.pth")
    save_model(ckpt, 3, wrapper, torch.optim.SGD(wrapper.parameters(), 0.1))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        opt = _opt(["--exp_id", "t8", "--load_model", ckpt])
        assert opt.tta == 8
        out = M.test(opt)
        enc = M.load_encoder(create_model("moco3d_18", {"proj": 256, "pred": 256}, -1), ckpt).cuda().eval()
        yield {"root": root, "ckpt": ckpt, "out": out, "opt": opt, "z": dict(np.load(out)), "enc": enc, "wrapper": wrapper}
    finally:
        os.chdir(cwd)


def _rec(run):
    from cet_pick_amd.datasets.tomo_files import load_listed_tomos
    return load_listed_tomos(run["opt"], "test")["t0"]


def test_output_file(run):
    from cet_pick_amd.datasets.tomo_files import TomoFileMocoLoader
    z = run["z"]
    assert run["out"] == os.path.join(str(run["root"]), "exp", "moco", "t8", "all_output_info.npz") and os.path.exists(run["out"])
    assert set(z) == {"proj", "pred", "name", "coords", "subvol", "tta", "bbox"}
    n = z["proj"].shape[0]
    assert n >= 4, "the picker kept %d picks: the tomogram of this test is too small for its box" % n
    assert z["proj"].shape == (n, 128) and z["proj"].dtype == np.float32
    assert np.all(np.abs(np.linalg.norm(z["proj"].astype(np.float64), axis=1) - 1.0) <= 1e-5)
    assert np.array_equal(z["pred"], z["proj"])
    assert int(z["tta"]) == 8 and int(z["bbox"]) == BBOX
    assert z["subvol"].shape == (n, 1, BBOX, BBOX) and np.isfinite(z["subvol"]).all()
    # the picks are what the training loader's border rule ("mirror": bbox // 2 + 1 voxels from every face) keeps of the picker's
    loader = TomoFileMocoLoader(run["opt"], crop=BBOX, device="cuda", split="test")
    assert np.array_equal(z["coords"], loader.centres) and z["coords"].shape == (n, 3)
    assert z["name"].shape == (n,) and set(z["name"]) == {"t0"}
    c = z["coords"]
    bd = BBOX // 2 + 1
    assert (c >= bd).all() and (c[:, 0] < SHAPE[2] - bd).all() and (c[:, 1] < SHAPE[1] - bd).all() and (c[:, 2] < SHAPE[0] - bd).all()
    # the pictures are simsiam_test_hm_3d's: the 8-bit round trip + Normalize of the min-max'ed z-sums
    from cet_pick_amd.datasets import subvols as S
    pics = S.extract_subvols(_rec(run), c, (3, BBOX, BBOX))
    mean, std = S.subvol_mean_std(pics)
    assert np.array_equal(z["subvol"], S.to_uint8_normalize(pics, mean, std).cpu().numpy())


def test_tta_1_is_the_normalised_eval_mode_embedding(run):
    from cet_pick_amd import moco_test_3d as M
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.models.model import create_model
    out = M.test(_opt(["--exp_id", "t1", "--load_model", run["ckpt"], "--tta", "1"]))
    z = np.load(out)
    assert int(z["tta"]) == 1 and np.array_equal(z["coords"], run["z"]["coords"])
    rec, enc, c = _rec(run), run["enc"], z["coords"]
    with torch.no_grad():
        want = torch.cat([F.normalize(enc.forward_test(S.crop_znorm(rec, c[i:i + 256], (BBOX,) * 3))["proj"], dim=1)
                          for i in range(0, len(c), 256)])
        err = float((torch.as_tensor(z["proj"]).cuda() - want).abs().max())
        print("--tta 1 against F.normalize(forward_test(crop_znorm)): %.3e" % err)
        assert err <= POOL_ATOL
        # ... and that is eval mode: the batch statistics of a training-mode copy give another embedding
        k = min(len(c), 32)
        tr = M.load_encoder(create_model("moco3d_18", {"proj": 256, "pred": 256}, -1), run["ckpt"]).cuda().train()
        other = F.normalize(tr.forward_test(S.crop_znorm(rec, c[:k], (BBOX,) * 3))["proj"], dim=1)
        diff = float((other - want[:k]).abs().max())
        print("training-mode copy differs by %.3e" % diff)
        assert diff > 100 * POOL_ATOL
    # the file of the default run pools eight poses: not the same rows
    assert float(np.abs(run["z"]["proj"] - z["proj"]).max()) > 100 * POOL_ATOL


CENTRES = np.array([[30, 30, 20], [40, 60, 18], [66, 40, 22], [70, 64, 20], [62, 24, 16], [24, 70, 24], [51, 47, 21]], np.int32)


def test_pose_pooled_embedding_is_invariant_under_a_quarter_turn(run):
    from cet_pick_amd import moco_test_3d as M
    from cet_pick_amd.datasets import subvols as S
    rec, enc = _rec(run), run["enc"]
    d, h, w = rec.shape
    turned = torch.rot90(rec, 1, dims=(1, 2)).contiguous()
    # turned[z, i, j] = rec[z, j, W - 1 - i]: x' = y, and the even window [c - s/2, c + s/2) of x maps onto [W - c - s/2, W - c + s/2)
    moved = np.stack([CENTRES[:, 1], w - CENTRES[:, 0], CENTRES[:, 2]], 1).astype(np.int32)
    size = (BBOX,) * 3
    raw0, raw1 = S.extract_subvols_3d(rec, CENTRES, size), S.extract_subvols_3d(turned, moved, size)
    assert torch.equal(raw1, torch.rot90(raw0, 1, dims=(-2, -1))), "the windows are not images of each other"
    p0, p1 = S.crop_znorm_poses(rec, CENTRES, size, range(8)), S.crop_znorm_poses(turned, moved, size, range(8))
    # (same voxels, summed in another order: mean and deviation agree to a unit of float32, the values to a few 1e-6)
    assert float((p1[:, 0] - p0[:, 1]).abs().max()) <= 1e-5
    with torch.no_grad():
        # what the forward pass itself moves when nothing but a crop's place in the batch changes
        batch = p0.reshape(-1, 1, *size).clone()
        x = batch[5].clone()
        a = batch.clone(); a[0] = x
        b = batch.clone(); b[37] = x
        ya = F.normalize(enc.forward_test(a)["proj"], dim=1)[0]
        yb = F.normalize(enc.forward_test(b)["proj"], dim=1)[37]
        moves = float((ya - yb).abs().max())
        tol = 8 * moves if moves > 0 else POOL_ATOL
        print("one crop at batch positions 0 and 37: %.3e -> tolerance %.3e" % (moves, tol))
        e8, f8 = M.embed_picks(enc, rec, CENTRES, BBOX, tta=8), M.embed_picks(enc, turned, moved, BBOX, tta=8)
        assert tuple(e8.shape) == (len(CENTRES), 128)
        assert float((e8.norm(dim=1) - 1).abs().max()) <= POOL_ATOL
        d8 = (e8 - f8).abs().amax(1)
        e1, f1 = M.embed_picks(enc, rec, CENTRES, BBOX, tta=1), M.embed_picks(enc, turned, moved, BBOX, tta=1)
        d1 = (e1 - f1).abs().amax(1)
        print("turned tomogram: --tta 8 %.3e, --tta 1 %.3e" % (float(d8.max()), float(d1.max())))
        assert float(d8.max()) <= tol
        assert float(d1.max()) > tol, "the encoder is invariant without pooling: this test shows nothing"
        # batches of three picks are the three calls on their shares
        parts = torch.cat([M.embed_picks(enc, rec, CENTRES[i:i + 3], BBOX, tta=8) for i in (0, 3, 6)])
        assert float((M.embed_picks(enc, rec, CENTRES, BBOX, tta=8, batch=3) - parts).abs().max()) <= tol


def test_checkpoint_forms(run, tmp_path):
    from cet_pick_amd import moco_test_3d as M
    from cet_pick_amd.models.model import create_model, save_model
    new = lambda: create_model("moco3d_18", {"proj": 256, "pred": 256}, -1)
    bare = str(tmp_path / "encoder.pth")
    save_model(bare, 0, run["wrapper"].encoder_q)
    enc = M.load_encoder(new(), bare).cuda().eval()
    rec = _rec(run)
    sd = run["enc"].state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in enc.state_dict().items()) and set(sd) == set(enc.state_dict())
    with torch.no_grad():
        same = (M.embed_picks(enc, rec, CENTRES, BBOX, tta=2) - M.embed_picks(run["enc"], rec, CENTRES, BBOX, tta=2)).abs().max()
        assert float(same) <= POOL_ATOL
    # the query encoder's weights, not the key encoder's
    assert torch.equal(sd["conv1.weight"].cpu(), run["wrapper"].encoder_q.state_dict()["conv1.weight"].cpu())
    assert not torch.equal(sd["conv1.weight"].cpu(), run["wrapper"].encoder_k.state_dict()["conv1.weight"].cpu())
    foreign = str(tmp_path / "foreign.pth")
    torch.save({"epoch": 1, "state_dict": {"backbone.stem.weight": torch.zeros(2), "head.bias": torch.zeros(2)}}, foreign)
    with pytest.raises(ValueError, match="backbone.stem.weight"):
        M.load_encoder(new(), foreign)
    with pytest.raises(ValueError):
        M.test(_opt(["--exp_id", "tf", "--load_model", foreign]))
