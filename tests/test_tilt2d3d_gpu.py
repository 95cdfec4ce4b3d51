"""The 2d3d exploration mode on the GPU: the tilt-patch kernel (csrc/tilt_patch.hip) against the reference fixture
tests/golden/tilt2d3d.npz and the numpy restatement of tests/test_oracle_tilt2d3d.py, the 2d3d datasets against the
reference's `load_data`, simsiam_main / simsiam_test_hm_2d3d on MRC files and on the synthetic twin, and the captured step
of simsiam2d3d_18 against the eager one."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_oracle_tilt2d3d import FIXTURE_B, b_tags, fixture_a_stack, ref_extract_patches

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _kernel(tilts, angles, zfull, centres, b):
    from cet_pick_amd.datasets import subvols as S
    t = torch.as_tensor(np.ascontiguousarray(tilts, dtype=np.float32)).cuda()
    p, v = S.tilt_patches(t, angles, zfull, np.asarray(centres, dtype=np.int32).reshape(-1, 3), b, b)
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy()


def test_kernel_equals_reference_fixture_a(golden):
    from cet_pick_amd.datasets import subvols as S
    g = golden("tilt2d3d.npz")
    vol, used, ang = fixture_a_stack()
    rec = torch.as_tensor(vol).cuda()
    for b in (16, 36):
        p, v = _kernel(used, ang, vol.shape[0], g["a_centres"], b)
        assert np.array_equal(v, g["a_valid_%d" % b])
        np.testing.assert_allclose(p[v], g["a_patch_%d" % b][v], rtol=0, atol=2e-6)
        assert not p[~v].any()
        ok = g["a_tomo_ok_%d" % b]
        t3 = S.extract_3d_tomo(rec, g["a_centres"], b, b).cpu().numpy()
        np.testing.assert_allclose(t3[ok], g["a_tomo_%d" % b][ok], rtol=0, atol=2e-6)


@pytest.mark.parametrize("cfg", FIXTURE_B)
def test_dataset_equals_reference_load_data(golden, cfg):
    from cet_pick_amd.datasets.simsiam2d3d import ArraySimSiam2D3DDataset
    from cet_pick_amd.synthetic import make_tilt_series, tilt2d3d_inputs
    g = golden("tilt2d3d.npz")
    vol, vol_c, tilts, angles = tilt2d3d_inputs()
    if cfg.startswith("s10_"):                                 # (b2): one tilt inside [-20, 20]
        angles = np.array([-30.0, 10.0, 30.0])
        tilts = make_tilt_series(vol, angles)
    compress, b = cfg.endswith(("c1_16", "c1_36")), int(cfg.rsplit("_", 1)[1])
    opt = SimpleNamespace(compress=compress, batch_size=2, seed=3)
    items = [("syn", tilts, vol_c if compress else vol, angles)]
    for split, tag in zip(("test", "train"), b_tags(cfg)):
        ds = ArraySimSiam2D3DDataset(opt, split, (3, b, b), items, sigma1=[2.5, 5], border_z=10)
        assert np.array_equal(np.asarray(ds.coords, dtype=np.int32).reshape(-1, 3), g["b_coords_" + tag]), tag
        assert list(ds.names_all) == list(g["b_names_" + tag])
        np.testing.assert_allclose([ds.mean_subvols, ds.std_subvols, ds.mean_subvols3d, ds.std_subvols3d], g["b_stats_" + tag],
                                   rtol=0, atol=2e-6)
        sv = ds.set_valid.cpu().numpy()
        assert np.array_equal(sv.sum(1), g["b_len_" + tag]) and sv[:, 0].all()
        # the sets flattened in the reference's order: the valid variants of each kept pick, variant order
        p2, p3 = ds.patches_2d.cpu().numpy(), ds.patches_3d.cpu().numpy()
        flat2 = [p2[i, v] for i in range(len(sv)) for v in np.nonzero(sv[i])[0]]
        flat3 = [p3[i, v] for i in range(len(sv)) for v in np.nonzero(sv[i])[0]]
        np.testing.assert_allclose([x.astype(np.float64).mean() for x in flat2], g["b_means_" + tag], rtol=0, atol=1e-6)
        np.testing.assert_allclose([x.astype(np.float64).mean() for x in flat3], g["b_means3d_" + tag], rtol=0, atol=1e-6)
        store = g["b_store_" + tag]
        got = [p2[i, v] for i in store for v in np.nonzero(sv[i])[0]]
        got3 = [p3[i, v] for i in store for v in np.nonzero(sv[i])[0]]
        if len(store):
            np.testing.assert_allclose(np.stack(got), g["b_sets_" + tag], rtol=0, atol=2e-6, err_msg=tag)
            np.testing.assert_allclose(np.stack(got3), g["b_sets3d_" + tag], rtol=0, atol=2e-6, err_msg=tag)
        # batches: the four tensors and nothing else, view 2 one of the pick's valid variants
        if split == "train":
            ds.set_epoch(2)
            batch = next(iter(ds))
            assert set(batch) == {"input", "input_3d", "input_aug", "input_aug_3d"}
            assert all(t.shape == (2, 1, b, b) and t.is_cuda for t in batch.values())
            order, var = ds.epoch_views()
            assert (var >= 1).all() and sv[np.arange(len(var)), var].all()


def test_kernel_equals_numpy_restatement_on_random_inputs():
    rng = np.random.default_rng(11)
    T, H, W, Z, b = 13, 300, 280, 120, 36
    tilts = rng.random((T, H, W), dtype=np.float32)
    angles = np.sort(rng.uniform(-20, 20, T))
    n = 3000
    picks = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, Z, n)], 1)
    cents = (picks[:, None, :] + np.array([(0, 0, 0), (0, 0, 1), (0, 0, -1), (-1, 0, -1), (0, 1, -1)])[None]).reshape(-1, 3)
    p, v = _kernel(tilts, angles, Z, cents, b)
    n_valid = 0
    for i, c in enumerate(cents):
        r = ref_extract_patches(tilts, c, angles, [W, H, Z], b)
        assert (r is not None) == bool(v[i]), (i, c)
        if r is not None:
            n_valid += 1
            np.testing.assert_allclose(p[i, 0], r, rtol=0, atol=2e-6, err_msg=str(c))
    assert 0.3 * len(cents) < n_valid < len(cents)
    # edge cases: one tilt, no tilt, every tilt out of bounds, no centre
    p1, v1 = _kernel(tilts[:1], angles[:1], Z, cents[:200], b)
    for i, c in enumerate(cents[:200]):
        r = ref_extract_patches(tilts[:1], c, angles[:1], [W, H, Z], b)
        assert (r is not None) == bool(v1[i])
        if r is not None:
            np.testing.assert_allclose(p1[i, 0], r, rtol=0, atol=2e-6)
    p0, v0 = _kernel(tilts[:0], angles[:0], Z, cents[:50], b)
    assert not v0.any() and not p0.any()
    far = np.array([[-5000, 100, 10], [100, -40, 10], [100, H + 3, 10], [W * 40, 150, 60]])
    pf, vf = _kernel(tilts, angles, Z, far, b)
    assert not vf.any() and not pf.any()
    pe, ve = _kernel(tilts, angles, Z, np.zeros((0, 3), np.int32), b)
    assert pe.shape == (0, 1, b, b) and ve.shape == (0,)


def _write_2d3d_files(tmp_path, n=2, shape=(40, 128, 128)):
    """Tomograms (stored 'xzy' as the 2d3d loader reads them), tilt series (stored 'zxy'), .tlt files and the 4-column list."""
    from cet_pick_amd.synthetic import make_tilt_series, make_tomo
    from cet_pick_amd.utils import mrc
    data = tmp_path / "data"
    data.mkdir()
    angles = np.arange(-60, 61, 3).astype(np.float64)
    lines = ["image_name\trec_path\ttilt_path\tangle_path"]
    for i in range(n):
        vol, _ = make_tomo(shape, seed=700 + i, margin_xy=24, margin_z=12)
        name = "tomo%d" % i
        mrc.write(str(data / (name + ".rec")), np.ascontiguousarray(vol.transpose(1, 0, 2)))
        mrc.write(str(data / (name + "_tilt.mrc")), make_tilt_series(vol, angles))
        np.savetxt(str(data / (name + ".tlt")), angles, fmt="%.2f")
        lines.append("%s\t%s.rec\t%s_tilt.mrc\t%s.tlt" % (name, name, name, name))
    (data / "train_images.txt").write_text("\n".join(lines) + "\n")
    (data / "test_images.txt").write_text("\n".join(lines) + "\n")


def test_simsiam_main_2d3d_and_exploration_on_mrc_files(tmp_path, monkeypatch):
    from cet_pick_amd import simsiam_main, simsiam_test_hm_2d3d
    from cet_pick_amd.opts import opts
    monkeypatch.chdir(tmp_path)
    _write_2d3d_files(tmp_path)
    common = ["simsiam2d3d", "--arch", "simsiam2d3d_18", "--dataset", "simsiam2d3d", "--bbox", "36", "--exp_id", "f",
              "--debug", "0", "--dog", "2.5,5"]
    opt = opts().parse(common + ["--batch_size", "8", "--num_epochs", "1", "--lr", "0.01"])
    assert opt.hipgraph
    simsiam_main.main(opt)
    save_dir = os.path.join(str(tmp_path), "exp", "simsiam2d3d", "f")
    line = open(os.path.join(save_dir, "log.txt")).read()
    assert line.startswith("epoch: 1 |loss ") and "cosine_loss" in line
    assert np.isfinite(float(line.split("|")[1].split()[1]))
    out = simsiam_test_hm_2d3d.test(opts().parse(common + ["--load_model", os.path.join(save_dir, "model_last_contrastive.pth")]))
    z = np.load(out)
    assert set(z.files) == {"proj", "pred", "name", "coords", "subvol", "subvols_2d"}
    n = z["proj"].shape[0]
    assert n > 8 and z["proj"].shape == (n, 128) and z["pred"].shape == (n, 128)
    assert z["coords"].shape == (n, 3) and set(np.unique(z["name"])) <= {"tomo0", "tomo1"}
    assert z["subvol"].shape == (n, 1, 36, 36) and z["subvols_2d"].shape == (n, 1, 36, 36)
    assert np.isfinite(z["proj"]).all() and float(np.std(z["proj"], axis=0).mean()) > 0
    for k in ("subvol", "subvols_2d"):                      # 8-bit round trip + Normalize: 256 levels at most per patch
        for i in (0, n - 1):
            assert len(np.unique(z[k][i])) <= 256
    c = z["coords"]                                         # the border rule of :189 (36 // 1.8 = 19)
    assert (c[:, 0] > 19).all() and (c[:, 0] < 128 - 19).all() and (c[:, 1] >= 19).all() and (c[:, 1] <= 128 - 19).all()


def test_simsiam_main_2d3d_trains_on_the_synthetic_twin(tmp_path, monkeypatch):
    from cet_pick_amd import simsiam_main
    from cet_pick_amd.opts import opts
    monkeypatch.chdir(tmp_path)
    simsiam_main.main(opts().parse(["simsiam2d3d", "--arch", "simsiam2d3d_18", "--dataset", "simsiam2d3d", "--bbox", "24",
                                    "--batch_size", "8", "--num_epochs", "1", "--num_iters", "5", "--lr", "0.01",
                                    "--exp_id", "syn", "--debug", "0"]))
    line = open(os.path.join(str(tmp_path), "exp", "simsiam2d3d", "syn", "log.txt")).read()
    assert line.startswith("epoch: 1 |loss ") and np.isfinite(float(line.split("|")[1].split()[1]))


def _trainer_2d3d(seed, hipgraph):
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.synthetic import seeded_state_dict
    from cet_pick_amd.trains.train_factory import train_factory
    net = create_model("simsiam2d3d_18", {"proj": 128, "pred": 128}, 128)
    net.load_state_dict(seeded_state_dict(net, seed=seed))
    opt = SimpleNamespace(task="simsiam2d3d", num_iters=-1, print_iter=0, hide_data_time=True, exp_id="t", lr=0.05,
                          hipgraph=hipgraph)
    tr = train_factory["simsiam2d3d"](opt, net, torch.optim.SGD(net.parameters(), lr=0.05))
    tr.set_device([0], None, "cuda")
    return net, tr


def test_graph_engine_equals_eager_engine_for_simsiam2d3d():
    """The captured (hipGraph-replayed) SimSiam step of simsiam2d3d_18 against the same engine run eagerly: weights, losses and
    BatchNorm buffers bit for bit after every one of 6 steps (steps 3.. are replays)."""
    net_g, tr_g = _trainer_2d3d(322, hipgraph=True)
    net_e, tr_e = _trainer_2d3d(322, hipgraph=False)
    assert tr_g.engine is not None and tr_g.engine.use_graph and not tr_e.engine.use_graph
    gen = torch.Generator().manual_seed(5)
    for it in range(6):
        batch = {k: torch.randn(16, 1, 36, 36, generator=gen).cuda() for k in ("input", "input_3d", "input_aug", "input_aug_3d")}
        lg = tr_g.engine.step_batch(batch)
        le = tr_e.engine.step_batch(batch)
        assert torch.equal(lg, le), (it, float(lg), float(le))
        assert torch.equal(tr_g.engine.arena.flat, tr_e.engine.arena.flat), it
        for (n1, b1), (_, b2) in zip(net_g.named_buffers(), net_e.named_buffers()):
            assert torch.equal(b1, b2), (it, n1)
    assert tr_g.engine._graph is not None and tr_e.engine._graph is None
    tr_g.close()
    tr_e.close()
