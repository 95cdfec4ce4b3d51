"""View augmentation on the GPU (csrc/augment2d.hip through datasets/augment.py): the chain against the PIL fixture, the
parameter draw's distributions and its purity, the `--augment reference` dataset, the step engine on its batches and the
entry point."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("hflip", "vflip", "bright_first", "brightness", "contrast", "s", "i", "j", "k")
N = 65536
BAND = 5 * math.sqrt(0.25 / N)                       # 5-sigma binomial band at p = 0.5 (wider than at p = 0.25)
KS = math.sqrt(math.log(2e6) / (2 * N))              # Kolmogorov-Smirnov critical value at 1e-6


def _ids(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).cuda()


# ---- 1. apply vs fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bbox", [36, 32])
def test_apply_matches_the_pil_fixture(golden, bbox):
    """Class 0 (flips and rotation only) exact; class 1 (jitter, no resize) exact as well: the kernel's blends are the
    library's single-precision operations; with a resize every pixel within 1 grey level (the library interpolates in two
    passes with an 8-bit intermediate, the kernel in one).  Then Normalize: (grey / 255 - mean) / std to f32 rounding."""
    from cet_pick_amd.datasets import augment as A
    z = golden("augment2d.npz")
    r = {k: z["%s_%d" % (k, bbox)] for k in FIELDS + ("cls",)}
    bank = torch.as_tensor((z["crops_%d" % bbox].astype(np.float32) + 0.5) / 255.0).cuda()
    table = torch.as_tensor(R.pack_params(*[r[k] for k in FIELDS])).cuda()
    ids = _ids(np.arange(32))
    y = A.apply(bank, ids, table, 0.0, 1.0)
    assert y.shape == (32, 1, bbox, bbox) and y.dtype == torch.float32
    grey = np.round(255.0 * y[:, 0].cpu().numpy().astype(np.float64)).astype(np.int32)
    d = np.abs(grey - z["views_%d" % bbox].astype(np.int32)).reshape(32, -1).max(1)
    print("bbox %d: worst difference per class" % bbox, {c: int(d[r["cls"] == c].max()) for c in range(4)},
          "identical pixels %.4f" % float((grey == z["views_%d" % bbox]).mean()))
    assert d[r["cls"] < 2].max() == 0, d
    assert d.max() <= 1, d
    # a permuted batch reads the right crops and records
    perm = np.random.default_rng(1).permutation(32)
    y2 = A.apply(bank.unsqueeze(1), _ids(perm), table[torch.as_tensor(perm).cuda()].contiguous(), 0.0, 1.0)
    assert torch.equal(y2, y[torch.as_tensor(perm).cuda()])
    mean, std = 0.4382, 0.1719
    yn = A.apply(bank, ids, table, mean, std).cpu().numpy()
    want = (grey.astype(np.float32)[:, None] / np.float32(255) - np.float32(mean)) / np.float32(std)
    err = np.abs(yn.astype(np.float64) - want.astype(np.float64))
    print("normalised: worst relative difference %.3e" % float((err / np.maximum(np.abs(want), 1e-30)).max()))
    assert (err <= 1e-6 * np.abs(want)).all()


def test_apply_picks_the_neighbour_bank_and_guards_its_inputs(golden):
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    z = golden("augment2d.npz")
    base = torch.as_tensor((z["crops_36"].astype(np.float32) + 0.5) / 255.0).cuda()
    banks = torch.stack([base.roll(m, 0) for m in range(4)], 0).contiguous()          # bank m, sample n = crop n - m
    n = 32
    one = np.ones(n, np.float32)
    zero = np.zeros(n, np.int32)
    nbr = np.arange(n) % 4
    table = torch.as_tensor(R.pack_params(zero, zero, zero, one, one, zero + 36, zero, zero, zero, nbr)).cuda()
    y = A.apply(banks, _ids(np.arange(n)), table, 0.0, 1.0, neighbours=True)
    grey = np.round(255.0 * y[:, 0].cpu().numpy()).astype(np.int32)
    for t in range(n):
        assert np.array_equal(grey[t], z["crops_36"][(t - nbr[t]) % n]), t
    # a record whose window would leave the crop is clamped into it; a sample id outside the bank gives NaN, not a read
    bad = torch.as_tensor(R.pack_params(zero[:2], zero[:2], zero[:2], one[:2], one[:2], [99, 20], [50, 30], [-4, 30], [0, 0])).cuda()
    out = A.apply(base, _ids([0, 1]), bad, 0.0, 1.0)
    assert torch.isfinite(out).all()
    assert torch.isnan(A.apply(base, _ids([32, -1]), bad, 0.0, 1.0)).all()
    with pytest.raises(_lib.HipExtensionError):
        A.apply(base, _ids([0, 1]), torch.zeros(3, 8, dtype=torch.int32).cuda().view(-1)[2:18].view(2, 8), 0.0, 1.0)  # 8 bytes off
    with pytest.raises(_lib.HipExtensionError):
        A.apply(base.cpu(), _ids([0, 1]), bad, 0.0, 1.0)


# ---- 2. parameters -----------------------------------------------------------------------------------------------------
def _ks_uniform(x, lo, hi):
    u = np.sort((np.asarray(x, np.float64) - lo) / (hi - lo))
    n = len(u)
    return max(float((np.arange(1, n + 1) / n - u).max()), float((u - np.arange(n) / n).max()))


@pytest.mark.parametrize("view,bbox", [(0, 36), (1, 36), (0, 32), (1, 32)])
def test_params_ranges_and_distributions(view, bbox):
    from cet_pick_amd.datasets import augment as A
    ids = np.arange(N) * 3 + 11
    p = R.unpack_params(A.draw_params(_ids(ids), 317, 2, view, bbox).cpu().numpy())
    lo = 0.9 if view else 0.8
    s_min = int(round(bbox * math.sqrt(lo)))
    assert set(np.unique(p["hflip"])) | set(np.unique(p["vflip"])) | set(np.unique(p["bright_first"])) <= {0, 1}
    assert p["brightness"].min() >= 0.5 and p["brightness"].max() <= 1.5
    assert p["contrast"].min() >= np.float32(0.8) and p["contrast"].max() <= np.float32(1.2)
    assert p["s"].min() >= s_min and p["s"].max() <= bbox
    assert (p["i"] >= 0).all() and (p["j"] >= 0).all() and (p["i"] <= bbox - p["s"]).all() and (p["j"] <= bbox - p["s"]).all()
    assert set(np.unique(p["k"])) == {0, 1, 2, 3} == set(np.unique(p["neighbour"]))
    for f in ("hflip", "vflip", "bright_first"):
        assert abs(p[f].mean() - 0.5) <= BAND, (f, p[f].mean())
    band4 = 5 * math.sqrt(0.25 * 0.75 / N)
    for f in ("k", "neighbour"):
        for v in range(4):
            assert abs((p[f] == v).mean() - 0.25) <= band4, (f, v)
    assert _ks_uniform(p["brightness"], 0.5, 1.5) < KS
    assert _ks_uniform(p["contrast"], 0.8, 1.2) < KS
    # s: the integer histogram against the exact probabilities of round(bbox sqrt(u)), as a distance of distribution functions
    probs = R.side_probabilities(bbox, lo, 1.0)
    assert set(np.unique(p["s"])) <= set(probs)
    cdf_w, cdf_g, dist = 0.0, 0.0, 0.0
    for s in sorted(probs):
        cdf_w += probs[s]
        cdf_g += float((p["s"] == s).mean())
        dist = max(dist, abs(cdf_w - cdf_g))
    assert dist < KS, dist
    # i, j uniform on [0, bbox - s] given s: (i + 0.5) / (bbox - s + 1) has mean 1/2 and variance below 1/12
    for f in ("i", "j"):
        q = (p[f] + 0.5) / (bbox - p["s"] + 1)
        assert abs(q.mean() - 0.5) <= 5 * math.sqrt(1.0 / 12 / N), f
    cols = [p[f].astype(np.float64) for f in ("hflip", "vflip", "bright_first", "brightness", "contrast", "s", "k", "neighbour")]
    cols += [(p[f] + 0.5) / (bbox - p["s"] + 1) for f in ("i", "j")]
    c = np.corrcoef(np.stack(cols))
    off = np.abs(c - np.eye(len(cols))).max()
    print("view %d bbox %d: worst pairwise correlation %.4f (bound %.4f)" % (view, bbox, off, 5 / math.sqrt(N)))
    assert off < 5 / math.sqrt(N)


def test_params_equal_the_host_restatement():
    """The integer fields bit for bit, the jitter factors to the last bit but one (the device may fuse lo + (hi - lo) u),
    s except where bbox sqrt(u) falls within that rounding of a half."""
    from cet_pick_amd.datasets import augment as A
    ids = np.concatenate([np.arange(5000), 2 ** 33 + np.arange(5000) * 7919])
    for view, area in ((0, (0.8, 1.0)), (1, (0.9, 1.0))):
        got = R.unpack_params(A.draw_params(_ids(ids), 2 ** 40 + 317, 3, view, 36).cpu().numpy())
        want = R.draw_records(ids, 2 ** 40 + 317, 3, view, 36, area=area)
        for f in ("hflip", "vflip", "bright_first", "k", "neighbour"):
            assert np.array_equal(got[f], want[f]), f
        for f in ("brightness", "contrast"):
            assert np.abs(got[f] - want[f]).max() <= 2.4e-7, f
        same = got["s"] == want["s"]
        assert same.mean() > 0.999
        for f in ("i", "j"):
            assert np.array_equal(got[f][same], want[f][same]), f


# ---- 3. pure function of (seed, epoch, sample, view) ---------------------------------------------------------------------
def test_record_depends_on_seed_epoch_sample_view_only():
    from cet_pick_amd.datasets import augment as A
    draw = lambda ids, seed=317, epoch=0, view=0: A.draw_params(_ids(ids), seed, epoch, view, 36).cpu().numpy()
    alone = draw([1234])[0]
    big = np.arange(5000, 5256)
    big[7] = 1234
    small = np.array([9, 8, 1234, 7, 6, 5, 4, 3])
    assert np.array_equal(draw(big)[7], alone) and np.array_equal(draw(small)[2], alone)
    assert not np.array_equal(draw([1234], epoch=1)[0], alone)
    assert not np.array_equal(draw([1234], view=1)[0], alone)
    assert not np.array_equal(draw([1234], seed=318)[0], alone)
    assert np.array_equal(draw(big), draw(big))


# ---- 4. dataset ----------------------------------------------------------------------------------------------------------
def _opt(augment, batch_size=16):
    return SimpleNamespace(batch_size=batch_size, seed=317, augment=augment)


def _dataset(augment, rank=0, world=1, batch_size=16):
    from cet_pick_amd.datasets.synthetic_datasets import SyntheticSimSiamDataset
    return SyntheticSimSiamDataset(_opt(augment, batch_size), "train", (3, 36, 36), rank=rank, world=world)


def _epoch(ds, epoch):
    ds.set_epoch(epoch)
    return [{k: v.clone() for k, v in b.items()} for b in ds]


def test_reference_dataset_batches():
    ds = _dataset("reference")
    mirror = _dataset("mirror")
    assert mirror.augmenter is None and ds.augmenter is not None and ds.num_samples == mirror.num_samples
    assert tuple(ds.augmenter.neighbours.shape) == (4,) + tuple(ds.sub_vols_3d.shape)
    e0, e0b, e1, m0 = _epoch(ds, 0), _epoch(ds, 0), _epoch(ds, 1), _epoch(mirror, 0)
    assert len(e0) == len(ds) == len(m0) > 2
    for a, b, m in zip(e0, e0b, m0):
        assert set(a) == set(m) == {"input", "input_aug"}
        for k in a:
            assert a[k].shape == m[k].shape == (16, 1, 36, 36) and a[k].dtype == m[k].dtype == torch.float32
            assert a[k].is_contiguous() and torch.isfinite(a[k]).all()
            assert torch.equal(a[k], b[k])                                       # epoch 0 twice: bit-identical
        assert not torch.equal(a["input"], a["input_aug"])
    assert any(not torch.equal(a["input"], b["input"]) for a, b in zip(e0, e1))
    # views are 8-bit images, normalised with the anchor bank's statistics
    lv = torch.unique(torch.round((e0[0]["input"] * ds.std_subvols3d + ds.mean_subvols3d) * 255))
    assert len(lv) <= 256 and lv.min() >= 0 and lv.max() <= 255
    # mirror: normed[idx] and its flip, bit for bit, as before
    order = np.random.default_rng(317).permutation(mirror.num_samples)
    for i, m in enumerate(m0):
        x = mirror.normed[torch.as_tensor(order[i * 16:(i + 1) * 16]).cuda()]
        assert torch.equal(m["input"], x) and torch.equal(m["input_aug"], x.flip(-1))
    # the test split serves no random views
    from cet_pick_amd.datasets.synthetic_datasets import SyntheticSimSiamDataset
    assert SyntheticSimSiamDataset(_opt("reference"), "test", (3, 36, 36)).augmenter is None


def test_reference_dataset_rank_striding():
    """The rows two ranks serve are the rows of the one-rank epoch in rank-strided order, sample by sample."""
    one = _dataset("reference", batch_size=8)
    rows = {k: torch.cat([b[k] for b in _epoch(one, 3)], 0) for k in ("input", "input_aug")}
    # the one-rank epoch drops the tail of the permutation; rows by sample id instead of by position
    order = np.random.default_rng(317 + 3000).permutation(one.num_samples)
    pos = {int(s): t for t, s in enumerate(order[:rows["input"].shape[0]])}
    for rank in (0, 1):
        ds = _dataset("reference", rank=rank, world=2, batch_size=8)
        got = {k: torch.cat([b[k] for b in _epoch(ds, 3)], 0) for k in ("input", "input_aug")}
        mine = order[rank::2][:got["input"].shape[0]]
        keep = [t for t, s in enumerate(mine) if int(s) in pos]
        assert len(keep) > 16
        sel = torch.as_tensor([pos[int(mine[t])] for t in keep]).cuda()
        for k in got:
            assert torch.equal(got[k][torch.as_tensor(keep).cuda()], rows[k][sel]), (rank, k)


def test_file_dataset_neighbour_banks_and_views(tmp_path, monkeypatch):
    """TomoFileSimSiamDataset with --augment reference on two listed tomograms: the neighbour banks are the crops at
    (x, y, clip(z+1)), (x, y, clip(z-1)), (x-1, y, clip(z-1)), (x, y+1, clip(z-1)) of each pick's own tomogram, and an
    identity record through `apply` returns the 8-bit round trip of the picked neighbour's crop."""
    from test_entry_points_gpu import _write_listed_tomograms
    from cet_pick_amd.datasets import augment as A
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.datasets.tomo_files import TomoFileSimSiamDataset
    from cet_pick_amd.opts import opts
    monkeypatch.chdir(tmp_path)
    _write_listed_tomograms(tmp_path, shape=(40, 200, 200))
    opt = opts().parse(["simsiam3d", "--dataset", "simsiam3d", "--order", "zxy", "--bbox", "36", "--batch_size", "8", "--debug", "0",
                        "--dog", "2.5,5", "--augment", "reference"])
    ds = TomoFileSimSiamDataset(opt, "train", (3, 36, 36), sigma1=opt.dog)
    n = ds.num_samples
    assert len(set(ds.names_all)) == 2 and tuple(ds.augmenter.neighbours.shape) == (4, n, 1, 36, 36)
    for t in (0, n // 2, n - 1):
        x, y, z = (int(v) for v in ds.coords[t])
        d = ds.tomos[ds.names_all[t]].shape[0]
        up, down = min(max(z + 1, 1), d - 2), min(max(z - 1, 1), d - 2)
        cents = np.array([[x, y, up], [x, y, down], [x - 1, y, down], [x, y + 1, down]])
        want = S.extract_subvols(ds.tomos[ds.names_all[t]], cents, (3, 36, 36))
        assert torch.equal(ds.augmenter.neighbours[:, t], want), t
    ids = _ids(np.arange(n))
    one, zero = np.ones(n, np.float32), np.zeros(n, np.int32)
    table = torch.as_tensor(R.pack_params(zero, zero, zero, one, one, zero + 36, zero, zero, zero, np.arange(n) % 4)).cuda()
    got = A.apply(ds.augmenter.neighbours, ids, table, ds.mean_subvols3d, ds.std_subvols3d, neighbours=True)
    pick = ds.augmenter.neighbours[torch.as_tensor(np.arange(n) % 4).cuda(), torch.arange(n).cuda()]
    assert torch.equal(got, S.to_uint8_normalize(pick, ds.mean_subvols3d, ds.std_subvols3d))
    batch = next(iter(ds))
    assert batch["input"].shape == batch["input_aug"].shape == (8, 1, 36, 36) and torch.isfinite(batch["input_aug"]).all()
    assert TomoFileSimSiamDataset(opt, "test", (3, 36, 36), sigma1=opt.dog).augmenter is None


# ---- 5. engine -------------------------------------------------------------------------------------------------------------
def test_graph_engine_equals_eager_engine_on_reference_batches():
    from test_simsiam2d_gpu import _simsiam_trainer
    batches = _epoch(_dataset("reference"), 0)[:4]
    assert len(batches) == 4
    net_g, tr_g = _simsiam_trainer(321, hipgraph=True)
    net_e, tr_e = _simsiam_trainer(321, hipgraph=False)
    assert tr_g.engine.use_graph and not tr_e.engine.use_graph
    losses = []
    for b in batches:
        lg = tr_g.train_step(b["input"], b["input_aug"])
        le = tr_e.train_step(b["input"], b["input_aug"])
        assert torch.equal(lg, le)
        losses.append(float(lg))
    assert tr_g.engine._graph is not None
    assert torch.equal(tr_g.engine.arena.flat, tr_e.engine.arena.flat)
    assert all(np.isfinite(losses)) and len(set(losses)) == 4, losses
    tr_g.close()
    tr_e.close()


# ---- 6. entry point ----------------------------------------------------------------------------------------------------------
def test_simsiam_main_with_reference_views(tmp_path):
    cmd = [sys.executable, "-m", "cet_pick_amd.simsiam_main", "simsiam3d", "--arch", "simsiam2d_18", "--dataset", "synthetic",
           "--bbox", "36", "--batch_size", "32", "--num_epochs", "1", "--augment", "reference", "--exp_id", "aug", "--debug", "0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, "stdout tail: " + r.stdout[-800:] + "\nstderr tail: " + r.stderr[-3000:]
    save_dir = os.path.join(str(tmp_path), "exp", "simsiam3d", "aug")
    lines = open(os.path.join(save_dir, "log.txt")).read().strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("epoch: 1 |loss ")
    for key in ("cosine_loss", "output_std", "time"):
        assert key in lines[0]
    loss = float(lines[0].split("|")[1].split()[1])
    assert np.isfinite(loss) and -1.0 <= loss <= 0.0
    from cet_pick_amd.models.model import create_model, load_model
    model = load_model(create_model("simsiam2d_18", {"proj": 128, "pred": 128}, 128), os.path.join(save_dir, "model_last_contrastive.pth"))
    assert all(torch.isfinite(p).all() for p in model.parameters())
