"""Random 3-D views of the MoCo training on the GPU (csrc/augment3d.hip, datasets/augment.py) against the float64 numpy
restatement (tests/augment3d_ref.py), the parameter records' distributions, the guards, the loaders and the entry point."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment3d_ref as R3

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65536
KS = math.sqrt(math.log(2e6) / (2 * N))              # Kolmogorov-Smirnov critical value at 1e-6


def _ids(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _band(p):
    return 5 * math.sqrt(p * (1 - p) / N)


def _ks_uniform(x, lo, hi):
    u = np.sort((np.asarray(x, np.float64) - lo) / (hi - lo))
    n = len(u)
    return max(float((np.arange(1, n + 1) / n - u).max()), float((u - np.arange(n) / n).max()))


# ---- 1. the chain against the restatement --------------------------------------------------------------------------------
def _tomograms(c):
    """two tomograms with three different extents each, just large enough for the S^3 box"""
    _, S, _, _ = R3.geometry(c)
    shapes = [(24, 40, 48), (26, 44, 38)] if S <= 24 else [(S + 2, S + 4, S + 8), (S + 6, S + 3, S + 4)]
    vols = []
    for i, sh in enumerate(shapes):
        g = np.random.default_rng(100 * c + i)
        z, y, x = np.meshgrid(*(np.arange(n) for n in sh), indexing="ij")
        vols.append((0.5 + 0.2 * np.sin(0.5 * z + 0.2 * y) * np.cos(0.3 * x) + 0.15 * g.normal(size=sh)).astype(np.float32))
    return vols


def _table_of(c):
    """CropTable of six samples over both tomograms: sample 0's box touches the low corner of tomogram 0, sample 1's the high
    corner of tomogram 1"""
    from cet_pick_amd.datasets import subvols as S
    _, Sb, _, _ = R3.geometry(c)
    vols = _tomograms(c)
    h = Sb // 2
    d0, d1 = vols[0].shape, vols[1].shape
    cen = [(h, h, h), (d1[2] - h, d1[1] - h, d1[0] - h), (h + 1, h + 2, h + 1), (d1[2] - h - 1, h + 1, d1[0] - h - 2),
           (d0[2] - h - 3, d0[1] - h - 1, h), (h + 2, d1[1] - h - 2, h + 1)]
    owner = [0, 1, 0, 1, 0, 1]
    table = S.CropTable([torch.as_tensor(v).cuda() for v in vols], np.array(owner, np.int32), np.array(cen, np.int32))
    return table, vols, np.array(cen), owner


def _box_of(vols, cen, owner, s, c):
    _, Sb, _, _ = R3.geometry(c)
    x, y, z = (int(v) - Sb // 2 for v in cen[s])
    b = vols[owner[s]][z:z + Sb, y:y + Sb, x:x + Sb]
    assert b.shape == (Sb, Sb, Sb)
    return b


def _cases(c):
    """(name, record, sample, exact): one step at a time, then all together"""
    cs = R3.corner_set(c)
    _, _, e, _ = R3.geometry(c)
    far, near = (cs[-1], cs[0], cs[-2]), ((cs[1],) * 3 if e > 1 else (cs[1], cs[2], cs[1]))     # near: overlaps box (0, 0, 0) when e > 1
    r = R3.record
    return [
        ("all off", r(c), 2, True),
        ("flip z", r(c, flip=R3.FLIP_Z), 3, True),
        ("flip y", r(c, flip=R3.FLIP_Y), 4, True),
        ("drop_out", r(c, erase=R3.DROP, box0=far), 5, True),
        ("center_out", r(c, erase=R3.CENTRE), 0, True),
        ("swap_out overlapping", r(c, erase=R3.SWAP, box0=(cs[0],) * 3, box1=near), 1, True),
        ("flip z + swap_out", r(c, flip=R3.FLIP_Z, erase=R3.SWAP, box0=far, box1=(cs[0], cs[1], cs[0])), 2, True),
        ("blur radius 4, 2, 0", r(c, blur=(0.9, 0.5, 0.1)), 3, False),
        ("noise", r(c, noise=0.2, key=(7, 9)), 4, False),
        ("rotation 0", r(c, angle=0.0), 5, False),
        ("rotation 60", r(c, angle=60.0), 2, False),
        ("rotation 37.5", r(c, angle=37.5), 3, False),
        ("all, flip z, swap_out", r(c, blur=(0.3, 0.95, 0.6), noise=0.25, angle=22.25, flip=R3.FLIP_Z, erase=R3.SWAP,
                                     box0=(cs[0],) * 3, box1=near, key=(11, 13)), 4, False),
        ("all, flip y, drop_out, low corner", r(c, blur=(1.0, 0.2, 0.8), noise=0.1, angle=60.0, flip=R3.FLIP_Y, erase=R3.DROP,
                                                 box0=far, key=(17, 19)), 0, False),
        ("all, center_out, high corner", r(c, blur=(0.5, 0.5, 0.99), noise=0.05, angle=48.0, erase=R3.CENTRE, key=(23, 29)), 1, False),
        ("blur + noise", r(c, blur=(0.95, 0.95, 0.95), noise=0.15, key=(31, 37)), 5, False),
    ]


@pytest.mark.parametrize("c", [8, 16, 32])
def test_chain_matches_the_float64_restatement(c):
    """Cases that move no value (flip only, erasure only) are bit-exact against the ZNORM_RESCALE_ZNORM cut of the same centre,
    flipped / erased on the host.  The others: max |device - float64 restatement| <= 8 x max |float32 restatement - float64
    restatement| of that case, with a floor of 16 ulp of the largest output magnitude; rotated cases may leave out voxels whose
    source coordinate lies within 1e-3 of the box boundary (at most 0.5 % of the case)."""
    from cet_pick_amd.datasets import augment as A
    from cet_pick_amd.datasets import subvols as S
    table, vols, cen, owner = _table_of(c)
    cases = _cases(c)
    assert len(cases) <= 16
    ids = [s for _, _, s, _ in cases]
    got = A.apply_3d(table, _ids(ids), torch.as_tensor(R3.pack([r for _, r, _, _ in cases])).cuda(), c)
    assert tuple(got.shape) == (len(cases), 1, c, c, c)
    worst = 0.0
    for t, (name, r, s, exact) in enumerate(cases):
        g = got[t, 0]
        if exact:
            cut = S.crop_znorm_rescale_znorm(table.vols[owner[s]], cen[s:s + 1], (c, c, c))[0, 0].cpu().numpy()
            want = R3.flip_erase(cut, c, r["flip"], r["erase"], r["box0"], r["box1"])
            assert np.array_equal(g.cpu().numpy(), want), (c, name)
        box = _box_of(vols, cen, owner, s, c)
        w64, mask = R3.chain(box, c, r)
        w32, _ = R3.chain(box, c, r, np.float32)
        share = float(mask.mean())
        assert share <= 0.005, (c, name, share)
        keep = ~mask
        err = float(np.abs(g.cpu().numpy().astype(np.float64) - w64)[keep].max())
        yard = float(np.abs(w32.astype(np.float64) - w64)[keep].max())
        floor = 16 * float(np.spacing(np.float32(np.abs(w64).max())))
        bound = max(8 * yard, floor)
        ratio = err / max(yard, floor / 8)
        worst = max(worst, ratio)
        print("c %2d %-36s err %.3e  f32 restatement %.3e  ratio %.2f  excluded %.4f %%" % (c, name, err, yard, ratio, 100 * share))
        assert err <= bound, (c, name, err, yard, floor)
    print("c %d: worst ratio %.2f (bound 8)" % (c, worst))


# ---- 2. parameters ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn():
    from cet_pick_amd.datasets import augment as A
    ids = np.arange(N, dtype=np.int64) * 3 + 11
    out = {}
    for c in (32, 8):
        t = A.draw_params_3d(_ids(ids), 317, 4, 1, c).cpu().numpy()
        out[c] = t
    return ids, out


@pytest.mark.parametrize("c", [32, 8])
def test_params_ranges_and_distributions(drawn, c):
    _, tables = drawn
    t = tables[c].view(np.uint32)
    f = t.view(np.float32)
    assert tuple(t.shape) == (N, 16)
    assert not (t[:, 0] & ~np.uint32(0x337)).any()
    blur, noise, rot = (t[:, 0] & 1) > 0, (t[:, 0] & 2) > 0, (t[:, 0] & 4) > 0
    flip, erase = (t[:, 0] >> 4) & 3, (t[:, 0] >> 8) & 3
    for name, hit, p in (("blur", blur, 0.15), ("noise", noise, 0.5), ("rotation", rot, 0.75), ("flip z", flip == 1, 0.33),
                         ("flip y", flip == 2, 0.34), ("drop_out", erase == 1, 0.25), ("center_out", erase == 2, 0.25),
                         ("swap_out", erase == 3, 0.25)):
        assert abs(hit.mean() - p) <= _band(p), (name, hit.mean())
    assert (flip <= 2).all()
    for k in (1, 2, 3):
        assert (f[:, k] >= 0).all() and (f[:, k] < 1).all() and _ks_uniform(f[:, k], 0.0, 1.0) < KS
    assert (f[:, 4] >= 0).all() and (f[:, 4] < 0.25).all() and _ks_uniform(f[:, 4], 0.0, 0.25) < KS
    assert (f[:, 5] >= 0).all() and (f[:, 5] < 60).all() and _ks_uniform(f[:, 5], 0.0, 60.0) < KS
    th = f[:, 5].astype(np.float64) * (np.pi / 180)
    assert np.abs(f[:, 6] - np.cos(th)).max() <= 6e-8 and np.abs(f[:, 7] - np.sin(th)).max() <= 6e-8
    cs = np.array(R3.corner_set(c))
    n_set = len(cs)
    for k in range(8, 14):
        col = t[:, k].astype(np.int64)
        assert np.isin(col, cs).all(), k
        for v in cs:
            assert abs((col == v).mean() - 1.0 / n_set) <= _band(1.0 / n_set), (k, v)
    for a in range(3):
        assert (t[:, 8 + a] != t[:, 11 + a]).all()
    # the draws are independent of each other
    u = np.stack([blur, noise, rot, flip == 1, erase == 1, f[:, 1], f[:, 4], f[:, 5], t[:, 8], t[:, 12], t[:, 14] / 2.0 ** 32],
                 1).astype(np.float64)
    corr = np.corrcoef(u.T)
    off = np.abs(corr - np.eye(len(corr))).max()
    assert off < 5 / math.sqrt(N), off


def test_params_equal_the_host_restatement_and_depend_on_seed_epoch_sample_view_only(drawn):
    from cet_pick_amd.datasets import augment as A
    ids, tables = drawn
    n = 2048
    for c in (32, 8):
        want = R3.pack(R3.draw_records(ids[:n], 317, 4, 1, c)).view(np.uint32)
        got = tables[c][:n].view(np.uint32)
        same = [k for k in range(16) if k not in (6, 7)]
        assert np.array_equal(got[:, same], want[:, same])
        assert np.abs(got[:, 6:8].view(np.float32) - want[:, 6:8].view(np.float32)).max() <= 6e-8       # (float) cos, sin of fp64
    # purity: the same id gives the same record whatever its position or batch
    perm = np.random.default_rng(1).permutation(n)
    sub = A.draw_params_3d(_ids(ids[:n][perm][:100]), 317, 4, 1, 32).cpu().numpy()
    assert np.array_equal(sub, tables[32][:n][perm][:100])
    both = A._draw_3d(_ids(ids[:n]), 317, 4, 0, 2, 32, None).cpu().numpy()
    assert np.array_equal(both[1], tables[32][:n])
    base = tables[32][:n]
    for kw in (dict(seed=318), dict(epoch=5), dict(view=0)):
        a = dict(seed=317, epoch=4, view=1)
        a.update(kw)
        other = A.draw_params_3d(_ids(ids[:n]), a["seed"], a["epoch"], a["view"], 32).cpu().numpy()
        assert (other != base).any(1).mean() > 0.99, kw
    assert np.array_equal(both[0], A.draw_params_3d(_ids(ids[:n]), 317, 4, 0, 32).cpu().numpy())
    # forced on / off through the ranges
    off = dict(A.RANGES_3D, blur_p=0.0, noise_p=0.0, rot_p=0.0, flip=(0.0, 1.0), erase=(0.0, 0.0, 0.0))
    assert not (A.draw_params_3d(_ids(ids[:n]), 1, 0, 0, 32, off)[:, 0] != 0).any()
    on = dict(A.RANGES_3D, blur_p=1.0, noise_p=1.0, rot_p=1.0, flip=(1.0, 1.0), erase=(0.0, 0.0, 1.0))
    assert (A.draw_params_3d(_ids(ids[:n]), 1, 0, 0, 32, on)[:, 0] == (7 | (1 << 4) | (3 << 8))).all()


# ---- 3. permutation, guards, reproducibility ------------------------------------------------------------------------------------
def test_permutation_guards_and_reproducibility():
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    from cet_pick_amd.datasets import subvols as S
    c = 16
    table, vols, cen, owner = _table_of(c)
    # (the random corners of a drawn record are valid whatever sample they are applied to)
    ids = np.array([2, 3, 4, 5, 2, 3, 4, 5, 0, 1, 2, 3])
    on = dict(A.RANGES_3D, blur_p=1.0, noise_p=1.0, rot_p=1.0)
    rec = A.draw_params_3d(_ids(ids), 9, 2, 0, c, on)
    a = A.apply_3d(table, _ids(ids), rec, c)
    assert torch.isfinite(a).all() and torch.equal(a, A.apply_3d(table, _ids(ids), rec, c))
    perm = np.random.default_rng(2).permutation(len(ids))
    p = torch.as_tensor(perm).cuda()
    assert torch.equal(A.apply_3d(table, _ids(ids[perm]), rec[p].contiguous(), c), a[p])
    two = A.apply_3d(table, _ids(ids), torch.stack([rec, rec[p][torch.argsort(p)]]).contiguous(), c)
    assert tuple(two.shape) == (2, len(ids), 1, c, c, c) and torch.equal(two[0], a) and torch.equal(two[1], a)
    # an id outside the table: NaN rows, the others untouched
    bad = ids.copy()
    bad[[1, 7]] = [6, -1]
    b = A.apply_3d(table, _ids(bad), rec, c)
    assert torch.isnan(b[[1, 7]]).all() and torch.equal(b[[0, 2, 3, 4, 5, 6, 8, 9, 10, 11]], a[[0, 2, 3, 4, 5, 6, 8, 9, 10, 11]])
    with pytest.raises(_lib.HipExtensionError):
        A.apply_3d(table, torch.as_tensor(ids), rec, c)                          # host ids
    with pytest.raises(_lib.HipExtensionError):
        A.apply_3d(table, _ids(ids), rec.cpu(), c)                               # host table
    wide = torch.zeros((len(ids) * 16 + 1,), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.HipExtensionError):
        A.apply_3d(table, _ids(ids), wide[1:].view(len(ids), 16), c)             # misaligned table
    for odd in (15, 17):
        with pytest.raises((ValueError, _lib.HipExtensionError)):
            A.apply_3d(table, _ids(ids), rec, odd)
        with pytest.raises((ValueError, _lib.HipExtensionError)):
            A.draw_params_3d(_ids(ids), 9, 2, 0, odd)
    with pytest.raises(ValueError):                                              # a box that would leave its tomogram
        low = S.CropTable(table.vols, np.array(owner, np.int32), cen - np.array([1, 0, 0]))
        A.apply_3d(low, _ids(ids), rec, c)
    with pytest.raises(_lib.HipExtensionError):
        A.draw_params_3d(_ids(ids), 9, 2, 0, c, dict(A.RANGES_3D, sigma=(0.0, 1.5)))


# ---- 4. loaders -----------------------------------------------------------------------------------------------------------------
def _epoch(loader, epoch):
    loader.set_epoch(epoch)
    return [{k: v.clone() for k, v in b.items()} for b in loader]


def test_synthetic_loader_serves_reference_views():
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.datasets.synthetic_moco import SyntheticMocoLoader
    kw = dict(shape=(48, 96, 96), crop=16, n_crops=32, seed=21)
    ref = SyntheticMocoLoader(batch_size=8, augment="reference", **kw)
    e1 = _epoch(ref, 1)
    assert len(e1) == 4
    for b in e1:
        assert b["input"].shape == b["input_aug"].shape == (8, 1, 16, 16, 16)
        assert torch.isfinite(b["input"]).all() and torch.isfinite(b["input_aug"]).all()
        assert not torch.equal(b["input"], b["input_aug"])
    lo = ref.centres - 10
    assert (lo >= 0).all() and (lo[:, 0] + 20 <= 96).all() and (lo[:, 2] + 20 <= 48).all()
    again = _epoch(SyntheticMocoLoader(batch_size=8, augment="reference", **kw), 1)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(e1, again) for k in a)
    e2 = _epoch(ref, 2)
    assert not torch.equal(torch.cat([b["input"] for b in e1]), torch.cat([b["input"] for b in e2]))
    # a sample's views do not depend on the batch it is served in
    four = _epoch(SyntheticMocoLoader(batch_size=4, augment="reference", **kw), 1)
    for k in ("input", "input_aug"):
        assert torch.equal(torch.cat([b[k] for b in e1]), torch.cat([b[k] for b in four]))
    # mirror: the parent's batches, whatever the new argument's default
    mir = SyntheticMocoLoader(batch_size=8, augment="mirror", **kw)
    dflt = SyntheticMocoLoader(batch_size=8, **kw)
    assert np.array_equal(mir.centres, dflt.centres) and mir.augmenter is None
    order = np.random.default_rng(21 + 1000).permutation(32)
    for b, (bm, bd) in enumerate(zip(_epoch(mir, 1), _epoch(dflt, 1))):
        first = b * 8
        want = mir.table.cut(mir.table.epoch_order(order), first, 8, (16,) * 3)
        want_aug = mir.table.cut(mir.table.epoch_order(order), first, 8, (16,) * 3, shifted=True, flip_x=True)
        assert torch.equal(bm["input"], want) and torch.equal(bm["input_aug"], want_aug)
        assert torch.equal(bd["input"], want) and torch.equal(bd["input_aug"], want_aug)
        assert not torch.equal(bm["input"], e1[b]["input"])
    with pytest.raises(ValueError):
        SyntheticMocoLoader(batch_size=8, augment="torchio", **kw)


def test_file_loader_serves_reference_views_with_and_without_prefetch(tmp_path, monkeypatch):
    from test_entry_points_gpu import _write_listed_tomograms
    from cet_pick_amd.datasets import augment as A
    from cet_pick_amd.datasets.tomo_files import TomoFileMocoLoader
    from cet_pick_amd.opts import opts
    monkeypatch.chdir(tmp_path)
    _write_listed_tomograms(tmp_path)
    o = opts().parse(["moco", "--arch", "moco3d_18", "--dataset", "simsiam3d", "--order", "zxy", "--batch_size", "8",
                      "--exp_id", "a3", "--debug", "0", "--dog", "2.5,5", "--augment", "reference"])
    monkeypatch.setenv("CETPICK_LOADER_PREFETCH", "1")
    pre = TomoFileMocoLoader(o, crop=16, device="cuda", augment=o.augment)
    monkeypatch.setenv("CETPICK_LOADER_PREFETCH", "0")
    plain = TomoFileMocoLoader(o, crop=16, device="cuda", augment=o.augment)
    assert pre.prefetch and not plain.prefetch and len(set(pre.owner.tolist())) == 2 and len(pre) >= 2
    c = pre.centres
    assert (c >= 11).all() and (c[:, 0] < 176 - 11).all() and (c[:, 1] < 160 - 11).all() and (c[:, 2] < 48 - 11).all()
    ea, eb = _epoch(pre, 3), _epoch(plain, 3)
    assert len(ea) == len(eb) == len(pre)
    for a, b in zip(ea, eb):
        assert a["input"].shape == (8, 1, 16, 16, 16) and torch.isfinite(a["input"]).all() and torch.isfinite(a["input_aug"]).all()
        assert torch.equal(a["input"], b["input"]) and torch.equal(a["input_aug"], b["input_aug"])
    # what a batch holds: the two views of the epoch's order, drawn from (seed, epoch, sample id)
    idx = _ids(pre.epoch_order()[:8])
    x, x_aug = A.VolumeAugmenter(pre.table, 16, pre.seed).views(idx, 3)
    assert torch.equal(ea[0]["input"], x) and torch.equal(ea[0]["input_aug"], x_aug)
    # mirror keeps the parent's centres and batches
    mir = TomoFileMocoLoader(o, crop=16, device="cuda")
    mir.set_epoch(3)
    first = next(iter(mir))
    order = mir.table.epoch_order(mir.epoch_order())
    assert torch.equal(first["input"], mir.table.cut(order, 0, 8, (16,) * 3))
    assert torch.equal(first["input_aug"], mir.table.cut(order, 0, 8, (16,) * 3, shifted=True, flip_x=True))
    assert len(mir.centres) >= len(pre.centres) and (mir.centres >= 9).all()


# ---- 5. entry point -----------------------------------------------------------------------------------------------------------
def test_moco_main_with_reference_views(tmp_path):
    cmd = [sys.executable, "-m", "cet_pick_amd.moco_main", "moco", "--arch", "moco3d_18", "--dataset", "synthetic",
           "--augment", "reference", "--batch_size", "8", "--num_epochs", "1", "--exp_id", "aug3d", "--debug", "0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, "stdout tail: " + r.stdout[-800:] + "\nstderr tail: " + r.stderr[-3000:]
    lines = open(os.path.join(str(tmp_path), "exp", "moco", "aug3d", "log.txt")).read().strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("epoch: 1 |loss ")
    assert np.isfinite(float(lines[0].split("|")[1].split()[1]))
