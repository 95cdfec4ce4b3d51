"""2d3d view augmentation on the GPU (csrc/augment2d3d.hip through datasets/augment.py): the chain against the PIL fixture,
the record draw's distributions, its agreement with the host restatement and its purity, the `--augment reference` 2d3d
dataset, the step engine on its batches and the entry point."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment2d3d_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65536
BAND = 5 * math.sqrt(0.25 / N)                       # 5-sigma binomial band at p = 0.5
BAND4 = 5 * math.sqrt(0.25 * 0.75 / N)               # ... at p = 0.25
KS = math.sqrt(math.log(2e6) / (2 * N))              # Kolmogorov-Smirnov critical value at 1e-6 (as test_augment_gpu.py)
KEYS = ("input", "input_3d", "input_aug", "input_aug_3d")


def _dev(a, dtype=np.int64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _fixture(z, bbox):
    """(banks (32, 2 variants, bbox, bbox) x 2 with variant 1 = the crops rolled by one sample, table (2, 32, 16), records)"""
    r = {k: z["%s_%d" % (k, bbox)] for k in R.FIELDS}
    crops = (z["crops_%d" % bbox].astype(np.float32) + 0.5) / 255.0
    banks = [torch.as_tensor(np.stack([crops[:, c], np.roll(crops[:, c], 1, 0)], 1)).cuda().contiguous() for c in (0, 1)]
    table = torch.as_tensor(R.pack_params(**r)).cuda()
    return banks, torch.stack([table, table.flip(0)], 0).contiguous(), r


def _levels(y):
    return np.round(255.0 * y.cpu().numpy().astype(np.float64)).astype(np.int32)


# ---- 1. apply vs fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bbox", [36, 12])
def test_apply_matches_the_pil_fixture(golden, bbox):
    """View 0 runs the fixture's record t on crop pair t (variant 0); view 1 runs record 31 - t on variant 1, which holds
    crop pair t - 1: every level of both channels equals PIL's, then Normalize to f32 rounding."""
    from cet_pick_amd.datasets import augment as A
    z = golden("augment2d3d.npz")
    (b2, b3), table, r = _fixture(z, bbox)
    views = z["views_%d" % bbox].astype(np.int32)
    ids, var = _dev(np.arange(32)), _dev(np.ones(32))
    y = A.apply_2d3d(b2, b3, ids, var, table, (0.0, 0.0), (1.0, 1.0))
    assert y.shape == (4, 32, 1, bbox, bbox) and y.dtype == torch.float32 and all(v.is_contiguous() for v in y.unbind(0))
    g = _levels(y[:, :, 0])
    bad = [int((g[c] != views[:, c]).sum()) for c in (0, 1)]
    print("bbox %d: pixels that differ from PIL, view 0: tilt %d, tomogram %d" % (bbox, bad[0], bad[1]))
    assert np.array_equal(g[0], views[:, 0]) and np.array_equal(g[1], views[:, 1])
    # view 1: record 31 - t on crop t - 1 (the host restatement equals PIL on the fixture: test_augment2d3d_cpu.py)
    crops = z["crops_%d" % bbox]
    want1 = np.stack([R.chain_levels(crops[(t - 1) % 32], *[r[k][31 - t] for k in R.FIELDS if k != "angle"]) for t in range(32)])
    assert np.array_equal(g[2], want1[:, 0]) and np.array_equal(g[3], want1[:, 1])
    # the 5-d banks of the dataset (n, V, 1, bbox, bbox) are taken as they are
    assert torch.equal(A.apply_2d3d(b2.unsqueeze(2), b3.unsqueeze(2), ids, var, table, (0.0, 0.0), (1.0, 1.0)), y)
    # a permuted batch gives permuted rows
    perm = np.random.default_rng(1).permutation(32)
    pt = torch.as_tensor(perm).cuda()
    y2 = A.apply_2d3d(b2, b3, _dev(perm), var, table[:, pt].contiguous(), (0.0, 0.0), (1.0, 1.0))
    assert torch.equal(y2, y[:, pt])
    # Normalize, per channel
    means, stds = (0.4382, 0.5127), (0.1719, 0.2203)
    yn = A.apply_2d3d(b2, b3, ids, var, table, means, stds)[:, :, 0].cpu().numpy()
    worst = 0.0
    for s in range(4):
        want = (g[s].astype(np.float32) / np.float32(255) - np.float32(means[s & 1])) / np.float32(stds[s & 1])
        err = np.abs(yn[s].astype(np.float64) - want.astype(np.float64))
        worst = max(worst, float((err / np.maximum(np.abs(want), 1e-30)).max()))
        assert (err <= 1e-6 * np.abs(want)).all(), s
    print("normalised: worst relative difference %.3e" % worst)


def test_apply_picks_the_variant_row_and_guards_its_inputs(golden):
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    z = golden("augment2d3d.npz")
    crops = z["crops_36"]
    n, V = 32, 5
    f = (crops.astype(np.float32) + 0.5) / 255.0
    b2, b3 = (torch.as_tensor(np.stack([np.roll(f[:, c], v, 0) for v in range(V)], 1)).cuda().contiguous() for c in (0, 1))
    ident = dict(hflip=np.zeros(n), vflip=np.zeros(n), erase=np.zeros(n), k=np.zeros(n), i=np.zeros(n), j=np.zeros(n),
                 h=np.zeros(n), w=np.zeros(n), angle=np.zeros(n, np.float32), coef=np.tile(np.array(R.IDENTITY), (n, 1)))
    t1 = torch.as_tensor(R.pack_params(**ident)).cuda()
    table = torch.stack([t1, t1], 0).contiguous()
    var = 1 + np.arange(n) % (V - 1)
    ids = _dev(np.arange(n))
    y = A.apply_2d3d(b2, b3, ids, _dev(var), table, (0.0, 0.0), (1.0, 1.0))
    g = _levels(y[:, :, 0])
    assert np.array_equal(g[0], crops[:, 0]) and np.array_equal(g[1], crops[:, 1])            # view 1: variant 0
    for t in range(n):                                                                       # view 2: variant var[t] = crop t - var[t]
        assert np.array_equal(g[2, t], crops[(t - var[t]) % n, 0]) and np.array_equal(g[3, t], crops[(t - var[t]) % n, 1]), t
    # records from a caller: whatever they hold, no read leaves the patch and the result is a level
    wild = dict(ident, erase=np.ones(n), i=np.linspace(-2 ** 31, 2 ** 31 - 1, n), j=np.arange(n) - 8, h=np.arange(n) * 2 ** 26 - 5,
                w=np.full(n, 2 ** 31 - 1), k=np.arange(n) * 977,
                coef=np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, (n, 6)))
    tw = torch.as_tensor(R.pack_params(**wild)).cuda()
    out = A.apply_2d3d(b2, b3, ids, _dev(var), torch.stack([tw, tw], 0).contiguous(), (0.0, 0.0), (1.0, 1.0))
    assert torch.isfinite(out).all() and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    # a sample id or a variant outside the banks gives NaN rows of that view, and no read
    bad_ids = ids.clone()
    bad_ids[3], bad_ids[4] = n, -1
    bad_var = _dev(var)
    bad_var[7], bad_var[8] = V, -1
    out = A.apply_2d3d(b2, b3, bad_ids, bad_var, table, (0.0, 0.0), (1.0, 1.0))
    nan_rows = torch.isnan(out).flatten(2).all(2).cpu().numpy()
    assert np.array_equal(np.isnan(out.cpu().numpy()).reshape(4, n, -1).any(2), nan_rows)
    want = np.zeros((4, n), bool)
    want[:, [3, 4]] = True
    want[2:, [7, 8]] = True
    assert np.array_equal(nan_rows, want)
    with pytest.raises(_lib.HipExtensionError):                                              # 8 bytes off
        A.apply_2d3d(b2, b3, ids, _dev(var), torch.zeros(2 * n * 16 + 4, dtype=torch.int32).cuda()[2:2 + 2 * n * 16].view(2, n, 16),
                     (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.HipExtensionError):
        A.apply_2d3d(b2.cpu(), b3, ids, _dev(var), table, (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.HipExtensionError):
        A.apply_2d3d(b2, b3, ids, _dev(var).int(), table, (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.HipExtensionError):
        A.apply_2d3d(b2, b3[:, :4].contiguous(), ids, _dev(var), table, (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.HipExtensionError):
        A.apply_2d3d(b2, b3, ids, _dev(var), table, (0.0, 0.0), (1.0, 0.0))                  # std 0


def test_params_refuse_what_the_chain_does_not_cover():
    """Ranges with which CornerErasing could reject its first try (h or w reaching bbox // 2), odd or out-of-range bbox."""
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    ids = _dev(np.arange(8))
    assert A.draw_params_2d3d(ids, 1, 0, 8).shape == (2, 8, 16) and A.draw_params_2d3d(ids, 1, 0, 128).shape == (2, 8, 16)
    for bbox in (6, 35, 130):
        with pytest.raises(_lib.HipExtensionError, match="unsupported"):
            A.draw_params_2d3d(ids, 1, 0, bbox)
    for bad in (dict(scale=(0.02, 0.33), ratio=(0.3, 3.3)),        # the class's defaults: h up to 1.04 bbox
                dict(scale=(0.01, 0.13)),                          # bbox 36: w = round(18.36) = mid
                dict(scale=(0.01, 0.1), ratio=(1.0, 2.6)),         # h = round(18.36) = mid
                dict(ratio=(0.07, 1.5)),                           # w = round(19.2)
                dict(erase_p=1.5), dict(angle=(30.0, -30.0)), dict(scale=(0.0, 0.02)), dict(flip_p=-0.1)):
        with pytest.raises(_lib.HipExtensionError, match="bad argument"):
            A.draw_params_2d3d(ids, 1, 0, 36, strong=dict(A.STRONG_RANGES_2D3D, **bad))
        with pytest.raises(_lib.HipExtensionError, match="bad argument"):
            A.draw_params_2d3d(ids, 1, 0, 36, weak=dict(A.WEAK_RANGES_2D3D, **bad))
    for good in (dict(scale=(0.01, 0.1)), dict(scale=(0.01, 0.1), ratio=(1.0, 2.3))):       # w = round(16.1); h = round(17.26)
        p = R.unpack_params(A.draw_params_2d3d(ids, 1, 0, 36, strong=dict(A.STRONG_RANGES_2D3D, **good)).cpu().numpy()[0])
        assert p["h"].max() < 18 and p["w"].max() < 18


# ---- 2. the record draw ------------------------------------------------------------------------------------------------
def _ks_uniform(x, lo, hi):
    u = np.sort((np.asarray(x, np.float64) - lo) / (hi - lo))
    n = len(u)
    return max(float((np.arange(1, n + 1) / n - u).max()), float((u - np.arange(n) / n).max()))


@pytest.mark.parametrize("bbox", [36, 12])
def test_params_ranges_and_distributions(bbox):
    from cet_pick_amd.datasets import augment as A
    ids = np.arange(N) * 3 + 11
    table = A.draw_params_2d3d(_dev(ids), 317, 2, bbox).cpu().numpy()
    mid = bbox // 2
    h_min, h_max, w_min, w_max = R.extent_bounds(bbox, R.STRONG)
    assert h_max < mid and w_max < mid
    for view in (0, 1):
        p = R.unpack_params(table[view])
        assert not p["reserved"].any() and not p["flag_rest"].any()
        for f in ("hflip", "vflip", "erase"):
            assert set(np.unique(p[f])) == {0, 1} and abs(p[f].mean() - 0.5) <= BAND, (view, f, p[f].mean())
        assert set(np.unique(p["k"])) == {0, 1, 2, 3}
        for v in range(4):
            assert abs((p["k"] == v).mean() - 0.25) <= BAND4, (view, v)
        # i, j, h, w inside the reference's ranges; the coins fair
        assert p["h"].min() >= h_min and p["h"].max() <= h_max and p["w"].min() >= w_min and p["w"].max() <= w_max
        cols = {f: p[f].astype(np.float64) for f in ("hflip", "vflip", "erase", "k", "h", "w")}
        for f, e in (("i", "h"), ("j", "w")):
            near = p[f] < mid + 6                                   # the near range ends at mid - 6 at the latest
            assert abs(near.mean() - 0.5) <= BAND, (view, f, near.mean())
            lo = np.where(near, 0, mid + 6)
            hi = np.where(near, np.maximum(1, mid - p[e] - 6), np.maximum(mid + 7, bbox - p[e] + 6))
            assert (p[f] >= lo).all() and (p[f] < hi).all(), (view, f)
            q = (p[f] - lo + 0.5) / (hi - lo)                       # uniform on its range given the side and the extent
            assert abs(q.mean() - 0.5) <= 5 * math.sqrt(1.0 / 12 / N), (view, f, q.mean())
            cols["near_" + f], cols["pos_" + f] = near.astype(np.float64), q
        if bbox == 36:                                              # (at bbox 12 the far range is one row, past the image)
            assert p["i"].max() >= bbox and (p["i"] + p["h"] > bbox).any() and (p["j"] + p["w"] <= mid).any()
        if view == 0:
            assert p["angle"].min() >= -30 and p["angle"].max() <= 30
            assert _ks_uniform(p["angle"], -30.0, 30.0) < KS
            cols["angle"] = p["angle"].astype(np.float64)
            # the coefficients are a rotation about the centre: a0 = a4, a1 = -a3 up to the rounding of FIX
            c = p["coef"].astype(np.int64)
            assert (np.abs(c[:, 0] - c[:, 4]) == 0).all() and (np.abs(c[:, 1] + c[:, 3]) <= 1).all()
            assert (c[:, 0] >= math.floor(65536 * math.cos(math.radians(30)))).all() and (c[:, 0] <= 65536).all()
        else:
            assert (p["angle"] == 0).all() and (p["coef"] == np.array(R.IDENTITY)).all()       # the identity matrix, exactly
        # pairwise correlations.  h and w are two functions of the same two draws (share, aspect) and correlate by
        # construction: that one pair is left out; a position is normalised to its range, so it carries no h or w.
        names = sorted(n for n in cols if cols[n].std() > 0)        # (bbox 12: pos_* of the one-row ranges are constant)
        cc = np.abs(np.corrcoef(np.stack([cols[n] for n in names])) - np.eye(len(names)))
        cc[names.index("h"), names.index("w")] = cc[names.index("w"), names.index("h")] = 0
        print("view %d bbox %d: worst pairwise correlation %.4f (bound %.4f)" % (view, bbox, cc.max(), 5 / math.sqrt(N)))
        assert cc.max() < 5 / math.sqrt(N), (view, names, cc.max())
    # the two views of a sample are drawn apart
    p0, p1 = R.unpack_params(table[0]), R.unpack_params(table[1])
    for f in ("hflip", "vflip", "erase"):
        assert abs((p0[f] == p1[f]).mean() - 0.5) <= BAND, f


# ---- 3. draw vs host restatement ---------------------------------------------------------------------------------------
def test_params_equal_the_host_restatement():
    """Flags, k and the angle bit for bit (the kernel does not contract lo + (hi - lo) u); h, w except where the device's
    single-precision exp / sqrt put them across a rounding boundary; i, j wherever h, w agree; the coefficients against the
    host formula on the angle the device reports."""
    from cet_pick_amd.datasets import augment as A
    ids = np.concatenate([np.arange(5000), 2 ** 33 + np.arange(5000) * 7919])
    seed = 2 ** 40 + 317
    for bbox in (36, 12):
        table = A.draw_params_2d3d(_dev(ids), seed, 3, bbox).cpu().numpy()
        for view in (0, 1):
            got, want = R.unpack_params(table[view]), R.draw_records(ids, seed, 3, view, bbox)
            for f in ("hflip", "vflip", "erase", "k"):
                assert np.array_equal(got[f], want[f]), (bbox, view, f)
            assert np.array_equal(got["angle"].view(np.int32), want["angle"].view(np.int32)), (bbox, view)
            same_h, same_w = got["h"] == want["h"], got["w"] == want["w"]
            print("bbox %d view %d: h equal %.5f, w equal %.5f" % (bbox, view, same_h.mean(), same_w.mean()))
            assert same_h.mean() > 0.999 and same_w.mean() > 0.999
            assert np.array_equal(got["i"][same_h], want["i"][same_h]) and np.array_equal(got["j"][same_w], want["j"][same_w])
            allowed = 0
            for t in range(len(ids)):
                v = R.fix_arguments(got["angle"][t], bbox)
                fixed = [int(math.floor(x * 65536.0 + 0.5)) for x in v]
                if list(got["coef"][t]) == fixed:
                    continue
                for c in range(6):
                    x = v[c] * 65536.0 + 0.5
                    assert got["coef"][t, c] == fixed[c] or (abs(int(got["coef"][t, c]) - fixed[c]) == 1 and abs(x - round(x)) <= 1e-6), \
                        (bbox, view, t, c, int(got["coef"][t, c]), fixed[c], x)
                allowed += 1
            print("bbox %d view %d: records that use the +-1 allowance: %d of %d" % (bbox, view, allowed, len(ids)))
            assert allowed <= len(ids) // 1000


# ---- 4. pure function of (seed, epoch, sample, view) -----------------------------------------------------------------------
def test_record_depends_on_seed_epoch_sample_view_only():
    from cet_pick_amd.datasets import augment as A
    draw = lambda ids, seed=317, epoch=0: A.draw_params_2d3d(_dev(ids), seed, epoch, 36).cpu().numpy()
    alone = draw([1234])[:, 0]
    big = np.arange(5000, 5256)
    big[7] = 1234
    small = np.array([9, 8, 1234, 7, 6, 5, 4, 3])
    assert np.array_equal(draw(big)[:, 7], alone) and np.array_equal(draw(small)[:, 2], alone)
    assert not np.array_equal(draw([1234], epoch=1)[0, 0], alone[0]) and not np.array_equal(draw([1234], epoch=1)[1, 0], alone[1])
    assert not np.array_equal(draw([1234], seed=318)[0, 0], alone[0]) and not np.array_equal(draw([1234], seed=318)[1, 0], alone[1])
    # another view: the weak record under the strong ranges is still not the strong record
    both_strong = A.draw_params_2d3d(_dev([1234]), 317, 0, 36, weak=A.STRONG_RANGES_2D3D).cpu().numpy()
    assert np.array_equal(both_strong[0, 0], alone[0]) and not np.array_equal(both_strong[1, 0], alone[0])
    assert np.array_equal(draw(big), draw(big))
    # and apart from the 2-D chain's stream: the flips of 4,096 samples agree with mi_aug2d_params's about half the time
    ids = _dev(np.arange(4096))
    f2 = A.draw_params(ids, 317, 0, 0, 36).cpu().numpy()[:, 0] & 1
    f23 = A.draw_params_2d3d(ids, 317, 0, 36).cpu().numpy()[0, :, 0] & 1
    assert abs((f2 == f23).mean() - 0.5) <= 5 * math.sqrt(0.25 / 4096)


# ---- 5. dataset ----------------------------------------------------------------------------------------------------------
def _dataset(augment, split="train", rank=0, world=1, batch_size=8):
    from cet_pick_amd.datasets.simsiam2d3d import SyntheticSimSiam2D3DDataset
    opt = SimpleNamespace(batch_size=batch_size, seed=317, compress=False)
    if augment is not None:
        opt.augment = augment
    return SyntheticSimSiam2D3DDataset(opt, split, (3, 36, 36), rank=rank, world=world)


def _epoch(ds, epoch):
    ds.set_epoch(epoch)
    return [{k: v.clone() for k, v in b.items()} for b in ds]


@pytest.fixture(scope="module")
def reference_dataset():
    return _dataset("reference")


def test_reference_dataset_batches(reference_dataset):
    ds = reference_dataset
    plain, unset = _dataset("mirror"), _dataset(None)
    assert ds.augmenter is not None and plain.augmenter is None and unset.augmenter is None
    assert _dataset("reference", split="test").augmenter is None
    assert ds.num_samples == plain.num_samples and ds.augmenter.patches_2d.shape == (ds.num_samples, 5, 36, 36)
    assert ds.augmenter.patches_2d.data_ptr() == ds.patches_2d.data_ptr()                  # the banks are not copied
    e0, e0b, e1, m0 = _epoch(ds, 0), _epoch(ds, 0), _epoch(ds, 1), _epoch(plain, 0)
    print("2d3d synthetic dataset: %d samples, %d batches of 8" % (ds.num_samples, len(e0)))
    assert len(e0) == len(ds) == len(m0) >= 2
    for a, b, m in zip(e0, e0b, m0):
        assert set(a) == set(m) == set(KEYS)
        for k in KEYS:
            assert a[k].shape == m[k].shape == (8, 1, 36, 36) and a[k].dtype == m[k].dtype == torch.float32
            assert a[k].is_contiguous() and torch.isfinite(a[k]).all()
            assert torch.equal(a[k], b[k])                                                 # epoch 0 twice: bit-identical
        assert not torch.equal(a["input"], m["input"]) and not torch.equal(a["input_aug"], m["input_aug"])
    assert any(not torch.equal(a["input"], b["input"]) for a, b in zip(e0, e1))
    # views are 8-bit images, each channel normalised with its own statistics
    for k, (mean, std) in zip(KEYS, [(ds.mean_subvols, ds.std_subvols), (ds.mean_subvols3d, ds.std_subvols3d)] * 2):
        lv = (e0[0][k].double() * std + mean) * 255
        assert float((lv - lv.round()).abs().max()) < 1e-3 and lv.round().min() >= 0 and lv.round().max() <= 255
    # one record acts on both channels: the erased rectangles (level 255 in both) and the fill coincide wherever they occur
    x = ((e0[0]["input"].double() * ds.std_subvols + ds.mean_subvols) * 255).round()
    x3 = ((e0[0]["input_3d"].double() * ds.std_subvols3d + ds.mean_subvols3d) * 255).round()
    rec = R.unpack_params(_first_table(ds, 0))
    for t in range(8):
        if rec["erase"][t]:
            i0, i1, j0, j1 = R.clip_rect(rec["i"][t], rec["j"][t], rec["h"][t], rec["w"][t], 36)
            box = torch.zeros(36, 36, dtype=torch.bool)
            box[i0:i1, j0:j1] = True
            box = torch.rot90(box, int(rec["k"][t]), dims=[0, 1]).cuda()
            assert (x[t, 0][box] == 255).all() and (x3[t, 0][box] == 255).all(), t
    # without the flag: normed_*[idx, variant], bit for bit, as before
    for dsp in (plain, unset):
        dsp.set_epoch(0)
        order, var = dsp.epoch_views()
        for i, m in enumerate(_epoch(dsp, 0)):
            idx = torch.as_tensor(order[i * 8:(i + 1) * 8]).cuda()
            v = torch.as_tensor(var).cuda()[idx]
            assert torch.equal(m["input"], dsp.normed_2d[idx, 0]) and torch.equal(m["input_3d"], dsp.normed_3d[idx, 0])
            assert torch.equal(m["input_aug"], dsp.normed_2d[idx, v]) and torch.equal(m["input_aug_3d"], dsp.normed_3d[idx, v])
    # the reference batches are `views` of the epoch's order and variant draw
    ds.set_epoch(0)
    order, var = ds.epoch_views()
    idx = torch.as_tensor(order[:8]).cuda()
    four = ds.augmenter.views(idx, torch.as_tensor(var).cuda()[idx], 0)
    assert all(torch.equal(four[s], e0[0][k]) for s, k in enumerate(KEYS))


def _first_table(ds, epoch):
    """the strong records of the epoch's first batch"""
    from cet_pick_amd.datasets import augment as A
    ds.set_epoch(epoch)
    order, _ = ds.epoch_views()
    return A.draw_params_2d3d(_dev(order[:ds.batch_size]), ds.seed, epoch, 36).cpu().numpy()[0]


def test_reference_dataset_rank_striding(reference_dataset):
    """The rows two ranks serve are the rows of the one-rank epoch in rank-strided order, sample by sample."""
    one = reference_dataset
    rows = {k: torch.cat([b[k] for b in _epoch(one, 3)], 0) for k in KEYS}
    order = np.random.default_rng(317 + 3000).permutation(one.num_samples)
    pos = {int(s): t for t, s in enumerate(order[:rows["input"].shape[0]])}
    for rank in (0, 1):
        ds = _dataset("reference", rank=rank, world=2)
        got = {k: torch.cat([b[k] for b in _epoch(ds, 3)], 0) for k in KEYS}
        mine = order[rank::2][:got["input"].shape[0]]
        keep = [t for t, s in enumerate(mine) if int(s) in pos]
        assert len(keep) > 16
        sel = torch.as_tensor([pos[int(mine[t])] for t in keep]).cuda()
        for k in KEYS:
            assert torch.equal(got[k][torch.as_tensor(keep).cuda()], rows[k][sel]), (rank, k)


# ---- 6. engine -------------------------------------------------------------------------------------------------------------
def test_graph_engine_equals_eager_engine_on_reference_batches(reference_dataset):
    from test_tilt2d3d_gpu import _trainer_2d3d
    batches = (_epoch(reference_dataset, 0) + _epoch(reference_dataset, 1) + _epoch(reference_dataset, 2))[:4]
    assert len(batches) == 4
    net_g, tr_g = _trainer_2d3d(323, hipgraph=True)
    net_e, tr_e = _trainer_2d3d(323, hipgraph=False)
    assert tr_g.engine.use_graph and not tr_e.engine.use_graph
    losses = []
    for b in batches:
        lg = tr_g.engine.step_batch(b)
        le = tr_e.engine.step_batch(b)
        assert torch.equal(lg, le)
        losses.append(float(lg))
    assert tr_g.engine._graph is not None
    assert torch.equal(tr_g.engine.arena.flat, tr_e.engine.arena.flat)
    assert all(np.isfinite(losses)) and len(set(losses)) == 4, losses
    tr_g.close()
    tr_e.close()


# ---- 7. entry point ----------------------------------------------------------------------------------------------------------
def test_simsiam_main_2d3d_with_reference_views(tmp_path):
    cmd = [sys.executable, "-m", "cet_pick_amd.simsiam_main", "simsiam2d3d", "--arch", "simsiam2d3d_18", "--dataset", "simsiam2d3d",
           "--bbox", "24", "--batch_size", "8", "--num_epochs", "1", "--num_iters", "5", "--lr", "0.01", "--exp_id", "syn",
           "--debug", "0", "--augment", "reference"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, "stdout tail: " + r.stdout[-800:] + "\nstderr tail: " + r.stderr[-3000:]
    save_dir = os.path.join(str(tmp_path), "exp", "simsiam2d3d", "syn")
    lines = open(os.path.join(save_dir, "log.txt")).read().strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("epoch: 1 |loss ")
    loss = float(lines[0].split("|")[1].split()[1])
    assert np.isfinite(loss) and -1.0 <= loss <= 0.0
    from cet_pick_amd.models.model import create_model, load_model
    model = load_model(create_model("simsiam2d3d_18", {"proj": 128, "pred": 128}, 128),
                       os.path.join(save_dir, "model_last_contrastive.pth"))
    assert all(torch.isfinite(p).all() for p in model.parameters())
