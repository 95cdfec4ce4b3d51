"""The host half of the detector's file-backed data path (cet_pick_amd/datasets/semi_files.py) on the CPU: the label stencils
and a numpy restatement of the label volumes against the reference fixture tests/golden/semi_labels.npz, the coordinate table
reader, and the epoch sampler's rules (datasets/particle_moco.py:34-131)."""
import os

import numpy as np
import pytest

from cet_pick_amd.datasets import semi_files as SF

FIXTURE_TAGS = ["%s_f%d_c%d_%d" % (s, f, c, b) for s in ("train", "val") for f in (0, 1) for c in (0, 1) for b in (16, 36)]


def np_labels(shape, centres, stencil, fill_unlabeled):
    """numpy restatement of `mi_semi_labels`: zero, max-combine the stencil at every centre clipped by box intersection, and
    turn every exact 0 into -1 when asked."""
    D, H, W = shape
    hm = np.zeros(shape, np.float32)
    r = (stencil.shape[0] - 1) // 2
    for x, y, z in np.asarray(centres, dtype=np.int64).reshape(-1, 3):
        lo = [max(c - r, 0) for c in (z, y, x)]
        hi = [min(c + r + 1, e) for c, e in zip((z, y, x), (D, H, W))]
        if any(a >= b for a, b in zip(lo, hi)):
            continue
        win = tuple(slice(a, b) for a, b in zip(lo, hi))
        sw = tuple(slice(a - c + r, b - c + r) for a, b, c in zip(lo, hi, (z, y, x)))
        hm[win] = np.maximum(hm[win], stencil[sw])
    if fill_unlabeled:
        hm[hm == 0] = -1
    return hm


def write_fixture_table(g, path):
    with open(path, "w") as f:
        f.write("x_coord\timage_name\tscore\ty_coord\tz_coord\n")             # (any column order; extra columns ignored)
        for n, (x, y, z) in zip(g["coord_names"], g["coord_xyz"]):
            f.write("%s\t%s\t0.5\t%s\t%s\n" % (repr(float(x)), n, repr(float(y)), repr(float(z))))


def fixture_labels_inputs(g, tag, tmp_path):
    """(name, label shape, downscaled centres, stencil, fill) per listed tomogram of a fixture tag, through read_coord_list"""
    split, f, c, b = tag.split("_")
    path = os.path.join(str(tmp_path), "coords_%s.txt" % tag)
    write_fixture_table(g, path)
    names = [str(n) for n in g["tomo_names"]]
    coords = SF.read_coord_list(path, names)
    stencil = SF.label_stencil(SF.label_radius(int(b)), fiber=f == "f1")
    out = []
    for n, (D, H, W) in zip(names, g["tomo_shapes"]):
        out.append((n, (int(D), int(H) // 2, int(W) // 2), SF.downscale(coords[n], compress=c == "c1"), stencil, split == "train"))
    return out


@pytest.mark.parametrize("bbox", (12, 16, 36))
def test_host_stencils_equal_the_reference_bit_for_bit(golden, bbox):
    g = golden("semi_labels.npz")
    r = SF.label_radius(bbox)
    assert r == int(g["radius_%d" % bbox])
    for f in (0, 1):
        want = g["stencil_%d_f%d" % (bbox, f)].astype(np.float32)
        got = SF.label_stencil(r, fiber=bool(f))
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (bbox, f)
        assert (got >= 0).all() and got[r, r, r] == 1.0


@pytest.mark.parametrize("tag", FIXTURE_TAGS)
def test_numpy_labels_from_the_coordinate_file_equal_the_reference(golden, tag, tmp_path):
    g = golden("semi_labels.npz")
    anns = []
    for i, (n, shape, c, st, fill) in enumerate(fixture_labels_inputs(g, tag, tmp_path)):
        want = g["hm_%s_%s" % (tag, n)]
        got = np_labels(shape, c, st, fill)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, n)
        anns += [list(p) + [i] for p in c]
    assert np.array_equal(np.array(anns, np.int32).reshape(-1, 4), g["anns_" + tag])


def test_read_coord_list_truncates_drops_and_rejects(tmp_path, capsys):
    p = tmp_path / "c.txt"
    p.write_text("image_name\tx_coord\ty_coord\tz_coord\tclass\n"
                 "a\t10.9\t-3.7\t4.2\t1\nb\t1\t2\t3\t0\nzz\t5\t5\t5\t0\nyy\t1\t1\t1\t0\na\t-0.5\t7\t8.999\t1\n")
    got = SF.read_coord_list(str(p), ["a", "b", "c"])
    assert set(got) == {"a", "b", "c"}
    assert got["a"].dtype == np.int32 and got["a"].tolist() == [[10, -3, 4], [0, 7, 8]]      # toward zero, as astype(int32)
    assert got["b"].tolist() == [[1, 2, 3]] and got["c"].shape == (0, 3)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and " 2 coordinate rows" in out and str(p) in out
    assert SF.downscale(got["a"]).tolist() == [[5, -2, 4], [0, 3, 8]]                          # floor division
    assert SF.downscale(got["a"], compress=True).tolist() == [[5, -2, 2], [0, 3, 4]]

    s = tmp_path / "s.txt"
    s.write_text("source\timage_name\tx_coord\ty_coord\tz_coord\nm\ta\t1\t2\t3\n")
    with pytest.raises(ValueError, match="source"):
        SF.read_coord_list(str(s), ["a"])
    m = tmp_path / "m.txt"
    m.write_text("image_name\tx_coord\ty_coord\na\t1\t2\n")
    with pytest.raises(ValueError, match="z_coord") as e:
        SF.read_coord_list(str(m), ["a"])
    assert str(m) in str(e.value)
    with pytest.raises(FileNotFoundError, match="nothere.txt"):
        SF.read_coord_list(str(tmp_path / "nothere.txt"), ["a"])


def _anns(seed=3):
    """annotations of three tomograms of different sizes: interior ones, and ones on / past the faces"""
    shapes = np.array([(24, 200, 240), (40, 96, 128), (8, 80, 72)], np.int64)
    rng = np.random.default_rng(seed)
    rows = []
    for t, (D, H, W) in enumerate(shapes):
        n = 40
        rows.append(np.stack([rng.integers(-3, W // 2 + 3, n), rng.integers(-3, H // 2 + 3, n), rng.integers(-2, D + 2, n),
                              np.full(n, t)], 1))
    return np.concatenate(rows, 0), shapes


def test_sampler_obeys_the_reference_rules():
    anns, shapes = _anns()
    bbox, ratio = 16, 0.5
    tp = int(bbox * ratio)
    n = len(anns)
    lo = np.array([17, 17, 3])
    dx_own, dx_par, dz_par, near = [], [], [], []
    for epoch in range(40):
        owner, cen, flip, a, b = SF.draw_pairs(anns, shapes, bbox, ratio, seed=317, epoch=epoch, batch_size=1, return_index=True)
        assert len(a) == n and len(flip) == n and np.array_equal(np.sort(a), np.arange(n))
        assert (a != b).all() and ((b >= 0) & (b < n)).all()
        assert owner.dtype == np.int32 and cen.dtype == np.int32 and cen.shape == (2 * n, 3)
        assert np.array_equal(owner[0::2], anns[a, 3]) and np.array_equal(owner[1::2], anns[b, 3])     # own_0, partner_0, ...
        s = shapes[owner]
        hi = np.stack([s[:, 2] // 2 - 17, s[:, 1] // 2 - 17, s[:, 0] - 3], 1)
        assert ((cen >= lo) & (cen <= hi)).all()
        SF.check_windows(owner, cen, shapes)
        assert ((flip >= 0) & (flip < 1)).all()
        own, par = cen[0::2].astype(np.int64), cen[1::2].astype(np.int64)
        # the own centre: the annotation + x, y in [-4, 4], z unchanged - clipped (clip is monotone)
        so = shapes[anns[a, 3]]
        lo_o, hi_o = SF.clip_centres(anns[a, :3] - [4, 4, 0], so), SF.clip_centres(anns[a, :3] + [4, 4, 0], so)
        assert ((own >= lo_o) & (own <= hi_o)).all()
        assert np.array_equal(own[:, 2], SF.clip_centres(anns[a, :3], so)[:, 2])
        inner = (lo_o == anns[a, :3] - [4, 4, 0]) & (hi_o == anns[a, :3] + [4, 4, 0])               # (per axis: no clip)
        dx_own += list((own - anns[a, :3])[inner[:, 0], 0])
        # the partner: x, y in [-5, 5) (p <= 0.8) or [-tp, tp), z in [-2, 2)
        sp = shapes[anns[b, 3]]
        lo_p, hi_p = SF.clip_centres(anns[b, :3] - [tp, tp, 2], sp), SF.clip_centres(anns[b, :3] + [tp - 1, tp - 1, 1], sp)
        assert ((par >= lo_p) & (par <= hi_p)).all()
        free = (lo_p == anns[b, :3] - [tp, tp, 2]) & (hi_p == anns[b, :3] + [tp - 1, tp - 1, 1])      # (per axis: no clip)
        d = par - anns[b, :3]
        dx_par += list(d[free[:, 0], 0])
        dz_par += list(d[free[:, 2], 2])
        near += list(((d[:, :2] >= -5) & (d[:, :2] <= 4)).all(1)[free[:, 0] & free[:, 1]])
    assert sorted(set(dx_own)) == list(range(-4, 5))
    assert sorted(set(dx_par)) == list(range(-tp, tp))
    assert sorted(set(dz_par)) == [-2, -1, 0, 1]
    # near branch 0.8, plus the far branch's draws that land in [-5, 4]^2 (0.2 * (10/16)^2)
    assert abs(np.mean(near) - (0.8 + 0.2 * (10 / (2 * tp)) ** 2)) < 0.03


@pytest.mark.parametrize("world,batch", [(1, 1), (2, 4), (3, 16), (4, 3)])
def test_sampler_splits_ranks_like_distributed_sampler(world, batch):
    anns, shapes = _anns(seed=7)
    n = len(anns)
    per = n // world
    seen = []
    for rank in range(world):
        owner, cen, flip, a, b = SF.draw_pairs(anns, shapes, 36, 0.5, seed=5, epoch=2, rank=rank, world=world, batch_size=batch,
                                              return_index=True)
        assert len(a) == (per // batch) * batch and len(owner) == 2 * len(a) and len(flip) == per // batch
        seen.append(a)
    allv = np.concatenate(seen)
    assert len(set(allv.tolist())) == len(allv)                                   # disjoint shards
    # the same epoch draws the same table; another epoch another one
    again = SF.draw_pairs(anns, shapes, 36, 0.5, seed=5, epoch=2, rank=0, world=world, batch_size=batch)
    first = SF.draw_pairs(anns, shapes, 36, 0.5, seed=5, epoch=2, rank=0, world=world, batch_size=batch)
    other = SF.draw_pairs(anns, shapes, 36, 0.5, seed=5, epoch=3, rank=0, world=world, batch_size=batch)
    assert all(np.array_equal(x, y) for x, y in zip(again, first))
    assert not np.array_equal(first[1], other[1])


def test_sampler_and_windows_reject_what_cannot_be_cut():
    anns, shapes = _anns()
    with pytest.raises(ValueError, match="at least 2"):
        SF.draw_pairs(anns[:1], shapes, 16, 0.5, 1, 0)
    with pytest.raises(ValueError, match="translation"):
        SF.draw_pairs(anns, shapes, 1, 0.5, 1, 0)
    with pytest.raises(ValueError, match="leaves"):
        SF.check_windows(np.array([0], np.int32), np.array([[15, 40, 5]], np.int32), shapes)
    with pytest.raises(ValueError, match="leaves"):
        SF.check_windows(np.array([2], np.int32), np.array([[20, 20, 6]], np.int32), shapes)


def test_val_window_and_net_extent():
    wi, wl = SF.val_window((112, 528, 528))
    a = np.zeros((112, 528, 528), np.float32)[wi]
    h = np.zeros((112, 264, 264), np.float32)[wl]
    assert a.shape == (110, 328, 328) and h.shape == (110, 164, 164)
    assert (SF.net_hm_extent(a.shape[1]), SF.net_hm_extent(a.shape[2])) == h.shape[1:]
    wi, wl = SF.val_window((99, 600, 600))
    assert np.zeros((99, 600, 600))[wi].shape == (99, 600, 600)
    assert SF.net_hm_extent(65) == 33 and SF.net_hm_extent(64) == 32
