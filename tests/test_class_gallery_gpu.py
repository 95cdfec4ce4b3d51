"""csrc/class_gallery.hip through the wrappers of hipops against the float64 restatements of tests/gallery_ref.py, and
plot_2d --class_gallery end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gallery_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 256                                # members per partial sum (GAL_CHUNK of the kernel file): the boundary the counts cross
assert CHUNK == R.CHUNK


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_moments(g):
    from cet_pick_amd import hipops as H
    mean, std, count = H.gallery_moments(dev(g["patches"]), dev(g["labels"]), g["k"])
    return mean.cpu().numpy(), std.cpu().numpy(), count.cpu().numpy()


def check_moments(g, name):
    """Counts exact.  Mean within 2^-23 max|x| of the float64 value.  Deviation within

        2^-24 sigma + 2^-40 (sigma + max|x|) + 2^-149

    of the float64 value sigma, which follows from the two-pass form.  With u = 2^-53 and N <= 3100 members: the float64 mean m
    differs from the true mean mu by e, |e| <= N u max|x|.  sum (x_i - m)^2 = sum (x_i - mu)^2 + N e^2 exactly (the cross term
    is zero), and the N differences, squares and additions of the second pass put a relative error of at most (N + 3) u on it, so
    the computed variance is V (1 + t) + e^2 with |t| <= (N + 3) u < 2^-41; its root, rounded once more, differs from sigma by at
    most sigma 2^-41 + |e| <= 2^-41 sigma + 2^-41 max|x|.  The result is then rounded to float32: half a unit in the last place,
    2^-24 sigma, or 2^-149 among the denormals.  The restatement's own float64 error is of the size of the 2^-41 terms, which is
    why the middle term carries 2^-40.  Nothing here grows with the mean, so a constant added to every patch costs only its share
    of max|x| 2^-40: E[x^2] - mean^2 would lose mean^2 2^-53 / sigma instead."""
    mean, std, count = run_moments(g)
    want_mean, want_std, want_count = R.moments(g["patches"], g["labels"], g["k"])
    assert mean.dtype == std.dtype == np.float32 and count.dtype == np.int32
    assert np.array_equal(count, want_count) and mean.shape == std.shape == want_mean.shape
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    top = float(np.abs(g["patches"]).max())
    err_mean = np.abs(mean.astype(np.float64) - want_mean)
    bound_std = 2.0 ** -24 * want_std + 2.0 ** -40 * (want_std + top) + 2.0 ** -149
    err_std = np.abs(std.astype(np.float64) - want_std)
    print("moments %s: mean error / bound %.3f, std error / bound %.3f" % (name, err_mean.max() / (2.0 ** -23 * top),
                                                                           (err_std / bound_std).max()))
    assert err_mean.max() <= 2.0 ** -23 * top
    assert (err_std <= bound_std).all()
    for c in np.flatnonzero(want_count == 0):
        assert not mean[c].any() and not std[c].any()
    return mean, std, count


MOMENT_CASES = {
    # n = 37: class 1 empty, class 2 a single member
    "base": dict(counts=[9, 0, 1, 20, 7], h=6, w=6),
    "odd": dict(counts=[9, 0, 1, 20, 7], h=5, w=7),
    "pixel": dict(counts=[9, 0, 1, 20, 7], h=1, w=1),
    "offset": dict(counts=[9, 0, 1, 20, 7], h=6, w=6, offset=1e4),
    # n = 3100, one class of 3000: 12 partial sums, the last one of 184 members
    "large": dict(counts=[60, 3000, 0, 40], h=6, w=6),
    "large_offset": dict(counts=[60, 3000, 0, 40], h=5, w=7, offset=1e4),
    "chunk": dict(counts=[CHUNK - 1, CHUNK, 0, CHUNK + 1, 2 * CHUNK], h=3, w=5),
}


@pytest.mark.parametrize("name", sorted(MOMENT_CASES))
def test_moments(name):
    g = R.case(seed=11, **MOMENT_CASES[name])
    assert name not in ("base", "odd", "pixel", "offset") or len(g["labels"]) == 37
    assert name != "large" or len(g["labels"]) == 3100
    mean, std, count = check_moments(g, name)
    single = g["patches"][g["labels"] == 2]
    if len(single) == 1:
        assert np.array_equal(mean[2], single[0]) and not std[2].any()
    again = run_moments(g)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((mean, std, count), again))         # two calls, the same bytes


def test_moments_of_permuted_picks():
    """A permutation changes the order of a class's members and with it the order of every float64 sum, so the last bits of the
    sums may move and, rarely, the float32 they round to: for general patches only the bounds are asserted.  Where every sum is
    exact the order cannot matter: patches of integers below 2^12, at most 3000 of them, add up below 2^24 without any rounding,
    and the mean is then one correctly rounded division and one rounding to float32 of the same two integers - equal bytes.  The
    deviation adds squares of differences from a rounded mean, which are not exact, so it keeps the bound alone."""
    g = R.case([60, 3000, 0, 40], 4, 4, seed=12)
    perm = np.random.RandomState(13).permutation(len(g["labels"]))
    p = dict(g, patches=g["patches"][perm], labels=g["labels"][perm])
    check_moments(g, "unpermuted")
    check_moments(p, "permuted")
    whole = dict(g, patches=np.rint(g["patches"] * 100).astype(np.float32))
    assert np.abs(whole["patches"]).max() < 2 ** 12
    mean, _, count = check_moments(whole, "integers")
    mean_p, _, count_p = check_moments(dict(whole, patches=whole["patches"][perm], labels=g["labels"][perm]), "integers permuted")
    assert mean.tobytes() == mean_p.tobytes() and count.tobytes() == count_p.tobytes()


def exemplar_case(dim):
    """700 picks.  Class 0: 400 members (two tiles of 256) on the centroids 0 and 1 - a merged class; class 1: 5 members, fewer than
    m = 8 or 64; class 2: empty; class 3: the rest on the centroids 2..5.  In class 0, four members on either side of the tile
    boundary share one embedding next to their centroid, and two more share another: ties among the very best."""
    rs = np.random.RandomState(21 + dim)
    labels = rs.permutation(np.repeat([0, 1, 3], [400, 5, 295])).astype(np.int32)
    centroids = (rs.standard_normal((6, dim)) * 4).astype(np.float32)
    assign = np.where(labels == 0, rs.randint(0, 2, 700), np.where(labels == 1, 1, rs.randint(2, 6, 700))).astype(np.int32)
    emb = (centroids[assign] + rs.standard_normal((700, dim))).astype(np.float32)
    first = np.flatnonzero(labels == 0)
    a = first[[3, 100, 300, 399]]
    assign[a] = 0
    emb[a] = centroids[0] + np.float32(0.01)
    b = first[[250, 260]]
    assign[b] = 1
    emb[b] = centroids[1] - np.float32(0.02)
    return emb, centroids, assign, labels


@pytest.mark.parametrize("m", [1, 8, 64])
@pytest.mark.parametrize("dim", [3, 64, 128])
def test_exemplars(dim, m):
    from cet_pick_amd import hipops as H
    emb, centroids, assign, labels = exemplar_case(dim)
    want_idx, want_d2 = R.exemplars(emb, centroids, assign, labels, 4, m)
    idx, d2 = H.gallery_exemplars(dev(emb), dev(centroids), dev(assign), dev(labels), 4, m)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and idx.shape == d2.shape == (4, m)
    assert np.array_equal(idx, want_idx)
    assert d2.tobytes() == want_d2.tobytes()                # bit-equal, the +inf padding included
    assert (idx[2] == -1).all() and np.isinf(d2[2]).all()   # the empty class
    assert (idx[1, 5:] == -1).all() and (idx[1, :5] >= 0).all()
    if m >= 8:
        first = np.flatnonzero(labels == 0)
        ties = set(first[[3, 100, 300, 399]].tolist()) | set(first[[250, 260]].tolist())
        assert ties <= set(idx[0].tolist())                 # the shared embeddings are among the best, and
        assert len(set(assign[idx[0, :8]].tolist())) == 2   # come from both centroids of the merged class
        for run in (first[[3, 100, 300, 399]], first[[250, 260]]):
            at = [idx[0].tolist().index(i) for i in run]
            assert at == list(range(at[0], at[0] + len(run))) and len(set(d2[0, at].tolist())) == 1         # by pick index
    again = H.gallery_exemplars(dev(emb), dev(centroids), dev(assign), dev(labels), 4, m)
    assert again[0].cpu().numpy().tobytes() == idx.tobytes() and again[1].cpu().numpy().tobytes() == d2.tobytes()


def run_raster(mean, std, count, idx, patches, m_show, scale):
    from cet_pick_amd import hipops as H
    rgb, order = H.gallery_raster(dev(mean), dev(std), dev(count), dev(idx), dev(patches), dev(R.DIGITS_5X7), m_show=m_show,
                                  scale=scale)
    return rgb.cpu().numpy(), order.cpu().numpy()


def test_raster():
    """3 classes of 4 x 4 patches, enlarged twice.  Classes 0 and 2 have equal counts (the lower class first), class 1 the most;
    the mean of class 2 and exemplar 0 of class 0 are constant patches; class 2 has one exemplar fewer than is shown."""
    rs = np.random.RandomState(31)
    patches = (rs.standard_normal((9, 4, 4)) * 5 + 2).astype(np.float32)
    patches[4] = -7.25
    mean = rs.standard_normal((3, 4, 4)).astype(np.float32)
    mean[2] = 3.5
    std = np.abs(rs.standard_normal((3, 4, 4))).astype(np.float32)
    count = np.array([4, 105, 4], np.int32)
    idx = np.array([[4, 0, 8], [1, 2, 3], [5, 6, -1]], np.int32)
    pic, order = run_raster(mean, std, count, idx, patches, 3, 2)
    assert order.tolist() == [1, 0, 2] == R.row_order(count).tolist()
    want = R.raster(mean, std, count, idx, patches, 3, 2)
    assert pic.shape == want.shape == (4 + 3 * 36, 102 + 5 * 12, 3) and pic.dtype == np.uint8
    assert np.array_equal(pic, want)
    assert (pic[4 + 72:4 + 80, 102:110] == 0).all()         # the constant mean of class 2, in the last row: 0 everywhere
    assert (pic[4 + 36:4 + 44, 126:134] == 0).all()         # the constant exemplar of class 0
    assert (pic[4 + 72:4 + 80, 150:158] == 255).all()       # no third exemplar in class 2
    # fewer exemplars shown than found, no enlargement, a deviation of zero everywhere, every count equal
    pic, order = run_raster(mean, np.zeros_like(std), np.full(3, 2, np.int32), idx, patches, 1, 1)
    assert order.tolist() == [0, 1, 2]
    assert np.array_equal(pic, R.raster(mean, np.zeros_like(std), np.full(3, 2, np.int32), idx, patches, 1, 1))
    pic, _ = run_raster(mean, std, count, idx, patches, 0, 3)
    assert np.array_equal(pic, R.raster(mean, std, count, idx, patches, 0, 3))


def test_raster_of_the_kernels_own_output():
    from cet_pick_amd import hipops as H
    g = R.case([9, 0, 1, 20, 7], 5, 7, seed=41)
    x, lab = dev(g["patches"]), dev(g["labels"])
    mean, std, count = H.gallery_moments(x, lab, 5)
    idx, _ = H.gallery_exemplars(dev(g["emb"]), dev(g["centroids"]), dev(g["assign"]), lab, 5, 4)
    rgb, order = H.gallery_raster(mean, std, count, idx, x, dev(R.DIGITS_5X7), scale=2)
    assert order.cpu().numpy().tolist() == [3, 0, 4, 2, 1]
    want = R.raster(mean.cpu().numpy(), std.cpu().numpy(), count.cpu().numpy(), idx.cpu().numpy(), g["patches"], 4, 2)
    assert np.array_equal(rgb.cpu().numpy(), want)


def test_bad_input_is_refused_before_any_launch(monkeypatch):
    import torch
    from cet_pick_amd import _lib as L
    from cet_pick_amd import hipops as H
    launched = []
    monkeypatch.setattr(L, "call", lambda name, *a, **k: launched.append(name))
    g = R.case([9, 0, 1, 20, 7], 6, 6, seed=51)
    x, lab, emb, cen, asg = (dev(g[key]) for key in ("patches", "labels", "emb", "centroids", "assign"))
    bad_label, bad_assign = lab.clone(), asg.clone()
    bad_label[5], bad_assign[7] = 5, 5
    low_label = lab.clone()
    low_label[0] = -1
    refused = [
        lambda: H.gallery_moments(x, bad_label, 5),
        lambda: H.gallery_moments(x, low_label, 5),
        lambda: H.gallery_exemplars(emb, cen, asg, bad_label, 5, 4),
        lambda: H.gallery_exemplars(emb, cen, bad_assign, lab, 5, 4),
        lambda: H.gallery_moments(x.transpose(1, 2), lab, 5),
        lambda: H.gallery_moments(x, torch.stack([lab, lab], 1)[:, 0], 5),
        lambda: H.gallery_exemplars(emb.t().contiguous().t(), cen, asg, lab, 5, 4),
        lambda: H.gallery_exemplars(emb, cen, torch.stack([asg, asg], 1)[:, 1], lab, 5, 4),
        lambda: H.gallery_exemplars(emb, cen, asg, lab, 5, 0),
        lambda: H.gallery_exemplars(emb, cen, asg, lab, 5, 65),
        lambda: H.gallery_moments(x[:0], lab[:0], 5),
        lambda: H.gallery_exemplars(emb[:0], cen, asg[:0], lab[:0], 5, 4),
    ]
    for k, f in enumerate(refused):
        with pytest.raises(ValueError):
            f()
        assert not launched, k
    assert L.lib().mi_gallery_workspace_bytes(37, 5, 36, 65) == 0 and L.lib().mi_gallery_workspace_bytes(37, 5, 36, 64) > 0
    H.gallery_moments(x, lab, 5)                            # the good input does reach the entry
    assert launched == ["mi_gallery_moments"]


def test_plot_2d_class_gallery_end_to_end(tmp_path):
    rs = np.random.RandomState(61)
    centres = rs.standard_normal((3, 16)).astype(np.float32) * 6
    pred = (centres[np.arange(200) % 3] + rs.standard_normal((200, 16))).astype(np.float32)
    subvol = (rs.standard_normal((200, 2, 6, 9)) + (np.arange(200) % 3)[:, None, None, None]).astype(np.float32)
    np.savez(tmp_path / "all_output_info.npz", pred=pred, name=np.array(["t"] * 200), coords=np.zeros((200, 3)), subvol=subvol)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "out"
    run = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path",
                          str(out), "--k", "8", "--n_cluster", "3", "--niter", "20", "--class_gallery"], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert os.path.exists(out / "class_gallery.npz") and os.path.exists(out / "class_gallery.png")
    g, km = np.load(out / "class_gallery.npz"), np.load(out / "kmeans_labels.npz")
    assert sorted(g.files) == ["count", "exemplar_d2", "exemplar_index", "mean", "order", "std"]
    assert g["mean"].shape == g["std"].shape == (3, 6, 9) and g["mean"].dtype == g["std"].dtype == np.float32
    assert g["count"].dtype == np.int32 and g["count"].sum() == 200
    assert g["exemplar_index"].shape == g["exemplar_d2"].shape == (3, 8) and g["exemplar_d2"].dtype == np.float64
    label, assign = km["label"], km["assign"]
    want_mean, want_std, want_count = R.moments(subvol[:, 0], label, 3)
    assert np.array_equal(g["count"], want_count)
    top = float(np.abs(subvol[:, 0]).max())                 # the bounds of check_moments
    assert np.abs(g["mean"] - want_mean).max() <= 2.0 ** -23 * top
    assert (np.abs(g["std"] - want_std) <= 2.0 ** -24 * want_std + 2.0 ** -40 * (want_std + top) + 2.0 ** -149).all()
    want_idx, want_d2 = R.exemplars(pred, km["centroids"], assign, label, 3, 8)
    assert np.array_equal(g["exemplar_index"], want_idx) and g["exemplar_d2"].tobytes() == want_d2.tobytes()
    assert g["order"].tolist() == R.row_order(want_count).tolist()
    from plot2d_ref import read_png
    pic = read_png(str(out / "class_gallery.png"))
    assert np.array_equal(pic, R.raster(g["mean"], g["std"], g["count"], g["exemplar_index"], subvol[:, 0], 8, 2))
