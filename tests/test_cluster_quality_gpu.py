"""csrc/cluster_quality.hip through hipops and utils/cluster_quality.py against the float64 restatement and the bounds of
tests/cluster_quality_ref.py, and plot_2d / scan_main --quality end to end.

The bounds come from the inputs alone: a squared distance of the row-product tile is within e = 2 band(d) (|x_i|^2 + |x_j|^2) of
float64 (tests/knn_ref.py), a distance delta therefore within min(sqrt(e), e / delta), a sum of distances within the sum of its
pairs' bounds, a = sum / (count - 1) within ea, b within eb (the largest bound over the other classes), s within
2 (ea + eb) / max(a, b).  Every test prints the largest share of its bound the device used."""
import argparse
import os

import numpy as np
import pytest

import cluster_quality_ref as R

pytestmark = pytest.mark.gpu

_cache = {}


def arbiter(name):
    """(x, labels, S, E, fin) of a variant, computed once and never changed"""
    if name not in _cache:
        x, labels = R.make(name)
        _cache[name] = (x, labels) + R.silhouette64(x, labels)
    return _cache[name]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def share(err, bound):
    """largest err / bound; an entry with bound 0 must have err 0"""
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("name", R.VARIANTS)
def test_sums_and_silhouette_within_the_derived_bounds(name):
    from cet_pick_amd import hipops as H
    x, labels, S, E, fin = arbiter(name)
    k = S.shape[1]
    ea, eb, es, decided = R.bounds(E, fin)
    assert (~decided).mean() <= 0.01                       # before the device's output is looked at
    xd, ld = dev(x), dev(labels)
    sums = H.silhouette_sums(xd, ld, k)
    assert sums.dtype.is_floating_point and sums.element_size() == 8 and tuple(sums.shape) == (len(x), k)
    got_S = sums.cpu().numpy()
    count = np.maximum(np.bincount(labels, minlength=k), 1)[None, :].astype(np.float64)
    sh_S = share(np.abs(got_S - S) / count, E / count)
    out = {key: v.cpu().numpy() for key, v in H.silhouette_finalise(sums, ld).items()}
    sh_a, sh_b, sh_s = share(np.abs(out["a"] - fin["a"]), ea), share(np.abs(out["b"] - fin["b"]), eb), share(np.abs(out["s"] - fin["s"]), es)
    differ = out["nearest"] != fin["nearest"]
    print("%s: N=%d d=%d k=%d: share of the bound used: S / count %.4f, a %.4f, b %.4f, s %.4f (largest s bound %.2e); nearest "
          "differs on %d picks, %d of them decided; undecided %.3f %%"
          % (name, len(x), x.shape[1], k, sh_S, sh_a, sh_b, sh_s, es.max(), differ.sum(), (differ & decided).sum(),
             100 * (~decided).mean()))
    assert sh_S <= 1.0 and sh_a <= 1.0 and sh_b <= 1.0 and sh_s <= 1.0
    assert not (differ & decided).any()
    # the finalise step is float64 throughout: given the device's own sums it is the restated formula
    own = R.finalise(got_S, labels)
    for key in ("s", "a", "b"):
        assert np.abs(out[key] - own[key]).max() <= 1e-12, key
    assert np.array_equal(out["nearest"], own["nearest"])
    # the summaries against the restatement applied to the device's s and nearest
    C = k
    assert np.array_equal(out["class_count"], fin["count"]) and out["class_count"].dtype == np.int32
    for c in range(C):
        m = labels == c
        if m.any():
            assert abs(out["class_mean"][c] - out["s"][m].mean()) <= 1e-12
        else:
            assert np.isnan(out["class_mean"][c])
    assert abs(float(out["mean"]) - out["s"].mean()) <= 1e-12
    conf = np.zeros((C, C), np.int32)
    np.add.at(conf, (labels, out["nearest"]), 1)
    assert np.array_equal(out["confusion"], conf) and out["confusion"].dtype == np.int32
    if name == "sizes":                                    # the only member of its class: a = s = 0, as sklearn
        lone = np.flatnonzero(labels == 0)
        assert len(lone) == 1 and out["s"][lone[0]] == 0 and out["a"][lone[0]] == 0 and out["b"][lone[0]] > 0


def test_agrees_with_sklearn_golden():
    """the device against scikit-learn's float64 silhouette_samples, within the same bound on s"""
    from cet_pick_amd.utils.cluster_quality import silhouette
    gold = np.load(R.GOLDEN)
    for name in ("ragged", "gaps"):
        x, labels, S, E, fin = arbiter(name)
        es = R.bounds(E, fin)[2]
        q = silhouette(dev(x), labels)
        assert share(np.abs(q.s - gold["sil_" + name]), es + 1e-13) <= 1.0
        assert abs(q.mean - gold["sil_" + name].mean()) <= es.max()


def test_merged_score_from_the_fine_sums():
    """k fine clusters merged by class_of: within the bound of the merged labels (not bit-equal to a direct run on them: the
    float64 additions come in another order)"""
    from cet_pick_amd.utils.cluster_quality import SilhouetteSums, silhouette
    x, labels, S, E, fin = arbiter("ragged")
    class_of = np.array([0, 1, 0, 2, 1, 2, 0], np.int32)
    merged = class_of[labels]
    Sm, Em, finm = R.silhouette64(x, merged)
    ea, eb, es, decided = R.bounds(Em, finm)
    assert (~decided).mean() <= 0.01
    sums = SilhouetteSums(dev(x), labels, 7)
    q = sums.score(class_of)
    print("merged 7 -> 3: share of the bound used: a %.4f b %.4f s %.4f" % (
        share(np.abs(q.a - finm["a"]), ea), share(np.abs(q.b - finm["b"]), eb), share(np.abs(q.s - finm["s"]), es)))
    assert share(np.abs(q.a - finm["a"]), ea) <= 1.0 and share(np.abs(q.b - finm["b"]), eb) <= 1.0
    assert share(np.abs(q.s - finm["s"]), es) <= 1.0
    assert not ((q.nearest != finm["nearest"]) & decided).any()
    assert np.array_equal(q.class_count, np.bincount(merged)) and q.confusion.shape == (3, 3)
    direct = silhouette(dev(x), merged)
    assert np.abs(direct.s - q.s).max() <= 2 * es.max()
    assert np.abs(sums.score().s - fin["s"]).max() <= R.bounds(E, fin)[2].max()          # the one S serves the fine score too


def test_two_runs_give_the_same_bytes():
    from cet_pick_amd import hipops as H
    x, labels = arbiter("chunks")[:2]
    xd, ld = dev(x), dev(labels)
    first = H.silhouette_sums(xd, ld, 3)
    f1 = H.silhouette_finalise(first, ld)
    f1 = {key: v.clone() for key, v in f1.items()}
    second = H.silhouette_sums(xd, ld, 3)
    f2 = H.silhouette_finalise(second, ld)
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
    for key in f1:
        assert f1[key].cpu().numpy().tobytes() == f2[key].cpu().numpy().tobytes(), key


def test_contingency_and_comparison():
    from cet_pick_amd import hipops as H
    from cet_pick_amd.utils.cluster_quality import compare_labelings
    gold = np.load(R.GOLDEN)
    rs = np.random.RandomState(2)
    a, b = rs.randint(0, 37, 70001).astype(np.int32), rs.randint(0, 5, 70001).astype(np.int32)
    want = np.zeros((37, 5), np.int64)
    np.add.at(want, (a, b), 1)
    got = H.label_contingency(dev(a), dev(b), 37, 5)
    assert got.cpu().numpy().dtype == np.int64 and np.array_equal(got.cpu().numpy(), want)
    labels = arbiter("sizes")[1]
    other = R.second_labeling(labels)
    cmp = compare_labelings(labels, other)
    assert np.array_equal(cmp.table, R.contingency(labels, other)[0]) and cmp.ids_b[0] == -1
    assert abs(cmp.ari - float(gold["ari_sizes"])) <= 1e-12 and abs(cmp.nmi - float(gold["nmi_sizes"])) <= 1e-12
    with pytest.raises(ValueError):
        H.label_contingency(dev(a), dev(b), 36, 5)


def test_refusals():
    import torch
    from cet_pick_amd import hipops as H
    from cet_pick_amd._lib import HipExtensionError
    from cet_pick_amd.utils.cluster_quality import silhouette
    x, labels = arbiter("ragged")[:2]
    xd, ld = dev(x), dev(labels)
    with pytest.raises(ValueError, match="2 classes"):     # one class
        silhouette(xd, np.zeros(len(x), np.int32))
    with pytest.raises(ValueError, match="largest has 1"): # every class a singleton
        silhouette(xd[:5].contiguous(), np.arange(5, dtype=np.int32))
    bad = labels.copy()
    bad[17] = 7
    with pytest.raises(ValueError, match="holds 7"):
        H.silhouette_sums(xd, dev(bad), 7)
    bad[17] = -2
    with pytest.raises(ValueError, match="holds -2"):
        H.silhouette_sums(xd, dev(bad), 7)
    with pytest.raises(HipExtensionError, match="unsupported"):
        H.silhouette_sums(xd, ld, H.SILHOUETTE_MAX_K + 1)
    with pytest.raises(HipExtensionError):
        H.silhouette_sums(xd.double(), ld, 7)
    with pytest.raises(HipExtensionError):
        H.silhouette_sums(xd.t().contiguous().t(), ld, 7)
    with pytest.raises(HipExtensionError):
        H.silhouette_sums(torch.from_numpy(x), ld, 7)
    with pytest.raises(HipExtensionError):
        silhouette(x, labels)                              # a host bank and no device named


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def three_blobs(tmp_path, n=150, d=16):
    rs = np.random.RandomState(8)
    blob = np.arange(n) % 3
    x = (3.0 * rs.randn(3, d)[blob] + 0.3 * rs.randn(n, d)).astype(np.float32)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["t%d" % (i % 2) for i in range(n)]),
             coords=np.arange(3 * n).reshape(-1, 3))
    return x, blob


def run_plot_2d(tmp_path, out, *flags):
    from cet_pick_amd import plot_2d as P
    args = P.add_arguments(argparse.ArgumentParser()).parse_args(
        ["--input", str(tmp_path / "all_output_info.npz"), "--path", str(out), "--k", "8", "--niter", "10", "--n_cluster", "3"] + list(flags))
    P.main(args)
    return sorted(os.listdir(out))


def test_plot_2d_quality_sweep_and_compare(tmp_path, capsys):
    pytest.importorskip("sklearn")
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils.cluster_quality import SilhouetteSums, compare_labelings
    x, blob = three_blobs(tmp_path)
    np.savez(tmp_path / "other.npz", label=blob.astype(np.int32))
    plain = run_plot_2d(tmp_path, tmp_path / "plain")
    assert "cluster_quality.npz" not in plain
    files = run_plot_2d(tmp_path, tmp_path / "q", "--quality", "--sweep_n_cluster", "2,3", "--compare_labels", str(tmp_path / "other.npz"))
    assert sorted(set(files) - set(plain)) == ["cluster_quality.npz"]
    text = capsys.readouterr().out
    assert text.count("mean silhouette ") >= 2 and "adjusted Rand index" in text
    q, km = np.load(tmp_path / "q" / "cluster_quality.npz"), np.load(tmp_path / "q" / "kmeans_labels.npz")
    n, k = len(x), 8
    shapes = dict(s=(n,), a=(n,), b=(n,), nearest=(n,), class_mean=(3,), class_count=(3,), confusion=(3, 3), mean=(),
                  fine_s=(n,), fine_a=(n,), fine_b=(n,), fine_nearest=(n,), fine_class_mean=(k,), fine_class_count=(k,),
                  fine_confusion=(k, k), fine_mean=(), sweep_n_cluster=(2,), sweep_mean=(2,), sweep_min_class_mean=(2,),
                  sweep_smallest_class=(2,), compare_table=(3, 3), compare_ari=(), compare_nmi=(), compare_ids=(3,),
                  compare_ids_other=(3,))
    assert sorted(q.files) == sorted(shapes)
    for key, shape in shapes.items():
        assert q[key].shape == shape, key
    assert np.array_equal(q["sweep_n_cluster"], [2, 3]) and np.array_equal(q["class_count"], np.bincount(km["label"], minlength=3))
    sums = SilhouetteSums(dev(x), km["assign"], k)
    for i, v in enumerate((2, 3)):
        r = sums.score(P.merge_centroids(km["centroids"], v))
        assert r.mean == q["sweep_mean"][i] and np.nanmin(r.class_mean) == q["sweep_min_class_mean"][i]
    assert q["sweep_mean"][1] == q["mean"] and -1.0 <= q["fine_mean"] <= 1.0     # --n_cluster 3 is the sweep's second entry
    cmp = compare_labelings(km["label"], blob)
    assert np.array_equal(q["compare_table"], cmp.table) and q["compare_table"].sum() == n
    assert q["compare_ari"] == cmp.ari and q["compare_nmi"] == cmp.nmi
    np.savez(tmp_path / "short.npz", label=blob[:-1])
    with pytest.raises(ValueError, match="labels 149 picks"):
        run_plot_2d(tmp_path, tmp_path / "bad", "--compare_labels", str(tmp_path / "short.npz"))


def run_scan_main(tmp_path, out, *flags):
    from cet_pick_amd import scan_main as M
    args = M.add_arguments(argparse.ArgumentParser()).parse_args(
        ["--input", str(tmp_path / "all_output_info.npz"), "--path", str(out), "--nclusters", "3", "--nheads", "2", "--num_neighbor",
         "5", "--num_epochs", "30", "--batch_size", "50", "--lr", "0.03"] + list(flags))
    M.main(args)
    return sorted(os.listdir(out))


def test_scan_main_quality(tmp_path):
    from cet_pick_amd.utils.cluster_quality import silhouette
    x, blob = three_blobs(tmp_path)
    plain = run_scan_main(tmp_path, tmp_path / "plain")
    assert plain == ["scan_heads.pth", "scan_labels.npz"]
    files = run_scan_main(tmp_path, tmp_path / "q", "--quality")
    assert files == ["scan_heads.pth", "scan_labels.npz", "scan_quality.npz"]
    lab, q = np.load(tmp_path / "q" / "scan_labels.npz"), np.load(tmp_path / "q" / "scan_quality.npz")
    assert np.array_equal(lab["label"], np.load(tmp_path / "plain" / "scan_labels.npz")["label"])
    assert lab["stats"].shape == (2, 4) and np.load(tmp_path / "plain" / "scan_labels.npz")["stats"].shape == (2, 3)
    assert sorted(q.files) == sorted(["head", "s", "a", "b", "nearest", "class_mean", "class_count", "mean", "confusion"])
    head = int(q["head"])
    assert head == int(lab["head"]) and q["s"].shape == (len(x),)
    assert np.float32(q["mean"]) == lab["stats"][head, 3]
    direct = silhouette(dev(x), lab["label"])
    assert direct.s.tobytes() == q["s"].tobytes() and np.array_equal(direct.confusion, q["confusion"])
    again = run_scan_main(tmp_path, tmp_path / "l", "--quality", "--load_model", str(tmp_path / "q" / "scan_heads.pth"))
    assert again == ["scan_labels.npz", "scan_quality.npz"]
    q2 = np.load(tmp_path / "l" / "scan_quality.npz")
    assert q2["s"].tobytes() == q["s"].tobytes() and int(q2["head"]) == head
    assert np.array_equal(np.load(tmp_path / "l" / "scan_labels.npz")["stats"][:, 3], lab["stats"][:, 3])
