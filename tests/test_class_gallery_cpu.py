"""The restatements of tests/gallery_ref.py against numpy's own mean, std and stable argsort, the refusals of the hipops wrappers
against a stub library, and the host side of plot_2d --class_gallery with every device step stubbed.  No GPU."""
import argparse
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import gallery_ref as R


@pytest.mark.parametrize("counts,h,w,offset", [([9, 0, 1, 20, 7], 6, 6, 0.0), ([5, 3], 5, 7, 0.0), ([4, 1, 0], 1, 1, 0.0),
                                               ([300, 0, 2], 3, 4, 1e4)])
def test_moments_restatement_is_numpys_mean_and_std(counts, h, w, offset):
    g = R.case(counts, h, w, seed=3, offset=offset)
    mean, std, count = R.moments(g["patches"], g["labels"], g["k"])
    assert count.tolist() == counts and count.dtype == np.int32 and mean.dtype == std.dtype == np.float64
    for c, n_c in enumerate(counts):
        if n_c == 0:
            assert not mean[c].any() and not std[c].any()
            continue
        members = g["patches"][g["labels"] == c].astype(np.float64)
        scale = np.abs(members).max()
        assert np.abs(mean[c] - np.mean(members, 0)).max() <= 1e-13 * scale
        assert np.abs(std[c] - np.std(members, 0)).max() <= 1e-13 * scale          # numpy.std divides by the count
        if n_c == 1:
            assert not std[c].any() and np.array_equal(mean[c], members[0])


@pytest.mark.parametrize("dim", [3, 64])
def test_exemplar_restatement_is_a_stable_argsort(dim):
    g = R.case([40, 3, 0, 25], 2, 2, seed=5, dim=dim, k_centroids=6)
    emb, assign, labels = g["emb"], g["assign"], g["labels"]
    first = np.flatnonzero(labels == 0)
    emb[first[7]] = emb[first[2]]                           # equal embeddings on one centroid: equal distances
    assign[first[7]] = assign[first[2]]
    d2 = R.distances(emb, g["centroids"], assign)
    assert d2[first[7]] == d2[first[2]]
    direct = ((emb.astype(np.float64) - g["centroids"].astype(np.float64)[assign]) ** 2).sum(1)
    assert np.abs(d2 - direct).max() <= 1e-13 * direct.max()
    for m in (1, 8, 64):
        idx, out = R.exemplars(emb, g["centroids"], assign, labels, 4, m)
        assert idx.shape == out.shape == (4, m) and idx.dtype == np.int32 and out.dtype == np.float64
        for c in range(4):
            members = np.flatnonzero(labels == c)           # ascending pick index: a stable sort breaks ties by it
            want = members[np.argsort(d2[members], kind="stable")][:m]
            assert idx[c, :len(want)].tolist() == want.tolist() and np.array_equal(out[c, :len(want)], d2[want])
            assert (idx[c, len(want):] == -1).all() and np.isinf(out[c, len(want):]).all()
    idx, _ = R.exemplars(emb, g["centroids"], assign, labels, 4, 64)
    at = idx[0].tolist()
    assert at.index(first[7]) == at.index(first[2]) + 1    # the tie, lower pick first


def test_raster_restatement():
    assert R.row_order([3, 7, 3, 0, 7]).tolist() == [1, 4, 0, 2, 3]
    assert R.grey(np.full((2, 2), 1.5, np.float32), 1.5, 0.0).tolist() == [[0, 0], [0, 0]]
    v = np.array([0, 0.5, 1, np.nan], np.float32)
    assert R.grey(v, 0, 1).tolist() == [0, 128, 255, 0]     # 127.5 rounds to the even 128
    assert R.canvas(3, 4, 4, 2, 2) == (4 + 3 * 36, 102 + 4 * 12)
    mean = np.arange(32, dtype=np.float32).reshape(2, 4, 4)
    pic = R.raster(mean, np.zeros_like(mean), np.array([1, 12], np.int32), np.array([[0], [-1]], np.int32), mean[:1], 1, 2)
    assert pic.shape == (76, 138, 3) and (pic[:, :, 0] == pic[:, :, 2]).all()
    assert pic[4, 102, 0] == 0 and pic[11, 109, 0] == 255   # the mean of a row: its least pixel first, its largest last
    assert (pic[4:12, 114:122] == 0).all()                  # no deviation anywhere: black
    assert (pic[4:12, 126:134] == 255).all() and not (pic[40:48, 126:134] == 255).all()      # class 1 first, it has no exemplar
    from cet_pick_amd.utils import plot2d as P2
    from cet_pick_amd import hipops as H
    assert np.array_equal(P2.DIGITS_5X7, R.DIGITS_5X7)
    assert H.gallery_canvas(3, 4, 4, 2, 2) == R.canvas(3, 4, 4, 2, 2) and H.gallery_canvas(48, 36, 36, 8, 2) == R.canvas(48, 36, 36, 8, 2)


class StubLib:
    """The library object of tests/test_lib_call_cpu.py: every mi_* entry records its arguments and returns `status`."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def stub(monkeypatch):
    from cet_pick_amd import _lib as L
    s = StubLib()
    monkeypatch.setattr(L, "_lib", s)
    monkeypatch.setattr(L, "stream", lambda: ctypes.c_void_p(0x5712))
    return s


def test_wrappers_refuse_on_the_host_before_the_library(stub):
    from cet_pick_amd import hipops as H
    x, lab = torch.zeros((6, 3, 3)), torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)
    emb, cen = torch.zeros((6, 4)), torch.zeros((2, 4))
    asg = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32)
    bad_label, bad_assign = lab.clone(), asg.clone()
    bad_label[4], bad_assign[2] = 3, -1
    with pytest.raises(ValueError, match=r"labels holds 3, outside \[0, 3\)"):
        H.gallery_moments(x, bad_label, 3)
    with pytest.raises(ValueError, match="labels"):
        H.gallery_exemplars(emb, cen, asg, bad_label, 3, 2)
    with pytest.raises(ValueError, match=r"assign holds -1, outside \[0, 2\)"):
        H.gallery_exemplars(emb, cen, bad_assign, lab, 3, 2)
    with pytest.raises(ValueError, match="patches must be contiguous"):
        H.gallery_moments(torch.zeros((6, 3, 6))[:, :, ::2], lab, 3)
    with pytest.raises(ValueError, match="labels must be contiguous"):
        H.gallery_moments(x, torch.zeros(12, dtype=torch.int32)[::2], 3)
    with pytest.raises(ValueError, match="emb must be contiguous"):
        H.gallery_exemplars(torch.zeros((6, 8))[:, ::2], cen, asg, lab, 3, 2)
    for m in (0, 65, -1):
        with pytest.raises(ValueError, match="m must be in 1..64"):
            H.gallery_exemplars(emb, cen, asg, lab, 3, m)
    with pytest.raises(ValueError, match="n == 0"):
        H.gallery_moments(x[:0], lab[:0], 3)
    with pytest.raises(ValueError, match="n == 0"):
        H.gallery_exemplars(emb[:0], cen, asg[:0], lab[:0], 3, 2)
    with pytest.raises(ValueError, match="labels must be torch.int32"):
        H.gallery_moments(x, lab.long(), 3)
    assert stub.calls == []


class KmeansStub:
    made = 0

    def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
        self.k, self.niter = k, niter
        KmeansStub.made += 1

    def train(self, p):
        self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

    def assign(self, p):
        return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]


@pytest.fixture
def stubbed(tmp_path, monkeypatch, stub):
    """plot_2d.main with every device step replaced, as tests/test_plot2d_cpu.py drives it; the library itself is the stub above,
    so an entry that were reached would be on record."""
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    calls = []
    KmeansStub.made = 0
    monkeypatch.setattr(KM, "Kmeans", KmeansStub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    monkeypatch.setattr(P, "merge_centroids", lambda centroids, n_cluster: np.arange(len(centroids)) % n_cluster)
    monkeypatch.setattr(P, "write_class_gallery", lambda path, patches, projs, centroids, assign, label, n_classes, m, device:
                        calls.append((patches.shape, patches.dtype, projs.shape, np.asarray(centroids).shape, int(label.max()),
                                      n_classes, m)))
    rs = np.random.RandomState(1)
    common = dict(pred=rs.standard_normal((40, 6)).astype(np.float32), name=np.array(["a"] * 40), coords=np.zeros((40, 3)))
    np.savez(tmp_path / "with.npz", subvol=rs.standard_normal((40, 2, 8, 10)).astype(np.float32), **common)
    np.savez(tmp_path / "without.npz", **common)
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args

    def run(name, *extra):
        out = tmp_path / ("o%d" % len(os.listdir(tmp_path)))
        P.main(parse(["--input", str(tmp_path / name), "--path", str(out), "--k", "4", "--niter", "2"] + list(extra)))
        return sorted(os.listdir(out))

    return run, calls


def test_class_gallery_needs_subvol_before_kmeans_runs(stubbed, stub):
    run, calls = stubbed
    with pytest.raises(ValueError, match="'subvol'"):
        run("without.npz", "--class_gallery")
    with pytest.raises(ValueError, match="gallery_exemplars"):
        run("with.npz", "--class_gallery", "--gallery_exemplars", "65")
    assert KmeansStub.made == 0 and not calls and stub.calls == []


def test_without_the_flag_nothing_is_added(stubbed, stub):
    run, calls = stubbed
    assert run("with.npz") == ["kmeans_labels.npz"] and run("without.npz") == ["kmeans_labels.npz"]
    assert not calls and stub.calls == []
    from cet_pick_amd import plot_2d as P
    a = P.add_arguments(argparse.ArgumentParser()).parse_args(["--input", "i", "--path", "o"])
    assert a.class_gallery is False and a.gallery_exemplars == 8


def test_the_flag_hands_the_final_classes_to_the_gallery(stubbed, stub):
    run, calls = stubbed
    run("with.npz", "--class_gallery")                      # no merge: the 4 centroids are the classes; channel 0 of subvol
    run("with.npz", "--class_gallery", "--n_cluster", "2", "--gallery_exemplars", "3")
    assert calls == [((40, 8, 10), np.float32, (40, 6), (4, 6), 3, 4, 8), ((40, 8, 10), np.float32, (40, 6), (4, 6), 1, 2, 3)]
    assert stub.calls == []
