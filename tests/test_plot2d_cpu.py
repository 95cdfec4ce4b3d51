"""The restatements of tests/plot2d_ref.py against the code they restate (the reference's loop, matplotlib's imsave, torch's
interpolation), the PNG writer, and the host side of plot_2d --min_dist_vis.  No GPU."""
import argparse
import contextlib
import os

import numpy as np
import pytest

import plot2d_ref as R


def random_map(n, seed):
    return np.random.RandomState(seed).uniform(0, 1, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("n,thr,seed", [(1, 1e-3, 0), (1, 0.0, 0), (400, 1.3e-3, 1), (400, 1e-12, 2), (200, 4.0, 3), (300, 0.0, 4)])
def test_selection_restatement_is_the_reference_loop(n, thr, seed):
    y = random_map(n, seed)
    y[n // 2] = y[0]                                         # an exact duplicate of pick 0
    want = R.select_literal(y, np.float32(thr))
    got = R.select(y, thr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (np.diff(got) > 0).all() and (0 not in got) == (thr > 0)
    if thr <= 0:
        assert len(got) == n


def test_selection_restatement_on_the_lattice():
    """Coordinates k / 32: neighbours are exactly 1/1024 apart (squared), which does not block; one ulp more blocks the
    axis neighbours and not the diagonal ones: the checkerboard that holds pick 0, without pick 0."""
    g = np.arange(16, dtype=np.float32) / 32
    y = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    assert R.select(y, 1 / 1024).tolist() == list(range(1, 256))
    more = R.select(y, np.nextafter(np.float32(1 / 1024), np.float32(1)))
    assert np.array_equal(more, R.select_literal(y, np.nextafter(np.float32(1 / 1024), np.float32(1))))
    assert more.tolist() == [i for i in range(1, 256) if (i // 16 + i % 16) % 2 == 0]


def test_patch_bytes_restatement_is_matplotlibs_imsave(tmp_path):
    plt = pytest.importorskip("matplotlib.pyplot")
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(5)
    patches = [rs.standard_normal((b, b)).astype(np.float32) * 7 + 3 for b in (9, 36, 36, 36)] + [np.full((9, 9), 1.5, np.float32)]
    for k, p in enumerate(patches):
        path = str(tmp_path / ("%d.png" % k))
        plt.imsave(path, p, cmap="gray")
        rgba = np.asarray(Image.open(path))
        assert rgba.shape == p.shape + (4,) and (rgba[:, :, 3] == 255).all()
        assert np.array_equal(rgba[:, :, 0], rgba[:, :, 1]) and np.array_equal(rgba[:, :, 0], rgba[:, :, 2])
        assert np.array_equal(R.patch_bytes(p), rgba[:, :, 0])
    assert not np.array_equal(R.GRAY_LUT, np.arange(256))    # the table is not the identity


@pytest.mark.parametrize("b", [9, 12, 17, 24, 33, 36, 40, 64])
def test_resize_restatement_is_torchs_interpolation(b):
    """T = 32 is a power of two: every weight is dyadic and the float32 result exact, so equality without a tolerance."""
    img = np.random.RandomState(b).randint(0, 256, (b, b)).astype(np.uint8)
    assert np.array_equal(R.resize(img, 32), R.resize_torch(img, 32))
    img[::2] = 255 - img[::2] // 2
    assert np.array_equal(R.resize(img, 32), R.resize_torch(img, 32))


def test_thumbnail_seeds_keep_the_float32_chain_within_the_excused_share():
    """What tests/test_plot2d_gpu.py relies on: per case at most 1 % of the pixels lie within 2^-10 of a rounding tie in
    float64, and the reference's own float32 chain differs from the float64 bytes on at most 1 % of them, by one level."""
    for name, patches in R.thumb_cases().items():
        both = [R.thumb_bytes64(p) for p in patches]
        want, excused = np.stack([w for w, _ in both]), np.stack([e for _, e in both])
        assert excused.mean() <= 0.01, name
        if name == "constant":
            assert not want.any()
            continue
        got = np.stack([R.thumb_bytes32(p) for p in patches])
        diff = np.abs(got.astype(int) - want.astype(int))
        print("%s: %d of %d pixels differ between float32 and float64, %d excused" % (name, (diff > 0).sum(), diff.size,
                                                                                     excused.sum()))
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01 and not (diff > 0)[~excused].any(), name


def test_write_png_round_trips(tmp_path):
    from cet_pick_amd.utils.plot2d import write_png
    rs = np.random.RandomState(6)
    for shape in [(7, 5), (1, 1), (9, 13, 3), (6, 4, 4), (300, 257, 3)]:
        a = rs.randint(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / "a.png")
        write_png(path, a)
        assert np.array_equal(R.read_png(path), a)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path)), a)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "b.png"), bad)


def test_layout_constants():
    from cet_pick_amd.utils import plot2d as P2
    lay = P2.layout(1500, 32)
    assert (lay["P"], lay["M"], lay["R"], lay["T"], lay["label_dx"], lay["label_dy"]) == (1500, 48, 42, 32, 35, 28)
    ref = R.layout(128, 8)
    lay = P2.layout(128, 8)
    assert (lay["R"], lay["label_dx"], lay["label_dy"]) == (ref["R"], ref["dx"], ref["dy"]) == (1, 1, 1)
    with pytest.raises(ValueError):
        P2.layout(127, 32)
    assert np.array_equal(P2.GRAY_LUT, R.GRAY_LUT) and P2.DIGITS_5X7.shape == (10, 7) and P2.DIGITS_5X7.max() < 32
    assert len({bytes(g) for g in P2.DIGITS_5X7}) == 10


def test_wrappers_refuse_before_the_device():
    import torch
    from cet_pick_amd import _lib
    from cet_pick_amd.utils import plot2d as P2
    with pytest.raises(ValueError, match="square"):
        P2.thumbnails(torch.zeros((2, 1, 8, 9)), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="square"):
        P2.patch_bytes(np.zeros((2, 1, 8, 9), np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipExtensionError):
            P2.select(torch.zeros((4, 2)), 1e-3)
        with pytest.raises(_lib.HipExtensionError):
            P2.patch_bytes(np.zeros((2, 1, 8, 8), np.float32))


class KmeansStub:
    def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
        self.k, self.niter = k, niter

    def train(self, p):
        self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

    def assign(self, p):
        return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]


@pytest.fixture
def stubbed(tmp_path, monkeypatch):
    """plot_2d.main with stubs for every device step, as tests/test_tsne_cpu.py drives it; calls of the new steps are recorded."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    calls = []

    def fake_map(projs, perplexity, seed, device):
        y = np.random.RandomState(0).standard_normal((len(projs), 2)).astype(np.float32) * 30
        return np.zeros((len(projs), perplexity), np.int32), np.zeros((len(projs), perplexity), np.float32), y, 1.25, 999

    monkeypatch.setattr(KM, "Kmeans", KmeansStub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "tsne_map", fake_map)
    monkeypatch.setattr(P, "knn_graph", lambda projs, k, device: (np.zeros((len(projs), k), np.int32),
                                                                  np.zeros((len(projs), k), np.float32)))
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    monkeypatch.setattr(P, "map_colours", lambda y01, table, device: np.zeros((len(y01), 3), np.uint8))     # (reached with a GPU)
    monkeypatch.setattr(P, "write_patch_images", lambda subvol, out_dir, device: calls.append(("imgs", subvol.shape)) or len(subvol))
    monkeypatch.setattr(P, "map_picture", lambda *a, **k: calls.append(("picture",)) or (np.zeros(0, np.int32),
                                                                                        np.zeros((128, 128, 3), np.uint8)))
    rs = np.random.RandomState(1)
    x = rs.standard_normal((40, 6)).astype(np.float32)
    common = dict(pred=x, name=np.array(["a"] * 40), coords=np.zeros((40, 3)))
    np.savez(tmp_path / "with.npz", subvol=rs.standard_normal((40, 1, 8, 8)).astype(np.float32), **common)
    np.savez(tmp_path / "without.npz", **common)
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args

    def run(name, *extra):
        out = tmp_path / ("o%d" % len(os.listdir(tmp_path)))
        P.main(parse(["--input", str(tmp_path / name), "--path", str(out), "--k", "4", "--niter", "2"] + list(extra)))
        return sorted(os.listdir(out))

    return run, calls


def test_plot_2d_needs_subvol_for_the_pictures(stubbed):
    run, calls = stubbed
    with pytest.raises(ValueError, match="subvol"):
        run("without.npz", "--min_dist_vis", "1.3e-3")
    with pytest.raises(ValueError, match="plot_size"):
        run("with.npz", "--min_dist_vis", "1.3e-3", "--plot_size", "100")
    assert not calls


def test_plot_2d_without_min_dist_vis_is_unchanged(stubbed, capsys):
    import torch
    run, calls = stubbed
    assert run("with.npz") == ["kmeans_labels.npz"]
    assert "plots, thumbnails and colour map are not made here" in capsys.readouterr().out
    files = run("with.npz", "--mode", "tsne", "--num_neighbor", "5")
    assert files == (["all_colors.npy"] if torch.cuda.is_available() else []) + ["embeddings_2d.npz", "kmeans_labels.npz",
                                                                                 "knn_graph.npz"]
    out = capsys.readouterr().out
    assert "the plots and thumbnails are not made here" in out and "--min_dist_vis" in out
    assert not calls and run("without.npz") == ["kmeans_labels.npz"]
    p = argparse.ArgumentParser()
    from cet_pick_amd import plot_2d as P
    a = P.add_arguments(p).parse_args(["--input", "i", "--path", "o"])
    assert a.min_dist_vis is None and a.save_out_img == 1 and a.plot_size == 1500


def test_plot_2d_with_min_dist_vis_and_no_map_writes_the_images_only(stubbed, capsys):
    run, calls = stubbed
    run("with.npz", "--min_dist_vis", "1.3e-3")
    out = capsys.readouterr().out
    assert calls == [("imgs", (40, 1, 8, 8))] and "are not made here" not in out and "there is no picture" in out
    run("with.npz", "--min_dist_vis", "1.3e-3", "--save_out_img", "0")
    assert calls == [("imgs", (40, 1, 8, 8))] and "no imgs/" in capsys.readouterr().out


def test_encoder_threads_follow_omp_num_threads(monkeypatch):
    from cet_pick_amd import plot_2d as P
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert P.encoder_threads() == 3
    monkeypatch.setenv("OMP_NUM_THREADS", "400")
    assert P.encoder_threads() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert P.encoder_threads() == 4
