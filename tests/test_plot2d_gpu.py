"""csrc/plot2d.hip through the wrappers of utils/plot2d.py against the restatements of tests/plot2d_ref.py, and
plot_2d --min_dist_vis end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plot2d_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_select(y, thr):
    from cet_pick_amd.utils import plot2d as P2
    y = np.ascontiguousarray(y, np.float32)
    got = P2.select(dev(y), thr).cpu().numpy()
    want = R.select(y, thr)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (len(got), len(want))
    return got


def uniform(n, seed=11):
    return np.random.RandomState(seed).uniform(0, 1, (n, 2)).astype(np.float32)


def test_select_one_pick():
    assert check_select(np.array([[0.25, 0.75]]), 1e-3).tolist() == []
    assert check_select(np.array([[0.25, 0.75]]), 0.0).tolist() == [0]


def test_select_duplicates_of_pick_0():
    y = uniform(300, seed=3)
    y[[7, 64, 65, 299]] = y[0]
    got = check_select(y, 1e-6)
    assert not set(got.tolist()) & {0, 7, 64, 65, 299}
    assert check_select(y, 0.0).tolist() == list(range(300))


def test_select_lattice_at_the_threshold():
    g = np.arange(16, dtype=np.float32) / 32
    y = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    assert check_select(y, 1 / 1024).tolist() == list(range(1, 256))         # a distance equal to thr does not block
    assert len(check_select(y, np.nextafter(np.float32(1 / 1024), np.float32(1)))) == 127


def test_select_chain_as_long_as_the_input():
    thr = 1.6e-7                                             # 2000 steps of 0.6 sqrt(thr) stay inside the unit square
    y = np.zeros((2000, 2), np.float32)
    y[:, 0] = np.arange(2000) * (0.6 * np.sqrt(thr))
    y[:, 1] = 0.5
    got = check_select(y, thr)
    assert 900 < len(got) < 1100                             # every second pick: each decision hangs on the one before


@pytest.mark.parametrize("thr,reverse", [(1.3e-3, False), (1e-12, False), (4.0, False), (1.3e-3, True)])
def test_select_uniform(thr, reverse):
    y = uniform(3000)
    got = check_select(y[::-1] if reverse else y, thr)
    assert (thr < 4.0) == (len(got) > 0)


def test_select_one_cell_long_list():
    y = 0.4 + 1e-3 * uniform(4000, seed=5)                   # the grid has at most 63 x 63 cells for 4000 picks: all in one
    assert 1000 < len(check_select(y, 1e-10)) < 4000         # discs of radius 1e-5 cover the 1e-3 square about 1.25 times


@pytest.mark.parametrize("name", ["b9", "b36", "b40", "two_channels", "constant", "outlier"])
def test_thumbnails(name):
    from cet_pick_amd.utils import plot2d as P2
    patches = R.thumb_cases()[name]
    n = len(patches)
    idx = np.arange(n - 1, -1, -1, dtype=np.int32)            # (not the identity)
    out, pre = P2.thumbnails(dev(patches), dev(idx), T=32, return_pre=True)
    out, pre = out.cpu().numpy(), pre.cpu().numpy()
    assert out.shape == (n, 32, 32) and pre.shape == patches.shape and out.dtype == pre.dtype == np.uint8
    both = [R.thumb_bytes64(patches[i]) for i in idx]
    want, excused = np.stack([w for w, _ in both]), np.stack([e for _, e in both])
    diff = np.abs(pre.astype(int) - want.astype(int))
    print("%s: %d of %d pre-resize bytes differ from float64, %d excused" % (name, (diff > 0).sum(), diff.size, excused.sum()))
    assert excused.mean() <= 0.01
    assert not diff[~excused].any() and diff.max() <= 1
    for k in range(n):                                       # the resize, from the kernel's own bytes, exactly
        assert np.array_equal(out[k], R.resize(pre[k, 0], 32)), (name, k)
    if name == "constant":
        assert not pre.any() and not out.any()
    assert np.array_equal(P2.thumbnails(dev(patches), dev(idx)).cpu().numpy(), out)


@pytest.mark.parametrize("name", ["b9", "b36", "b40", "two_channels", "constant", "outlier"])
def test_patch_bytes(name):
    from cet_pick_amd.utils import plot2d as P2
    patches = R.thumb_cases()[name]
    want = np.stack([R.patch_bytes(p[0]) for p in patches])
    got = P2.patch_bytes(patches, budget_bytes=2 * 4 * patches[0].size)          # two patches at a time
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(P2.patch_bytes(dev(patches)), want)
    if name == "constant":
        assert (got == R.GRAY_LUT[0]).all()


GLYPHS = np.array([[(17 * d + 3 * r + 1) % 32 for r in range(7)] for d in range(10)], np.uint8)       # not the default table


def raster_case():
    rs = np.random.RandomState(8)
    y = np.array([[0.5, 0.5], [0.5, 0.5], [0.3, 0.7], [0.33, 0.68], [0.0, 0.0], [1.0, 1.0], [0.8, 0.2], [0.1, 0.9]], np.float32)
    idx = np.array([0, 1, 2, 3, 4, 5], np.int32)             # same pixel twice, two overlapping, both far corners
    thumbs = rs.randint(0, 256, (6, 8, 8)).astype(np.uint8)
    colours = rs.randint(0, 255, (8, 3)).astype(np.uint8)
    labels = np.array([0, 7, 10, 255, 7, 10, 3, 3], np.int32)
    return y, idx, thumbs, colours, labels


def test_raster_out():
    from cet_pick_amd.utils import plot2d as P2
    y, idx, thumbs, colours, labels = raster_case()
    got = P2.draw_out(dev(y), dev(idx), dev(thumbs), colours, 128).cpu().numpy()
    want = R.draw_out(y, idx, thumbs, colours, 128)
    assert got.shape == (128, 128, 3) and np.array_equal(got, want), int((got != want).any(2).sum())
    assert (want != 255).any()


def test_raster_clipped_at_the_canvas():
    """The margin keeps the unit square clear of the edge at this size, so picks outside it: discs, frames, thumbnails and
    class boxes that cross the left, top, right and bottom edges, and two that lie outside altogether."""
    from cet_pick_amd.utils import plot2d as P2
    rs = np.random.RandomState(10)
    y = np.array([[-1.5, 0.5], [0.5, 2.6], [2.55, -1.5], [0.5, -1.55], [-1.6, 2.6], [40.0, 0.5], [0.5, -1e30]], np.float32)
    idx = np.arange(7, dtype=np.int32)
    thumbs = rs.randint(0, 256, (7, 8, 8)).astype(np.uint8)
    colours = rs.randint(0, 255, (7, 3)).astype(np.uint8)
    labels = np.array([1234567890, 5, 66, 777, 8, 9, 1], np.int32)
    want = R.draw_out(y, idx, thumbs, colours, 128)
    assert all((edge != 255).any() for edge in (want[0], want[-1], want[:, 0], want[:, -1]))
    assert np.array_equal(P2.draw_out(dev(y), dev(idx), dev(thumbs), colours, 128).cpu().numpy(), want)
    want = R.draw_labels(y, idx, thumbs, labels, GLYPHS, 128)
    assert np.array_equal(P2.draw_labels(dev(y), dev(idx), dev(thumbs), labels, 128, glyphs=GLYPHS).cpu().numpy(), want)


def test_raster_labels():
    from cet_pick_amd.utils import plot2d as P2
    y, idx, thumbs, colours, labels = raster_case()
    got = P2.draw_labels(dev(y), dev(idx), dev(thumbs), labels, 128, glyphs=GLYPHS).cpu().numpy()
    want = R.draw_labels(y, idx, thumbs, labels, GLYPHS, 128)
    assert np.array_equal(got, want), int((got != want).any(2).sum())
    other = P2.draw_labels(dev(y), dev(idx), dev(thumbs), labels, 128).cpu().numpy()
    assert np.array_equal(other, R.draw_labels(y, idx, thumbs, labels, P2.DIGITS_5X7, 128)) and not np.array_equal(other, got)


def test_raster_empty():
    from cet_pick_amd.utils import plot2d as P2
    y, idx, thumbs, colours, labels = raster_case()
    for pic in (P2.draw_out(dev(y), dev(idx[:0]), dev(thumbs[:0]), colours, 128),
                P2.draw_labels(dev(y), dev(idx[:0]), dev(thumbs[:0]), labels, 128)):
        assert tuple(pic.shape) == (128, 128, 3) and bool((pic == 255).all())


def test_plot_2d_end_to_end(tmp_path):
    from cet_pick_amd.utils import plot2d as P2
    rs = np.random.RandomState(9)
    centres = rs.standard_normal((3, 16)).astype(np.float32) * 6
    pred = (centres[np.arange(600) % 3] + rs.standard_normal((600, 16))).astype(np.float32)
    subvol = rs.standard_normal((600, 1, 12, 12)).astype(np.float32)
    np.savez(tmp_path / "all_output_info.npz", pred=pred, name=np.array(["t"] * 600), coords=np.zeros((600, 3)), subvol=subvol)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--mode", "umap",
            "--num_neighbor", "10", "--label_map", "--plot_size", "256", "--k", "16", "--niter", "10", "--n_cluster", "0"]
    out = tmp_path / "vis"
    run = subprocess.run(base + ["--path", str(out), "--min_dist_vis", "1.3e-3"], env=env, cwd=REPO, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "are not made here" not in run.stdout
    assert sorted(os.listdir(out / "imgs"), key=lambda f: int(f[:-4])) == ["%d.png" % i for i in range(600)]
    grey = P2.patch_bytes(subvol)
    for i in (0, 417):
        rgba = R.read_png(str(out / "imgs" / ("%d.png" % i)))
        assert rgba.shape == (12, 12, 4) and (rgba[:, :, 3] == 255).all()
        assert all(np.array_equal(rgba[:, :, c], grey[i]) for c in range(3))
        assert np.array_equal(grey[i], R.patch_bytes(subvol[i, 0]))
    pic, pic_l = R.read_png(str(out / "2d_visualization_out.png")), R.read_png(str(out / "2d_visualization_labels.png"))
    assert pic.shape == pic_l.shape == (256, 256, 3)
    shown = np.load(out / "plot_2d_shown.npz")
    assert int(shown["plot_size"]) == 256 and int(shown["thumb"]) == 32 and shown["min_dist_vis"] == np.float32(1.3e-3)
    y01, y01_l = np.load(out / "embeddings_2d.npz")["y01"], np.load(out / "embeddings_2d_labels.npz")["y01"]
    assert np.array_equal(shown["shown_idx"], R.select(y01, 1.3e-3))
    assert np.array_equal(shown["shown_idx_labels"], R.select(y01_l, 1.3e-3))
    idx = shown["shown_idx"]
    thumbs = P2.thumbnails(dev(subvol), dev(idx)).cpu().numpy()
    assert np.array_equal(pic, R.draw_out(y01, idx, thumbs, np.load(out / "all_colors.npy"), 256))
    plain = tmp_path / "plain"
    run = subprocess.run(base + ["--path", str(plain)], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "are not made here" in run.stdout
    assert not [f for f in os.listdir(plain) if f == "imgs" or f.startswith("2d_visualization") or f.startswith("plot_2d_shown")]
