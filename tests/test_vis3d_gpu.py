"""csrc/vis3d.hip on the MI355X against scipy's own bytes (tests/golden/vis3d_small.npz) and the restatements of
tests/vis3d_ref.py: the 8-bit Gaussian bit for bit, the volume chain within the rule below, the painter and the colour
sampler exactly, and the two commands end to end as subprocesses.

Volume chain rule: bytes within 1 level of the float64 restatement everywhere, and equal wherever the restated level is
farther than 1e-3 from a half-integer.  The fp32 chain is estimated at <= 5e-5 level of error (values of order 1, 46 levels
per unit, 1e-6 relative); 1e-3 is 20 x that.  The fixture's generator asserts that at most 1 % of the voxels are excluded."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis3d_ref as R  # noqa: E402
from golden import gen_golden_vis3d as G  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec(golden):
    return golden("vis3d_small.npz")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", range(len(G.GAUSS_SHAPES)))
def test_gaussian_is_scipys_bit_for_bit(vec, case):
    from cet_pick_amd.utils import vis3d as V
    got = V.gaussian_u8(_dev(vec["gauss_in_%d" % case])).cpu().numpy()
    want = vec["gauss_out_%d" % case]
    print("gauss %s: %d of %d bytes differ" % (G.GAUSS_SHAPES[case], int((got != want).sum()), want.size))
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_gaussian_keeps_constant_levels(vec):
    from cet_pick_amd.utils import vis3d as V
    for j, shape in enumerate(G.CONST_SHAPES):
        for level in G.CONST_LEVELS:
            got = V.gaussian_u8(_dev(np.full(shape, level, np.uint8))).cpu().numpy()
            assert np.array_equal(got, vec["const_out_%d_%d" % (j, level)]), (shape, level, np.unique(got))


def test_gaussian_byte_form_on_an_unaligned_view(vec):
    """C a multiple of 4 but the input one byte off a word: the byte-wide form must run, and give the same bytes."""
    import torch
    from cet_pick_amd.utils import vis3d as V
    vol = vec["gauss_in_3"]
    buf = torch.empty(vol.size + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(vol.shape)
    view.copy_(_dev(vol))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    assert np.array_equal(V.gaussian_u8(view).cpu().numpy(), vec["gauss_out_3"])


def _chain_check(got, block, order, compress):
    want, level = R.volume_chain(R.reorder(block, order, compress))
    clear = np.abs(level - np.floor(level) - 0.5) > G.CHAIN_MARGIN
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print("chain %s compress=%s: %d bytes differ, %d of them clear of a half level, %.3f %% excluded, largest difference %d"
          % (order, compress, int((diff > 0).sum()), int(((diff > 0) & clear).sum()), 100 * (1 - clear.mean()), int(diff.max())))
    assert got.shape == want.shape and got.dtype == np.uint8
    assert 1 - clear.mean() <= G.CHAIN_SHARE
    assert diff.max() <= 1
    assert np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("order,compress", G.CHAIN_CONFIGS)
def test_volume_chain(vec, order, compress):
    from cet_pick_amd.utils import vis3d as V
    block = G.chain_file_block(vec["chain_vol"], order)
    vol = V.load_volume(block, order=order, compress=compress)
    assert tuple(vol.shape) == ((4 if compress else 8), 24, 20)
    got = V.volume_bytes(vol).cpu().numpy()
    _chain_check(got, block, order, compress)
    assert not got[-1].any() and got[0].std() > 20            # the slices of zero variance give 0


@pytest.mark.parametrize("budget", [1 << 30, 4 * 40 * 44 * 2])
def test_painter(vec, budget):
    """budget: the whole index image at once, and slabs of two painted slices (picks reach across the slab borders)."""
    from cet_pick_amd.utils import vis3d as V
    names, coords, colours = vec["paint_name"], vec["paint_coords"], vec["paint_colours"]
    rows, picks = V.tomogram_picks(coords, names, "tomoA", G.PAINT_SHAPE[0])
    got = V.paint(picks, colours[rows], G.PAINT_SHAPE, index_budget_bytes=budget).cpu().numpy()
    rows_r, picks_r = R.tomogram_picks(coords, names, "tomoA")
    want = R.paint(picks_r, colours[rows_r], G.PAINT_SHAPE)
    print("paint: %d of %d pixels differ" % (int((got != want).any(-1).sum()), want[..., 0].size))
    assert np.array_equal(got, want)
    assert not got[2].any() and not got[4].any()


def test_painter_byte_form():
    """C not a multiple of 4: the byte-wide paint pass."""
    from cet_pick_amd.utils import vis3d as V
    picks = np.array([[3, 4, 1], [30, 10, 1], [17, 9, 2], [18, 9, 0]], np.int32)
    colours = np.array([[1, 2, 3], [40, 50, 60], [255, 0, 7], [9, 9, 200]], np.uint8)
    got = V.paint(picks, colours, (4, 19, 35)).cpu().numpy()
    assert np.array_equal(got, R.paint(picks.astype(np.int64), colours, (4, 19, 35)))


def test_colours(vec, tmp_path):
    from cet_pick_amd.utils import vis3d as V
    y01 = vec["colour_y01"]
    assert len(y01) >= 1000
    np.save(tmp_path / "table.npy", vec["colour_table_9x5"])
    for table in (V.load_colormap(None), V.load_colormap(str(tmp_path / "table.npy")), vec["colour_table_7x5"]):
        got = V.sample_colours(_dev(y01), table).cpu().numpy()
        assert got.shape == (len(y01), 3) and got.dtype == np.uint8
        assert np.array_equal(got, R.sample_colours(y01, table)), table.shape


def _run(module, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], cwd=REPO, env=env, timeout=timeout,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_plot_2d_writes_the_colours(vec, tmp_path):
    rng = np.random.RandomState(2)
    pred = (rng.standard_normal((200, 16)) + 4.0 * rng.randint(0, 3, size=(200, 1))).astype(np.float32)
    names = np.array(["tomoA"] * 120 + ["tomoB"] * 80)
    np.savez(tmp_path / "all_output_info.npz", pred=pred, name=names, coords=rng.randint(0, 40, size=(200, 3)))
    np.save(tmp_path / "table.npy", vec["colour_table_9x5"])
    base = ["--input", tmp_path / "all_output_info.npz", "--n_cluster", 0, "--k", 8, "--niter", 5]
    out = _run("cet_pick_amd.plot_2d", base + ["--path", tmp_path / "plain", "--num_neighbor", 5])
    assert "are not made here" in out and "colour map" in out and not (tmp_path / "plain" / "all_colors.npy").exists()
    for sub, extra, table in (("map", [], R.default_colormap()),
                              ("file", ["--colormap", tmp_path / "table.npy"], vec["colour_table_9x5"])):
        out = _run("cet_pick_amd.plot_2d", base + ["--path", tmp_path / sub, "--mode", "tsne", "--num_neighbor", 5] + extra)
        colours = np.load(tmp_path / sub / "all_colors.npy")
        y01 = np.load(tmp_path / sub / "embeddings_2d.npz")["y01"]
        assert colours.shape == (200, 3) and colours.dtype == np.uint8
        assert np.array_equal(colours, R.sample_colours(y01, table))
        assert "all_colors.npy" in out and "colour map" not in out
        assert len(np.unique(colours, axis=0)) > 5


def _rec_check(rec, vol):
    """{name}_rec3d.npy by the chain's rule carried through the filter: a byte in front of the filter may differ from the
    restatement (by 1) only where the restated level is within the margin of a half-integer, and a voxel of the smoothed
    volume depends on the 7 x 7 x 7 voxels around it (each pass: a weighted mean with weights of sum 1, floored, so
    inputs that differ by at most 1 give outputs that differ by at most 1).  So: equal to scipy's filter of the restated
    bytes outside the 7 x 7 x 7 surroundings of those voxels, within 1 inside."""
    from scipy.ndimage import maximum_filter
    want, level = R.volume_chain(vol)
    doubt = np.abs(level - np.floor(level) - 0.5) <= G.CHAIN_MARGIN
    assert doubt.mean() <= G.CHAIN_SHARE
    near = maximum_filter(doubt, size=7, mode="constant", cval=False)
    smooth = R.gaussian_scipy(want)
    diff = np.abs(rec.astype(np.int64) - smooth.astype(np.int64))
    print("rec3d: %d voxels in doubt, %d bytes differ, largest difference %d" % (int(doubt.sum()), int((diff > 0).sum()), int(diff.max())))
    assert diff.max() <= 1 and not diff[~near].any()


def test_visualize_3dhm_end_to_end(tmp_path):
    from cet_pick_amd.utils import mrc
    rng = np.random.RandomState(4)
    blocks = {"tomoA": (rng.standard_normal((24, 8, 20)) * 30 + 5).astype(np.float32),      # xzy: (x, z, y) -> (8, 24, 20)
              "tomoB": (rng.standard_normal((21, 6, 26)) * 3 - 50).astype(np.float32)}      # -> (6, 21, 26)
    for name, b in blocks.items():
        mrc.write(str(tmp_path / (name + ".rec")), b)
        assert np.array_equal(mrc.open_data(str(tmp_path / (name + ".rec"))), b)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("image_name\trec_path\n" + "".join("%s\t%s\n" % (n, tmp_path / (n + ".rec")) for n in ("tomoA", "tomoB", "tomoC")))
    names = np.array(["tomoA"] * 12 + ["tomoB"] * 9 + ["tomoC"] * 2)
    coords = np.concatenate([rng.uniform(-3, 27, size=(23, 2)), rng.randint(0, 6, size=(23, 1))], 1)
    colours = rng.randint(1, 256, size=(23, 3)).astype(np.uint8)
    np.savez(tmp_path / "all_output_info.npz", name=names, coords=coords)
    np.save(tmp_path / "all_colors.npy", colours)
    common = ["--input", tmp_path / "all_output_info.npz", "--color", tmp_path / "all_colors.npy"]
    out = _run("cet_pick_amd.visualize_3dhm", common + ["--dir_simsiam", tmp_path / "out", "--image_txt", tmp_path / "list.txt"])
    assert "skipping 3D tomogram visualization for tomoC, file not found" in out
    assert not (tmp_path / "out" / "tomoC_rec3d.npy").exists()
    for name, b in blocks.items():
        vol = R.reorder(b, "xzy", False)
        rec, hm = np.load(tmp_path / "out" / (name + "_rec3d.npy")), np.load(tmp_path / "out" / (name + "_hm3d_simsiam.npy"))
        assert rec.shape == vol.shape + (3,) and hm.shape == rec.shape and rec.dtype == hm.dtype == np.uint8
        rows, picks = R.tomogram_picks(coords, names, name)
        assert np.array_equal(hm, R.paint(picks, colours[rows], vol.shape))
        _rec_check(rec, vol)
    # --rec_dir / --ext, --compress, another order: tomoB alone has a file with this extension
    mrc.write(str(tmp_path / "tomoB.mrc"), np.ascontiguousarray(np.transpose(blocks["tomoB"], (1, 0, 2))))
    half = np.concatenate([coords[:, :2], coords[:, 2:] // 2], 1)
    np.savez(tmp_path / "half.npz", name=names, coords=half)
    out = _run("cet_pick_amd.visualize_3dhm", ["--input", tmp_path / "half.npz", "--color", tmp_path / "all_colors.npy", "--dir_simsiam",
                                               tmp_path / "out2", "--rec_dir", tmp_path, "--ext", ".mrc", "--order", "zxy", "--compress"])
    assert out.count("file not found") == 2 and sorted(os.listdir(tmp_path / "out2")) == ["tomoB_hm3d_simsiam.npy", "tomoB_rec3d.npy"]
    vol = R.reorder(np.transpose(blocks["tomoB"], (1, 0, 2)), "zxy", True)
    rows, picks = R.tomogram_picks(half, names, "tomoB")
    assert vol.shape == (3, 21, 26)
    assert np.array_equal(np.load(tmp_path / "out2" / "tomoB_hm3d_simsiam.npy"), R.paint(picks, colours[rows], vol.shape))
    _rec_check(np.load(tmp_path / "out2" / "tomoB_rec3d.npy"), vol)
