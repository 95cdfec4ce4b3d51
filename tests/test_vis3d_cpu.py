"""Host side of the 3-D visualisation (no GPU): the restatements of tests/vis3d_ref.py against scipy and against the sampling
rule written out, the command line of cet_pick_amd.visualize_3dhm, and its refusals."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis3d_ref as R  # noqa: E402
from golden import gen_golden_vis3d as G  # noqa: E402


@pytest.fixture(scope="module")
def vec(golden):
    return golden("vis3d_small.npz")


@pytest.mark.parametrize("case", range(len(G.GAUSS_SHAPES)))
def test_restated_gaussian_is_scipys_bit_for_bit(vec, case):
    vol, want = vec["gauss_in_%d" % case], vec["gauss_out_%d" % case]
    assert vol.shape == G.GAUSS_SHAPES[case] and want.shape == vol.shape + (3,)
    assert np.array_equal(R.gaussian_scipy(vol), want)              # the fixture is what this scipy computes
    assert np.array_equal(R.gaussian_u8(vol), want)


def test_restated_gaussian_keeps_every_level(vec):
    for j, shape in enumerate(G.CONST_SHAPES):
        for level in range(256):
            want = vec["const_out_%d_%d" % (j, level)] if level in G.CONST_LEVELS else np.full(tuple(shape) + (3,), level, np.uint8)
            assert np.array_equal(R.gaussian_u8(np.full(shape, level, np.uint8)), want), (shape, level)


def test_product_weights_are_scipys():
    from scipy.ndimage import _filters
    from cet_pick_amd.utils import vis3d as V
    want = _filters._gaussian_kernel1d(0.8, 0, 3)
    assert np.array_equal(V.gaussian_weights(), want) and np.array_equal(R.gaussian_weights(), want)
    assert np.array_equal(want, want[::-1])


def test_sampler_restatement_is_the_rule_written_out(vec):
    y01, table = vec["colour_y01"], vec["colour_table_7x5"]
    assert table.shape == (7, 5, 3)
    got = R.sample_colours(y01, table)
    assert np.array_equal(got, R.sample_colours_direct(y01, table))
    # half-way positions go to the even index, positions outside [0, 1] to the border
    t = np.arange(7 * 5 * 3).reshape(7, 5, 3).astype(np.uint8)
    pick = lambda x, y: tuple(R.sample_colours(np.array([[x, y]], np.float32), t)[0])
    assert pick(0.0, 0.125) == tuple(t[0, 0]) and pick(0.0, 0.375) == tuple(t[0, 2]) and pick(0.0, 0.625) == tuple(t[0, 2])
    assert pick(-0.2, 1.3) == tuple(t[0, 4]) and pick(1.001, -1e-3) == tuple(t[6, 0])
    assert np.array_equal(R.default_colormap()[3, 250], [3, 250, 255 - 253 // 2])


def test_default_colormap_is_the_arithmetic_table():
    from cet_pick_amd.utils import vis3d as V
    t = V.default_colormap()
    assert t.shape == (256, 256, 3) and t.dtype == np.uint8 and np.array_equal(t, R.default_colormap())
    assert np.array_equal(V.load_colormap(None), t)


def test_chain_fixture_keeps_clear_of_half_levels(vec):
    vol = vec["chain_vol"]
    assert vol.shape == G.CHAIN_SHAPE and vol.dtype == np.float32
    assert np.array_equal(vol, G.chain_volume(int(vec["chain_seed"])))
    assert G.chain_excluded(vol) <= G.CHAIN_SHARE
    b, level = R.volume_chain(R.reorder(vol, "zxy", False))
    assert np.all(b[6:8] == 0) and b[:6].std() > 20                 # zero variance gives 0; the rest uses the byte range


def test_painter_restatement_on_the_fixture(vec):
    names, coords, colours = vec["paint_name"], vec["paint_coords"], vec["paint_colours"]
    rows, picks = R.tomogram_picks(coords, names, "tomoA")
    assert 28 <= len(rows) <= 32 and len(names) > len(rows)
    hm = R.paint(picks, colours[rows], G.PAINT_SHAPE)
    assert not hm[2].any() and not hm[4].any() and all(hm[s].any() for s in (0, 1, 3, 5))
    # (20, 20) on slice 3: picks 9..12 of tomoA overlap there and the last one of the input wins
    last = [i for i, p in enumerate(picks) if p[2] == 3 and (20 - p[0]) ** 2 + (20 - p[1]) ** 2 <= 144][-1]
    assert tuple(hm[3, 20, 20]) == tuple(colours[rows][last])
    from cet_pick_amd.utils import vis3d as V
    rows_p, picks_p = V.tomogram_picks(coords, names, "tomoA", G.PAINT_SHAPE[0])
    assert np.array_equal(rows_p, rows) and np.array_equal(picks_p, picks) and picks_p.dtype == np.int32


def test_command_line_of_the_reference():
    from cet_pick_amd import visualize_3dhm as M
    p = M.add_arguments(argparse.ArgumentParser())
    a = p.parse_args(["--input", "exp/simsiam2d3d/test_sample/all_output_info.npz", "--color", "exp/simsiam2d3d/test_sample/all_colors.npy",
                      "--dir_simsiam", "exp/simsiam2d3d/test_sample/", "--rec_dir", "sample_data/"])
    assert (a.order, a.ext, a.compress, a.image_txt, str(a.gpus)) == ("xzy", ".rec", False, None, "0")
    a = p.parse_args(["--input", "i.npz", "--color", "c.npy", "--dir_simsiam", "out", "--image_txt", "list.txt", "--compress",
                      "--order", "zxy", "--ext", ".mrc", "--gpus", "1"])
    assert (a.order, a.ext, a.compress, a.image_txt, str(a.gpus), a.rec_dir) == ("zxy", ".mrc", True, "list.txt", "1", None)


def test_cpu_mode_is_refused(tmp_path):
    from cet_pick_amd import visualize_3dhm as M
    a = M.add_arguments(argparse.ArgumentParser()).parse_args(["--input", str(tmp_path / "none.npz"), "--color", "c.npy",
                                                               "--dir_simsiam", str(tmp_path), "--rec_dir", ".", "--gpus", "-1"])
    with pytest.raises(RuntimeError, match="no CPU mode"):
        M.main(a)


def test_odd_z_with_compress_is_refused():
    from cet_pick_amd.utils import vis3d as V
    for order, shape in (("xzy", (6, 7, 5)), ("zxy", (7, 6, 5)), ("xyz", (6, 5, 7)), ("yxz", (6, 5, 7))):
        with pytest.raises(ValueError, match="even number of slices"):
            V.reordered_slices(shape, order, True)
        with pytest.raises(ValueError, match="even number of slices"):       # before any device work
            V.load_volume(np.zeros(shape, np.float32), order=order, compress=True)
        assert V.reordered_slices(shape, order, False) == 7
    assert V.reordered_slices((6, 8, 5), "xzy", True) == 4


def test_pick_outside_the_volume_is_refused():
    from cet_pick_amd.utils import vis3d as V
    names = np.array(["a", "b", "a"])
    for z in (-1, 6, 100):
        with pytest.raises(ValueError, match="outside the volume"):
            V.tomogram_picks(np.array([[1.5, 2.5, 0], [3, 3, 99], [4, 4, z]], np.float64), names, "a", 6)
    with pytest.raises(ValueError, match="outside the volume"):              # before any launch, on a box without a GPU too
        V.paint(np.array([[1, 1, 6]], np.int32), np.zeros((1, 3), np.uint8), (6, 8, 8))
    rows, picks = V.tomogram_picks(np.array([[1.9, -2.5, 0], [3, 3, 99], [4, 4, 5]], np.float64), names, "a", 6)
    assert rows.tolist() == [0, 2] and picks.tolist() == [[1, -2, 0], [4, 4, 5]]
    assert len(V.tomogram_picks(np.zeros((3, 3)), names, "c", 6)[0]) == 0
