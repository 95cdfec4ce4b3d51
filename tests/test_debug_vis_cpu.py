"""Host side of the validation pictures (no GPU): the restatements of tests/debug_vis_ref.py against the properties they must
have, the detection-table writer against a hand-written file, and the ground-truth shift of the validation window."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_vis_ref as R  # noqa: E402


def test_ring_mask_of_radius_8():
    pts = R.ring_offsets(8)
    m = R.ring_mask(8)
    assert m.shape == (17, 17) and int(m.sum()) == len(pts)
    # the eight reflections
    for t in (m[::-1], m[:, ::-1], m[::-1, ::-1], m.T, m.T[::-1], m.T[:, ::-1], m.T[::-1, ::-1]):
        assert np.array_equal(m, t)
    for dx, dy in ((8, 0), (-8, 0), (0, 8), (0, -8)):
        assert (dx, dy) in pts and m[dy + 8, dx + 8]
    assert max(max(abs(dx), abs(dy)) for dx, dy in pts) == 8
    # no gaps: walking the first octant from (8, 0) up to the diagonal every step moves by one pixel at most in x and y,
    # and every pixel of the ring has exactly two ring neighbours or more (a closed 8-connected curve)
    octant = sorted((p for p in pts if p[0] >= p[1] >= 0), key=lambda p: p[1])
    assert octant[0] == (8, 0) and len({p[1] for p in octant}) == len(octant)
    for a, b in zip(octant, octant[1:]):
        assert b[1] - a[1] == 1 and 0 <= a[0] - b[0] <= 1
    assert octant[-1][0] - octant[-1][1] <= 1
    for dx, dy in pts:
        assert sum((dx + i, dy + j) in pts for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)) >= 2
    # every pixel is within half a pixel's diagonal of the circle
    assert all(abs(np.hypot(dx, dy) - 8) < 0.75 for dx, dy in pts)


def test_upsampling_keeps_a_constant_and_a_ramp_monotone():
    for c in (0, 1, 137, 255):
        assert np.array_equal(R.upsample2x(np.full((5, 7), c)), np.full((10, 14), c))
    ramp = np.tile(np.arange(0, 240, 20), (4, 1))
    up = R.upsample2x(ramp)
    assert up.shape == (8, 24) and (np.diff(up, axis=1) >= 0).all() and (up == up[0]).all()
    assert up[0, 0] == 0 and up[0, -1] == 220 and up.min() >= 0 and up.max() <= 255
    # the weights: one step of 16 between two source pixels gives 4 and 12 at the two output pixels between their centres
    assert R.upsample2x(np.array([[0, 16]])).tolist() == [[0, 4, 12, 16]] * 2


def test_blend_and_bytes_at_the_ends():
    assert R.blend(np.array([0, 255]), np.array([0, 255])).tolist() == [0, 255]
    assert R.blend(np.array([255, 0]), np.array([0, 255])).tolist() == [int(255 * (1.0 - 0.7)), int(255 * 0.7)]
    one_below = np.nextafter(np.float32(1), np.float32(0))
    assert R.unit_bytes(np.array([0.0, 1.0, one_below, -0.5, 2.0], np.float32)).tolist() == [0, 255, 254, 0, 255]
    assert R.grey_slice(np.full((3, 4), 2.5, np.float32)).tolist() == [[0] * 4] * 3
    g = R.grey_slice(np.array([[-1.0, 0.0], [1.0, 3.0]], np.float32))
    assert g.tolist() == [[0, 63], [127, 255]]


def test_detection_table_equals_a_hand_written_file(tmp_path):
    from cet_pick_amd.utils.debug_vis import write_detection_table
    post = {3: [[10.0, 20.5, 3.0, 0.9, 0.9],              # x, y, z, score, conf: columns come out as x, z, y, score
                [11.9, 7.0, 3.0, 0.5, 0.3],               # conf == 0.3: left out
                [12.0, 7.0, 3.0, 0.25, 0.30000001]],
            7: [[0.5, 99.75, 7.25, 0.75, 0.75]]}          # fractional y and z are floored, x truncated
    path = tmp_path / "tomo_0.txt"
    write_detection_table(str(path), post)
    assert path.read_text() == "10\t3\t20\t0.9\n12\t3\t7\t0.25\n0\t7\t99\t0.75\n"
    write_detection_table(str(path), {})
    assert path.read_text() == ""


def test_gt_det_is_shifted_into_the_val_window_and_filtered():
    from cet_pick_amd.datasets.semi_files import val_window, window_gt_det
    shape = (110, 600, 600)                               # the sub-window rule applies: labels [0:110, 100:300, 100:300]
    wi, wl = val_window(shape)
    assert (wl[1].start, wl[2].start) == (100, 100)
    c = np.array([[100, 100, 0],                          # the window's first voxel
                  [299, 299, 109],                        # its last (the label volume is 300 wide: slice(100, 350) ends there)
                  [99, 150, 5], [150, 99, 5],             # left of / above the window
                  [300, 150, 5],                          # past the label volume
                  [150, 160, 110],                        # below the last slice
                  [180, 120, 40]], np.int64)
    got = window_gt_det(c, shape)
    assert got.dtype == np.float32 and got.tolist() == [[0, 0, 0], [199, 199, 109], [80, 20, 40]]
    # a tomogram without the sub-window keeps its centres
    assert window_gt_det([[5, 6, 7], [40, 36, 7]], (44, 72, 72)).tolist() == [[5, 6, 7]]
    assert window_gt_det(np.zeros((0, 3)), shape).shape == (0, 3)
    # D >= 100 and wide enough for the whole window
    got = window_gt_det([[349, 100, 109], [350, 100, 0]], (128, 720, 720))
    assert got.tolist() == [[249, 0, 109]]
