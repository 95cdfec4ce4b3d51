"""Writes tests/golden/vis3d_small.npz: inputs of the vis3d tests and scipy's own outputs for the 8-bit Gaussian.

    python tests/golden/gen_golden_vis3d.py

scipy.ndimage.gaussian_filter (scipy 1.15.3 when this file was written) is the oracle of the filter; everything else is
input data made from seeds here.  Nothing comes from the reference's program text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vis3d_ref as R  # noqa: E402

# (Z, R, C): the issue's four, then the edges of the kernels' own forms - the word-wide form (C a multiple of 4) with no
# interior word (C = 4), one interior word between two border words (C = 12), and every axis shorter than the radius
GAUSS_SHAPES = [(7, 20, 37), (2, 9, 8), (1, 4, 3), (9, 33, 64), (3, 5, 12), (2, 2, 4)]
CONST_LEVELS = [0, 1, 200, 255]
CONST_SHAPES = [(3, 4, 5), (2, 3, 8)]                      # byte-wide and word-wide form
CHAIN_SHAPE = (8, 24, 20)
CHAIN_CONFIGS = [("zxy", False), ("zxy", True), ("xzy", False), ("xzy", True)]
CHAIN_MARGIN, CHAIN_SHARE = 1e-3, 0.01
PAINT_SHAPE = (6, 40, 44)


def chain_file_block(vol, order):
    """The MRC data block whose reorder is `vol` (Z, R, C)."""
    return np.ascontiguousarray(vol if order == "zxy" else np.transpose(vol, (1, 0, 2)))


def chain_volume(seed):
    rng = np.random.RandomState(seed)
    z, r, c = CHAIN_SHAPE
    vol = rng.standard_normal(CHAIN_SHAPE) * 40.0 + 100.0
    zz, rr, cc = np.meshgrid(np.arange(z), np.arange(r), np.arange(c), indexing="ij")
    for _ in range(6):                                     # a few dark blobs on the noise, as particles are
        cz, cr, c_c = rng.uniform(0, z), rng.uniform(0, r), rng.uniform(0, c)
        vol -= 120.0 * np.exp(-((zz - cz) ** 2 / 4.0 + (rr - cr) ** 2 / 9.0 + (cc - c_c) ** 2 / 9.0))
    vol[6:8] = 17.25                                       # two slices of zero variance (one pair under --compress)
    return vol.astype(np.float32)


def chain_excluded(vol):
    """The largest share, over the four configurations, of voxels whose restated level is within the margin of a half-integer."""
    worst = 0.0
    for order, compress in CHAIN_CONFIGS:
        _, level = R.volume_chain(R.reorder(chain_file_block(vol, order), order, compress))
        worst = max(worst, float(np.mean(np.abs(level - np.floor(level) - 0.5) <= CHAIN_MARGIN)))
    return worst


def paint_input():
    """About 30 picks of 'tomoA' on (6, 40, 44), with picks of 'tomoB' between them, and a colour per pick."""
    a = [  # x (column), y (row), z
        (2.0, 20.0, 0), (41.9, 18.2, 0), (22.5, 1.7, 1), (20.3, 38.9, 1),          # clipped by the four borders
        (-5.0, 10.0, 1), (50.7, 30.2, 3), (10.0, -9.5, 5), (25.0, 49.0, 5),          # centres outside the image
        (-30.0, -30.0, 3),                                                           # far outside: paints nothing
        (20.0, 20.0, 3), (24.6, 22.4, 3), (22.2, 17.9, 3), (20.0, 20.0, 3),          # overlap on one slice: the order decides
        (21.0, 21.0, 5), (19.0, 19.5, 1),                                            # overlap from two slices away
        (30.5, 30.5, 0), (31.5, 29.5, 1),                                            # slice 2 is in reach of these, but holds
        (8.9, 30.1, 3), (9.9, 31.1, 3),                                              # no pick: it stays zero
        (35.0, 8.0, 5), (36.99, 8.99, 5), (5.01, 5.99, 5), (0.0, 0.0, 0), (43.0, 39.0, 5),
        (43.999, 39.999, 0), (-0.9, -0.9, 1), (12.0, 12.0, 0), (12.0, 12.0, 1), (12.0, 12.0, 3), (12.0, 12.0, 5),
    ]
    b = [(20.0, 20.0, 2), (10.0, 10.0, 4), (30.0, 30.0, 3), (20.5, 20.5, 3)]       # another tomogram: ignored (slices 2, 4!)
    names, coords = [], []
    for i, p in enumerate(a):
        names.append("tomoA"); coords.append(p)
        if i % 8 == 3:
            names.append("tomoB"); coords.append(b[i // 8])
    rng = np.random.RandomState(5)
    colours = rng.randint(1, 256, size=(len(names), 3)).astype(np.uint8)
    return np.array(names), np.array(coords, np.float64), colours


def colour_input():
    rng = np.random.RandomState(11)
    y = rng.uniform(0, 1, size=(1000, 2)).astype(np.float32)
    eighths = (2 * np.arange(8) + 1) / 16.0                # exact halves of x 8 and of x 4 (every second one): ties
    ties = np.array([(a, b) for a in eighths for b in eighths], np.float32)
    edge = np.array([(0, 0), (1, 1), (0, 1), (1, 0), (-1e-3, 0.5), (0.5, 1.001), (-0.2, 1.3), (1.0 + 1e-7, -1e-7),
                     (0.0625, 0.125), (0.1875, 0.375)], np.float32)
    return np.concatenate([y, ties, edge]), rng.randint(0, 256, size=(7, 5, 3)).astype(np.uint8), \
        rng.randint(0, 256, size=(9, 5, 3)).astype(np.uint8)


def main():
    out = {}
    rng = np.random.RandomState(3)
    for i, shape in enumerate(GAUSS_SHAPES):
        vol = rng.randint(0, 256, size=shape).astype(np.uint8)
        if i == 0:
            vol[:, :4] = 255                                # saturated and empty patches next to the borders
            vol[:, -3:] = 0
        out["gauss_in_%d" % i], out["gauss_out_%d" % i] = vol, R.gaussian_scipy(vol)
    for j, shape in enumerate(CONST_SHAPES):
        for level in CONST_LEVELS:
            got = R.gaussian_scipy(np.full(shape, level, np.uint8))
            assert np.all(got == level), (shape, level)     # scipy keeps every level
            out["const_out_%d_%d" % (j, level)] = got
    out["const_shapes"], out["const_levels"] = np.array(CONST_SHAPES), np.array(CONST_LEVELS)

    seed = next(s for s in range(100) if chain_excluded(chain_volume(s)) <= CHAIN_SHARE)
    vol = chain_volume(seed)
    assert chain_excluded(vol) <= CHAIN_SHARE
    out["chain_vol"], out["chain_seed"] = vol, np.int32(seed)

    out["paint_name"], out["paint_coords"], out["paint_colours"] = paint_input()
    out["colour_y01"], out["colour_table_7x5"], out["colour_table_9x5"] = colour_input()
    path = os.path.join(HERE, "vis3d_small.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, chain seed %d (%.3f %% of the voxels within %g of a half level)"
          % (path, os.path.getsize(path), seed, 100 * chain_excluded(vol), CHAIN_MARGIN))


if __name__ == "__main__":
    main()
