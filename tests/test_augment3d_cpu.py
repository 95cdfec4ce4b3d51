"""The numpy restatement of the random 3-D views (tests/augment3d_ref.py) against scipy and against its own description;
the wrapper's geometry.  No GPU."""
import math

import numpy as np
import pytest

import augment3d_ref as R3

ANGLES = (0.0, 60.0, 37.5)                           # the angles test_augment3d_gpu.py rotates by
CROPS = (8, 16, 32)


def _box(S, seed):
    g = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(S),) * 3, indexing="ij")
    return g.normal(size=(S, S, S)) + 2.0 * np.sin(0.7 * z) * np.cos(0.4 * y + 0.3 * x)


def test_blur_equals_scipy_gaussian_filter():
    import scipy.ndimage as ndi
    g = np.random.default_rng(5)
    cases = [tuple(g.uniform(0, 1, 3)) for _ in range(6)] + [(0.1, 0.7, 0.99), (0.95, 0.124, 0.3), (0.0, 0.0, 0.5)]
    for S, sig in zip([10, 20, 42] * 3, cases):
        box = _box(S, S)
        want = ndi.gaussian_filter(box, sig)                   # torchio's call: mode reflect, truncate 4
        assert np.abs(R3.blur(box, sig) - want).max() <= 1e-12, sig


@pytest.mark.parametrize("c", CROPS)
def test_rotation_equals_scipy_map_coordinates_outside_the_band(c):
    import scipy.ndimage as ndi
    m, S, _, _ = R3.geometry(c)
    box = _box(S, c)
    for deg in ANGLES:
        th = np.float64(np.float32(deg)) * (np.pi / 180.0)
        cos, sin = np.float32(np.cos(th)), np.float32(np.sin(th))
        got, band = R3.rotate(box, cos, sin)
        fy, fx = R3.source_coords(S, cos, sin)
        want = np.stack([ndi.map_coordinates(p, [fy, fx], order=1, mode="constant", cval=box.min()) for p in box])
        keep = ~band
        assert np.abs(got - want)[:, keep].max() <= 1e-12, deg
        # the band holds few voxels (by area about 0.03 %), and no coordinate of these cases sits where single precision
        # could put it on the other side of the boundary
        share = band[m:m + c, m:m + c].mean()
        assert share <= 0.005, (deg, share)
        edge = np.minimum.reduce([np.abs(f - b) for f in (fy, fx) for b in (0.0, S - 1.0)])
        if deg != 0.0:
            assert edge.min() > 2e-5, (deg, edge.min())
    assert np.array_equal(R3.rotate(box, 1.0, 0.0)[0], box)


@pytest.mark.parametrize("c", CROPS)
def test_every_step_off_is_the_normalised_inner_crop(c):
    m, S, _, _ = R3.geometry(c)
    box = _box(S, 3 * c)
    got, mask = R3.chain(box, c, R3.record(c))
    x = box[m:m + c, m:m + c, m:m + c]
    x = (x - x.mean()) / x.std(ddof=1)
    x = (x - x.min()) / (x.max() - x.min()) * 6 - 3
    x = (x - x.mean()) / x.std(ddof=1)
    assert np.array_equal(got, x) and not mask.any()
    assert abs(got.mean()) < 1e-12 and abs(got.std(ddof=1) - 1) < 1e-12


def test_noise_is_standard_normal():
    n, sigma_n = 1 << 18, 0.2
    z = sigma_n * R3.normals(n, 0x1234ABCD, 0x0F0F0F0F)
    assert abs(z.mean()) <= 5 * sigma_n / math.sqrt(n)
    # variance of a normal sample: standard error sigma^2 sqrt(2 / (n - 1))
    assert abs(z.var(ddof=1) - sigma_n ** 2) <= 5 * sigma_n ** 2 * math.sqrt(2.0 / (n - 1))
    u = np.sort(np.array([0.5 * (1 + math.erf(v / (sigma_n * math.sqrt(2)))) for v in z]))
    ks = max(float((np.arange(1, n + 1) / n - u).max()), float((u - np.arange(n) / n).max()))
    assert ks < math.sqrt(math.log(2e6) / (2 * n)), ks
    assert not np.array_equal(z, sigma_n * R3.normals(n, 0x1234ABCD, 0x0F0F0F10))
    assert np.isfinite(z).all()


def test_erasure_corner_sets_and_small_crops():
    from cet_pick_amd.datasets import augment as A
    want = {8: [0, 1, 5, 6], 12: [0, 1, 8, 9], 16: [0, 1, 2, 3, 10, 11, 12, 13], 32: [0, 1, 2, 3, 4, 5, 21, 22, 23, 24, 25, 26]}
    for c, corners in want.items():
        m, S, e, q = A.geometry_3d(c)
        assert (m, S, e, q) == (c // 6, c + 2 * (c // 6), (c + 2 * (c // 6)) // 8, (c + 2 * (c // 6)) // 4) and S // 8 == m
        assert A.erase_corners_3d(c) == corners == R3.corner_set(c)
        assert all(k + e <= c for k in corners)
    assert A.geometry_3d(32)[:2] == (5, 42)
    for c in (2, 4, 7, 33, 34):
        with pytest.raises(ValueError):
            A.erase_corners_3d(c)


def test_flip_and_erasure_of_the_restatement():
    c = 16
    _, _, e, q = R3.geometry(c)
    x = np.arange(c ** 3, dtype=np.float64).reshape(c, c, c) + 1
    assert np.array_equal(R3.flip_erase(x, c, R3.FLIP_Z, 0, None, None), x[::-1])
    assert np.array_equal(R3.flip_erase(x, c, R3.FLIP_Y, 0, None, None), x[:, ::-1])
    d = R3.flip_erase(x, c, 0, R3.DROP, (1, 2, 10), None)
    assert (d == 0).sum() == e ** 3 and (d[1:1 + e, 2:2 + e, 10:10 + e] == 0).all()
    k = R3.flip_erase(x, c, 0, R3.CENTRE, None, None)
    assert np.array_equal(k[:, c // 2 - q:c // 2 + q, c // 2 - q:c // 2 + q], x[:, c // 2 - q:c // 2 + q, c // 2 - q:c // 2 + q])
    assert (k != 0).sum() == c * (2 * q) ** 2
    s = R3.flip_erase(x, c, 0, R3.SWAP, (0, 0, 0), (1, 1, 1))             # overlapping: box 1 is written last
    assert np.array_equal(s[1:1 + e, 1:1 + e, 1:1 + e], x[0:e, 0:e, 0:e]) and s[0, 0, 0] == x[1, 1, 1]
