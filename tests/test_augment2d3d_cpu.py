"""2d3d view augmentation, host side: the tests' numpy restatement of the chain (tests/augment2d3d_ref.py) against what PIL
makes of the same records (tests/golden/augment2d3d.npz, written by tests/golden/gen_golden_augment2d3d.py), the record
draw's ranges, the clipping rule of the erased rectangle, and the wrappers' refusal of host tensors."""
import math

import numpy as np
import pytest

import augment2d3d_ref as R


def fixture_records(z, b):
    return {k: z["%s_%d" % (k, b)] for k in R.FIELDS + ("weak", "kind")}


@pytest.mark.parametrize("bbox", [36, 12])
def test_restatement_reproduces_the_pil_fixture(golden, bbox):
    """Every pixel of both channels: the chain is a gather of 8-bit levels, so there is nothing to round."""
    z = golden("augment2d3d.npz")
    r = fixture_records(z, bbox)
    crops, views = z["crops_%d" % bbox], z["views_%d" % bbox]
    assert crops.shape == views.shape == (32, 2, bbox, bbox) and crops.dtype == views.dtype == np.uint8
    assert not np.array_equal(crops[:, 0], crops[:, 1])                     # a channel swap would show
    for half in (slice(0, 16), slice(16, 32)):                              # every flag combination with every k, twice
        assert len({(int(a), int(b), int(c)) for a, b, c in zip(r["hflip"][half], r["vflip"][half], r["k"][half])}) == 16
    assert set(r["kind"]) == {0, 1, 2, 3, 4} and r["weak"].sum() == 8
    assert [float(a) for a in r["angle"][:5]] == [-30.0, 30.0, 0.0, float(np.float32(1e-9)), float(np.float32(-1e-9))]
    for n in range(32):
        want = R.IDENTITY if r["weak"][n] else R.rotation_coefficients(r["angle"][n], bbox)
        assert list(r["coef"][n]) == list(want), n
        got = R.chain_levels(crops[n], *[r[k][n] for k in R.FIELDS if k != "angle"])
        assert np.array_equal(got, views[n]), (bbox, n, int(r["kind"][n]))
    assert list(R.rotation_coefficients(0.0, bbox)) == list(R.IDENTITY)


@pytest.mark.parametrize("bbox", [36, 12])
def test_fixture_rectangles_are_of_the_four_kinds(golden, bbox):
    z = golden("augment2d3d.npz")
    r = fixture_records(z, bbox)
    h_min, h_max, w_min, w_max = R.extent_bounds(bbox, R.STRONG)
    seen = set()
    for n in range(32):
        i, j, h, w = (int(r[f][n]) for f in "ijhw")
        i0, i1, j0, j1 = R.clip_rect(i, j, h, w, bbox)
        kind = int(r["kind"][n])
        assert bool(r["erase"][n]) == (kind > 0)
        if kind == 1:
            assert i + h <= bbox // 2 and j + w <= bbox // 2 and (i1 - i0, j1 - j0) == (h, w)
        elif kind == 2:
            assert i < bbox < i + h or j < bbox < j + w
            assert 0 < (i1 - i0) * (j1 - j0) < h * w
        elif kind == 3:
            assert i >= bbox and i1 == i0
        elif kind == 4:
            assert (h, w) in ((h_min, w_min), (h_max, w_max))
            seen.add((h, w))
    assert seen == {(h_min, w_min), (h_max, w_max)}


@pytest.mark.parametrize("bbox", [36, 12])
def test_clipping_rule_of_the_erased_rectangle(bbox):
    """[i, i + h) x [j, j + w) clipped to the image, as the slice assignment of F.erase clips it: against a brute-force mask
    over every start the reference's ranges allow and a few beyond."""
    h_min, h_max, w_min, w_max = R.extent_bounds(bbox, R.STRONG)
    for h, w in ((h_min, w_min), (h_max, w_max), (h_min, w_max)):
        starts_i = list(range(*R.corner_range(True, h, bbox))) + list(range(*R.corner_range(False, h, bbox))) + [bbox + 40]
        starts_j = list(range(*R.corner_range(True, w, bbox))) + list(range(*R.corner_range(False, w, bbox))) + [bbox + 40]
        for i in starts_i:
            for j in starts_j:
                mask = np.zeros((bbox, bbox), bool)
                mask[i:i + h, j:j + w] = True
                i0, i1, j0, j1 = R.clip_rect(i, j, h, w, bbox)
                want = np.zeros((bbox, bbox), bool)
                want[i0:i1, j0:j1] = True
                assert np.array_equal(mask, want), (i, j, h, w)
                assert 0 <= i0 <= i1 <= bbox and 0 <= j0 <= j1 <= bbox
    # the far side's last start lies outside the image for a small extent: bbox - e + 5 >= bbox for e <= 5
    assert R.corner_range(False, h_min, bbox)[1] - 1 >= bbox and R.clip_rect(bbox - h_min + 5, 0, h_min, 3, bbox)[:2] == (bbox, bbox)
    # a record from a caller: negative starts and sizes clip too
    assert R.clip_rect(-3, -50, 5, 20, bbox) == (0, 2, 0, 0) and R.clip_rect(2, 2, -1, 4, bbox)[:2] == (2, 2)


@pytest.mark.parametrize("view,bbox", [(0, 36), (1, 36), (0, 12), (1, 12)])
def test_draw_restatement_has_the_right_ranges(view, bbox):
    n = 20000
    p = R.draw_records(np.arange(n) * 5 + 3, 317, 1, view, bbox)
    mid = bbox // 2
    h_min, h_max, w_min, w_max = R.extent_bounds(bbox, R.STRONG)
    for f in ("hflip", "vflip", "erase"):
        assert set(np.unique(p[f])) == {0, 1} and abs(p[f].mean() - 0.5) <= 5 * math.sqrt(0.25 / n), f
    assert set(np.unique(p["k"])) == {0, 1, 2, 3}
    assert p["h"].min() >= h_min and p["h"].max() <= h_max and p["w"].min() >= w_min and p["w"].max() <= w_max
    assert p["h"].max() < mid and p["w"].max() < mid                        # CornerErasing's first try always passes
    for f, e, near in (("i", "h", "near_i"), ("j", "w", "near_j")):
        for side in (True, False):
            m = p[near] == side
            assert abs(m.mean() - 0.5) <= 5 * math.sqrt(0.25 / n)
            for ext in np.unique(p[e][m]):
                lo, hi = R.corner_range(side, int(ext), bbox)
                sel = p[f][m & (p[e] == ext)]
                assert sel.min() >= lo and sel.max() < hi, (f, side, ext)
    if view == 0:
        assert p["angle"].dtype == np.float32 and p["angle"].min() >= -30 and p["angle"].max() <= 30
        assert p["angle"].min() < -29.9 and p["angle"].max() > 29.9 and len(np.unique(p["coef"], axis=0)) > n // 2
    else:
        assert (p["angle"] == 0).all() and (p["coef"] == np.array(R.IDENTITY)).all()
    # the two views and the 2-D chain's stream draw different words for one sample
    q = R.draw_records(np.arange(n) * 5 + 3, 317, 1, 1 - view, bbox)
    assert abs((p["k"] == q["k"]).mean() - 0.25) < 0.02 and abs((p["hflip"] == q["hflip"]).mean() - 0.5) < 0.02


def test_table_layout_round_trip():
    rec = R.draw_records(np.arange(100), 317, 0, 0, 36)
    t = R.pack_params(**rec)
    assert t.shape == (100, 16) and t.dtype == np.int32
    back = R.unpack_params(t)
    for k in R.FIELDS:
        assert np.array_equal(back[k], rec[k]), k
    assert not back["reserved"].any() and not back["flag_rest"].any()


def test_wrappers_have_no_cpu_path():
    import torch
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    with pytest.raises(_lib.HipExtensionError):
        A.draw_params_2d3d(torch.arange(4), 317, 0, 36)
    bank = torch.zeros(4, 5, 36, 36)
    with pytest.raises(_lib.HipExtensionError):
        A.apply_2d3d(bank, bank, torch.arange(4), torch.ones(4, dtype=torch.int64), torch.zeros(2, 4, 16, dtype=torch.int32),
                     (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.HipExtensionError):
        A.PairViewAugmenter(bank, bank, (0.0, 0.0), (1.0, 1.0), 317)
    assert A.STRONG_RANGES_2D3D["angle"] == (-30.0, 30.0) and A.WEAK_RANGES_2D3D["angle"] == (0.0, 0.0)
    assert {k: v for k, v in A.STRONG_RANGES_2D3D.items() if k != "angle"} == {k: v for k, v in A.WEAK_RANGES_2D3D.items() if k != "angle"}
    assert A.STRONG_RANGES_2D3D == R.STRONG and A.WEAK_RANGES_2D3D == R.WEAK
