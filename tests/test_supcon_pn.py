"""--pn on the host: the partner draws of `draw_pairs(pn=True)`, and the float64 restatements of `SupConLossV2_more`
(tests/supcon_pn_ref.py) against each other and against the reference's recorded values (tests/golden/supcon_pn_small.npz,
gen_golden_supcon_pn.py)."""
import numpy as np
import pytest
import torch

import supcon_pn_ref as R
from cet_pick_amd.datasets import semi_files as SF

SHAPE = (40, 128, 160)                    # (D, H, W): downscaled clip window x [17, 63], y [17, 47], z [3, 37]
BBOX, RATIO = 16, 0.5                     # tp = 8


def _annotations(n, rng):
    """n annotations of one tomogram far enough inside the clip window that no near-branch partner is clipped"""
    tp = int(BBOX * RATIO)
    return np.stack([rng.integers(17 + tp, 63 - tp + 1, n), rng.integers(17 + tp, 47 - tp + 1, n), rng.integers(3 + 5, 37 - 4 + 1, n),
                     np.zeros(n, np.int64)], 1)


def test_pn_false_table_is_the_one_drawn_without_the_argument():
    rng = np.random.default_rng(5)
    anns = _annotations(200, rng)
    for kw in (dict(), dict(rank=1, world=2, batch_size=4)):
        old = SF.draw_pairs(anns, [SHAPE], BBOX, RATIO, seed=3, epoch=2, **kw)
        new = SF.draw_pairs(anns, [SHAPE], BBOX, RATIO, seed=3, epoch=2, pn=False, **kw)
        for a, b in zip(old, new):
            assert np.array_equal(a, b)
        # pn=True draws after everything else: the same annotations, partners, own centres and flips
        o5 = SF.draw_pairs(anns, [SHAPE], BBOX, RATIO, seed=3, epoch=2, return_index=True, **kw)
        p6 = SF.draw_pairs(anns, [SHAPE], BBOX, RATIO, seed=3, epoch=2, return_index=True, pn=True, **kw)
        assert len(o5) == 5 and len(p6) == 6
        assert np.array_equal(o5[0], p6[0]) and np.array_equal(o5[2], p6[2])
        assert np.array_equal(o5[3], p6[3]) and np.array_equal(o5[4], p6[4])
        assert np.array_equal(o5[1][0::2], p6[1][0::2]) and not np.array_equal(o5[1][1::2], p6[1][1::2])


def test_pn_partner_draws():
    rng = np.random.default_rng(6)
    n, tp = 4000, int(BBOX * RATIO)
    anns = _annotations(n, rng)
    owner, centres, flip, a, b, anywhere = SF.draw_pairs(anns, [SHAPE], BBOX, RATIO, seed=9, epoch=1, return_index=True, pn=True)
    assert len(a) == n and anywhere.dtype == bool
    share = anywhere.mean()
    print("random-place share %.4f of %d" % (share, n))
    assert abs(share - 0.5) <= 0.03
    SF.check_windows(owner, centres, [SHAPE])
    D, H, W = SHAPE
    lo, hi = np.array([17, 17, 3]), np.array([W // 2 - 17, H // 2 - 17, D - 3])
    assert (centres >= lo).all() and (centres <= hi).all()
    par = centres[1::2].astype(np.int64)
    # the near branch: the partner's annotation + x, y in [-tp, tp), z in [-5, 5); nothing is clipped for these annotations
    off = par[~anywhere] - anns[b[~anywhere], :3]
    assert off[:, :2].min() == -tp and off[:, :2].max() == tp - 1
    assert off[:, 2].min() == -5 and off[:, 2].max() == 4
    # the random-place branch draws over the FULL-resolution extents: about half of x and y end on the upper clip, and z,
    # whose extent is not downscaled, covers its whole window
    far = par[anywhere]
    assert abs((far[:, 0] == hi[0]).mean() - (1 - hi[0] / W)) <= 0.04
    assert abs((far[:, 1] == hi[1]).mean() - (1 - hi[1] / H)) <= 0.04
    assert far[:, 2].min() == 3 and far[:, 2].max() == D - 3 and len(np.unique(far[:, 2])) == D - 5
    assert far[:, 0].min() == 17 and far[:, 1].min() == 17


def test_pn_draws_over_several_tomograms_stay_inside():
    shapes = np.array([(12, 96, 96), (30, 256, 200), (6, 68, 69)], np.int64)
    rng = np.random.default_rng(7)
    anns = np.concatenate([np.stack([rng.integers(0, s[2] // 2, 30), rng.integers(0, s[1] // 2, 30), rng.integers(0, s[0], 30),
                                     np.full(30, t)], 1) for t, s in enumerate(shapes)], 0)
    for epoch in range(4):
        owner, centres, _ = SF.draw_pairs(anns, shapes, 36, 0.5, seed=1, epoch=epoch, batch_size=2, pn=True)
        SF.check_windows(owner, centres, shapes)
        s = shapes[owner]
        assert (centres[:, 0] >= 17).all() and (centres[:, 0] <= s[:, 2] // 2 - 17).all()
        assert (centres[:, 1] >= 17).all() and (centres[:, 1] <= s[:, 1] // 2 - 17).all()
        assert (centres[:, 2] >= 3).all() and (centres[:, 2] <= s[:, 0] - 3).all()


@pytest.mark.parametrize("kind,thresh,T", [("binary", 0.85, 0.07), ("mixed", 0.85, 0.07), ("mixed", 0.3, 0.5), ("binary", 0.3, 0.07)])
def test_dense_form_equals_closed_form_and_its_gradient_pieces(kind, thresh, T):
    f, f_cr, lab = R.case_inputs(24, 16, thresh, kind)
    pos, un = R.masks(lab, thresh)
    assert pos.any() and un.any() and (kind == "binary" or int(pos.sum() + un.sum()) < 48)      # mixed: some labels equal thresh
    a, b = f.double().requires_grad_(), f_cr.double().requires_grad_()
    dense = R.dense_loss(a, b, lab, thresh, T)
    dense.backward()
    loss, pieces = R.closed_form(f.double(), f_cr.double(), lab, thresh, T)
    assert abs(float(dense.detach()) - float(loss)) <= 1e-12 * abs(float(loss))
    grad = torch.cat([a.grad, b.grad], 0)
    total = pieces[0] + pieces[1] + pieces[2]
    assert float((grad - total).abs().max()) <= 1e-12 * float(grad.abs().max())
    assert all(float(p.abs().max()) > 0 for p in pieces)


def test_restatement_reproduces_the_reference_fixture(golden):
    g = golden("supcon_pn_small.npz")
    assert int(g["cases"]) == 4
    for k in range(int(g["cases"])):
        f, f_cr, lab = (torch.as_tensor(g["%s_%d" % (n, k)]) for n in ("f", "f_cr", "labels"))
        assert f.shape == (48, 16) and f.dtype == torch.float32
        thresh, T, want = float(g["thresh_%d" % k]), float(g["T_%d" % k]), float(g["loss_%d" % k])
        assert abs(float(R.dense_loss(f.double(), f_cr.double(), lab, thresh, T)) - want) <= 1e-12 * abs(want), k
        assert abs(float(R.closed_form(f.double(), f_cr.double(), lab, thresh, T)[0]) - want) <= 1e-11 * abs(want), k
