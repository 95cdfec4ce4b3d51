"""The inputs of tests/test_loss_ops_gpu.py, checked from the float64 oracle alone (no GPU): no case of a data-dependent branch
sits where float32 could flip it, every label mix holds the classes its name claims, the range-decision inputs have the spreads
they state, and a float32 evaluation of each case is finite wherever the float64 one is."""
import numpy as np
import pytest
import torch

import loss_cases as C

F32, F64 = torch.float32, torch.float64


def _finite_where(a32, a64, what):
    a32, a64 = torch.as_tensor(a32), torch.as_tensor(a64)
    assert bool(torch.isfinite(a32)[torch.isfinite(a64)].all()), what


@pytest.mark.parametrize("n,mix", [(n, m) for n in C.MIX_SIZES for m in C.MIXES] + [(255, "standard"), (2049, "standard")])
def test_label_mixes_hold_what_they_claim(n, mix):
    gt = C.voxel_labels(mix, n)
    assert gt.dtype == F32 and gt.shape == (n,)
    masks = C.label_classes(gt)
    assert int(sum(m.sum() for m in masks)) == n
    for claim, m in zip(C.MIXES[mix], masks):
        assert (int(m.sum()) >= 2) if claim else (int(m.sum()) == 0), (mix, n, [int(m.sum()) for m in masks])
    if mix == "soft_edges":
        assert int((gt == 0).sum()) >= 2 and int(((gt > -1) & (gt < 0)).sum()) >= 2
        assert int(((gt < 1) & (gt >= 1 - 1e-3)).sum()) >= 2
    if mix == "all_soft":
        assert int((gt == 0).sum()) >= 2 and int((gt < 0).sum()) >= 2


@pytest.mark.parametrize("kind", C.PRED_KINDS)
@pytest.mark.parametrize("n", C.MIX_SIZES)
def test_predictions(n, kind):
    p = C.voxel_pred(kind, "standard", n)
    assert p.dtype == F32 and float(p.min()) >= C.P_LO and float(p.max()) <= C.P_HI
    if kind == "clamp_ends":
        assert int((p == C.P_LO).sum()) >= n // 10 and int((p == C.P_HI).sum()) >= n // 10


@pytest.mark.parametrize("n,mix,kind", C.PU_CASES)
def test_pu_branch_margins(n, mix, kind):
    """neg_total lies at least 10 % of |neg_total| + beta away from -beta, on the side the case states"""
    pred, gt = C.voxel_case(n, mix, kind)
    seen = set()
    for tau, beta, keep in C.pu_settings(n, mix, kind):
        _, neg_total = C.pu_terms(pred.double(), gt.double(), tau)
        neg_total = float(neg_total)
        assert (neg_total >= -beta) == keep, (tau, beta, neg_total)
        assert abs(neg_total + beta) >= 0.1 * (abs(neg_total) + beta), (tau, beta, neg_total)
        seen.add((tau, beta))
        if n != C.BIG:
            ref = C.pu_reference(n, mix, kind, tau, beta)
            _finite_where(ref[F32][0], ref[F64][0], "loss")
            _finite_where(ref[F32][1], ref[F64][1], "gradient")
            assert bool(torch.isfinite(ref[F64][0]))
    assert {t for t, _ in seen} == {0.05, 0.6} and {b for _, b in seen} == {0.0, 0.1}


@pytest.mark.parametrize("n", [n for n in C.N_SIZES if n > 1])
def test_size_sweep_branch_margin(n):
    pred, gt = C.size_case(n)
    tau, beta = C.SIZE_PU
    neg_total = float(C.pu_terms(pred.double(), gt.double(), tau)[1])
    assert neg_total >= -beta and abs(neg_total + beta) >= 0.1 * (abs(neg_total) + beta), neg_total


def test_pu_cases_reach_both_branches_at_every_size():
    for n in C.MIX_SIZES:
        keeps = {keep for n_, m, k in C.PU_CASES if n_ == n for _, _, keep in C.pu_settings(n, m, k)}
        assert keeps == {True, False}, n
    assert {(n, m) for n, m, _ in C.FOCAL_CASES} == {(n, m) for n in C.MIX_SIZES for m in C.MIXES}
    assert {(n, m) for n, m, _ in C.PU_CASES} == {(n, m) for n in C.MIX_SIZES for m in C.PU_MIXES}
    for n in C.MIX_SIZES:
        assert {k for n_, _, k in C.FOCAL_CASES if n_ == n} == set(C.PRED_KINDS)
        assert {k for n_, _, k in C.PU_CASES if n_ == n} == set(C.PRED_KINDS)


@pytest.mark.parametrize("n,mix,kind", [c for c in C.FOCAL_CASES if c[0] != C.BIG])
def test_focal_cases_are_finite(n, mix, kind):
    ref = C.focal_reference(n, mix, kind)
    assert bool(torch.isfinite(ref[F64][0])) and bool(torch.isfinite(ref[F64][1]).all())
    _finite_where(ref[F32][0], ref[F64][0], "loss")
    _finite_where(ref[F32][1], ref[F64][1], "gradient")


@pytest.mark.parametrize("dim", C.UCL_DIMS)
@pytest.mark.parametrize("n2", C.UCL_SIZES)
def test_ucl_cases(n2, dim):
    combos = C.ucl_combos(n2)
    assert {c[1] for c in combos} == set(C.CLASS_KINDS) and {c[2] for c in combos} == set(C.INV_TS)
    for fkind, ckind, inv_T in combos:
        f, cls, ref = C.ucl_reference(n2, dim, fkind, ckind, inv_T)
        assert f.shape == (n2, dim) and f.dtype == F32 and cls.dtype == torch.uint8
        h, m = n2 // 2, ref[F64][0]
        diag = (f.double() * f.double()).sum(1) * inv_T
        if fkind == "twin":                                # an off-diagonal element ties the maximum of rows 0 and 1
            assert torch.equal(f[0], f[1]) and h > 1 and float(m[0]) == float(m[1]) and abs(float(m[0] - diag[0])) <= 1e-12 * float(diag[0])
        if fkind == "same_views":
            assert torch.equal(f[:h], f[h:])
        if fkind == "zero_row":
            assert not bool(f[n2 - 1].any()) and float(m[n2 - 1]) == 0.0
        if fkind == "spread":
            norms = f.norm(dim=1)
            assert 0.49 < float(norms.min()) and float(norms.max()) < 2.01 and float(norms.max() / norms.min()) > (1.5 if n2 > 2 else 1.0)
        c = cls.long()
        if ckind == "all0":
            assert not bool(c.any())
        if ckind == "all3":
            assert bool((c == 3).all())
        if ckind == "bit0_first_half":
            assert bool(((c & 1) == (torch.arange(n2) < h).long()).all())
        for a32, a64 in zip(ref[F32], ref[F64]):
            assert bool(torch.isfinite(a64).all())
            _finite_where(a32, a64, (fkind, ckind, inv_T))


@pytest.mark.parametrize("n2", C.RANGE_SIZES)
@pytest.mark.parametrize("side", ["near", "far"])
def test_range_inputs_have_the_stated_spreads(side, n2):
    _, _, ref = C.range_case(side, n2)
    spread = C.rowmax_spread(ref[F64][0])
    assert C.RANGE_BOUND[side](spread), spread
    assert spread <= 12.0 if side == "near" else spread >= 20.0
    for a32, a64 in zip(ref[F32], ref[F64]):
        _finite_where(a32, a64, side)


@pytest.mark.parametrize("n,dim,thresh,kind", [c for c in C.TAIL_CASES if c[0] != 777 or c[3] in ("no_hi", "one_pos")])
def test_tail_cases(n, dim, thresh, kind):
    lab, o1, o2, f, f_cr = C.tail_case(n, dim, kind)
    sets = C.tail_sets(lab, o1, o2)
    for k, cnt in sets.items():
        assert (cnt == 0) if kind == "no_" + k else (cnt >= 2), (kind, sets)
    if kind == "one_pos":
        assert int((lab == 1).sum()) == 1
    assert int((lab == 1).sum()) >= 1 and f.shape == (n, dim)
    ref = C.tail_reference(n, dim, thresh, kind)
    assert all(bool(torch.isfinite(t).all()) for t in ref[F64][:2] + tuple(ref[F64][2]))
    for a32, a64 in zip(ref[F32][:2] + tuple(ref[F32][2]), ref[F64][:2] + tuple(ref[F64][2])):
        _finite_where(a32, a64, (n, dim, thresh, kind))
