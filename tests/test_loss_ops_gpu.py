"""The kernels of csrc/loss_ops.hip - the voxel losses (focal, PU, MSE), the contrastive row sums with their four backward forms and
the range decision between them - and the tail of UnbiasedConLoss, each against a plain float64 evaluation of the same operation
(oracle/loss_ref.py, or the dense restatement in tests/loss_cases.py), at sizes taken from the kernels' own constants: below and
past a workgroup, ragged last blocks, past both grid caps, 2N below one row block, pairs that straddle column tiles.

Numeric results go through conftest.f32_equivalent (the GPU may lie as far from float64 as `factor` x a CPU float32 evaluation of
the same formula does, plus the default floor); counts, copies and selects are compared exactly.  tests/test_loss_inputs_cpu.py
checks the cases themselves (branch margins, class counts, spreads) from the float64 oracle alone.

Factors.  The voxel losses keep f32_equivalent's 2.  The contrastive groups do not fit it: the kernels form their products from
bf16x3 cuts of operands scaled by sqrt(log2(e) / T) and exponentiate with the hardware exp2, and at the smallest sizes a CPU float32
matmul is nearly exact.  Measured over all cases, as norm-relative errors against float64 (GPU, CPU float32, largest GPU / CPU
ratio among results above the 2e-6 floor):
    ucl_sums   3.1e-06   2.5e-06    5.4     factor 16
    ucl_grad   2.7e-06   2.9e-06   12.2     factor 32
    ucl_tail   9.3e-06   1.2e-05    5.9     factor 16
    focal 2.8e-07 / 3.0e-07, pu 3.1e-07 / 2.9e-07, mse 8.3e-08 / 1.1e-07: factor 2
(each factor: twice the ratio, rounded up to a power of two).  Whatever the factor, no row sum is accepted further than rtol 2e-4
from float64, and the row maxima are held to 1e-5."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_cases as C

pytestmark = pytest.mark.gpu

ERRORS = {}                                # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64, largest ratio]
F32, F64 = torch.float32, torch.float64
UCL_FACTOR = {"ucl_sums": 16.0, "ucl_grad": 32.0, "ucl_tail": 16.0}       # (the module docstring has the figures)
ROW_RTOL = 2e-4                            # no row sum is accepted further than this from float64, whatever the factor


def _ML():
    from cet_pick_amd.models import loss as ML
    return ML


def _err():
    from cet_pick_amd._lib import HipExtensionError
    return HipExtensionError


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _eq(group, got, cpu32, ref64, what, factor=2.0):
    from conftest import f32_equivalent
    g, c, r = (np.asarray(_np(t), np.float64).ravel() for t in (got, cpu32, ref64))
    scale = float(np.linalg.norm(r)) + 1e-30
    e_g, e_c = float(np.linalg.norm(g - r)) / scale, float(np.linalg.norm(c - r)) / scale
    print("%-10s %-64s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    rec = ERRORS.setdefault(group, [0.0, 0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e_g), max(rec[1], e_c)
    if e_g > 2e-6:                                         # (below the floor the ratio says nothing)
        rec[2] = max(rec[2], e_g / max(e_c, 1e-30))
    f32_equivalent(g, c, r, factor=factor, what=what)
    return e_g, e_c


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, (e_g, e_c, ratio) in sorted(ERRORS.items()):
        print("\nlargest error, %-10s GPU %.3e  CPU fp32 %.3e  largest GPU / CPU ratio above the floor %.2f" % (group, e_g, e_c, ratio))


# ------------------------------------------------------------------------------------------------
# 1. voxel losses
# ------------------------------------------------------------------------------------------------
def _run_voxel(module, pred, gt):
    """one evaluation on the GPU: (loss, d(UPSTREAM x loss)/d pred, the kernel's sums)"""
    p = pred.cuda().requires_grad_(True)
    loss = module(p, gt.cuda())
    sums = loss.grad_fn.sums
    (C.UPSTREAM * loss).backward()
    return loss.detach(), p.grad, sums.clone()


def _check_voxel(group, module, pred, gt, ref, what, keep=None):
    loss, grad, sums = _run_voxel(module, pred, gt)
    (l32, g32), (l64, g64) = ref[F32], ref[F64]
    n = pred.numel()
    masks = C.label_classes(gt)
    assert [float(s) for s in sums[:3].cpu()] == [float(m.sum()) for m in masks], what + ": class counts"
    assert float(sums[10]) == float(n)
    if keep is not None:
        assert float(sums[9]) == float(keep), what + ": the kernel took the other branch of the negative risk"
    _eq(group, loss, l32, l64, what + " loss")
    assert grad.shape == pred.shape
    grad = grad.cpu()
    _eq(group, grad, g32, g64, what + " dpred")
    # a positive voxel's gradient is about nu / np times an unlabeled one's: a wrong coefficient of one class vanishes in the whole norm
    for name, m in zip(("pos", "soft", "unl"), masks):
        if not bool(m.any()):
            continue
        if not bool(g64[m].any()):                         # (focal's unlabeled voxels, PU's when the negative risk is dropped)
            assert not bool(grad[m].any()), what + ": dpred is not zero on the %s voxels" % name
        else:
            _eq(group, grad[m], g32[m], g64[m], what + " dpred[%s]" % name)
    # the deterministic tree: a second evaluation gives the same bits
    loss2, grad2, sums2 = _run_voxel(module, pred, gt)
    assert torch.equal(loss, loss2) and torch.equal(grad2.cpu(), grad) and torch.equal(sums, sums2), what + ": not deterministic"


@pytest.mark.parametrize("n,mix,kind", C.FOCAL_CASES)
def test_focal(n, mix, kind):
    pred, gt = C.voxel_case(n, mix, kind)
    _check_voxel("focal", _ML().FocalLoss(), pred, gt, C.focal_reference(n, mix, kind), "focal n=%d %s %s" % (n, mix, kind))


@pytest.mark.parametrize("n,mix,kind", C.PU_CASES)
def test_pu(n, mix, kind):
    pred, gt = C.voxel_case(n, mix, kind)
    for tau, beta, keep in C.pu_settings(n, mix, kind):
        ref = C.pu_reference(n, mix, kind, tau, beta)
        # the float64 reference took the branch this case is about
        pos_risk, neg_total = C.pu_terms(pred.double(), gt.double(), tau)
        assert bool(neg_total >= -beta) == keep
        np.testing.assert_allclose(float(ref[F64][0]), float(pos_risk + neg_total if keep else pos_risk), rtol=1e-12)
        _check_voxel("pu", _ML().PULoss(tau, beta), pred, gt, ref, "pu n=%d %s %s tau=%g beta=%g" % (n, mix, kind, tau, beta), keep=keep)


@pytest.mark.parametrize("n", C.MIX_SIZES)
@pytest.mark.parametrize("mix", ["no_pos", "all_soft"])
def test_pu_without_positives_raises(n, mix):
    from oracle import loss_ref as O
    pred, gt = C.voxel_case(n, mix, "uniform")
    with pytest.raises(ValueError):
        O.pu_neg_loss(pred.double(), gt.double(), 0.05)
    with pytest.raises(ValueError):
        _ML().PULoss(0.05)(pred.cuda(), gt.cuda())


@pytest.mark.parametrize("n", C.N_SIZES)
def test_voxel_sizes(n):
    from oracle import loss_ref as O
    pred, gt = C.size_case(n)
    ref = lambda fn: {dt: C._with_grad(lambda p: fn(p, gt.to(dt)), pred, dt) for dt in (F32, F64)}
    _check_voxel("focal", _ML().FocalLoss(), pred, gt, ref(O.neg_loss), "focal n=%d" % n)
    if n > 1:
        tau, beta = C.SIZE_PU
        assert float(C.pu_terms(pred.double(), gt.double(), tau)[1]) >= -beta
        _check_voxel("pu", _ML().PULoss(tau, beta), pred, gt, ref(lambda p, g: O.pu_neg_loss(p, g, tau, beta)), "pu n=%d" % n, keep=True)


def test_pu_without_unlabeled_is_nan():
    """nu = 0: the reference's negative risk is 0 / 0 and its loss NaN; the kernel's is too.  (The gradient is unspecified:
    PULoss's docstring.)"""
    from oracle import loss_ref as O
    n = C.RAGGED
    pred, gt = C.voxel_case(n, "standard", "uniform")
    gt = torch.where(gt == -1, torch.zeros_like(gt), gt)
    assert bool(torch.isnan(O.pu_neg_loss(pred.double(), gt.double(), 0.6)))
    p = pred.cuda().requires_grad_(True)
    loss = _ML().PULoss(0.6)(p, gt.cuda())
    assert bool(torch.isnan(loss))
    assert float(loss.grad_fn.sums[2]) == 0.0


@pytest.mark.parametrize("n,offset", [(n, 0.0) for n in C.N_SIZES] + [(257, 1e3), (C.BIG, 1e3)])       # 1e3: the difference cancels
def test_mse(n, offset):
    a, b = C.mse_case(n, offset)
    ref = C.mse_reference(a, b)
    (l32, da32, db32), (l64, da64, db64) = ref[F32], ref[F64]
    what = "mse n=%d offset=%g" % (n, offset)
    results = []
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        x, y = a.cuda().requires_grad_(need_a), b.cuda().requires_grad_(need_b)
        loss = _ML().ConsistencyLoss()(x, y)
        sums = loss.grad_fn.sums
        (C.UPSTREAM * loss).backward()
        assert float(sums[10]) == float(n) and not bool(sums[:3].any())
        _eq("mse", loss, l32, l64, what + " loss")
        assert (x.grad is not None) == need_a and (y.grad is not None) == need_b
        if need_a:
            _eq("mse", x.grad, da32, da64, what + " da (a=%s b=%s)" % (need_a, need_b))
        if need_b:
            _eq("mse", y.grad, db32, db64, what + " db (a=%s b=%s)" % (need_a, need_b))
        results.append((loss.detach(), x.grad, y.grad))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][0], results[2][0])
    assert torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[2][2])
    assert torch.equal(results[0][2], -results[0][1])


def test_voxel_plumbing():
    """pred (2, 1, D, H, W) against gt (2, D, H, W), and a permuted view as pred: the gradient comes back in pred's shape."""
    from oracle import loss_ref as O
    d, h, w = 3, 5, 7
    n = 2 * d * h * w
    flat_pred, flat_gt = C.voxel_case(n, "standard", "uniform")
    gt = flat_gt.view(2, d, h, w)
    base = flat_pred.view(2, 1, d, h, w).permute(4, 1, 3, 2, 0).contiguous()          # (W, 1, H, D, 2) in memory
    for tag, make in (("contiguous", lambda t: t.permute(4, 1, 3, 2, 0).contiguous()), ("permuted view", lambda t: t.permute(4, 1, 3, 2, 0))):
        for name, module, fn in (("focal", _ML().FocalLoss(), O.neg_loss), ("pu", _ML().PULoss(0.6, 0.1), lambda p, g: O.pu_neg_loss(p, g, 0.6, 0.1))):
            ref = {dt: C._with_grad(lambda p: fn(p, flat_gt.to(dt)), flat_pred, dt) for dt in (F32, F64)}
            leaf = base.cuda().requires_grad_(True)
            pred = make(leaf)
            assert pred.shape == (2, 1, d, h, w) and pred.is_contiguous() == (tag == "contiguous")
            loss = module(pred, gt.cuda())
            (C.UPSTREAM * loss).backward()
            what = "%s, %s pred" % (name, tag)
            _eq(name, loss, ref[F32][0], ref[F64][0], what + " loss")
            assert leaf.grad.shape == base.shape
            got = leaf.grad.permute(4, 1, 3, 2, 0).reshape(-1)      # back to pred's logical order
            _eq(name, got, ref[F32][1], ref[F64][1], what + " dpred")
    with pytest.raises(ValueError, match=r"\(2, 1, 3, 5, 7\).*\(2, 3, 5, 6\)"):
        _ML().FocalLoss()(base.permute(4, 1, 3, 2, 0).cuda(), gt[..., :6].cuda())


# ------------------------------------------------------------------------------------------------
# 2. contrastive row sums
# ------------------------------------------------------------------------------------------------
FORMS = {"default": None, "two_exp": "MI_UCL_BWD_TWO_EXP", "split": "MI_UCL_BWD_SPLIT"}
SUM_NAMES = ("s_all", "s_pos", "s_other", "e_pair")
SUM_ATOL = (0.0, 1e-6, 1e-6, 1e-7)         # (as tests/test_losses_gpu.py: a class sum may be a few tiny terms, a pair element exp(-50))


def _ucl_run(f, cls, inv_T, gouts, form, monkeypatch):
    """(outputs, dfeat) of one forward and backward under one backward form; gouts[k] None: that output takes no part"""
    from cet_pick_amd.models.loss import _UclRowSumsFn
    for env in ("MI_UCL_BWD_TWO_EXP", "MI_UCL_BWD_SPLIT"):
        monkeypatch.delenv(env, raising=False)
    if FORMS[form]:
        monkeypatch.setenv(FORMS[form], "1")
    fa = f.cuda().requires_grad_(True)
    outs = _UclRowSumsFn.apply(fa, cls.cuda(), inv_T)
    used = [(o, g.cuda()) for o, g in zip(outs[1:], gouts) if g is not None]
    torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    torch.cuda.synchronize()
    for env in ("MI_UCL_BWD_TWO_EXP", "MI_UCL_BWD_SPLIT"):
        monkeypatch.delenv(env, raising=False)
    return [o.detach().cpu() for o in outs], fa.grad.cpu()


def _check_ucl_forward(outs, ref, what):
    r32, r64 = ref[F32], ref[F64]
    assert all(bool(torch.isfinite(o).all()) for o in outs), what + ": not finite"
    np.testing.assert_allclose(_np(outs[0]), _np(r64[0]), rtol=1e-5, atol=1e-30, err_msg=what + " rowmax")
    for k, name in enumerate(SUM_NAMES):
        _eq("ucl_sums", outs[1 + k], r32[1 + k], r64[1 + k], what + " " + name, factor=UCL_FACTOR["ucl_sums"])
        np.testing.assert_allclose(_np(outs[1 + k]), _np(r64[1 + k]), rtol=ROW_RTOL, atol=SUM_ATOL[k], err_msg=what + " " + name)


@pytest.mark.parametrize("dim", C.UCL_DIMS)
@pytest.mark.parametrize("n2", C.UCL_SIZES)
def test_ucl_rowsums(n2, dim, monkeypatch):
    gouts = C.ucl_gouts(n2)
    for fkind, ckind, inv_T in C.ucl_combos(n2):
        f, cls, ref = C.ucl_reference(n2, dim, fkind, ckind, inv_T)
        what = "ucl 2N=%d dim=%d %s %s 1/T=%.3g" % (n2, dim, fkind, ckind, inv_T)
        for form in FORMS:
            outs, grad = _ucl_run(f, cls, inv_T, gouts, form, monkeypatch)
            if form == "default":
                _check_ucl_forward(outs, ref, what)
                if fkind == "same_views":                  # the pair element of identical views is exp(0) - unless another row is larger
                    on_diag = torch.isclose(ref[F64][0], (f.double() * f.double()).sum(1) * inv_T, rtol=1e-12, atol=0)
                    assert bool((outs[4][on_diag] == 1.0).all()), what + ": e_pair of identical views"
            assert bool(torch.isfinite(grad).all()), what + " " + form + ": dfeat not finite"
            _eq("ucl_grad", grad, ref[F32][5], ref[F64][5], what + " dfeat " + form, factor=UCL_FACTOR["ucl_grad"])


@pytest.mark.parametrize("dim", C.UCL_DIMS)
@pytest.mark.parametrize("only", range(4), ids=SUM_NAMES)
def test_ucl_backward_of_one_output(only, dim, monkeypatch):
    """three of the four upstream gradients absent"""
    n2, inv_T = 130, C.INV_TS[0]
    f, cls = C.ucl_features("spread", n2, dim, key=only), C.ucl_classes("random", n2, key=only)
    gouts = [g if k == only else None for k, g in enumerate(C.ucl_gouts(n2))]
    ref = {dt: C.ucl_dense(f, cls, inv_T, gouts, dt) for dt in (F32, F64)}
    for form in FORMS:
        _, grad = _ucl_run(f, cls, inv_T, gouts, form, monkeypatch)
        _eq("ucl_grad", grad, ref[F32][5], ref[F64][5], "ucl 2N=130 dim=%d only %s, %s" % (dim, SUM_NAMES[only], form),
            factor=UCL_FACTOR["ucl_grad"])


@pytest.mark.parametrize("n2", C.RANGE_SIZES)
@pytest.mark.parametrize("side", ["near", "far"])
def test_ucl_range_decision(side, n2, monkeypatch):
    """Row maxima spread over less than 2^16 take the one-exponential kernel, over more the general one: near the boundary on
    either side.  On the far side the default form IS the two-exponential launch: the same bits."""
    f, cls, ref = C.range_case(side, n2)
    gouts = C.ucl_gouts(n2)
    what = "range %s 2N=%d" % (side, n2)
    outs, g_default = _ucl_run(f, cls, C.RANGE_INV_T, gouts, "default", monkeypatch)
    _check_ucl_forward(outs, ref, what)
    assert C.RANGE_BOUND[side](C.rowmax_spread(outs[0])), C.rowmax_spread(outs[0])
    _, g_two = _ucl_run(f, cls, C.RANGE_INV_T, gouts, "two_exp", monkeypatch)
    _, g_split = _ucl_run(f, cls, C.RANGE_INV_T, gouts, "split", monkeypatch)
    for form, g in (("default", g_default), ("two_exp", g_two), ("split", g_split)):
        _eq("ucl_grad", g, ref[F32][5], ref[F64][5], what + " dfeat " + form, factor=UCL_FACTOR["ucl_grad"])
    if side == "far":
        assert torch.equal(g_default, g_two), what + ": the default form did not take the general kernel"


def test_ucl_refuses_shapes_it_cannot_serve():
    from cet_pick_amd.models.loss import _UclRowSumsFn
    f = C.ucl_features("normalised", 66, 32).cuda()
    cls = C.ucl_classes("random", 66).cuda()
    wide = torch.zeros(66, 48, device="cuda")
    for feat, c, shape in ((f[:65].contiguous(), cls[:65].contiguous(), "(65, 32)"), (wide, cls, "(66, 48)"), (f[:0], cls[:0], "(0, 32)"),
                           (f[:, :16].contiguous(), cls, "(66, 16)"), (f, cls[:64].contiguous(), "(64,)"),
                           (torch.zeros(66, 64, device="cuda")[:, :32], cls, "(66, 32)")):
        with pytest.raises((_err(), ValueError)) as info:
            _UclRowSumsFn.apply(feat, c, C.INV_TS[0])
        assert shape.replace(" ", "") in str(info.value).replace(" ", ""), str(info.value)
    with pytest.raises(_err()):
        _UclRowSumsFn.apply(f, cls.long(), C.INV_TS[0])
    opt = SimpleNamespace(thresh=1.0, device=torch.device("cuda"))
    lab, o1, o2, _, _ = [t.cuda() for t in C.tail_case(33, 32, "standard")]
    with pytest.raises((_err(), ValueError), match="65"):
        _ML().UnbiasedConLoss(C.TAIL_T, C.TAIL_TAU_PLUS)(lab, o1, o2, torch.zeros(33, 65, device="cuda"), torch.zeros(33, 65, device="cuda"), opt)
    for shape in ((0,), (2, 0, 4)):
        with pytest.raises((_err(), ValueError)) as info:
            _ML().FocalLoss()(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
        assert str(shape).replace(" ", "") in str(info.value).replace(" ", "")


# ------------------------------------------------------------------------------------------------
# 3. UnbiasedConLoss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,thresh,kind", C.TAIL_CASES)
def test_unbiased_con_loss(n, dim, thresh, kind):
    lab, o1, o2, f, f_cr = C.tail_case(n, dim, kind)
    ref = C.tail_reference(n, dim, thresh, kind)
    (sup32, unsup32, g32), (sup64, unsup64, g64) = ref[F32], ref[F64]
    leaves = [t.cuda().requires_grad_(True) for t in (f, f_cr, o1, o2)]
    opt = SimpleNamespace(thresh=thresh, device=torch.device("cuda"))
    sup, unsup = _ML().UnbiasedConLoss(C.TAIL_T, C.TAIL_TAU_PLUS)(lab.cuda(), leaves[2], leaves[3], leaves[0], leaves[1], opt)
    (sup + 0.1 * unsup).backward()
    what = "UnbiasedConLoss N=%d dim=%d thresh=%g %s" % (n, dim, thresh, kind)
    assert bool(torch.isfinite(sup)) and bool(torch.isfinite(unsup)), what
    _eq("ucl_tail", torch.stack([sup, unsup]), torch.stack([sup32, unsup32]), torch.stack([sup64, unsup64]), what + " (sup, unsup)",
        factor=UCL_FACTOR["ucl_tail"])
    for name, leaf, a, b in zip(("df", "df_cr", "do", "do_cr"), leaves, g32, g64):
        assert leaf.grad.shape == a.shape
        _eq("ucl_tail", leaf.grad, a, b, what + " " + name, factor=UCL_FACTOR["ucl_tail"])
