"""The GE-binomial heat-map loss of `main semi --ge` (csrc/loss_ge.hip, models/loss.py `PUGELoss`) against the float64 restatement
of tests/ge_loss_cases.py - scipy's log Binom and the full softmax over all N + 1 counts - at voxel counts taken from the kernels' own
constants, every label mix and regime of the predictions, and at count windows below, at and past one workgroup and past the count
grid.  Each case checks the loss, the gradient of UPSTREAM x loss (whole, and per label class), and the counts, mu and v the
kernel leaves in `sums`.  Then `TomoCRSemiLoss` and two optimiser steps of the `semi` trainer with ge=True.

Numeric results go through conftest.f32_equivalent at the voxel losses' factor 2: the GPU may lie as far from float64 as twice a
float32 torch evaluation of the same formula, plus the default floor.  Counts are compared exactly.  mu and v are double sums of
exact products of float32 inputs: held to 1e-12.  tests/test_ge_cases_cpu.py checks the cases and the restatement themselves.

Measured on the MI355X over all cases, as norm-relative errors against float64: GPU 1.4e-7 at the most, the float32 evaluation
1.1e-2 at the most; no GPU result lies above the 2e-6 floor, factor 2 stands.  The restatement takes b_k relative
to b_k* like the kernel: against the plain b_k - B the kernel is 1.3e-4 away on the p in [1e-6, 1e-5] cases, which is the plain
form's own rounding error (test_ge_cases_cpu.py::test_count_stage_against_400_digit_arithmetic)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ge_loss_cases as C

pytestmark = pytest.mark.gpu

ERRORS = {}                                # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64, largest ratio above the floor]


def _ML():
    from cet_pick_amd.models import loss as ML
    return ML


def _eq(group, got, cpu32, ref64, what):
    from conftest import f32_equivalent
    g, c, r = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64).ravel() for t in (got, cpu32, ref64))
    scale = float(np.linalg.norm(r)) + 1e-30
    e_g, e_c = float(np.linalg.norm(g - r)) / scale, float(np.linalg.norm(c - r)) / scale
    print("%-8s %-72s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    rec = ERRORS.setdefault(group, [0.0, 0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e_g), max(rec[1], e_c)
    if e_g > 2e-6:
        rec[2] = max(rec[2], e_g / max(e_c, 1e-30))
    f32_equivalent(g, c, r, factor=2.0, what=what)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, (e_g, e_c, ratio) in sorted(ERRORS.items()):
        print("\nlargest error, %-8s GPU %.3e  CPU fp32 %.3e  largest GPU / CPU ratio above the floor %.2f" % (group, e_g, e_c, ratio))


def _run(module, pred, gt):
    p = pred.cuda().requires_grad_(True)
    loss = module(p, gt.cuda())
    sums = loss.grad_fn.sums
    (C.UPSTREAM * loss).backward()
    return loss.detach(), p.grad, sums.clone()


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_ge_loss(case):
    pred, gt = C.case_inputs(case)
    loss64, grad64, info, loss32, grad32 = C.case_reference(case)
    module = _ML().PUGELoss(case.tau, criteria=_ML().FocalLoss(), slack=case.slack, entropy_penalty=case.entropy_penalty)
    loss, grad, sums = _run(module, pred, gt)
    s = sums.cpu().numpy()
    what = case.id
    assert s.shape == (16,) and [float(x) for x in s[:3]] == [float(c) for c in info["counts"]], what + ": class counts"
    assert s[10] == float(case.n)
    np.testing.assert_allclose(s[5:7], [info["mu"], info["v"]], rtol=1e-12, atol=0, err_msg=what + ": mu, v")
    assert 0 <= s[14] <= s[15] <= info["N"]
    if case.walked:
        assert C.WALKED[case.walked](int(s[15] - s[14]) + 1), (case.walked, s[14], s[15])
    _eq("ge", loss, loss32, loss64, what + " loss")
    _eq("ge", s[9], float(np.float32(info["pen"])), info["pen"], what + " pen")        # a double on the device: to float32's rounding
    assert grad.shape == pred.shape
    grad = grad.cpu()
    _eq("ge", grad, grad32, grad64, what + " dpred")
    g64 = torch.from_numpy(grad64)
    for name, m in zip(("pos", "soft", "unl"), (torch.from_numpy(m) for m in C.classes(gt.numpy()))):
        if not bool(m.any()):
            continue
        if not bool(g64[m].any()):
            assert not bool(grad[m].any()), what + ": dpred is not zero on the %s voxels" % name
        else:
            _eq("ge", grad[m], grad32[m], g64[m], what + " dpred[%s]" % name)
    # the classifier part is the focal loss on the whole volume, with the bits mi_focal_loss_fwd gives
    focal = _ML().FocalLoss()(pred.cuda().requires_grad_(True), gt.cuda())
    assert float(focal.grad_fn.sums[8]) == s[7], what + ": focal part"
    # deterministic: a second evaluation gives the same bits
    loss2, grad2, sums2 = _run(module, pred, gt)
    assert torch.equal(loss, loss2) and torch.equal(grad2.cpu(), grad) and torch.equal(sums, sums2), what + ": not deterministic"


@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_tau_at_the_ends_is_refused_before_any_launch(tau):
    from cet_pick_amd.models.loss import _PUGELossFn
    from cet_pick_amd import _lib
    pred, gt = C.case_inputs(C.CASES[0])
    with pytest.raises(ValueError, match="tau"):
        _ML().PUGELoss(tau)
    with pytest.raises(ValueError, match="tau"):
        _PUGELossFn.apply(pred.cuda(), gt.cuda(), tau, 1.0, 0.0)
    # the entry point itself: MI_E_ARG, and neither output is written
    p, g = pred.cuda(), gt.cuda()
    sums = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    loss = torch.full((), -7.0, device="cuda")
    ws = torch.zeros(_lib.lib().mi_pu_ge_loss_workspace_bytes(p.numel()), dtype=torch.uint8, device="cuda")
    rc = _lib.lib().mi_pu_ge_loss_fwd(_lib.ptr(p), _lib.ptr(g), p.numel(), tau, 1.0, 0.0, _lib.ptr(sums), _lib.ptr(loss), _lib.ptr(ws),
                                      ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and float(loss) == -7.0 and bool((sums == -7.0).all()) and not bool(ws.any())


def test_criteria_other_than_the_focal_loss_is_refused():
    from cet_pick_amd._lib import HipExtensionError
    with pytest.raises(HipExtensionError, match="FocalLoss"):
        _ML().PUGELoss(0.1, criteria=torch.nn.BCELoss())


def _semi_opt(**kw):
    o = dict(pn=False, ge=False, tau=0.1, temp=0.07, thresh=0.5, cr_weight=0.1, num_stacks=1, contrastive=True, device=torch.device("cuda"))
    o.update(kw)
    return SimpleNamespace(**o)


@pytest.mark.parametrize("flip_prob", [0.2, 0.8])
def test_tomo_cr_semi_loss_with_ge(flip_prob):
    """hm_loss is the GE loss of the clamped sigmoid heat-map; the contrastive and consistency entries are, bit for bit, what the
    same inputs give with ge=False."""
    from cet_pick_amd.trains.tomo_cr_semi_trainer import TomoCRSemiLoss
    from cet_pick_amd.synthetic import semi_loss_inputs
    gt, hm, hm_cr, pj, pj_cr = semi_loss_inputs(flip_prob)
    stats, grads = {}, {}
    for ge in (False, True):
        dev_in = [t.clone().cuda().requires_grad_() for t in (hm, hm_cr, pj, pj_cr)]
        out = [{"hm": dev_in[0] * 1.0, "proj": dev_in[2]}]
        out_cr = [{"hm": dev_in[1] * 1.0, "proj": dev_in[3]}]
        loss, stats[ge] = TomoCRSemiLoss(_semi_opt(ge=ge))(out, {"hm": gt.cuda(), "flip_prob": flip_prob}, 1, "train", out_cr)
        loss.backward()
        grads[ge] = [t.grad for t in dev_in]
    for k in ("cr_loss", "consis_loss"):
        assert torch.equal(stats[True][k], stats[False][k]), k
    p = torch.clamp(torch.sigmoid(hm), 1e-4, 1 - 1e-4).reshape(-1)           # models/utils.py `_sigmoid`, in float32 as the device has it
    loss64, _, _ = C.reference64(p, gt.reshape(-1), 0.1)
    loss32, _ = C.evaluate32(p, gt.reshape(-1), 0.1)
    _eq("semi", stats[True]["hm_loss"], loss32, loss64, "TomoCRSemiLoss ge=True hm_loss, flip_prob %g" % flip_prob)
    total = stats[True]["hm_loss"] + stats[True]["cr_loss"] * 0.1 + stats[True]["consis_loss"]
    assert torch.equal(stats[True]["loss"], total)
    assert float(stats[True]["hm_loss"].detach()) != float(stats[False]["hm_loss"].detach())
    # the projections see the heat-map loss through nothing: their gradients are the PU run's
    assert torch.equal(grads[True][2], grads[False][2]) and torch.equal(grads[True][3], grads[False][3])
    assert bool(torch.isfinite(grads[True][0]).all()) and not torch.equal(grads[True][0], grads[False][0])
    val_loss, _ = TomoCRSemiLoss(_semi_opt(ge=True))([{"hm": hm.cuda().clone(), "proj": None}], {"hm": gt.cuda()}, 1, "val")
    val_pu, _ = TomoCRSemiLoss(_semi_opt(ge=False))([{"hm": hm.cuda().clone(), "proj": None}], {"hm": gt.cuda()}, 1, "val")
    assert torch.equal(val_loss, val_pu)


def test_tomo_cr_semi_loss_with_pn_still_raises():
    from cet_pick_amd.trains.tomo_cr_semi_trainer import TomoCRSemiLoss
    for ge in (False, True):
        with pytest.raises(NotImplementedError, match="--pn"):
            TomoCRSemiLoss(_semi_opt(pn=True, ge=ge))


def test_semi_trainer_two_steps_with_ge():
    """unet_4 through TomoCRSemiTrainer with ge=True, set up as tests/test_trainer_gpu.py sets up its PU run"""
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.synthetic import seeded_state_dict
    from cet_pick_amd.trains.train_factory import train_factory
    heads = {"hm": 1, "proj": 32}
    opt = SimpleNamespace(task="semi", arch="unet_4", pn=False, ge=True, tau=0.1, temp=0.07, thresh=0.5, cr_weight=0.1,
                          num_stacks=1, contrastive=True, device=torch.device("cuda"), num_iters=-1, print_iter=0,
                          hide_data_time=True, exp_id="t", lr=1e-3, hipgraph=False)
    model = create_model(opt.arch, heads, 32)
    sd0 = seeded_state_dict(model, seed=323)
    for k in ("hm.weight", "proj.weight"):
        sd0[k] = sd0[k] * 0.3
    model.load_state_dict(sd0)
    trainer = train_factory["semi"](opt, model, torch.optim.SGD(model.parameters(), lr=opt.lr))
    trainer.set_device([0], None, "cuda")
    g = torch.Generator().manual_seed(2)
    b, d, h, w = 2, 4, 48, 48
    x = torch.randn(b, d, h, w, generator=g)
    x_aug = x.flip(-1) + 0.05 * torch.randn(b, d, h, w, generator=g)
    gt = torch.full((b, 1, d, h // 2, w // 2), -1.0)
    r = torch.rand(gt.shape, generator=g)
    gt[r < 0.3] = 0.0
    gt[(r >= 0.3) & (r < 0.4)] = 0.6
    gt[r > 0.96] = 1.0
    batch = {"input": x, "input_aug": x_aug, "hm": gt, "flip_prob": 0.2, "meta": {}}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for epoch in (1, 2):
        stats, _ = trainer.train(epoch, [dict(batch)])
        print("epoch %d: %s" % (epoch, {k: v for k, v in stats.items() if k != "time"}))
        assert set(stats) == {"loss", "hm_loss", "cr_loss", "consis_loss", "time"}
        assert all(np.isfinite(stats[k]) for k in ("loss", "hm_loss", "cr_loss", "consis_loss")), (epoch, stats)
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters()), epoch
        if epoch == 1:                         # the penalty is a sum over voxels, not a mean: its first step is a large one
            moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
            assert "hm.weight" in moved and len(moved) >= len(before) // 2, (epoch, moved)
    val, _ = trainer.val(2, [dict(batch)])
    assert np.isfinite(val["loss"]) and val["cr_loss"] == 0
