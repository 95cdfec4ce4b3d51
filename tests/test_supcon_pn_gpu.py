"""--pn on the GPU: `SupConLossV2_more` (mi_ucl_rowsums + mi_supcon_pn_rows) against the float64 dense restatement of
tests/supcon_pn_ref.py, loss and d / d features, at the tolerances tests/test_losses_gpu.py holds `UnbiasedConLoss` to against its
oracle (loss rtol 1e-4, gradient 3e-4 of its largest entry); `TomoCRSupLoss` and one trainer step under --pn."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import supcon_pn_ref as R

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_ATOL = 1e-4, 3e-4          # tests/test_losses_gpu.py::test_unbiased_con_loss_vs_oracle_ragged


def _opt(thresh):
    return SimpleNamespace(thresh=thresh, device=torch.device("cuda"))


# N = 16: 2N <= 32, the row-sum kernel's second column half stays empty; 96: 2N is no multiple of 64; 160: three row blocks.
# dim 16 is padded to 32.
@pytest.mark.parametrize("dim", [16, 32, 64])
@pytest.mark.parametrize("n", [16, 48, 96, 160])
def test_supcon_pn_loss_and_gradient_vs_dense_float64(n, dim):
    from cet_pick_amd.models.loss import SupConLossV2_more
    for T in (0.07, 0.5):
        for thresh in (0.85, 0.3):
            for kind in ("binary", "mixed"):
                f, f_cr, lab = R.case_inputs(n, dim, thresh, kind)
                want, ga, gb = R.case_reference(n, dim, thresh, kind, T)
                a, b = f.cuda().requires_grad_(), f_cr.cuda().requires_grad_()
                loss = SupConLossV2_more(T)(lab.cuda(), None, None, a, b, _opt(thresh))
                (1.5 * loss).backward()
                tag = (n, dim, T, thresh, kind)
                eg = max(float((t.grad.cpu().double() / 1.5 - r).abs().max()) for t, r in ((a, ga), (b, gb)))
                gmax = max(float(ga.abs().max()), float(gb.abs().max()))
                got = float(loss.detach())
                print("%s: loss %.7f want %.7f rel %.2e, grad err %.2e of %.3e" % (tag, got, want, abs(got - want) / abs(want), eg, gmax))
                assert loss.shape == () and loss.dtype == torch.float32
                np.testing.assert_allclose(got, want, rtol=LOSS_RTOL, err_msg=str(tag))
                for t, r in ((a, ga), (b, gb)):
                    assert t.grad.shape == r.shape
                    np.testing.assert_allclose(t.grad.cpu().double().numpy() / 1.5, r.numpy(), rtol=0,
                                               atol=GRAD_ATOL * float(r.abs().max()) + 1e-9, err_msg=str(tag))


def test_supcon_pn_record_and_row_weights():
    """the 72-double record of the forward (counts, G, the two masked sums) and g_all = d loss / d Z against float64"""
    from cet_pick_amd.models.loss import _SupConPNFn, _pad_features
    n, dim, thresh, T = 96, 32, 0.3, 0.07
    f, f_cr, lab = R.case_inputs(n, dim, thresh, "mixed")
    pos, un = R.masks(lab, thresh)
    feat = _pad_features(torch.cat([f, f_cr]).cuda()).requires_grad_()
    cls = (pos.to(torch.uint8) | (un.to(torch.uint8) << 1)).cuda()
    loss = _SupConPNFn.apply(feat, cls, 1.0 / T)
    sums = loss.grad_fn.sums.cpu()
    F = torch.cat([f, f_cr]).double()
    assert sums[0] == float(pos.sum()) and sums[1] == float(un.sum())
    np.testing.assert_allclose(sums[8:8 + dim].numpy(), F[pos].sum(0).numpy(), rtol=0, atol=1e-12)
    assert float(sums[8 + dim:].abs().max()) == 0.0
    np.testing.assert_allclose(float(-sums[2] / sums[0] - sums[3] / sums[1]), float(sums[4]), rtol=1e-14)
    assert float(loss.detach()) == float(sums[4].float())


def test_supcon_pn_same_scalar_at_another_width():
    """dim 16 features padded to 32 by the class, and the same rows padded to 64 by hand: other kernels of the row-sum walk, other
    template instances of the row pass, twice the lanes' columns - the zero columns change no bit of the scalar, and the
    gradient's first 16 columns agree to the gradient tolerance."""
    from cet_pick_amd.models.loss import SupConLossV2_more
    n, thresh, T = 160, 0.85, 0.07
    f, f_cr, lab = R.case_inputs(n, 16, thresh, "mixed")
    out = []
    for width in (16, 64):
        a = torch.nn.functional.pad(f, (0, width - 16)).cuda().requires_grad_()
        b = torch.nn.functional.pad(f_cr, (0, width - 16)).cuda().requires_grad_()
        loss = SupConLossV2_more(T)(lab.cuda(), None, None, a, b, _opt(thresh))
        loss.backward()
        out.append((loss.detach().cpu(), a.grad.cpu()))
    assert torch.equal(out[0][0], out[1][0]), (float(out[0][0]), float(out[1][0]))
    assert float(out[1][1][:, 16:].abs().max()) == 0.0
    assert float((out[0][1] - out[1][1][:, :16]).abs().max()) <= GRAD_ATOL * float(out[0][1].abs().max())


def test_supcon_pn_error_cases():
    from cet_pick_amd._lib import HipExtensionError
    from cet_pick_amd.models.loss import SupConLossV2_more, _NO_POS
    f, f_cr, lab = R.case_inputs(16, 16, 0.3, "binary")
    crit = SupConLossV2_more(0.07)
    with pytest.raises(ValueError, match="true positive is zero") as e:
        crit(torch.zeros(16).cuda(), None, None, f.cuda(), f_cr.cuda(), _opt(0.3))
    assert str(e.value) == _NO_POS
    with pytest.raises(ValueError, match="below --thresh"):                       # every label above thresh: no negative row
        crit(torch.ones(16).cuda(), None, None, f.cuda(), f_cr.cuda(), _opt(0.3))
    with pytest.raises(HipExtensionError, match="> 64"):
        crit(lab.cuda(), None, None, torch.zeros(16, 65).cuda(), torch.zeros(16, 65).cuda(), _opt(0.3))
    with pytest.raises(HipExtensionError):
        crit(lab, None, None, f, f_cr, _opt(0.3))                                 # host tensors: there is no CPU path


def _semi_opt(**kw):
    o = dict(pn=False, ge=False, tau=0.1, temp=0.07, thresh=0.5, cr_weight=0.1, num_stacks=1, contrastive=True, device=torch.device("cuda"))
    o.update(kw)
    return SimpleNamespace(**o)


def _pn_loss_inputs(flip_prob):
    from cet_pick_amd.synthetic import semi_loss_inputs
    gt, hm, hm_cr, pj, pj_cr = semi_loss_inputs(flip_prob)
    return torch.where(gt < 0, torch.zeros_like(gt), gt), hm, hm_cr, pj, pj_cr       # fully annotated: no -1


@pytest.mark.parametrize("flip_prob", [0.2, 0.8])
@pytest.mark.parametrize("ge", [False, True])
def test_tomo_cr_semi_loss_with_pn(flip_prob, ge):
    """hm_loss is FocalLoss on the clamped sigmoid heat-map, cr_loss the single SupConLossV2_more scalar of the un-flipped second view
    (checked against the dense float64 form), the consistency term what the PU run has; with --ge as well, --pn wins."""
    from cet_pick_amd.models.loss import ConsistencyLoss, FocalLoss
    from cet_pick_amd.models.utils import _sigmoid
    from cet_pick_amd.trains.tomo_cr_semi_trainer import TomoCRSupLoss
    gt, hm, hm_cr, pj, pj_cr = _pn_loss_inputs(flip_prob)
    dev_in = [t.clone().cuda().requires_grad_() for t in (hm, hm_cr, pj, pj_cr)]
    out = [{"hm": dev_in[0] * 1.0, "proj": dev_in[2]}]
    out_cr = [{"hm": dev_in[1] * 1.0, "proj": dev_in[3]}]
    loss, stats = TomoCRSupLoss(_semi_opt(pn=True, ge=ge))(out, {"hm": gt.cuda(), "flip_prob": flip_prob}, 1, "train", out_cr)
    loss.backward()
    assert all(bool(torch.isfinite(stats[k])) for k in ("loss", "hm_loss", "cr_loss", "consis_loss"))
    p, p_cr = _sigmoid(hm.clone().cuda()), _sigmoid(hm_cr.clone().cuda())
    assert torch.equal(stats["hm_loss"].detach(), FocalLoss()(p, gt.cuda()))
    flip = -2 if flip_prob > 0.5 else -1
    assert torch.equal(stats["consis_loss"].detach(), ConsistencyLoss()(p.reshape(-1), p_cr.flip(flip).reshape(-1).contiguous()))
    assert torch.equal(stats["loss"], stats["hm_loss"] + stats["cr_loss"] * 0.1 + stats["consis_loss"])
    rows = lambda t: t.reshape(t.shape[0], t.shape[1], -1).permute(1, 0, 2).reshape(t.shape[1], -1).T
    fa, fb = rows(pj.double()).requires_grad_(), rows(pj_cr.flip(flip).double()).requires_grad_()
    want = R.dense_loss(fa, fb, gt.reshape(-1), 0.5, 0.07)
    np.testing.assert_allclose(float(stats["cr_loss"].detach()), float(want.detach()), rtol=LOSS_RTOL)
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in dev_in)
    val_loss, vstats = TomoCRSupLoss(_semi_opt(pn=True, ge=ge))([{"hm": hm.cuda().clone(), "proj": None}], {"hm": gt.cuda()}, 1, "val")
    assert torch.equal(val_loss, FocalLoss()(p, gt.cuda())) and float(vstats["cr_loss"]) == 0.0


@pytest.mark.parametrize("ge", [False, True])
def test_tomo_cr_semi_loss_without_pn_is_its_parts_bit_for_bit(ge):
    """pn=False: the module's four numbers and gradients are those of its loss classes called directly, in the order it calls them"""
    from cet_pick_amd.models import loss as ML
    from cet_pick_amd.models.utils import _sigmoid
    from cet_pick_amd.synthetic import semi_loss_inputs
    from cet_pick_amd.trains.tomo_cr_semi_trainer import TomoCRSemiLoss
    flip_prob = 0.2
    gt, hm, hm_cr, pj, pj_cr = semi_loss_inputs(flip_prob)
    opt = _semi_opt(ge=ge)

    def leaves():
        return [t.clone().cuda().requires_grad_() for t in (hm, hm_cr, pj, pj_cr)]

    a = leaves()
    loss, stats = TomoCRSemiLoss(opt)([{"hm": a[0] * 1.0, "proj": a[2]}], {"hm": gt.cuda(), "flip_prob": flip_prob}, 1, "train",
                                      [{"hm": a[1] * 1.0, "proj": a[3]}])
    loss.backward()
    b = leaves()
    p, p_cr = _sigmoid(b[0] * 1.0), _sigmoid(b[1] * 1.0)
    crit = ML.PUGELoss(opt.tau, criteria=ML.FocalLoss()) if ge else ML.PULoss(opt.tau)
    hm_loss = crit(p, gt.cuda())
    rows = lambda t: t.reshape(t.shape[0], t.shape[1], -1).permute(1, 0, 2).reshape(t.shape[1], -1).T
    hm_f, hm_cr_f = p.reshape(-1).contiguous(), p_cr.flip(-1).reshape(-1).contiguous()
    sup, unsup = ML.UnbiasedConLoss(opt.temp, opt.tau)(gt.cuda().reshape(-1).contiguous(), hm_f, hm_cr_f, rows(b[2]), rows(b[3].flip(-1)), opt)
    cr = 0 + sup + 0.1 * unsup
    cons = 0 + ML.ConsistencyLoss()(hm_f, hm_cr_f)
    total = hm_loss + cr * opt.cr_weight + cons
    total.backward()
    for k, v in (("loss", total), ("hm_loss", hm_loss), ("cr_loss", cr), ("consis_loss", cons)):
        assert torch.equal(stats[k], v), k
    for x, y in zip(a, b):
        assert torch.equal(x.grad, y.grad)


def test_semi_trainer_steps_with_pn_on_two_small_tomograms():
    """one `semi` step with --pn --contrastive on two 12 x 96 x 96 tomograms with 6 annotations each, through the file dataset's
    in-memory form and TomoCRSemiTrainer; a second step must run, nothing about its loss is asserted"""
    from cet_pick_amd.datasets.semi_files import TomoFileDetectorDataset, TomoFileSupervisedDataset, detector_dataset
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.synthetic import seeded_state_dict
    from cet_pick_amd.trains.train_factory import train_factory
    heads = {"hm": 1, "proj": 32}
    opt = SimpleNamespace(task="semi", arch="unet_4", pn=True, ge=False, tau=0.1, temp=0.07, thresh=0.5, cr_weight=0.1,
                          num_stacks=1, contrastive=True, device=torch.device("cuda"), num_iters=-1, print_iter=0,
                          hide_data_time=True, exp_id="t", lr=1e-3, hipgraph=False, down_ratio=2, bbox=16, translation_ratio=0.5,
                          fiber=False, compress=False, batch_size=1, seed=11)
    rng = np.random.default_rng(3)
    tomos = {"t%d" % i: torch.as_tensor(rng.standard_normal((12, 96, 96)).astype(np.float32)).cuda() for i in range(2)}
    coords = {k: np.stack([rng.integers(30, 66, 6), rng.integers(30, 66, 6), rng.integers(3, 9, 6)], 1) for k in tomos}
    assert detector_dataset(opt) is TomoFileSupervisedDataset and detector_dataset(SimpleNamespace(pn=False)) is TomoFileDetectorDataset
    ds = detector_dataset(opt).from_arrays(opt, "train", tomos, coords)
    assert len(ds) == 12 and all(float(lab.min()) == 0.0 and float(lab.max()) == 1.0 for lab in ds.labels)      # no -1 under --pn
    ds.set_epoch(1)
    batches = [b for _, b in zip(range(2), ds)]
    assert batches[0]["hm"].shape == (2, 1, 6, 32, 32) and float(batches[0]["hm"].min()) >= 0.0
    model = create_model(opt.arch, heads, 32)
    sd0 = seeded_state_dict(model, seed=323)
    for k in ("hm.weight", "proj.weight"):
        sd0[k] = sd0[k] * 0.3
    model.load_state_dict(sd0)
    trainer = train_factory["semi"](opt, model, torch.optim.SGD(model.parameters(), lr=opt.lr))
    trainer.set_device([0], None, "cuda")
    from cet_pick_amd.trains.tomo_cr_semi_trainer import TomoCRSupLoss
    assert isinstance(trainer.loss, TomoCRSupLoss)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for epoch, batch in enumerate(batches, start=1):
        stats, _ = trainer.train(epoch, [dict(batch)])
        print("epoch %d: %s" % (epoch, {k: v for k, v in stats.items() if k != "time"}))
        assert set(stats) == {"loss", "hm_loss", "cr_loss", "consis_loss", "time"}
        assert all(np.isfinite(stats[k]) for k in ("loss", "hm_loss", "cr_loss", "consis_loss")), (epoch, stats)
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters()), epoch
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "hm.weight" in moved and "proj.weight" in moved
    val, _ = trainer.val(2, [dict(batches[0])])
    assert np.isfinite(val["loss"]) and val["cr_loss"] == 0


def test_detector_main_with_pn_on_mrc_files(tmp_path, monkeypatch, capsys):
    """`main semi --pn` end to end on two listed MRC tomograms: main picks the supervised dataset, the trainer the supervised loss"""
    import os
    from cet_pick_amd import main as det_main
    from cet_pick_amd.opts import opts
    from cet_pick_amd.synthetic import make_tomo
    from cet_pick_amd.utils import mrc
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data"
    data.mkdir()
    lines, rows = ["image_name\trec_path"], ["image_name\tx_coord\ty_coord\tz_coord"]
    for i in range(2):
        vol, c = make_tomo((32, 160, 160), seed=700 + i, margin_xy=40, margin_z=8)
        mrc.write(str(data / ("tomo%d.rec" % i)), vol)
        lines.append("tomo%d\ttomo%d.rec" % (i, i))
        rows += ["tomo%d\t%d\t%d\t%d" % (i, x, y, z) for x, y, z in c]
    (data / "train_images.txt").write_text("\n".join(lines) + "\n")
    (data / "coords.txt").write_text("\n".join(rows) + "\n")
    det_main.main(opts().parse(["semi", "--arch", "unet_4", "--contrastive", "--pn", "--dataset", "semi", "--order", "zxy", "--bbox", "16",
                                "--batch_size", "2", "--num_epochs", "1", "--lr", "0.001", "--val_intervals", "1", "--exp_id", "pn",
                                "--debug", "0", "--train_img_txt", "train_images.txt", "--train_coord_txt", "coords.txt"]))
    assert "Loaded train %d samples" % (len(rows) - 1) in capsys.readouterr().out
    log = open(os.path.join(str(tmp_path), "exp", "semi", "pn", "log.txt")).read().strip().split("\n")
    assert len(log) == 1 and log[0].startswith("epoch: 1 |loss ")
    vals = [float(v.split()[1]) for v in log[0].split("|")[1:] if v.strip() and v.split()[0] in ("loss", "hm_loss", "cr_loss", "consis_loss")]
    assert len(vals) == 8 and np.isfinite(vals).all() and vals[2] > 0                   # train + val columns; a contrastive term in training
