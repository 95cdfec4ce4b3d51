"""Mirror of the loss half of `cet_pick/trains/tomo_cr_semi_trainer.py` (`TomoCRSemiLoss` :18-112): PU focal risk on
the heat-map + debiased contrastive regularisation between the two augmented views + consistency, composed from the
HIP losses in models/loss.py.  `--ge` swaps the PU risk for the GE-binomial loss (PUGELoss, csrc/loss_ge.hip).  `--pn`, for fully
annotated tomograms, is a loss module of its own, `TomoCRSupLoss`: the focal loss and `SupConLossV2_more`'s single scalar as the
contrastive term; the trainer picks it, and with both switches `--pn` wins, as in the reference (:25-37).
`TomoCRSemiLoss` itself stays the positive-unlabeled module and refuses `opt.pn`.

`TomoCRSemiTrainer` drives it through the shared `BaseTrainer` loop (two forward passes per step).  Its `debug`
(:123-186) is utils/debug_vis.py: the detection table and, under --debug 4, the slice pictures of every validation sample.
"""
import torch

from .base_trainer import BaseTrainer
from ..models.loss import ConsistencyLoss, FocalLoss, PUGELoss, PULoss, SupConLossV2_more, UnbiasedConLoss
from ..models.utils import _sigmoid


class TomoCRSemiLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        if opt.pn:
            raise NotImplementedError("--pn is not a variant of the positive-unlabeled TomoCRSemiLoss: the fully supervised loss "
                                      "is TomoCRSupLoss (TomoCRSemiTrainer picks it)")
        self.crit = PUGELoss(opt.tau, criteria=FocalLoss()) if opt.ge else PULoss(opt.tau)      # :27-31
        self.crit2 = FocalLoss()
        self.cr_loss = UnbiasedConLoss(opt.temp, opt.tau)
        self.cons_loss = ConsistencyLoss()
        self.opt = opt

    def contrastive(self, gt_f, hm_f, hm_cr_f, feat, feat_cr):
        """the contrastive term of the two views' voxel rows (:93-100)"""
        sup, unsup = self.cr_loss(gt_f, hm_f, hm_cr_f, feat, feat_cr, self.opt)
        return sup + 0.1 * unsup

    def forward(self, outputs, batch, epoch, phase, output_cr=None):
        opt = self.opt
        cr_loss, hm_loss, consis_loss = 0, 0, 0
        for s in range(opt.num_stacks):
            output = outputs[s]
            if output_cr is not None:
                output_cr = output_cr[s]
            output["hm"] = _sigmoid(output["hm"])
            if output_cr is not None:
                output_cr["hm"] = _sigmoid(output_cr["hm"])
        crit = self.crit if phase == "train" else self.crit2
        hm_loss = hm_loss + crit(output["hm"], batch["hm"]) / opt.num_stacks
        if opt.contrastive and phase == "train":
            fm = output["proj"]
            b, ch = fm.shape[:2]
            flip_dim = -2 if batch["flip_prob"] > 0.5 else -1          # undo the second view's flip (:69-74)
            fm_cr = output_cr["proj"].flip(flip_dim)
            hm_cr = output_cr["hm"].flip(flip_dim)
            # (b, ch, d, h, w) -> (b*d*h*w, ch), voxels of a batch element contiguous (:75-80)
            feat = fm.reshape(b, ch, -1).permute(1, 0, 2).reshape(ch, -1).T
            feat_cr = fm_cr.reshape(b, ch, -1).permute(1, 0, 2).reshape(ch, -1).T
            gt_f = batch["hm"].reshape(-1).contiguous()
            hm_f = output["hm"].reshape(-1).contiguous()
            hm_cr_f = hm_cr.reshape(-1).contiguous()
            cr_loss = cr_loss + self.contrastive(gt_f, hm_f, hm_cr_f, feat, feat_cr)
            consis_loss = consis_loss + self.cons_loss(hm_f, hm_cr_f)
            loss = hm_loss + cr_loss * opt.cr_weight + consis_loss
        else:
            cr_loss = hm_loss * 0
            loss = hm_loss
            consis_loss = hm_loss * 0
        return loss, {"loss": loss, "hm_loss": hm_loss, "cr_loss": cr_loss, "consis_loss": consis_loss}


class TomoCRSupLoss(TomoCRSemiLoss):
    """`TomoCRSemiLoss` of the reference under `opt.pn` (:25-37, :93-95), for fully annotated tomograms (labels in [0, 1]): the
    heat-map loss is the focal loss in training as in validation, the contrastive term `SupConLossV2_more`'s ONE scalar, added as it
    is; the consistency loss and the flip handling are the parent's.  `opt.ge` and `opt.tau` are not consulted."""

    def __init__(self, opt):
        torch.nn.Module.__init__(self)
        self.crit = FocalLoss()
        self.crit2 = FocalLoss()
        self.cr_loss = SupConLossV2_more(opt.temp)
        self.cons_loss = ConsistencyLoss()
        self.opt = opt

    def contrastive(self, gt_f, hm_f, hm_cr_f, feat, feat_cr):
        return self.cr_loss(gt_f, hm_f, hm_cr_f, feat, feat_cr, self.opt)


class TomoCRSemiTrainer(BaseTrainer):
    """tomo_cr_semi_trainer.py:114-125: the semi-supervised detector trainer (task 'semi')."""

    def __init__(self, opt, model, optimizer=None):
        super().__init__(opt, model, optimizer=optimizer)

    def _get_losses(self, opt):
        return ["loss", "hm_loss", "cr_loss", "consis_loss"], (TomoCRSupLoss(opt) if opt.pn else TomoCRSemiLoss(opt))

    def debug(self, batch, output, iter_id):
        """tomo_cr_semi_trainer.py:123-186 on the device; the files are complete after `debug_finish()`."""
        from ..utils.debug_vis import render_validation_sample
        render_validation_sample(self.opt, batch, output, iter_id)

    def debug_finish(self):
        from ..utils.debug_vis import finish
        finish()

    def save_result(self, output, batch, results):
        """:189-193 `save_results`: the decoded picks (1, K, 5) in heat-map coordinates."""
        from ..models.decode import tomo_decode
        dets = tomo_decode(output["hm"], K=self.opt.K, if_fiber=self.opt.fiber)
        return dets.detach().cpu().numpy().reshape(1, -1, dets.shape[2])

    save_results = save_result
